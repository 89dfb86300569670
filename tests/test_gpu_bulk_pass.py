"""GPU: the bulk launch of a chain (k_fbc3: tile blocks that stream the tableau through the chain's steps with the step
operands requested groups ahead, patch blocks that write the chain's pivot rows, pivot columns and column 0 beside
them) leaves the same bits as the oracle at the smallest shapes where it can go wrong: chain lengths around the group
size and its multiples, tiles that straddle row m, pairs that straddle column n, pivot columns that share a pair (with
each other, with column 0), rows that leave twice, bound flips at either end of a chain, passes that follow each other
on one handle.  Resident-tableau kernel off; both ways of choosing a chain's steps; every case solved twice, the second
time on the slab the first one gave back; no cluster launch may give up."""
import numpy as np
import pytest

from mvolps_amd import capi, synth

from . import lpgen
from .test_gpu_chain import cluster_counts, twice
from .test_gpu_parity import assert_same_state

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[1, 0], ids=["cluster", "two-launch"])
def chained(gpu, request):
    """Both ways of choosing a chain's steps; wherever the cluster kernel ran, none of its launches gave up."""
    gpu.set_persist(0)
    gpu.set_cluster(request.param)
    before = cluster_counts(gpu)
    yield gpu
    after = cluster_counts(gpu)
    gpu.set_tuning(0, 1, -1)
    gpu.set_chain(0)
    gpu.set_cluster(1)
    gpu.set_persist(1)
    assert after[1] == before[1], "a k_chain launch gave up waiting for its peers"


def dense(m, n, seed):
    A, b, c = synth.dense_lp(m, n, seed)

    def load(api):
        P = api.create()
        P.load_dense(A, b, c)
        return P

    return load


def boxed(m, n, seed, ubd=2):
    """dense_lp with two columns in three boxed to [0, k / ubd], k = 1..3: bound flips from the first step on"""
    A, b, c = synth.dense_lp(m, n, seed)
    rng = np.random.default_rng(5)
    col_b = [(capi.DB, 0.0, float(rng.integers(1, 4)) / ubd) if j % 3 else (capi.LO, 0.0, 0.0) for j in range(n)]
    row_b = [(capi.UP, 0.0, float(v)) for v in b]

    def load(api):
        P = api.create()
        P.load_general(A, row_b, col_b, c, direction=capi.MAX)
        return P

    return load


def degenerate(m, n, seed, frac0):
    A, b, c = lpgen.degenerate_lp(m, n, seed, frac0=frac0)
    return lambda api: lpgen.load_degenerate(api, A, b, c)


def oracle_steps(orc, load, pivots):
    """The first steps of the oracle's solve, in order, up to `pivots` pivots: ("flip", 0, q) / ("pivot", p, q).  Read
    off the bases after load + simplex(it_lim=t), t = 0..pivots: a limited call stops in front of the step that follows
    its last pivot, so what lies between two of these bases is the bound flips of the stretch, then its pivot."""
    out, prev = [], None
    for t in range(pivots + 1):
        P = load(orc)
        P.simplex(it_lim=t)
        cur = P.basis()
        if prev is not None:
            dp, dq = np.flatnonzero(prev[0] != cur[0]), np.flatnonzero(prev[1] != cur[1])
            out += [("flip", 0, int(j)) for j in np.flatnonzero(prev[2] != cur[2]) if j not in dq]
            if not len(dq):
                break
            assert len(dp) == 1 and len(dq) == 1
            out.append(("pivot", int(dp[0]), int(dq[0])))
        prev = cur
    return out


def solve_both_ways(chained, orc, load, what):
    o = load(orc)
    o.rc = o.simplex()

    def check(rep, g):
        assert g.rc == o.rc
        assert_same_state(g, o, "%s run %d" % (what, rep))

    twice(chained, load, check)


# chain lengths around the group of four steps and its multiples (two groups make a round of the loop), the longest
# chain, and 0: the length by tableau size
@pytest.mark.parametrize("chain", [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17, 32, 0])
def test_group_and_tail_boundaries(chained, orc, chain):
    chained.set_chain(chain)
    for (m, n, seed) in ((64, 128, 1), (100, 37, 5), (300, 700, 11)):
        solve_both_ways(chained, orc, dense(m, n, seed), "dense %dx%d chain %d" % (m, n, chain))


@pytest.mark.parametrize("nt", [0, 1, 2])
@pytest.mark.parametrize("tr", [4, 8, 16])
def test_tile_and_pair_edges(chained, orc, tr, nt):
    """m below, at and one above the tile depth (the last tile reaches into the zeroed spare rows); n with the last
    pair half filled, and with a second column block of one pair; a 5 x 7 LP."""
    chained.set_tuning(tr, 1, nt)
    chained.set_chain(5)
    shapes = [(5, 7)] + [(m, n) for m in (tr - 1, tr, tr + 1) for n in (510, 511, 512, 1023, 1026)]
    for k, (m, n) in enumerate(shapes):
        solve_both_ways(chained, orc, dense(m, n, 100 + k), "dense %dx%d tr %d nt %d" % (m, n, tr, nt))


OWNERSHIP = [("degenerate", 40, 11, 55, 0.5), ("degenerate", 20, 11, 108, 0.5), ("dense", 40, 12, 216, None)]


@pytest.mark.parametrize("case", OWNERSHIP, ids=lambda c: "%s-%dx%d-%d" % c[:4])
def test_pivot_columns_that_share_a_pair_and_rows_that_leave_twice(chained, orc, case):
    """Few columns, chains of 16: within the solve's first chain column 1 is a pivot column (it shares its pair with
    column 0, which no tile stores), two columns of one pair are pivot columns, a row leaves twice and a column
    enters again -- found in the oracle's own pivot sequence, so the case cannot lose its point silently."""
    kind, m, n, seed, frac0 = case
    load = dense(m, n, seed) if kind == "dense" else degenerate(m, n, seed, frac0)
    span = oracle_steps(orc, load, 16)[:16]
    assert len(span) == 16
    rows = [p for k, p, q in span if k == "pivot"]
    cols = [q for k, p, q in span if k == "pivot"]
    assert 1 in cols, "column 1 is no pivot column of the first chain"
    assert any(q >= 2 and (q ^ 1) in cols for q in cols), "no two pivot columns of one pair in the first chain"
    assert len(set(rows)) < len(rows), "no row leaves twice in the first chain"
    assert len(set(cols)) < len(cols), "no column enters twice in the first chain"
    for tr in (4, 16):
        chained.set_tuning(tr, 1, -1)
        chained.set_chain(16)
        solve_both_ways(chained, orc, load, "%s %dx%d seed %d tr %d" % (kind, m, n, seed, tr))


# (m, n, seed, box divisor, chain length, where the first chain has a bound flip)
FLIPS = [(96, 400, 3, 2, 5, "first"), (96, 400, 3, 2, 4, "all"), (40, 90, 3, 2, 3, "last"), (60, 200, 8, 2, 4, "first"),
         (30, 60, 1, 2, 8, "first-and-last"), (40, 90, 3, 2, 1, "only"), (200, 300, 8, 2, 13, "middle")]


@pytest.mark.parametrize("case", FLIPS, ids=lambda c: "%dx%d-%d-chain%d-%s" % (c[0], c[1], c[2], c[4], c[5]))
def test_bound_flips_at_either_end_of_a_chain(chained, orc, case):
    """Boxed columns: the first chain of the solve has a bound flip as its first step, as its last, as every step, as
    its only step (chains of one) -- read off the oracle's sequence."""
    m, n, seed, ubd, chain, where = case
    load = boxed(m, n, seed, ubd)
    kinds = [k for k, p, q in oracle_steps(orc, load, 16)]
    span = kinds[:chain]
    assert len(span) == chain
    if where in ("first", "first-and-last"):
        assert span[0] == "flip" and "pivot" in span
    if where in ("last", "first-and-last"):
        assert span[-1] == "flip" and "pivot" in span
    if where == "all":
        assert set(span) == {"flip"}
    if where == "only":
        assert "flip" in kinds
    if where == "middle":
        assert "flip" in span[1:-1]
    chained.set_chain(chain)
    solve_both_ways(chained, orc, load, "boxed %dx%d seed %d chain %d" % (m, n, seed, chain))


@pytest.mark.parametrize("chain", [1, 6, 32])
def test_passes_that_follow_each_other_on_one_handle(chained, orc, chain):
    """40 row tiles of 8 rows, two column blocks: a handle stepped by calls of a few pivots each, compared after every
    call, so that each bulk launch starts from what the one before it left in memory and in the caches."""
    chained.set_tuning(8, 1, -1)
    chained.set_chain(chain)
    load = dense(320, 700, 9)
    for rep in range(2):
        g, o = load(chained), load(orc)
        for call in range(5):
            lim = 3 * max(chain, 2)
            assert g.simplex(it_lim=lim) == o.simplex(it_lim=lim)
            assert_same_state(g, o, "call %d chain %d run %d" % (call, chain, rep))
        del g
