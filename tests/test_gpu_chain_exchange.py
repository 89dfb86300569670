"""GPU: the all-to-all exchange of k_chain (xchg in kernels.hip) at the smallest shapes where its records can go wrong.
A record holds only what the receiver cannot rebuild: the pricing exchange sends no second key (it is 0.0 by
construction), the ratio-test exchange sends |a| as its second key and the sign of the pivot element a as one bit of
the aux word, next to the candidate's own aux (low 16 bits) and the cluster-wide flag (bit 16).  Every case runs the
chained primal path with the resident-tableau kernel off, is solved twice (the second time on the slab the first run
gave back) and must leave the oracle's bits; every case must also have launched k_chain, and no launch may have given up
waiting for a peer (that would silently move the rest of the process to k_pc / k_pr)."""
import numpy as np
import pytest

from mvolps_amd import capi, synth

from . import lpgen
from .test_gpu_chain import cluster_counts
from .test_gpu_parity import assert_same_state

pytestmark = pytest.mark.gpu


@pytest.fixture
def cluster(gpu):
    gpu.set_persist(0)
    gpu.set_cluster(1)
    yield gpu
    gpu.set_chain(0)
    gpu.set_cluster(1)
    gpu.set_persist(1)


def solve_twice(api, orc, load, what, it_lim=None):
    """Oracle once, engine twice (fresh handle, then the recycled slab); k_chain launched, none aborted."""
    o = load(orc)
    o.rc = o.simplex(it_lim=it_lim)
    before = cluster_counts(api)
    for rep in range(2):
        g = load(api)
        assert g.simplex(it_lim=it_lim) == o.rc, (what, rep)
        assert_same_state(g, o, "%s run %d" % (what, rep))
        del g  # the last reference: the slab goes back to the cache
    after = cluster_counts(api)
    assert after[0] > before[0], (what, "no k_chain launch was made")
    assert after[1] == before[1], (what, "a k_chain launch gave up waiting for its peers")
    return o


def dense_loader(A, b, c):
    def load(api):
        P = api.create()
        P.load_dense(A, b, c)
        return P

    return load


def general_loader(A, row_b, col_b, c):
    def load(api):
        P = api.create()
        P.load_general(A, row_b, col_b, c, direction=capi.MAX)
        return P

    return load


@pytest.mark.parametrize("chain", [2, 16])
def test_one_workgroup_exchanges_with_itself(cluster, orc, chain):
    """40x60: nw = 1, the only record a sweep finds is the workgroup's own; 14 pivots, so a chain of 16 also ends on
    `none` inside the launch."""
    cluster.set_chain(chain)
    solve_twice(cluster, orc, dense_loader(*synth.dense_lp(40, 60, 2)), "40x60 chain %d" % chain)


@pytest.mark.parametrize("m,n,seed", [(64, 257, 3), (257, 64, 4), (256, 513, 5)])
def test_one_column_or_row_alone_in_the_last_workgroup(cluster, orc, m, n, seed):
    """Column (row) 257 / 513 is thread 0 of the last workgroup: that workgroup's record comes from one valid lane at
    most, three of its waves hold nothing valid and still need the winner, its payload and the flag."""
    cluster.set_chain(5)
    solve_twice(cluster, orc, dense_loader(*synth.dense_lp(m, n, seed)), "%dx%d chain 5" % (m, n))


def negated_columns_lp(m, n, seed):
    """dense_lp with every second column x_j replaced by -x_j <= 0: those columns enter from their upper bound moving
    down (sdir = -1), and the pivot element of their ratio tests is negative."""
    A, b, c = synth.dense_lp(m, n, seed)
    neg = np.arange(n) % 2 == 1
    A, c = A.copy(), c.copy()
    A[:, neg] *= -1.0
    c[neg] *= -1.0
    col_b = [(capi.UP, 0.0, 0.0) if neg[j] else (capi.LO, 0.0, 0.0) for j in range(n)]
    row_b = [(capi.UP, 0.0, float(v)) for v in b]
    return A, row_b, col_b, c


def oracle_pivot_log(orc, load):
    """(row, column, pivot element) of every pivot of the oracle's full solve: the state after j pivots is the same
    solve cut off at j (the limit only truncates), the element is read from the tableau before the pivot."""
    full = load(orc)
    assert full.simplex() == 0
    log = []
    prev = load(orc)
    prev.simplex(it_lim=0)
    for j in range(1, full.it_cnt + 1):
        cur = load(orc)
        cur.simplex(it_lim=j)
        (h0, nb0, _), (h1, nb1, _) = prev.basis(), cur.basis()
        ps, qs = np.nonzero(h0 != h1)[0], np.nonzero(nb0 != nb1)[0]
        assert len(ps) == 1 and len(qs) == 1, (j, ps, qs)
        log.append((int(ps[0]), int(qs[0]), float(prev.tableau()[ps[0], qs[0]])))
        prev = cur
    assert np.array_equal(prev.tableau(), full.tableau())
    return log


_SIGN_LOGS = {}


@pytest.mark.parametrize("chain", [5, 16])
@pytest.mark.parametrize("m,n,seed", [(300, 120, 1), (520, 100, 3)])
def test_pivot_elements_of_either_sign_win_across_workgroups(cluster, orc, m, n, seed, chain):
    """The ratio-test record carries |a| and one sign bit: both signs of the pivot element must come through, from the
    first workgroup's rows and from the others' (two and three workgroups here).  That the instances do contain them
    is read from the oracle alone."""
    load = general_loader(*negated_columns_lp(m, n, seed))
    if (m, n, seed) not in _SIGN_LOGS:
        _SIGN_LOGS[(m, n, seed)] = oracle_pivot_log(orc, load)
    log = _SIGN_LOGS[(m, n, seed)]
    for far in (False, True):  # leaving row in workgroup 0 / in a later workgroup
        signs = [a < 0 for (p, q, a) in log if (p > 256) == far]
        assert any(signs) and not all(signs), ("the instance does not cover both signs", far, len(signs))
    cluster.set_chain(chain)
    o = solve_twice(cluster, orc, load, "negated columns %dx%d chain %d" % (m, n, chain))
    assert o.it_cnt == len(log)


@pytest.mark.parametrize("chain", [2, 3, 16])
def test_ratio_test_ties_across_workgroups(cluster, orc, chain):
    """Degenerate 300x600 with rows 1..40 repeated as rows 261..300: a zero ratio ties the first key in most ratio tests,
    a repeated row ties the second key |a| as well, and the two copies sit in different workgroups: the index decides,
    in the record exactly as inside a workgroup."""
    A, b, c = lpgen.degenerate_lp(300, 600, 41000, frac0=0.9)
    A[260:300] = A[0:40]
    b[260:300] = b[0:40]
    o = lpgen.load_degenerate(orc, A, b, c)
    o.rc = o.simplex()
    cluster.set_chain(chain)
    before = cluster_counts(cluster)
    for rep in range(2):
        g = lpgen.load_degenerate(cluster, A, b, c)
        assert g.simplex() == o.rc
        assert g.pert_cnt == o.pert_cnt and g.bland_cnt == o.bland_cnt
        assert_same_state(g, o, "tied rows chain %d run %d" % (chain, rep))
        del g
    after = cluster_counts(cluster)
    assert after[0] > before[0] and after[1] == before[1]


@pytest.mark.parametrize("chain", [3, 16])
def test_bound_flips_share_the_aux_word_with_the_sign(cluster, orc, chain):
    """Boxed columns at 300x700 (two of three), half of all columns negated: bound flips come into the chains in both
    directions while the flag bit, the sign bit and the candidate's own aux travel in one word."""
    rng = np.random.default_rng(5)
    A, row_b, col_b, c = negated_columns_lp(300, 700, 17)
    for j in range(700):
        if j % 3:
            w = float(rng.integers(1, 4)) / 2
            col_b[j] = (capi.DB, -w, 0.0) if j % 2 else (capi.DB, 0.0, w)
    solve_twice(cluster, orc, general_loader(A, row_b, col_b, c), "boxed 300x700 chain %d" % chain)


@pytest.mark.parametrize("m,n,seed,lim", [(48, 8300, 3, 40), (8300, 48, 5, 40)])
def test_two_to_a_thread_at_its_smallest(cluster, orc, m, n, seed, lim):
    """More than 8192 columns (rows): k_chain<2, 2>, whose candidates are the better of a thread's two before they meet
    the exchange."""
    cluster.set_chain(0)
    solve_twice(cluster, orc, dense_loader(*synth.dense_lp(m, n, seed)), "%dx%d, %d pivots" % (m, n, lim), it_lim=lim)


def test_pivot_limits_inside_a_chain_and_on_its_end(cluster, orc):
    """64x128, chains of 4, one handle, limits 1, 2, 3, 4, 4, 5, 8, ...: a limit inside a chain, one that ends with the
    chain (the next launch finds an entering column and no pivot left), and the optimum inside a chain."""
    cluster.set_chain(4)
    A, b, c = synth.dense_lp(64, 128, 9)
    g, o = cluster.create(), orc.create()
    for P in (g, o):
        P.load_dense(A, b, c)
    before = cluster_counts(cluster)
    for call, lim in enumerate((1, 2, 3, 4, 4, 5, 8, 8, 100)):
        rcs = [P.simplex(it_lim=lim) for P in (g, o)]
        assert rcs[0] == rcs[1], (call, lim, rcs)
        assert_same_state(g, o, "call %d limit %d" % (call, lim))
        if rcs[0] == 0:
            break
    assert g.status == capi.OPT
    after = cluster_counts(cluster)
    assert after[0] > before[0] and after[1] == before[1]
