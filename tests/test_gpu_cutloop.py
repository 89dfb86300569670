"""GPU: the root cut rounds on the device (DESIGN.md "Root cut rounds").  k_cutrows through mvx_add_cut_rows against the per-row
path (add_rows, set_mat_row, set_row_bnds) on a clone and on the oracle; k_cutgram through mvx_cut_scores against the host twin
mvx_bnb_cut_scores; the whole loop and whole trees on the HIP table against the same driver over the oracle's table.  Every
comparison is bitwise."""
import json
import os

import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import LO, NU, OPT, UNDEF

from . import lpgen
from .test_bnb_cutloop import COUNTERS, rows_behind
from .test_bnb_general import INSTANCES, check_pin, failures, instance, run
from .test_bnb_host import same_result
from .test_gpu_parity import assert_same_state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 8  # CUT_TILE of k_cutrows


def cut_like_rows(rng, x, k, zeros=0.3):
    """k dense rows v . x >= rhs with zeros and both signs that cut off the vertex x and keep the origin: (vals (k, n + 1), rhs)."""
    n = len(x)
    vals = np.zeros((k, n + 1))
    rhs = np.zeros(k)
    for t in range(k):
        v = np.round(rng.uniform(-2.0, 2.0, n), 3) * (rng.random(n) >= zeros)
        if t % 3 == 2:
            v = -np.abs(v)  # no cancellation: sums that can end at -0.0
        s = float(v @ x)
        if s > 0:
            v, s = -v, -s
        if s == 0:
            v[int(np.argmax(x))] -= 1.0
            s = float(v @ x)
        vals[t, 1:] = v
        vals[t, 0] = 77.0  # entry 0 is not read
        rhs[t] = s / 2
    return vals, rhs


def append_per_row(P, vals, rhs):
    api, n = P.api, P.n
    ind = np.arange(n + 1, dtype=np.int32)
    for t in range(len(rhs)):
        i = api.add_rows(P.h, 1)
        P.set_mat_row(i, ind, np.ascontiguousarray(vals[t]))
        api.set_row_bnds(P.h, i, LO, float(rhs[t]), 0.0)


def model_rows(P, m0):
    api = P.api
    return [(c.tolist(), lb, api.get_row_ub(P.h, m0 + 1 + i), api.get_row_type(P.h, m0 + 1 + i)) for i, (c, lb) in enumerate(rows_behind(api, P, m0))]


def assert_same_unsolved(X, Y, m0, what):
    """Two handles after the same appends, before their next solve: model, status, basis, tableau and column values."""
    assert X.m == Y.m and model_rows(X, m0) == model_rows(Y, m0), what
    assert X.status == Y.status == UNDEF, what
    for a, b, nm in zip(X.basis(), Y.basis(), ("head", "nonbasic", "flag")):
        assert np.array_equal(a, b), (what, nm)
    tx, ty = X.tableau(), Y.tableau()
    assert np.array_equal(tx.view(np.uint64), ty.view(np.uint64)), (what, "tableau", int((tx.view(np.uint64) != ty.view(np.uint64)).sum()))
    assert np.array_equal(X.col_prim(), Y.col_prim()) and np.array_equal(X.col_stat(), Y.col_stat()), what


def batched_vs_per_row(gpu, orc, G, O, rng, ks, what):
    """On clones of the solved pair (G on the device, O on the oracle): one mvx_add_cut_rows call against k single appends on
    the device and on the oracle, before and after the next solve."""
    x = G.col_prim()
    for k in ks:
        vals, rhs = cut_like_rows(rng, x, k)
        gb, gr, oo = G.copy(), G.copy(), O.copy()
        m0 = gb.m
        assert bnb.add_cut_rows(gb, vals, rhs) == 0
        append_per_row(gr, vals, rhs)
        append_per_row(oo, vals, rhs)
        w = "%s k=%d" % (what, k)
        assert_same_unsolved(gb, gr, m0, w)
        assert_same_unsolved(gb, oo, m0, w + " (oracle)")
        for H in (gb, gr, oo):
            H.simplex()
        assert_same_state(gb, gr, w)
        assert_same_state(gb, oo, w + " (oracle)")
        assert gb.it_cnt > G.it_cnt, w  # the rows cut the vertex off: the dual simplex had work to do


@pytest.mark.parametrize("n1", [255, 256, 257])
@pytest.mark.parametrize("m", [63, 64, 65, 128, 129])
def test_add_cut_rows_equals_the_per_row_path(gpu, orc, m, n1):
    """m = 63 and 64 bring a trailing chunk of zero weights into the first and second single append, 128 into the second;
    k runs over the kernel's cut tile and its neighbours; twice, the second time on recycled slabs."""
    A, b, c = synth.dense_lp(m, n1 - 1, 11 + m + n1)
    rng = np.random.default_rng(m * 1000 + n1)
    for again in range(2):
        G, O = gpu.create(), orc.create()
        for P in (G, O):
            P.load_dense(A, b, c)
            assert P.simplex() == 0 and P.status == OPT
        batched_vs_per_row(gpu, orc, G, O, rng, (1, 2, TILE - 1, TILE, TILE + 1), "%dx%d pass %d" % (m, n1 - 1, again))
        del G, O


def test_add_cut_rows_on_a_handle_that_carries_cut_rows(gpu, orc):
    """Appends behind appends, without a solve in between: the pending bound edits of the first call overflow in the second
    (MAX_EDITS = 8), rows of both calls among them; then a solve, and appends behind solved cut rows."""
    A, b, c = synth.dense_lp(70, 140, 5)
    rng = np.random.default_rng(99)
    G, O = gpu.create(), orc.create()
    for P in (G, O):
        P.load_dense(A, b, c)
        P.simplex()
    x = G.col_prim()
    gb, gr, oo = G.copy(), G.copy(), O.copy()
    m0 = gb.m
    for k in (5, 9, 3, 20):
        vals, rhs = cut_like_rows(rng, x, k)
        assert bnb.add_cut_rows(gb, vals, rhs) == 0
        append_per_row(gr, vals, rhs)
        append_per_row(oo, vals, rhs)
        assert_same_unsolved(gb, gr, m0, "stacked k=%d" % k)
        assert_same_unsolved(gb, oo, m0, "stacked k=%d (oracle)" % k)
    for H in (gb, gr, oo):
        H.simplex()
    assert_same_state(gb, gr, "stacked")
    assert_same_state(gb, oo, "stacked (oracle)")
    assert gb.status == OPT
    batched_vs_per_row(gpu, orc, gb, oo, rng, (1, TILE + 1), "behind solved cut rows")


def test_add_cut_rows_with_columns_at_their_upper_bound(gpu, orc):
    """A dense_ilp root: columns non-basic at their upper bound give the new rows a value at the non-basic point (the fma
    chain of base[0]); the rows are the root's own repaired GMI cuts."""
    A, b, c, U = synth.dense_ilp(65, 130, 7, 3)
    G, O = lpgen.load_ilp(gpu, A, b, c, U), lpgen.load_ilp(orc, A, b, c, U)
    for P in (G, O):
        P.simplex()
    assert any(s == NU for s in G.col_stat())
    cuts = [bnb.generate_cut_gmi(G, j) for j in range(1, G.n + 1)]
    cuts = [g for g in cuts if g is not None]
    assert len(cuts) >= TILE + 1
    vals, rhs = np.array([g[0] for g in cuts]), np.array([g[1] for g in cuts])
    for k in (1, TILE + 1, len(cuts)):
        gb, gr, oo = G.copy(), G.copy(), O.copy()
        assert bnb.add_cut_rows(gb, vals[:k], rhs[:k]) == 0
        append_per_row(gr, vals[:k], rhs[:k])
        append_per_row(oo, vals[:k], rhs[:k])
        assert_same_unsolved(gb, gr, G.m, "ilp k=%d" % k)
        assert_same_unsolved(gb, oo, G.m, "ilp k=%d (oracle)" % k)
        for H in (gb, gr, oo):
            H.simplex()
        assert_same_state(gb, gr, "ilp k=%d" % k)
        assert_same_state(gb, oo, "ilp k=%d (oracle)" % k)


def test_add_cut_rows_tall(gpu, orc):
    A, b, c = synth.dense_lp(1200, 300, 3)
    G, O = gpu.create(), orc.create()
    for P in (G, O):
        P.load_dense(A, b, c)
        P.simplex()
    batched_vs_per_row(gpu, orc, G, O, np.random.default_rng(1200), (TILE + 3,), "1200x300")


def test_add_cut_rows_bad_lists_change_nothing(gpu):
    A, b, c = synth.dense_lp(20, 40, 2)
    G = gpu.create()
    G.load_dense(A, b, c)
    vals, rhs = cut_like_rows(np.random.default_rng(1), np.ones(40), 3)
    assert bnb.add_cut_rows(G, vals, rhs) == -1 and G.m == 20  # no tableau yet
    G.simplex()
    before = (G.tableau().tolist(), [a.tolist() for a in G.basis()], G.status, G.m)
    nan_v, nan_r = vals.copy(), rhs.copy()
    nan_v[2, 17] = np.nan
    nan_r[1] = np.nan
    for v, r in ((np.zeros((0, 41)), np.zeros(0)), (nan_v, rhs), (vals, nan_r), (vals[:, :40], rhs), (vals, rhs[:2])):
        assert bnb.add_cut_rows(G, v, r) == -1
        assert (G.tableau().tolist(), [a.tolist() for a in G.basis()], G.status, G.m) == before
    assert bnb.lib().mvx_add_cut_rows(G.h, 3, None, None) == -1 and bnb.lib().mvx_add_cut_rows(None, 3, None, None) == -1
    assert bnb.add_cut_rows(G, vals, rhs) == 0 and G.m == 23


# ------------------------------------------------------------------------------------------------ scores


def scores_match(P, vals):
    rc, dot, gram = bnb.cut_scores(P, vals)
    trc, tdot, tgram = bnb.cut_scores(P, vals, table=None)  # the twin through the engine's own table
    assert rc == 0 and trc == 0
    assert np.array_equal(dot.view(np.uint64), tdot.view(np.uint64))
    assert np.array_equal(gram.view(np.uint64), tgram.view(np.uint64))
    assert np.array_equal(gram, gram.T)
    nrm = [bnb.cut_scores(P, vals[t:t + 1], table=None)[2][0, 0] for t in range(len(vals))]
    assert np.array_equal(np.diag(gram), np.array(nrm))


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_cut_scores_integer_rows(gpu, n):
    A, b, c = synth.dense_lp(8, n, n)
    P = gpu.create()
    P.load_dense(A, b, c)
    P.simplex()
    rng = np.random.default_rng(n)
    for k in (1, 15, 16, 17, 33):
        vals = rng.integers(-3, 4, size=(k, n + 1)).astype(np.float64) * (rng.random((k, n + 1)) < 0.7)
        vals[vals == 0] = 0.0
        scores_match(P, vals)
    before = (P.tableau().tolist(), P.status, P.obj)
    assert bnb.cut_scores(P, vals)[0] == 0 and (P.tableau().tolist(), P.status, P.obj) == before  # pure
    Q = gpu.create()
    Q.load_dense(A, b, c)
    assert bnb.cut_scores(Q, vals)[0] == -1  # not solved
    assert bnb.cut_scores(P, np.zeros((0, n + 1)))[0] == -1


def test_cut_scores_real_gmi_cuts(gpu):
    """The repaired GMI cuts of a solved 65x130 dense_ilp root; one round yields fewer than 33, so the root's cuts are appended,
    the LP is solved again and the next round's cuts join them.  All are scored on the last solved handle."""
    A, b, c, U = synth.dense_ilp(65, 130, 7, 3)
    P = lpgen.load_ilp(gpu, A, b, c, U)
    P.simplex()
    vals = np.zeros((0, P.n + 1))
    while True:
        cuts = [g for g in (bnb.generate_cut_gmi(P, j) for j in range(1, P.n + 1)) if g is not None]
        assert len(cuts) >= 8
        vals = np.concatenate([vals, np.array([g[0] for g in cuts])])
        if len(vals) >= 33:
            break
        assert bnb.add_cut_rows(P, np.array([g[0] for g in cuts]), np.array([g[1] for g in cuts])) == 0
        P.simplex()
        assert P.status == OPT
    for k in (1, 15, 16, 17, 33, len(vals)):
        scores_match(P, vals[:k])
    # generateCutGMI's efficacy is (rhs - dot) / sqrt(nrm) of these numbers, for the cuts of the handle they are scored on
    last = np.array([g[0] for g in cuts])
    rc, dot, gram = bnb.cut_scores(P, last)
    eff, rhs = np.array([g[2] for g in cuts]), np.array([g[1] for g in cuts])
    assert rc == 0 and np.array_equal(eff, (rhs - dot) / np.sqrt(np.diag(gram)))


# ------------------------------------------------------------------------------------------------ the loop, trees


def loop_pair(gpu, orc, tab, load, **kw):
    G, O = load(gpu), load(orc)
    if bnb.integral_bounds(G) == 2:
        assert bnb.integral_bounds(O, table=tab) == 2
        return 0
    bnb.integral_bounds(O, table=tab)
    m0 = G.m
    grc, gout = bnb.cut_loop(G, rounds=5, **kw)
    orc_, oout = bnb.cut_loop(O, rounds=5, table=tab, **kw)
    assert grc == orc_ == 0 and gout == oout, (gout, oout)
    assert G.m == O.m and model_rows(G, m0) == model_rows(O, m0)
    assert_same_state(G, O, "after the loop")
    return gout["cutloop_rows"]


@pytest.mark.parametrize("case", [(24, 48, 5, 3), (65, 130, 7, 3)], ids=lambda c: "%dx%d" % (c[0], c[1]))
def test_cut_loop_equals_the_oracle_table_loop(gpu, orc, case):
    tab = bnb.table_from(orc)
    A, b, c, U = synth.dense_ilp(*case)
    load = lambda api: lpgen.load_ilp(api, A, b, c, U)  # noqa: E731
    # every cut of a dense_ilp round is more than 0.9 parallel to the most effective one: a round at the defaults takes one
    assert loop_pair(gpu, orc, tab, load) >= 1
    # without the filter a round takes up to K cuts: the batched append with more rows than its tile, 64 rows in all
    assert loop_pair(gpu, orc, tab, load, K=32, maxpar=1.0) >= TILE + 1
    assert loop_pair(gpu, orc, tab, load, K=3, maxpar=1.0) >= 3


def test_cut_loop_equals_the_oracle_table_loop_on_fixtures(gpu, orc):
    tab = bnb.table_from(orc)
    rows = []

    def one(rec):
        inst = instance(rec)
        rows.append(loop_pair(gpu, orc, tab, lambda api: lpgen.load_milp(api, inst)))

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)
    assert sum(1 for k in rows if k > 0) >= 5 and sum(rows) >= 10, rows  # the comparison is not an empty one


@pytest.mark.parametrize("window", [1, 64])
def test_fixture_trees_match_oracle_table_and_pins(gpu, orc, window):
    tab = bnb.table_from(orc)

    def one(rec):
        inst = instance(rec)
        got = run(gpu, rec, inst, cut_rounds=5, window=window)
        check_pin(rec, inst, got)
        ref = run(orc, rec, inst, table=tab, cut_rounds=5, window=window)
        same_result(got, ref)
        for k in COUNTERS:
            assert got[k] == ref[k], k

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)


def test_config5_reaches_20_behind_the_loop(gpu):
    from .test_gpu_chain import cluster_counts
    from .test_gpu_rcfix import config5

    A, b, c, U = config5()
    aborts0 = cluster_counts(gpu)[1]
    r = bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), quirks=0, cut_rounds=5, heur=2, window=64, max_nodes=2 * 15697)
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "milp_pins.json")))
    assert pins["config5"]["milp_obj"] == 20.0
    assert r["rc"] == 0 and r["hit_limit"] == 0 and r["has_incumbent"] and abs(r["best_lower"] - 20.0) <= 1e-6 * 21, (r["hit_limit"], r["count"], r["best_lower"])
    assert r["cutloop_rounds"] >= 1 and r["cutloop_rows"] >= 1 and r["cutloop_bound"] <= r["cutloop_bound0"] + 1e-7 * max(1.0, abs(r["cutloop_bound0"]))
    assert cluster_counts(gpu)[1] == aborts0


def test_cli_cut_rounds_on_f1(gpu):
    import subprocess

    exe = os.path.join(ROOT, "mvolps_amd", "bin", "mvolps")
    f1 = os.path.join(ROOT, "tests", "golden", "f1.lp")
    plain = subprocess.run([exe, "-f", f1, "--repaired", "-v"], capture_output=True, text=True)
    r = subprocess.run([exe, "-f", f1, "--repaired", "-v", "--cut-rounds", "--cut-round-max", "8", "--cut-maxpar", "0.8"], capture_output=True, text=True)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    assert "Root cut rounds:" in r.stdout and "Root cut rounds:" not in plain.stdout
    assert plain.stdout.splitlines()[-2] == r.stdout.splitlines()[-3]  # the solution line in front of the verbose ones
