"""CPU: clique cuts in the tree (DESIGN.md "Clique cuts in the tree (node_cliques)") over the ORACLE's table.  That table has
neither clique_cuts_many nor add_cut_rows_many nor add_cut_rows, so the host twin mvx_bnb_clique_masks separates every node and
the rows go in one by one: the driver's side of the definition runs -- the graph of the model at tree start, the separation on
the LP as solved, the booking by the replay, the rows on both children behind the purge, the ages, the counters.

The twin equals mvx_bnb_clique_cuts set for set and s for s; every fixture instance closes on its enumerated pin with
node_cliques = 4, alone, with the tree's purge and with a GMI cut per node; all-integer models close on the optimum of their
enumeration; windows give the serial tree and counters; node_cliques = 0 is the result without the keyword; the dense binary
cases shrink to the pinned node counts; refusals return their codes."""
import os
import subprocess

import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import CV, FR, FX, MAX, OPT

from . import lpgen
from .test_bnb_clique import BINARY, feasible_points, integer_model, random_graph
from .test_bnb_general import INSTANCES, check_pin, failures, instance, run
from .test_bnb_host import same_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (m, n, seed, U, cap) of synth.dense_ilp -> (optimum of DESIGN.md, nodes with node_cliques = 0, with node_cliques = 4): the
# counts of this test's own runs over the oracle's table, without root rounds (the trees are deterministic)
DENSE = {
    (24, 48, 5, 1, 0.06): (38, 401, 21),
    (32, 64, 7, 1, 0.05): (36, 665, 181),
    (32, 64, 7, 1, 0.045): (32, 545, 19),
    (64, 128, 7, 1, 0.025): (40, 2173, 47),
}


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    # the twin and the per-row append run
    assert not bnb.table_entry(t, "clique_cuts_many") and not bnb.table_entry(t, "add_cut_rows_many") and not t.add_cut_rows
    return t


def check_counters(r):
    assert r["node_clique_conflicts"] >= 0 and 0 <= r["node_clique_calls"] and r["node_clique_rows"] >= 0
    assert r["node_clique_rows"] <= 64 * r["node_clique_calls"]
    if r["node_clique_conflicts"] == 0:
        assert r["node_clique_calls"] == 0 and r["node_clique_rows"] == 0


def same(a, b):
    same_result(a, b)
    for k in bnb.NODE_CLIQUE_COUNTERS + bnb.NODE_PURGE_COUNTERS:
        assert a[k] == b[k], k


# ------------------------------------------------------------------------------------------------ the twin


def fixed_point(api, x):
    """A solved handle whose column values are x[1..n]: one free row, every column fixed (no pivot, MVX_OPT)."""
    n = len(x) - 1
    P = api.create()
    P.load_general(np.zeros((1, n)), [(FR, 0.0, 0.0)], [(FX, float(v), float(v)) for v in x[1:]], np.zeros(n), kinds=[CV] * n, direction=MAX)
    assert P.simplex() == 0 and P.status == OPT
    return P


def masks_vs_cuts(words, n, P, x, max_cuts, tab):
    """mvx_bnb_clique_masks on the handle against mvx_bnb_clique_cuts on the numbers: the sets, their order and every s."""
    rc, cnt, q, s = bnb.clique_cuts_many(P, [P], max_cuts, table=tab, adj=words)
    crc, vals, rhs = bnb.clique_cuts(bnb.words_to_bool(words, n), x, max_cuts)
    assert rc == crc == 0 and cnt[0] == len(vals) <= max_cuts, (rc, crc, cnt, len(vals))
    sets = bnb.words_to_bool(q[0], n)
    for t in range(cnt[0]):
        assert np.array_equal(sets[t], vals[t] == -1.0), t
        want = 0.0
        for j in np.flatnonzero(sets[t]):
            want = want + float(x[j])
        assert s[0, t] == want and want - 1.0 > 1e-6, (t, s[0, t], want)
    assert not q[0, cnt[0]:].any() and not s[0, cnt[0]:].any()  # the slots behind the kept ones are zero
    return int(cnt[0])


def test_masks_equal_clique_cuts_on_random_graphs(orc, tab):
    rng = np.random.default_rng(77)
    kept = capped = 0
    for trial in range(120):
        n = int(rng.integers(2, 90)) if trial % 10 else int(rng.integers(120, 140))
        adj = random_graph(rng, n)
        x = np.round(rng.random(n + 1) * 4) / 4 * (rng.random(n + 1) < 0.7)
        if trial % 3 == 0:
            x = x * rng.random(n + 1)
        x[0] = 0.0
        words = bnb.bool_to_words(adj)
        P = fixed_point(orc, x)
        got = np.array([orc.get_col_prim(P.h, j) for j in range(1, n + 1)])
        assert np.array_equal(got, x[1:])
        for max_cuts in (64, 2, 1):
            k = masks_vs_cuts(words, n, P, x, max_cuts, tab)
            kept += k
            capped += k == max_cuts
    assert kept > 150 and capped >= 20, (kept, capped)


@pytest.mark.parametrize("case", list(BINARY), ids=lambda c: "%dx%d_cap%g" % (c[0], c[1], c[4]))
def test_masks_equal_clique_cuts_on_solved_roots(orc, tab, case):
    A, b, c, U = synth.dense_ilp(*case)
    P = lpgen.load_ilp(orc, A, b, c, U)
    rc, words, edges = bnb.conflict_words(P, table=tab)
    assert rc == 0 and edges > 0
    assert P.simplex() == 0 and P.status == OPT
    x = np.concatenate([[0.0], [orc.get_col_prim(P.h, j) for j in range(1, P.n + 1)]])
    assert sum(masks_vs_cuts(words, P.n, P, x, k, tab) for k in (64, 4, 1)) >= 3


def test_masks_argument_errors(orc, tab):
    L = bnb.lib()
    C = bnb.C
    x = np.array([0.0, 0.75, 0.75, 0.0])
    adj = np.zeros((4, 4), dtype=bool)
    adj[1:, 1:] = True  # a triangle: the zero-valued column 3 joins the violated pair
    np.fill_diagonal(adj, False)
    words = bnb.bool_to_words(adj)
    P = fixed_point(orc, x)
    UP_, DP_ = C.POINTER(C.c_ulonglong), C.POINTER(C.c_double)
    cnt, q, s = C.c_int(7), np.zeros((2, 1), dtype=np.uint64), np.zeros(2)
    tptr = C.cast(C.pointer(tab), C.c_void_p)
    call = lambda prob, n, w, k, pc, pq, ps: L.mvx_bnb_clique_masks(tptr, prob, n, w, k, pc, pq, ps)  # noqa: E731
    wp, qp, sp = words.ctypes.data_as(UP_), q.ctypes.data_as(UP_), s.ctypes.data_as(DP_)
    assert call(None, 3, wp, 2, C.byref(cnt), qp, sp) == -1 and call(P.h, 3, None, 2, C.byref(cnt), qp, sp) == -1
    assert call(P.h, 3, wp, 2, None, qp, sp) == -1 and call(P.h, 3, wp, 2, C.byref(cnt), None, sp) == -1
    assert call(P.h, 3, wp, 2, C.byref(cnt), qp, None) == -1
    for k in (0, -1, 65):
        assert call(P.h, 3, wp, k, C.byref(cnt), qp, sp) == -1
    assert call(P.h, 4, wp, 2, C.byref(cnt), qp, sp) == -1  # another column count
    assert cnt.value == 7 and not q.any()
    fresh = P.copy()
    orc.set_col_bnds(fresh.h, 1, FX, 0.5, 0.5)  # not solved any more
    assert fresh.status != OPT and call(fresh.h, 3, wp, 2, C.byref(cnt), qp, sp) == -3
    assert call(P.h, 3, wp, 2, C.byref(cnt), qp, sp) == 0 and cnt.value == 1 and q[0, 0] == 0b1110 and s[0] == 1.5


# ------------------------------------------------------------------------------------------------ whole trees

MODES = {"plain": dict(), "node_purge": dict(node_purge=2), "cut_strat": dict(cut_strat=1)}


@pytest.mark.parametrize("window", [1, 64])
@pytest.mark.parametrize("mode", list(MODES))
def test_fixture_trees_close_on_the_enumerated_optimum(orc, tab, mode, window):
    """The general fixture has no pair of conflicting binaries (its graphs are empty), so this is the rule switched on where
    it has nothing to do; the models with conflicts are the enumerated ones and the dense binary cases below."""

    def one(rec):
        inst = instance(rec)
        r = run(orc, rec, inst, table=tab, node_cliques=4, window=window, **MODES[mode])
        check_pin(rec, inst, r)
        check_counters(r)

    bad = failures(INSTANCES, one)
    assert not bad, "\n".join(bad)


def test_integer_models_close_on_the_enumerated_optimum(orc, tab):
    rng = np.random.default_rng(4242)
    with_rows = 0
    bad = []
    for index in range(120):
        inst = integer_model(rng)
        pts = feasible_points(inst)
        assert len(pts) >= 1
        vals = pts @ np.asarray(inst["c"], dtype=float) + inst["c0"]
        best = vals.max() if inst["direction"] == MAX else vals.min()
        for kw in (dict(window=1), dict(window=64, node_purge=1, cut_strat=1)):
            r = bnb.branch_and_bound(lpgen.load_milp(orc, inst), quirks=0, table=tab, node_cliques=4, max_nodes=200000, **kw)
            check_counters(r)
            with_rows += r["node_clique_rows"] > 0
            if not (r["rc"] == 0 and r["hit_limit"] == 0 and r["has_incumbent"] and abs(r["best_lower"] - best) <= 1e-6 * (1 + abs(best))):
                bad.append("model %d %r: rc %d, %r against the enumerated %r" % (index, kw, r["rc"], r["best_lower"], best))
    assert not bad, "\n".join(bad[:20])
    assert with_rows >= 20, with_rows


def test_windows_give_the_serial_tree(orc, tab):
    for case in list(DENSE)[:3]:
        A, b, c, U = synth.dense_ilp(*case)
        for extra in (dict(), dict(node_purge=2), dict(cut_strat=1, node_purge=1), dict(heur=2, rc_fix=1, prop=4)):
            ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), quirks=0, table=tab, node_cliques=4, window=1, **extra)
            assert ref["rc"] == 0 and ref["node_clique_rows"] >= 1
            for w in (8, 64):
                same(bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), quirks=0, table=tab, node_cliques=4, window=w, **extra), ref)

    def one(rec):
        inst = instance(rec)
        for extra in (dict(), dict(cut_strat=1, node_purge=1), dict(cut_rounds=5, cut_families=3)):
            ref = run(orc, rec, inst, table=tab, window=1, node_cliques=4, **extra)
            check_counters(ref)
            for w in (8, 64):
                same(run(orc, rec, inst, table=tab, window=w, node_cliques=4, **extra), ref)

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)


def test_node_cliques_0_is_the_result_without_the_keyword(orc, tab):
    def one(rec):
        inst = instance(rec)
        for kw in (dict(window=1), dict(window=64, cut_strat=1, node_purge=1), dict(node_strat=1, window=1, cut_strat=1),
                   dict(window=64, cut_rounds=5, cut_families=3)):
            ref = run(orc, rec, inst, table=tab, **kw)
            got = run(orc, rec, inst, table=tab, node_cliques=0, **kw)
            assert got == ref, kw
            assert all(got[k] == 0 for k in bnb.NODE_CLIQUE_COUNTERS)

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)
    for case in list(DENSE)[:2]:
        A, b, c, U = synth.dense_ilp(*case)
        for w in (1, 64):
            ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), quirks=0, table=tab, window=w)
            assert bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), quirks=0, table=tab, window=w, node_cliques=0) == ref


@pytest.mark.parametrize("case", list(DENSE), ids=lambda c: "%dx%d_cap%g" % (c[0], c[1], c[4]))
def test_dense_binary_trees_shrink(orc, tab, case):
    """Without root rounds: the optimum is DESIGN.md's, rows were appended, and the tree is strictly smaller than with K = 0; the
    node counts are the pinned ones."""
    optimum, nodes0, nodes4 = DENSE[case]
    A, b, c, U = synth.dense_ilp(*case)
    off = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), quirks=0, table=tab, node_cliques=0)
    on = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), quirks=0, table=tab, node_cliques=4)
    print(case, off["n_nodes"], on["n_nodes"], on["best_lower"], [on[k] for k in bnb.NODE_CLIQUE_COUNTERS])
    for r in (off, on):
        assert r["rc"] == 0 and r["hit_limit"] == 0 and r["has_incumbent"]
        assert abs(r["best_lower"] - optimum) <= 1e-6 * (1 + optimum), r["best_lower"]
    assert on["node_clique_rows"] >= 1 and on["node_clique_conflicts"] > 0 and on["node_clique_calls"] >= 1
    assert on["n_nodes"] < off["n_nodes"]
    assert (off["n_nodes"], on["n_nodes"]) == (nodes0, nodes4)
    assert on["node_cut_rows_peak"] >= 1 and off["node_cut_rows_peak"] == 0


def test_model_without_a_binary_column(orc, tab):
    A, b, c, U = synth.dense_ilp(10, 20, 4, 3)
    for kw in (dict(window=1), dict(window=64), dict(node_strat=1, window=1)):
        ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), quirks=0, table=tab, **kw)
        got = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), quirks=0, table=tab, node_cliques=16, **kw)
        assert ref["n_nodes"] >= 3 and got == ref
        assert all(got[k] == 0 for k in bnb.NODE_CLIQUE_COUNTERS)


def test_the_callers_handle_is_left_as_it_was(orc, tab):
    A, b, c, U = synth.dense_ilp(24, 48, 5, 1, 0.06)
    P = lpgen.load_ilp(orc, A, b, c, U)
    m0 = P.m
    before = [P.get_mat_row(i) for i in range(1, m0 + 1)]
    r = bnb.branch_and_bound(P, quirks=0, table=tab, node_cliques=4)
    assert r["rc"] == 0 and r["node_clique_rows"] >= 1
    assert P.m == m0 and orc.get_num_rows(P.h) == m0
    for i, (ind, val) in enumerate(before, start=1):
        got = P.get_mat_row(i)
        assert np.array_equal(got[0], ind) and np.array_equal(got[1], val)


# ------------------------------------------------------------------------------------------------ refusals, front end


def test_refusals(orc, tab):
    from mvolps_amd import capi, dist_bnb, dist_native

    A, b, c, U = synth.dense_ilp(8, 16, 3, 1, 0.1)
    for kw in (dict(quirks=0, node_cliques=-1), dict(quirks=0, node_cliques=65), dict(quirks=1, node_cliques=1), dict(node_cliques=4),
               dict(quirks=0, node_strat=1, best_window=8, node_cliques=4), dict(quirks=0, node_strat=1, best_window=1, node_cliques=1),
               dict(quirks=1, node_cliques=-1)):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, **kw)
        assert r["rc"] == -1 and r["n_nodes"] == 0 and r["count"] == 0, kw
    for kw in (dict(node_cliques=0), dict(node_cliques=1), dict(node_cliques=64, cut_strat=1), dict(node_cliques=4, node_strat=1),
               dict(node_cliques=4, cut_rounds=5, cut_families=3, cut_purge=1, node_purge=2),
               dict(node_cliques=4, cut_strat=1, heur=2, rc_fix=1, prop=4, dive=7, pump=30, polish=10)):
        assert bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0, **kw)["rc"] == 0, kw
    P = lpgen.load_ilp(orc, A, b, c, U)
    with pytest.raises(ValueError):
        dist_native.branch_and_bound(P, table=tab, node_cliques=4, quirks=0)
    with pytest.raises(ValueError):
        dist_bnb.branch_and_bound(None, P, node_cliques=4, quirks=0)
    pr = bnb.make_params(quirks=0, node_cliques=4)
    L = dist_native._lib()
    res, st = bnb.BnbResult(), dist_native.DistStats()
    tptr = bnb.C.cast(bnb.C.pointer(tab), bnb.C.c_void_p)
    assert L.mvx_branchAndBound_dist(tptr, None, P.h, bnb.C.byref(pr), None, None, bnb.C.byref(res), bnb.C.byref(st)) == capi.EFAIL
    # a graph that cannot be computed: an error with the unsolved root as the tree, not a run without the rule
    bare = bnb.table_from(orc)
    bare.get_mat_row = None
    for w in (1, 64):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bare, quirks=0, node_cliques=4, window=w)
        assert r["rc"] == -2 and r["n_nodes"] == 1 and r["count"] == 0 and not r["has_incumbent"], w


def test_python_front_end_lists_the_new_names():
    """The binding keeps the field lists it had and reaches what the C structs have gained behind them by name: the tail sits
    where the C headers put it (right behind the listed fields), an instance is allocated over the whole struct, and the
    library's own table has both entries."""
    C = bnb.C
    assert bnb._TABLE_TAIL == ["clique_cuts_many", "add_cut_rows_many"]
    assert list(bnb.BnbParams._tail_) == ["node_cliques"] and tuple(bnb.BnbResult._tail_) == bnb.NODE_CLIQUE_COUNTERS
    for cls, first in ((bnb.LpApiTable, "clique_cuts_many"), (bnb.BnbParams, "node_cliques"), (bnb.BnbResult, "node_clique_conflicts")):
        assert cls._tail_[first][0] == C.sizeof(cls) and C.sizeof(cls._full_) > C.sizeof(cls)
    hdr = open(os.path.join(ROOT, "include", "mvx_bnb.h")).read()
    assert hdr.index("(*del_rows_many)") < hdr.index("(*clique_cuts_many)") < hdr.index("(*add_cut_rows_many)") < hdr.index("} mvx_lp_api;")
    assert hdr.index("int node_purge;") < hdr.index("int node_cliques;") < hdr.index("} mvx_bnb_params;")
    assert hdr.index("node_cut_rows_peak;") < hdr.index("node_clique_conflicts;") < hdr.index("node_clique_rows;") < hdr.index("} mvx_bnb_result;")
    t = bnb.LpApiTable.from_address(bnb.lib().mvx_hip_lp_api())
    assert bnb.table_entry(t, "clique_cuts_many") and bnb.table_entry(t, "add_cut_rows_many") and t.del_rows_many
    mine = bnb.LpApiTable()  # a fresh table is whole and null
    assert bnb.table_entry(mine, "clique_cuts_many") is None and bnb.table_entry(mine, "add_cut_rows_many") is None
    bnb.set_table_entry(mine, "add_cut_rows_many", 5)
    assert bnb.table_entry(mine, "add_cut_rows_many") == 5 and bnb.table_entry(mine, "clique_cuts_many") is None and not mine.del_rows_many
    pr = bnb.BnbParams()
    assert pr.node_cliques == 0
    bnb.lib().mvx_bnb_default_params(C.byref(pr))
    assert pr.node_cliques == 0 and pr.window == 64
    assert bnb.make_params(quirks=0).node_cliques == 0 and bnb.make_params(quirks=0, node_cliques=7).node_cliques == 7
    res = bnb.BnbResult()
    assert all(getattr(res, k) == 0 for k in bnb.NODE_CLIQUE_COUNTERS)


def test_cli_flag_parses():
    """--node-cliques on tests/golden/f1.lp.  Without a device the front end can not solve, so the flag is followed up to its
    refusal: it needs --repaired and says so; values out of range are refused by the parser itself."""
    exe = os.path.join(ROOT, "mvolps_amd", "bin", "mvolps")
    f1 = os.path.join(ROOT, "tests", "golden", "f1.lp")

    def cli(*flags):
        return subprocess.run([exe, "-f", f1, *flags], capture_output=True, text=True)

    assert "--node-cliques" in subprocess.run([exe, "-h"], capture_output=True, text=True).stdout
    for flags in (("--node-cliques",), ("--node-cliques", "4"), ("--node-cliques", "64", "-cm", "1"), ("--node-cliques", "-cm", "1")):
        r = cli(*flags)
        assert r.returncode != 0 and "--node-cliques needs --repaired" in r.stderr and "Unknown parameter" not in r.stderr, (flags, r.stderr)
    for bad in ("0", "65", "x", "4x"):
        r = cli("--repaired", "--node-cliques", bad)
        assert r.returncode != 0 and "Unknown parameter value for --node-cliques" in r.stderr, (bad, r.stderr)
