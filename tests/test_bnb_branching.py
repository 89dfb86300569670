"""CPU: branching on the node LP (var_strat 3 penalties, var_strat 4 strong branching), driver over the ORACLE's table.

The one-step dual penalties of mvx_bnb_penalties are checked bit for bit against a numpy restatement of their definition
(DESIGN.md "Branching on the node LP"), certified as bounds by solving both children of every candidate, and the new rules
are checked for serial-window equivalence, for closing on the HiGHS optimum and for their refusals."""
import json
import os

import numpy as np
import pytest

from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import DB, IV, MAX, NOFEAS, OPT, UP

from . import lpgen
from .test_bnb_host import same_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9


def np_penalties(P, cols, tol=TOL):
    """The definition, restated from the exported tableau and basis: x_B = T x_N, row 0 the reduced costs."""
    T = P.tableau()
    head, nb, flag = P.basis()
    m = P.m
    out = []
    for j in cols:
        i = int(np.nonzero(head == m + j)[0][0])
        v = T[i, 0]
        fd, fu = v - np.floor(v), np.ceil(v) - v
        best = {"d": (np.inf, 0), "u": (np.inf, 0)}
        for q in range(1, P.n + 1):
            a = T[i, q]
            if not abs(a) > tol:
                continue
            f = int(flag[q])
            dirs = {capi.NL: (1,), capi.NU: (-1,), capi.NF: (1, -1)}.get(f, ())
            r = abs(T[0, q]) / abs(a)
            for side, ok in (("d", any(s * a < 0 for s in dirs)), ("u", any(s * a > 0 for s in dirs))):
                if ok and r < best[side][0]:
                    best[side] = (r, q)
        pd = fd * best["d"][0] if best["d"][1] else np.inf
        pu = fu * best["u"][0] if best["u"][1] else np.inf
        out.append((pd, pu, best["d"][1], best["u"][1]))
    return out


def basic_fractional(P, tab):
    """Basic structural integer columns with a fractional value: the candidates a branching would see."""
    stat = P.col_stat()
    x = P.col_prim()
    return [j for j in range(1, P.n + 1) if stat[j - 1] == capi.BS and abs(x[j - 1] - np.round(x[j - 1])) > 1e-9]


def check_twin(P, tab, cols=None):
    cols = basic_fractional(P, tab) if cols is None else cols
    rc, (pd, pu, ad, au) = bnb.penalties(P, cols, TOL, table=tab)
    assert rc == 0
    ref = np_penalties(P, cols)
    for k, (d, u, qd, qu) in enumerate(ref):
        assert pd[k] == d or (np.isinf(pd[k]) and np.isinf(d)), (cols[k], pd[k], d)
        assert pu[k] == u or (np.isinf(pu[k]) and np.isinf(u)), (cols[k], pu[k], u)
        assert (ad[k], au[k]) == (qd, qu)
    return cols, pd, pu


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    assert t.get_tableau and t.get_basis and not t.branch_penalties_many  # the host twin is what runs over the oracle
    return t


def test_twin_matches_definition_root_and_children(orc, tab):
    A, b, c, U = synth.dense_ilp(12, 24, 5, 3)
    P = lpgen.load_ilp(orc, A, b, c, U)
    P.simplex()
    cols, _, _ = check_twin(P, tab)
    assert len(cols) >= 2
    for quirks in (1, 0):
        S2, S3 = bnb.make_children(P, cols[0], quirks=quirks, table=tab)
        for S in (S2, S3):
            S.simplex()
            if S.status == OPT:
                check_twin(S, tab)


def test_twin_matches_definition_general_bounds(orc, tab):
    """Every bound type on rows and columns: NU, free and fixed non-basic positions all occur."""
    rng = np.random.default_rng(7)
    seen = set()
    checked = 0
    for _ in range(60):
        A, row_b, col_b, c, d = lpgen.random_general_lp(rng, 10, 12)
        P = orc.create()
        P.load_general(A, row_b, col_b, c, kinds=[IV] * len(c), direction=d)
        P.simplex()
        if P.status != OPT:
            continue
        head, _nb, flag = P.basis()
        seen |= set(flag[1:].tolist())
        cols = [int(k) - P.m for k in head[1:] if k > P.m]  # every basic column, integral or not
        if cols:
            check_twin(P, tab, cols)
            checked += 1
    assert checked > 20
    assert {capi.NL, capi.NU, capi.NS} <= seen


def test_twin_matches_definition_with_cut_row(orc, tab):
    A, b, c, U = synth.dense_ilp(10, 20, 4, 3)
    P = lpgen.load_ilp(orc, A, b, c, U)
    P.simplex()
    m0 = P.m
    assert bnb.node_cuts(P, dict(cut_strat=1, quirks=0), table=tab) >= 1
    P.simplex()
    assert P.m > m0 and P.status == OPT
    cols, _, _ = check_twin(P, tab)
    assert cols


def test_infinite_side_is_infeasible(orc, tab):
    """max x1, 2 x1 + x2 <= 3, 0 <= x <= 10 integer: x1 = 1.5 is basic, only the row's slack (at its upper bound, free to
    decrease) and x2 move it, both downwards -- the up side has no position and its child (x1 >= 2) is infeasible."""
    P = orc.create()
    P.load_general(np.array([[2.0, 1.0]]), [(UP, 0.0, 3.0)], [(DB, 0.0, 10.0)] * 2, np.array([1.0, 0.0]), kinds=[IV, IV], direction=MAX)
    P.simplex()
    assert P.status == OPT
    cols, pd, pu = check_twin(P, tab)
    assert cols and np.isinf(pu).any()
    for k, j in enumerate(cols):
        if np.isinf(pu[k]):
            _, S3 = bnb.make_children(P, j, quirks=0, table=tab)
            S3.simplex()
            assert S3.status == NOFEAS
    assert np.isfinite(pd).all()


def certify_node(P, tab, quirks):
    """Both children of every candidate solved to optimality: a finite penalty is a bound on the child's objective drop
    in the LP's own sense, an infinite one means an infeasible child."""
    z = P.obj
    sg = 1.0 if P.api.get_obj_dir(P.h) == MAX else -1.0
    cols, pd, pu = check_twin(P, tab)
    n = 0
    for k, j in enumerate(cols):
        S2, S3 = bnb.make_children(P, j, quirks=quirks, table=tab)
        for S, pen in ((S2, pd[k]), (S3, pu[k])):
            S.simplex()
            n += 1
            if np.isinf(pen):
                assert S.status == NOFEAS, (j, pen)
            elif S.status != NOFEAS:
                assert S.status == OPT
                assert sg * (z - S.obj) >= pen - 1e-7 * (1 + abs(z)), (j, pen, sg * (z - S.obj))
    return n


@pytest.mark.parametrize("quirks", [1, 0])
def test_penalty_certificate(orc, tab, quirks):
    n = 0
    for case in [(10, 20, 4, 3), (12, 24, 5, 3), (16, 32, 5, 2), ("setcover", 40, 60, 3)]:
        P = lpgen.load_case(orc, case)
        P.simplex()
        n += certify_node(P, tab, quirks)
        cols = basic_fractional(P, tab)
        assert cols
        S2, S3 = bnb.make_children(P, cols[-1], quirks=quirks, table=tab)
        for S in (S2, S3):
            S.simplex()
            if S.status == OPT and basic_fractional(S, tab):
                n += certify_node(S, tab, quirks)
    assert n > 40


@pytest.mark.parametrize("cut_strat", [0, 1])
@pytest.mark.parametrize("quirks", [1, 0])
@pytest.mark.parametrize("var_strat", [3, 4])
def test_window_equals_serial(orc, tab, var_strat, quirks, cut_strat):
    A, b, c, U = synth.dense_ilp(10, 20, 4, 3)
    kw = dict(var_strat=var_strat, quirks=quirks, cut_strat=cut_strat, max_nodes=400, table=tab)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), window=1, **kw)
    assert ref["rc"] == 0 and ref["count"] > 50
    assert (ref["sb_lps"] > 0) == (var_strat == 4)
    for w in (2, 64):
        got = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), window=w, **kw)
        assert got["rc"] == 0
        same_result(got, ref)
        assert (got["sb_lps"], got["sb_pivots"]) == (ref["sb_lps"], ref["sb_pivots"])


def test_strong_branching_batch_split_does_not_matter(orc, tab, monkeypatch):
    A, b, c, U = synth.dense_ilp(10, 20, 4, 3)
    kw = dict(var_strat=4, quirks=0, max_nodes=300, table=tab, window=64, sb_cands=4)
    whole = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), **kw)
    monkeypatch.setenv("MVX_SB_BUDGET_MB", "0")  # one candidate's children per batch
    split = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), **kw)
    same_result(split, whole)
    assert (split["sb_lps"], split["sb_pivots"]) == (whole["sb_lps"], whole["sb_pivots"])


# HiGHS (scipy.optimize.milp 1.15.3) optima of the instances below
HIGHS = {(10, 20, 4, 3): 122.0, (16, 32, 5, 2): 210.0, (20, 40, 7, 3): 246.0, ("setcover", 40, 60, 3): 22.0, ("setcover", 30, 50, 4): 18.0}


@pytest.mark.parametrize("var_strat", [3, 4])
@pytest.mark.parametrize("case", list(HIGHS), ids=str)
def test_trees_close_on_the_optimum(orc, tab, case, var_strat):
    r = bnb.branch_and_bound(lpgen.load_case(orc, case), var_strat=var_strat, quirks=0, table=tab)
    assert r["rc"] == 0 and r["hit_limit"] == 0 and r["has_incumbent"]
    assert abs(r["best_lower"] - HIGHS[case]) <= 1e-6 * (1 + abs(HIGHS[case]))


def test_pinned_cut_ilp_optimum_is_what_the_tests_use():
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "milp_pins.json")))
    assert [p["milp_obj"] for p in pins["cut_ilps"]] == [20.0, 20.0]  # closed on the GPU in test_gpu_branching.py


def test_strong_branching_closes_in_fewer_nodes():
    """Measured over the oracle's table, repaired mode, FIFO order, default sb_cands = 2 / sb_iters = 4 (loop iterations to
    close; VO / VGO / var_strat 3 / var_strat 4):
      dense_ilp(16, 32, 5, 2):  4 639 / 2 905 / 2 435 /   925
      dense_ilp(20, 40, 7, 3): 13 749 / 11 273 / 3 881 / 4 105
      setcover_ilp(40, 60, 3):      15 /     11 /     7 /     7
    Not everywhere: dense_ilp(10, 20, 4, 3) takes 685 / 277 / 861 / 675 and dense_ilp(12, 24, 5, 3) 237 / 151 / 253 / 299."""
    from oracle import oracle

    orc = oracle.api()
    tab = bnb.table_from(orc)
    for case, expect in (((16, 32, 5, 2), 925), ((20, 40, 7, 3), 4105), (("setcover", 40, 60, 3), 7)):
        n = {vs: bnb.branch_and_bound(lpgen.load_case(orc, case), var_strat=vs, quirks=0, table=tab)["count"] for vs in (0, 2, 4)}
        assert n[4] == expect, (case, n)
        assert n[4] < n[0] and n[4] < n[2], (case, n)


def test_refusals(orc, tab):
    from mvolps_amd import dist_bnb, dist_native

    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    for kw in (dict(var_strat=3, node_strat=1, best_window=8), dict(var_strat=4, best_window=1), dict(var_strat=5), dict(var_strat=-1)):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, **kw)
        assert r["rc"] == -1 and r["n_nodes"] == 0 and r["count"] == 0, kw
    # best-bound order node at a time is fine
    r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, var_strat=3, node_strat=1, quirks=0)
    assert r["rc"] == 0 and r["has_incumbent"]
    # neither penalties entry nor tableau export: an error, not another rule
    bare = bnb.table_from(orc)
    bare.get_tableau = bare.get_basis = None
    for vs in (3, 4):
        for w in (1, 64):
            r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bare, var_strat=vs, window=w)
            assert r["rc"] == -2 and r["count"] == 0
    P = lpgen.load_ilp(orc, A, b, c, U)
    P.simplex()
    out = (bnb.C.c_double * 5)()
    assert bnb.lib().mvx_bnb_classify(bnb.C.cast(bnb.C.pointer(tab), bnb.C.c_void_p), P.h, P.h, 1, 3, out) == -1
    assert bnb.lib().mvx_bnb_classify(bnb.C.cast(bnb.C.pointer(tab), bnb.C.c_void_p), P.h, P.h, 1, 4, out) == -1
    with pytest.raises(ValueError):
        dist_native.branch_and_bound(P, table=tab, var_strat=3)
    with pytest.raises(ValueError):
        dist_bnb.branch_and_bound(None, P, var_strat=4)
    # mvx_bnb_penalties' own codes
    cols = basic_fractional(P, tab)
    assert bnb.penalties(P, [0], table=tab)[0] == -1
    assert bnb.penalties(P, [P.n + 1], table=tab)[0] == -1
    nonbasic = [j for j in range(1, P.n + 1) if P.col_stat()[j - 1] != capi.BS]
    assert bnb.penalties(P, nonbasic[:1], table=tab)[0] == -4
    Q = P.copy()
    orc.set_col_bnds(Q.h, cols[0], UP, 0.0, 0.0)  # an edit: not solved, not OPT
    assert bnb.penalties(Q, cols[:1], table=tab)[0] == -3
    assert bnb.penalties(P, cols[:1], table=bare)[0] == -5
