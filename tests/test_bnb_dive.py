"""CPU: the LP diving heuristic (mvx_bnb_params.dive, DESIGN.md "LP diving heuristic"), driver over the ORACLE's table, so the
host twins run (mvx_bnb_dive_pick for the picks, set_col_bnds per entry, the oracle's sequential batch solve, mvx_bnb_round for
the integral ends).

The pick twin is checked with == against a plain-Python restatement of the definition built from the test's own arrays; whole
dives against a restatement written with the oracle's copy / set_col_bnds / simplex; the points the dives find on the
enumerated fixture are feasible and no better than the pinned optimum; the trees close on the pins under every option set; the
FIFO window gives the serial tree, counters included, for every window size; dive = 0 is the parent's driver; the refusals and
return codes are pinned."""
import math

import numpy as np
import pytest

from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import CV, DB, FR, FX, IV, LO, MAX, MIN, OPT, UP

from . import lpgen
from .test_bnb_branching import HIGHS
from .test_bnb_general import INSTANCES, check_pin, failures, instance, run
from .test_bnb_host import same_result

RULES = (1, 2, 4)
COUNTERS = ("dive_calls", "dive_found", "dive_improved", "dive_lps", "dive_pivots", "prop_calls", "prop_fixed", "prop_tightened",
            "prop_infeasible", "rc_calls", "rc_fixed", "rc_tightened", "heur_calls", "heur_found", "heur_improved", "incumbent_heur",
            "sb_lps", "sb_pivots")


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    assert not t.dive_pick_many and not t.set_col_bnds_many and not t.round_many  # the host twins are what runs over the oracle
    return t


class Model:
    """What the rules read of the root's model, from the test's own arrays: per column the rows that lock it down / up, its
    non-zeros, the objective, the kinds and the sense."""

    def __init__(self, A, rlo, rhi, c, isint, maximize):
        A = np.asarray(A, dtype=float)
        m, n = A.shape
        self.n = n
        self.dl, self.ul, self.len = [0] * n, [0] * n, [0] * n
        for i in range(m):
            lo, hi = math.isfinite(rlo[i]), math.isfinite(rhi[i])
            for j in range(n):
                a = A[i, j]
                if a == 0.0:
                    continue
                self.len[j] += 1
                self.dl[j] += (a > 0 and lo) or (a < 0 and hi)
                self.ul[j] += (a > 0 and hi) or (a < 0 and lo)
        self.c = [float(t) for t in c]
        self.isint = [bool(t) for t in isint]
        self.sg = 1.0 if maximize else -1.0


def general_model(A, row_b, c, kinds, direction):
    rlo, rhi = lpgen.bounds_arrays(row_b)
    return Model(A, rlo, rhi, c, [k != CV for k in kinds], direction == MAX)


def ilp_model(A, b, c):
    m, n = np.asarray(A).shape
    return Model(A, [-math.inf] * m, [float(t) for t in b], c, [True] * n, True)


def case_model(case):
    if case[0] == "setcover":
        A, c = lpgen.setcover_ilp(*case[1:])
        return Model(A, [1.0] * A.shape[0], [math.inf] * A.shape[0], c, [True] * A.shape[1], False)
    A, b, c, _U = synth.dense_ilp(*case)
    return ilp_model(A, b, c)


def milp_model(inst):
    A, rlo, rhi, _clo, _chi, c, _c0, isint, maximize = lpgen.milp_arrays(inst)
    return Model(A, rlo, rhi, c, isint, maximize)


def py_pick(M, v, rule):
    """The definition, one operation at a time on Python floats: (nfrac, col 1-based or 0, dir, val)."""
    best, nfrac = None, 0
    for j in range(M.n):
        t = float(v[j])
        if not M.isint[j] or not abs(t - float(np.rint(t))) > 1e-9:
            continue
        nfrac += 1
        fd, fu = t - math.floor(t), math.ceil(t) - t
        near = 0 if fd <= fu else 1
        if rule == 1:
            d, key = near, (min(fd, fu), 0.0, j)
        elif rule == 2:
            d = 0 if M.dl[j] < M.ul[j] else 1 if M.ul[j] < M.dl[j] else near
            key = (float(min(M.dl[j], M.ul[j])), fu if d else fd, j)
        else:
            s = M.sg * M.c[j]
            d = 0 if s > 0 else 1 if s < 0 else near
            key = ((abs(M.c[j]) * (fu if d else fd)) / float(M.len[j] + 1), 0.0, j)
        if best is None or key < best[0]:
            best = (key, d, t)
    if best is None:
        return 0, 0, 0, 0.0
    return nfrac, best[0][2] + 1, best[1], best[2]


def check_pick(M, root, node, tab, seen=None):
    v = node.col_prim()
    for rule in RULES:
        rc, got = bnb.dive_pick_node(node, root, rule, table=tab)
        want = py_pick(M, v, rule)
        assert rc == 0 and got == want, (rule, got, want)
        if seen is not None and want[0]:
            seen.add(("dir", want[2]))
    return py_pick(M, v, 1)[0]


def test_pick_twin_matches_the_restatement_mixed_rows(orc, tab):
    rng = np.random.default_rng(11)
    seen, checked, fractional, negative, continuous = set(), 0, 0, 0, 0
    for _ in range(120):
        A, row_b, col_b, c, d = lpgen.random_general_lp(rng, 10, 12)
        kinds = [IV if rng.random() < 0.7 else CV for _ in c]
        root = orc.create()
        root.load_general(A, row_b, col_b, c, kinds=kinds, direction=d)
        node = root.copy()
        node.simplex()
        if node.status != OPT:
            continue
        seen |= {("row", t) for t, _, _ in row_b} | {("col", t) for t, _, _ in col_b} | {("sense", d)}
        negative += int((np.asarray(A) < 0).any())
        continuous += int(CV in kinds)
        fractional += check_pick(general_model(A, row_b, c, kinds, d), root, node, tab, seen) > 0
        checked += 1
    assert checked > 40 and fractional > 20, (checked, fractional)
    assert {("row", t) for t in (LO, UP, DB, FX, FR)} <= seen and {("col", t) for t in (LO, UP, DB, FX, FR)} <= seen
    assert {("dir", 0), ("dir", 1), ("sense", MIN), ("sense", MAX)} <= seen
    assert negative > 20 and continuous > 20


def test_pick_twin_matches_the_restatement_on_children(orc, tab):
    """Nodes with tightened column bounds: the model is the root's, not the node's."""
    A, b, c, U = synth.dense_ilp(12, 24, 5, 3)
    M = ilp_model(A, b, c)
    root = lpgen.load_ilp(orc, A, b, c, U)
    queue, done = [root.copy()], 0
    while queue and done < 12:
        P = queue.pop(0)
        P.simplex()
        if P.status != OPT:
            continue
        check_pick(M, root, P, tab)
        done += 1
        _st, viol = bnb.print_info(P, quirks=0, table=tab)
        if viol:
            queue += list(bnb.make_children(P, viol[0], quirks=0, table=tab))
    assert done >= 8


def tie_model(orc, last=2.0):
    """n = 300 columns, rows a_j x_j <= 1 with a_j = 2 (the last one `last`), c = 1, maximise: every x_j = 1 / a_j."""
    n = 300
    A = np.diag([2.0] * (n - 1) + [last])
    root = orc.create()
    root.load_general(A, [(UP, 0.0, 1.0)] * n, [(DB, 0.0, 3.0)] * n, [1.0] * n, kinds=[IV] * n, direction=MAX)
    node = root.copy()
    node.simplex()
    assert node.status == OPT
    return ilp_model(A, [1.0] * n, [1.0] * n), root, node


def test_ties_go_to_the_lowest_column(orc, tab):
    """All keys equal across five waves' worth of columns (x_j = 0.5, fd = fu, one up-lock each, c = 1): column 1 going down
    wins under every rule.  With 4 x_300 <= 1 the last column is the closest to an integer and rule 1 picks it."""
    M, root, node = tie_model(orc)
    check_pick(M, root, node, tab)
    for rule in RULES:
        assert bnb.dive_pick_node(node, root, rule, table=tab) == (0, (300, 1, 0, 0.5))
    M, root, node = tie_model(orc, last=4.0)
    check_pick(M, root, node, tab)
    assert bnb.dive_pick_node(node, root, 1, table=tab) == (0, (300, 300, 0, 0.25))
    assert bnb.dive_pick_node(node, root, 2, table=tab)[1][1] == 300  # no down-lock, the smallest f_dir
    assert bnb.dive_pick_node(node, root, 4, table=tab)[1][1] == 300  # the smallest |c| f / (len + 1)


def test_a_value_within_1e_9_of_an_integer_is_no_candidate(orc, tab):
    A = np.array([[3.0, 0.0], [1.0, -1.0]])
    row_b = [(UP, 0.0, 6.000000000000001), (LO, -7.5, 0.0)]
    root = orc.create()
    root.load_general(A, row_b, [(LO, 0.0, 0.0), (LO, 0.0, 0.0)], [1.0, 1.0], kinds=[IV, IV], direction=MAX)
    node = root.copy()
    node.simplex()
    v = node.col_prim()
    assert node.status == OPT and v[0] != 2.0 and abs(v[0] - 2.0) < 1e-9
    check_pick(general_model(A, row_b, [1.0, 1.0], [IV, IV], MAX), root, node, tab)
    for rule in RULES:  # x2 = 9.5: near is down, its one lock is an up-lock, and down is what costs objective
        rc, (nfrac, col, side, val) = bnb.dive_pick_node(node, root, rule, table=tab)
        assert (rc, nfrac, col, side, val) == (0, 1, 2, 0, v[1])


# ------------------------------------------------------------------------------------------------ whole dives

def col_range(orc, P, j):
    t = orc.get_col_type(P.h, j)
    l = orc.get_col_lb(P.h, j) if t in (LO, DB, FX) else -math.inf
    u = l if t == FX else orc.get_col_ub(P.h, j) if t in (UP, DB) else math.inf
    return l, u


def set_range(orc, P, j, l, u):
    hl, hu = math.isfinite(l), math.isfinite(u)
    t = (FX if l == u else DB) if hl and hu else LO if hl else UP if hu else FR
    orc.set_col_bnds(P.h, j, t, l if hl else 0.0, u if hu else 0.0)


def py_dive(orc, tab, M, root, node, rule, depth=0, stats=None):
    """One dive, written with the oracle's copy / set_col_bnds / simplex: (found, obj, x, lps, pivots)."""
    cur, d, lps, piv = node, 0, 0, 0
    limit = depth if depth > 0 else 4 * M.n + 64
    note = (lambda k: stats.__setitem__(k, stats.get(k, 0) + 1)) if stats is not None else (lambda k: None)
    while True:
        nfrac, col, side, val = py_pick(M, cur.col_prim(), rule)
        if nfrac == 0:
            note("integral")
            rc, obj, found, x = bnb.round_node(cur, root, 1, table=tab)
            assert rc == 0
            return found, obj, x, lps, piv
        if d >= limit:
            note("depth")
            return 0, 0.0, None, lps, piv
        nxt = None
        for attempt, s in enumerate((side, 1 - side)):
            l, u = col_range(orc, cur, col)
            l, u = (float(math.ceil(val)), u) if s else (l, float(math.floor(val)))
            if attempt:
                note("flip")
            if l > u:
                continue
            kid = cur.copy()
            set_range(orc, kid, col, l, u)
            before = kid.it_cnt
            kid.simplex()
            lps += 1
            piv += kid.it_cnt - before
            if kid.status == OPT:
                nxt = kid
                break
        if nxt is None:
            note("infeasible")
            return 0, 0.0, None, lps, piv
        cur, d = nxt, d + 1


def py_dives(orc, tab, M, root, node, rules, depth=0, stats=None):
    best, lps, piv = (0, 0.0, None), 0, 0
    for rule in RULES:
        if not rules & rule:
            continue
        found, obj, x, l, p = py_dive(orc, tab, M, root, node, rule, depth, stats)
        lps, piv = lps + l, piv + p
        if found and (not best[0] or M.sg * obj > M.sg * best[1]):
            best = (1, obj, x)
    return best + (lps, piv)


def check_dives(orc, tab, M, root, node, rules, depth=0, stats=None):
    rc, obj, found, x, lps, piv = bnb.dive_node(node, root, rules, depth, table=tab)
    want = py_dives(orc, tab, M, root, node, rules, depth, stats)
    assert rc == 0 and (found, lps, piv) == (want[0], want[3], want[4]), (rules, depth, (found, lps, piv), want)
    if found:
        assert obj == want[1] and np.array_equal(x[1:], want[2][1:])
    return found, obj, x


def solved_root(orc, tab, P):
    """(root with integer-rounded bounds, its solved clone), or None when the box is empty."""
    if bnb.integral_bounds(P, table=tab) == 2:
        return None
    node = P.copy()
    node.simplex()
    return P, node


@pytest.mark.parametrize("case", list(HIGHS), ids=str)
def test_whole_dives_match_the_restatement(orc, tab, case):
    root, node = solved_root(orc, tab, lpgen.load_case(orc, case))
    M = case_model(case)
    stats = {}
    for rules in (1, 2, 4, 7):
        check_dives(orc, tab, M, root, node, rules, stats=stats)
    check_dives(orc, tab, M, root, node, 7, depth=2, stats=stats)
    assert stats.get("depth", 0) > 0 and stats.get("integral", 0) > 0


def test_whole_dives_match_the_restatement_on_the_fixture(orc, tab):
    ran = []

    def one(rec):
        inst = instance(rec)
        got = solved_root(orc, tab, lpgen.load_milp(orc, inst))
        if got is None or got[1].status != OPT:
            return
        for rules in (1, 2, 4, 7):
            check_dives(orc, tab, milp_model(inst), got[0], got[1], rules)
        ran.append(rec["index"])

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)
    assert len(ran) >= 20


def test_fixture_roots(orc, tab):
    """Every fixture instance whose integer-rounded root solves OPT, each rule's root dive: nothing, or a point that is exactly
    integral, within the root's rows and bounds and no better than the enumerated optimum; nothing on a model without one."""
    roots, stats = 0, {}
    found_by = {r: 0 for r in RULES}

    def one(rec):
        nonlocal roots
        inst = instance(rec)
        got = solved_root(orc, tab, lpgen.load_milp(orc, inst))
        if got is None or got[1].status != OPT:
            return
        roots += 1
        root, node = got
        M = milp_model(inst)
        A, rlo, rhi, clo, chi, c, c0, isint, _mx = lpgen.milp_arrays(inst)
        for rule in RULES:
            found, obj, x = check_dives(orc, tab, M, root, node, rule, stats=stats)
            if not found:
                continue
            assert rec["status"] == "optimal", "a point on a model without one"
            found_by[rule] += 1
            x = x[1:]
            assert np.array_equal(x[isint], np.round(x[isint]))
            act = A @ x
            assert np.all(act >= rlo - 1e-9 * np.maximum(1, np.abs(rlo))) and np.all(act <= rhi + 1e-9 * np.maximum(1, np.abs(rhi)))
            assert np.all(x >= clo) and np.all(x <= chi)
            assert abs(float(c @ x) + c0 - obj) <= 1e-9 * (1 + abs(obj))
            assert M.sg * obj <= M.sg * rec["optimum"] + 1e-6 * (1 + abs(rec["optimum"])), (rule, obj, rec["optimum"])

    bad = failures(INSTANCES, one)
    assert not bad, "%d fail:\n%s" % (len(bad), "\n".join(bad))
    print("roots", roots, "found", found_by, stats)
    assert roots >= 240 and all(found_by[r] >= 170 for r in RULES), (roots, found_by)
    assert stats.get("flip", 0) >= 1 and stats.get("infeasible", 0) >= 1, stats


# ------------------------------------------------------------------------------------------------ trees

TREE_OPTIONS = {
    "serial": dict(window=1),
    "window64": dict(window=64),
    "heur2_rcfix_prop8_window64": dict(window=64, heur=2, rc_fix=1, prop=8),
    "cuts": dict(window=1, cut_strat=1),
    "best": dict(node_strat=1, window=1),
}


@pytest.mark.parametrize("family", "abcd")
@pytest.mark.parametrize("name", list(TREE_OPTIONS))
def test_trees_close_on_the_enumerated_optimum(orc, tab, name, family):
    recs = [r for r in INSTANCES if r["family"] == family]
    assert len(recs) >= 25
    ran = []

    def one(rec):
        inst = instance(rec)
        r = run(orc, rec, inst, table=tab, dive=7, dive_freq=1, **TREE_OPTIONS[name])
        check_pin(rec, inst, r)
        ran.append(r["dive_calls"])

    bad = failures(recs, one)
    assert not bad, "%d of %d fail:\n%s" % (len(bad), len(recs), "\n".join(bad))
    if family in "ab":
        assert sum(1 for c in ran if c > 0) >= 20  # the dives ran


def same_counters(a, b):
    for k in COUNTERS:
        assert a[k] == b[k], k


@pytest.mark.parametrize("cut_strat", [0, 1])
@pytest.mark.parametrize("rc_fix", [0, 1])
@pytest.mark.parametrize("heur", [0, 2])
def test_windows_equal_serial(orc, tab, heur, rc_fix, cut_strat):
    A, b, c, U = synth.dense_ilp(10, 20, 4, 3)
    kw = dict(quirks=0, cut_strat=cut_strat, max_nodes=400, table=tab, heur=heur, rc_fix=rc_fix, dive=7, dive_freq=3)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), window=1, **kw)
    assert ref["rc"] == 0 and ref["count"] > 50 and ref["dive_calls"] > 5 and ref["dive_found"] > 0
    assert heur or ref["dive_improved"] > 0  # behind heur 2 the dives of this instance find nothing better
    assert ref["dive_lps"] > ref["dive_calls"] and ref["dive_pivots"] > 0
    for w in (2, 8, 64):
        got = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), window=w, **kw)
        assert got["rc"] == 0
        same_result(got, ref)
        same_counters(got, ref)


def test_windows_give_the_serial_tree_on_the_fixture(orc, tab):
    recs = INSTANCES[::10]
    assert len({r["family"] for r in recs}) == 4

    def one(rec):
        inst = instance(rec)
        for extra in (dict(), dict(heur=2, rc_fix=1), dict(cut_strat=1)):
            ref = run(orc, rec, inst, table=tab, window=1, dive=7, dive_freq=3, **extra)
            for w in (2, 8, 64):
                got = run(orc, rec, inst, table=tab, window=w, dive=7, dive_freq=3, **extra)
                same_result(got, ref)
                same_counters(got, ref)

    bad = failures(recs, one)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", list(HIGHS), ids=str)
def test_no_more_nodes_on_a_closed_tree(orc, tab, case):
    """FIFO order without rc_fix: node LPs and branching choices depend on the path only, and an incumbent found earlier prunes
    at least what a later one would."""
    off = bnb.branch_and_bound(lpgen.load_case(orc, case), table=tab, quirks=0)
    on = bnb.branch_and_bound(lpgen.load_case(orc, case), table=tab, quirks=0, dive=7)
    assert on["rc"] == off["rc"] == 0 and on["hit_limit"] == off["hit_limit"] == 0
    assert on["count"] <= off["count"], (on["count"], off["count"])
    assert abs(on["best_lower"] - HIGHS[case]) <= 1e-6 * (1 + abs(HIGHS[case]))
    assert abs(off["best_lower"] - HIGHS[case]) <= 1e-6 * (1 + abs(HIGHS[case]))
    assert on["dive_calls"] == 1 and off["dive_calls"] == 0


def test_the_root_dive_beats_the_rounding_heuristic(orc, tab):
    A, b, c, U = synth.dense_ilp(64, 128, 3, 3, 0.4)
    h = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0, max_nodes=1, heur=2)
    d = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0, max_nodes=1, dive=7)
    assert h["rc"] == d["rc"] == 0 and h["has_incumbent"] and d["has_incumbent"]
    assert (h["incumbent_heur"], d["incumbent_heur"]) == (1, 2)
    assert d["best_lower"] > h["best_lower"], (d["best_lower"], h["best_lower"])
    assert (h["best_lower"], d["best_lower"]) == (783.0, 825.0)  # the figures of the definition's prototype
    x = np.array(d["x"])
    assert np.array_equal(x, np.round(x)) and (x >= 0).all() and (x <= U).all() and (A @ x <= b).all() and float(c @ x) == 825.0


def test_dive_0_is_the_parent(orc, tab):
    for case in [(10, 20, 4, 3), ("setcover", 40, 60, 3)]:
        for kw in (dict(window=1), dict(window=64), dict(node_strat=1), dict(heur=2, cut_strat=1, rc_fix=1, prop=8)):
            a = bnb.branch_and_bound(lpgen.load_case(orc, case), table=tab, quirks=0, **kw)
            z = bnb.branch_and_bound(lpgen.load_case(orc, case), table=tab, quirks=0, dive=0, dive_freq=5, dive_depth=3, **kw)
            same_result(z, a)
            same_counters(z, a)
            assert (z["dive_calls"], z["dive_found"], z["dive_improved"], z["dive_lps"], z["dive_pivots"]) == (0, 0, 0, 0, 0)
    pr = bnb.make_params()
    assert (pr.dive, pr.dive_freq, pr.dive_depth) == (0, 0, 0)


def test_refusals_and_return_codes(orc, tab):
    from mvolps_amd import dist_bnb, dist_native

    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    for kw in (dict(dive=8, quirks=0), dict(dive=-1, quirks=0), dict(dive=7, quirks=1), dict(dive=7), dict(dive=1, quirks=0, dive_freq=-1),
               dict(dive=1, quirks=0, dive_depth=-1), dict(dive=7, quirks=0, node_strat=1, best_window=8),
               dict(dive=1, quirks=0, best_window=1)):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, **kw)
        assert r["rc"] == -1 and r["n_nodes"] == 0 and r["count"] == 0, kw
    for d in (1, 7):
        assert bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0, dive=d, dive_freq=2, dive_depth=5)["rc"] == 0
    P = lpgen.load_ilp(orc, A, b, c, U)
    with pytest.raises(ValueError):
        dist_native.branch_and_bound(P, table=tab, dive=7, quirks=0)
    with pytest.raises(ValueError):
        dist_bnb.branch_and_bound(None, P, dive=7, quirks=0)
    pr = bnb.make_params(quirks=0, dive=7)
    L = dist_native._lib()
    res, st = bnb.BnbResult(), dist_native.DistStats()
    tptr = bnb.C.cast(bnb.C.pointer(tab), bnb.C.c_void_p)
    assert L.mvx_branchAndBound_dist(tptr, None, P.h, bnb.C.byref(pr), None, None, bnb.C.byref(res), bnb.C.byref(st)) == capi.EFAIL
    # the twins' own codes
    node = P.copy()
    node.simplex()
    assert node.status == OPT
    for rule in (0, 3, 5, 7, 8):
        assert bnb.dive_pick_node(node, P, rule, table=tab)[0] == -1
    assert bnb.dive_pick_node(P, P, 1, table=tab)[0] == -3  # never solved
    assert bnb.dive_node(P, P, 7, table=tab)[0] == -3
    assert bnb.dive_node(node, P, 0, table=tab)[0] == -1 and bnb.dive_node(node, P, 8, table=tab)[0] == -1
    assert bnb.dive_node(node, P, 7, depth=-1, table=tab)[0] == -1
    A2, b2, c2, U2 = synth.dense_ilp(8, 15, 3, 2)
    other = lpgen.load_ilp(orc, A2, b2, c2, U2)
    assert bnb.dive_pick_node(node, other, 1, table=tab)[0] == -1 and bnb.dive_node(node, other, 7, table=tab)[0] == -1  # another column count
    # neither dive_pick_many nor the twin's accessors: an error with the tree so far, not a run without the dives
    for missing in ("get_mat_row", "get_col_kind", "get_row_ub", "get_obj_coef"):
        bare = bnb.table_from(orc)
        setattr(bare, missing, None)
        assert bnb.dive_pick_node(node, P, 1, table=bare)[0] == -2
        assert bnb.dive_node(node, P, 7, table=bare)[0] == -2
        if missing == "get_mat_row":
            for kw in (dict(window=1), dict(window=64), dict(node_strat=1)):
                r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bare, dive=7, quirks=0, **kw)
                assert r["rc"] == -2 and r["count"] == 0 and r["has_incumbent"] == 0 and r["n_nodes"] == 1, kw


def test_the_callers_handle_is_left_as_it_was(orc, tab):
    def state(P):
        return ([(orc.get_col_type(P.h, j), orc.get_col_lb(P.h, j), orc.get_col_ub(P.h, j), orc.get_col_stat(P.h, j)) for j in range(1, P.n + 1)],
                P.m, P.status, P.it_cnt, P.obj)

    A, b, c, U = synth.dense_ilp(10, 20, 4, 3)
    P = lpgen.load_ilp(orc, A, b, c, U)
    before = state(P)
    r = bnb.branch_and_bound(P, quirks=0, table=tab, window=1, dive=7, dive_freq=2)
    assert r["rc"] == 0 and r["dive_lps"] > 0
    assert state(P) == before
    node = P.copy()
    node.simplex()
    before = state(node), node.col_prim().tolist()
    assert bnb.dive_node(node, P, 7, table=tab)[0] == 0
    assert (state(node), node.col_prim().tolist()) == before
