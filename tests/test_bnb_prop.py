"""CPU: node bound propagation (mvx_bnb_params.prop, DESIGN.md "Node bound propagation"), driver over the ORACLE's table, so
the host twin runs (mvx_bnb_propagate for the lists, set_col_bnds per entry for the apply).

The twin is checked with == against a plain-Python restatement of the definition built from the test's own arrays; on the
enumerated fixture no pinned optimum leaves the propagated root box and only infeasible models are proved infeasible; the
trees close on the enumerated pins under every option set; the FIFO window gives the serial tree, counters included, for every
window size; prop = 0 is the parent's driver; the refusals and return codes are pinned; and on a tight-capacity binary
instance the tree gets smaller with the same optimum."""
import math

import numpy as np
import pytest

from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import CV, DB, FX, IV, LO, UP

from . import lpgen
from .test_bnb_branching import HIGHS
from .test_bnb_general import INSTANCES, check_pin, failures, instance, run
from .test_bnb_host import same_result
from .test_bnb_rcfix import DENSE

INF = math.inf
COUNTERS = ("prop_calls", "prop_fixed", "prop_tightened", "prop_infeasible", "rc_calls", "rc_fixed", "rc_tightened", "heur_calls",
            "heur_found", "heur_improved", "incumbent_heur")
# the tight-capacity binary instance (b_i about twice the mean coefficient) and its node counts without / with prop = 8
TIGHT = (10, 20, 3, 1, 0.1)
TIGHT_COUNTS = (195, 19)


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    assert not t.propagate_many and not t.set_col_bnds_many  # the host twin and set_col_bnds per entry are what runs here
    return t


def tol(v):
    return 1e-9 * max(1.0, abs(v))


def restate(A, rlo, rhi, isint, l0, u0, K, seen=None):
    """The definition, one operation at a time on Python floats.  A: list of rows, each a list of (j, a_ij) in ascending j
    (0-based j); l0 / u0 the handle's bounds (+-inf when absent).  Returns (infeasible, rounds, [(column 1-based, lb, ub)])."""
    n = len(l0)
    l, u = list(l0), list(u0)
    note = seen.add if seen is not None else (lambda s: None)
    rounds = 0
    for _ in range(K):
        rounds += 1
        act = []
        bad = False
        for i, row in enumerate(A):
            lmin = lmax = 0.0
            kmin = kmax = 0
            for j, a in row:
                bmin, bmax = (l[j], u[j]) if a > 0 else (u[j], l[j])
                if math.isinf(bmin):
                    kmin += 1
                else:
                    lmin = lmin + a * bmin
                if math.isinf(bmax):
                    kmax += 1
                else:
                    lmax = lmax + a * bmax
            act.append((lmin, lmax, kmin, kmax))
            if kmin == 0 and math.isfinite(rhi[i]) and lmin > rhi[i] + tol(rhi[i]):
                bad = True
            if kmax == 0 and math.isfinite(rlo[i]) and lmax < rlo[i] - tol(rlo[i]):
                bad = True
        if bad:
            note("contradictory row")
            return 1, rounds, []
        nl, nu = list(l), list(u)
        for j in range(n):
            lows, ups = [l[j]], [u[j]]
            for i, row in enumerate(A):
                a = dict(row).get(j, 0.0)
                if a == 0.0:
                    continue
                lmin, lmax, kmin, kmax = act[i]
                bmin, bmax = (l[j], u[j]) if a > 0 else (u[j], l[j])
                for bound, L, k, b, upper_side in ((rhi[i], lmin, kmin, bmin, True), (rlo[i], lmax, kmax, bmax, False)):
                    if not math.isfinite(bound):
                        continue
                    if k == 0:
                        res = L - a * b
                    elif k == 1 and math.isinf(b):
                        res = L
                    else:
                        continue
                    q = (bound - res) / a
                    if not math.isfinite(q):
                        continue
                    if not isint[j]:
                        note("continuous")
                        continue
                    if k == 1:
                        note("single infinite term")
                    if (a > 0) == upper_side:
                        ups.append(float(math.floor(q + tol(q))))
                    else:
                        lows.append(float(math.ceil(q - tol(q))))
            nl[j], nu[j] = max(lows), min(ups)
        crossed = any(nl[j] > nu[j] for j in range(n))
        changed = nl != l or nu != u
        l, u = nl, nu
        if crossed:
            note("crossing")
            return 1, rounds, []
        if not changed:
            break
    out = []
    for j in range(n):
        if l[j] != l0[j] or u[j] != u0[j]:
            out.append((j + 1, l[j], u[j]))
            if l[j] > l0[j] and math.isfinite(l0[j]):
                note("lower bound raised")
            if u[j] < u0[j] and math.isfinite(u0[j]):
                note("upper bound lowered")
            if (math.isinf(l0[j]) and math.isfinite(l[j])) or (math.isinf(u0[j]) and math.isfinite(u[j])):
                note("absent bound made finite")
    return 0, rounds, out


def sparse_rows(A):
    return [[(j, float(a)) for j, a in enumerate(row) if a != 0.0] for row in np.asarray(A, dtype=float)]


def set_bounds(api, P, j, lb, ub):
    """Column j (1-based) of P takes [lb, ub], +-inf for an absent bound."""
    hl, hu = math.isfinite(lb), math.isfinite(ub)
    t = (FX if lb == ub else DB) if hl and hu else LO if hl else UP if hu else capi.FR
    api.set_col_bnds(P.h, j, t, lb if hl else 0.0, ub if hu else 0.0)


def test_twin_matches_the_restatement(orc, tab):
    rng = np.random.default_rng(31)
    seen, handles, entries, many_rounds = set(), 0, 0, 0
    for _ in range(400):
        A, row_b, col_b, c, d = lpgen.random_general_lp(rng, 10, 12)
        kinds = [IV if rng.random() < 0.7 else CV for _ in c]
        root = orc.create()
        root.load_general(A, row_b, col_b, c, kinds=kinds, direction=d)
        rows = sparse_rows(A)
        rlo, rhi = (list(map(float, v)) for v in lpgen.bounds_arrays(row_b))
        clo, chi = (list(map(float, v)) for v in lpgen.bounds_arrays(col_b))
        isint = [k != CV for k in kinds]
        # the root itself, then clones with a pending edit of one or two columns' bounds (as a branching or a list leaves them)
        for variant in range(4):
            P, l, u = root, list(clo), list(chi)
            if variant:
                P = root.copy()
                for j in rng.choice(len(c), size=min(len(c), variant), replace=False):
                    j = int(j)
                    mid = float(rng.integers(-2, 5))
                    if rng.random() < 0.5:
                        u[j] = min(u[j], mid) if l[j] <= mid else u[j]
                    else:
                        l[j] = max(l[j], mid) if mid <= u[j] else l[j]
                    set_bounds(orc, P, j + 1, l[j], u[j])
            for K in (1, 8):
                rc, got = bnb.propagate_node(P, root, K, table=tab)
                assert rc == 0
                want = restate(rows, rlo, rhi, isint, l, u, K, seen)
                assert got == want, (variant, K, got, want)
                entries += len(want[2])
                many_rounds += want[1] >= 3
            handles += 1
    assert handles == 1600 and entries > 1000 and many_rounds > 20, (handles, entries, many_rounds)
    assert seen >= {"lower bound raised", "upper bound lowered", "absent bound made finite", "single infinite term", "contradictory row",
                    "crossing", "continuous"}, seen


def test_fixture_roots_keep_their_pinned_optimum(orc, tab):
    """K = 8 on the integer-rounded root box of every fixture instance whose box is not empty: the enumerated optimum stays
    inside on every integer column, and only models without an integer point are proved infeasible."""
    boxes = changed = proved = 0
    for rec in INSTANCES:
        inst = instance(rec)
        root = lpgen.load_milp(orc, inst)
        if bnb.integral_bounds(root, table=tab) == 2:
            continue
        boxes += 1
        rc, (infeasible, rounds, lst) = bnb.propagate_node(root, root, 8, table=tab)
        assert rc == 0 and 1 <= rounds <= 8
        if infeasible:
            assert rec["status"] != "optimal", "instance %d has the optimum %r" % (rec["index"], rec["optimum"])
            assert lst == []
            proved += 1
            continue
        changed += bool(lst)
        if rec["status"] == "optimal":
            for j, lb, ub in lst:
                if inst["kinds"][j - 1] != CV:
                    assert lb <= rec["x"][j - 1] <= ub, (rec["index"], j, lb, ub, rec["x"][j - 1])
        assert all(inst["kinds"][j - 1] != CV for j, _, _ in lst)
    assert boxes >= 300 and changed >= 200 and proved >= 55, (boxes, changed, proved)


TREE_OPTIONS = {
    "serial": dict(window=1, prop=8),
    "window64": dict(window=64, prop=8),
    "heur2_rcfix_window64": dict(window=64, prop=8, heur=2, rc_fix=1),
    "cuts": dict(window=1, prop=8, cut_strat=1),
    "best": dict(node_strat=1, window=1, prop=8),
    "var3": dict(window=1, prop=8, var_strat=3),
    "prop1": dict(window=1, prop=1),
}


@pytest.mark.parametrize("family", "abcd")
@pytest.mark.parametrize("name", list(TREE_OPTIONS))
def test_trees_close_on_the_enumerated_optimum(orc, tab, name, family):
    recs = [r for r in INSTANCES if r["family"] == family]
    assert len(recs) >= 25
    ran = []

    def one(rec):
        inst = instance(rec)
        r = run(orc, rec, inst, table=tab, **TREE_OPTIONS[name])
        check_pin(rec, inst, r)
        ran.append(r["prop_calls"])

    bad = failures(recs, one)
    assert not bad, "%d of %d fail:\n%s" % (len(bad), len(recs), "\n".join(bad))
    assert sum(1 for c in ran if c > 0) >= 20  # the rule ran (a root with an empty integer range is booked in front of it)


def same_counters(a, b):
    for k in COUNTERS:
        assert a[k] == b[k], k


def test_windows_give_the_serial_tree_on_the_fixture(orc, tab):
    recs = INSTANCES[::10]
    assert len({r["family"] for r in recs}) == 4

    def one(rec):
        inst = instance(rec)
        for extra in (dict(), dict(heur=2, rc_fix=1), dict(cut_strat=1)):
            ref = run(orc, rec, inst, table=tab, window=1, prop=8, **extra)
            for w in (2, 8, 64):
                got = run(orc, rec, inst, table=tab, window=w, prop=8, **extra)
                same_result(got, ref)
                same_counters(got, ref)

    bad = failures(recs, one)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cut_strat", [0, 1])
@pytest.mark.parametrize("rc_fix", [0, 1])
@pytest.mark.parametrize("heur", [0, 2])
def test_windows_equal_serial(orc, tab, heur, rc_fix, cut_strat):
    A, b, c, U = synth.dense_ilp(10, 20, 4, 3)
    kw = dict(quirks=0, cut_strat=cut_strat, max_nodes=400, table=tab, heur=heur, rc_fix=rc_fix, prop=8)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), window=1, **kw)
    assert ref["rc"] == 0 and ref["count"] > 50 and ref["prop_calls"] == ref["n_nodes"]  # the root and every child
    for w in (2, 8, 64):
        got = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), window=w, **kw)
        assert got["rc"] == 0
        same_result(got, ref)
        same_counters(got, ref)


def test_prop_0_is_the_parent(orc, tab):
    for case in [(10, 20, 4, 3), ("setcover", 40, 60, 3)]:
        for kw in (dict(window=1), dict(window=64), dict(node_strat=1), dict(heur=2, cut_strat=1, rc_fix=1)):
            a = bnb.branch_and_bound(lpgen.load_case(orc, case), table=tab, quirks=0, **kw)
            z = bnb.branch_and_bound(lpgen.load_case(orc, case), table=tab, quirks=0, prop=0, **kw)
            same_result(z, a)
            same_counters(z, a)
            assert (z["prop_calls"], z["prop_fixed"], z["prop_tightened"], z["prop_infeasible"]) == (0, 0, 0, 0)
    assert bnb.make_params().prop == 0


def test_the_callers_handle_is_left_as_it_was(orc, tab):
    P = lpgen.load_case(orc, TIGHT)
    before = [(orc.get_col_type(P.h, j), orc.get_col_lb(P.h, j), orc.get_col_ub(P.h, j)) for j in range(1, P.n + 1)]
    r = bnb.branch_and_bound(P, quirks=0, table=tab, window=1, prop=8)
    assert r["rc"] == 0 and r["prop_fixed"] > 0
    assert before == [(orc.get_col_type(P.h, j), orc.get_col_lb(P.h, j), orc.get_col_ub(P.h, j)) for j in range(1, P.n + 1)]


def test_an_infeasible_root_is_booked_without_a_solve(orc, tab):
    """2 x1 + 2 x2 = 3 over integers in [0, 3]: the LP is feasible, the propagation crosses a column's bounds.  Booked exactly
    as an integer column whose range holds no integer is."""
    for direction, inf in ((capi.MAX, -INF), (capi.MIN, INF)):
        P = orc.create()
        P.load_general(np.array([[2.0, 2.0]]), [(FX, 3.0, 3.0)], [(DB, 0.0, 1.0), (DB, 0.0, 1.0)], [1.0, 1.0], kinds=[IV, IV], direction=direction)
        rc, (infeasible, rounds, lst) = bnb.propagate_node(P, P, 8, table=tab)
        assert (rc, infeasible, lst) == (0, 1, [])
        for kw in (dict(window=1), dict(window=64), dict(node_strat=1)):
            r = bnb.branch_and_bound(P, quirks=0, table=tab, prop=8, **kw)
            assert (r["rc"], r["count"], r["has_incumbent"], r["n_nodes"], r["prune"], r["total_pivots"]) == (0, 0, 0, 1, [1], 0)
            assert r["best_lower"] == inf and r["events"] == []
            assert (r["prop_calls"], r["prop_infeasible"], r["prop_fixed"], r["prop_tightened"]) == (1, 1, 0, 0)
        Q = orc.create()  # the rounding rule's own case, for comparison
        Q.load_general(np.array([[1.0, 1.0]]), [(UP, 0.0, 9.0)], [(DB, 1.25, 1.75), (DB, 0.0, 3.0)], [1.0, 1.0], kinds=[IV, IV], direction=direction)
        q = bnb.branch_and_bound(Q, quirks=0, table=tab, window=1)
        r = bnb.branch_and_bound(P, quirks=0, table=tab, window=1, prop=8)
        for k in ("count", "has_incumbent", "n_nodes", "prune", "total_pivots", "events", "best_lower", "parent", "hit_limit"):
            assert r[k] == q[k], k


def test_refusals_and_return_codes(orc, tab):
    from mvolps_amd import dist_bnb, dist_native

    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    for kw in (dict(prop=17, quirks=0), dict(prop=-1, quirks=0), dict(prop=8, quirks=1), dict(prop=8),
               dict(prop=8, quirks=0, node_strat=1, best_window=8), dict(prop=1, quirks=0, best_window=1)):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, **kw)
        assert r["rc"] == -1 and r["n_nodes"] == 0 and r["count"] == 0, kw
    for k in (1, 16):
        assert bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0, prop=k)["rc"] == 0
    P = lpgen.load_ilp(orc, A, b, c, U)
    with pytest.raises(ValueError):
        dist_native.branch_and_bound(P, table=tab, prop=8, quirks=0)
    with pytest.raises(ValueError):
        dist_bnb.branch_and_bound(None, P, prop=8, quirks=0)
    pr = bnb.make_params(quirks=0, prop=8)
    L = dist_native._lib()
    res, st = bnb.BnbResult(), dist_native.DistStats()
    tptr = bnb.C.cast(bnb.C.pointer(tab), bnb.C.c_void_p)
    assert L.mvx_branchAndBound_dist(tptr, None, P.h, bnb.C.byref(pr), None, None, bnb.C.byref(res), bnb.C.byref(st)) == capi.EFAIL
    # neither propagate_many nor the twin's accessors: an error, not a run without the rule
    for missing in ("get_mat_row", "get_col_kind", "get_row_ub"):
        bare = bnb.table_from(orc)
        setattr(bare, missing, None)
        assert bnb.propagate_node(P, P, 8, table=bare)[0] == -2
        if missing == "get_mat_row":
            for kw in (dict(window=1), dict(window=64)):
                r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bare, prop=8, quirks=0, **kw)
                assert r["rc"] == -2 and r["count"] == 0 and r["has_incumbent"] == 0 and r["n_nodes"] == 1, kw
    # mvx_bnb_propagate's own codes
    assert bnb.propagate_node(P, P, 8, table=tab)[0] == 0  # never solved: it need not be
    assert bnb.propagate_node(P, P, 0, table=tab)[0] == -1
    A2, b2, c2, U2 = synth.dense_ilp(8, 15, 3, 2)
    assert bnb.propagate_node(lpgen.load_ilp(orc, A2, b2, c2, U2), P, 8, table=tab)[0] == -1  # another column count


def test_fewer_nodes_on_a_tight_binary_instance(orc, tab):
    A, b, c, U = synth.dense_ilp(*TIGHT)
    assert U == 1 and np.all(np.abs(b - 21) <= 4)  # about twice the mean coefficient, 10.5
    off = bnb.branch_and_bound(lpgen.load_case(orc, TIGHT), table=tab, quirks=0)
    on = bnb.branch_and_bound(lpgen.load_case(orc, TIGHT), table=tab, quirks=0, prop=8)
    assert off["rc"] == on["rc"] == 0 and off["hit_limit"] == on["hit_limit"] == 0
    # integer data and an integral point: both optima are the same integer, each up to its own LP's rounding
    z = round(off["best_lower"])
    assert on["has_incumbent"] and abs(on["best_lower"] - z) <= 1e-9 * (1 + abs(z)) and abs(off["best_lower"] - z) <= 1e-9 * (1 + abs(z))
    assert (off["count"], on["count"]) == TIGHT_COUNTS and on["count"] < off["count"]
    assert on["prop_fixed"] > 0 and on["prop_calls"] == on["n_nodes"]  # the root and every child


@pytest.mark.parametrize("case", DENSE, ids=str)
def test_no_more_nodes_on_the_dense_cases(orc, tab, case):
    off = bnb.branch_and_bound(lpgen.load_case(orc, case), table=tab, quirks=0)
    on = bnb.branch_and_bound(lpgen.load_case(orc, case), table=tab, quirks=0, prop=8)
    assert on["rc"] == off["rc"] == 0 and on["hit_limit"] == 0
    assert abs(on["best_lower"] - HIGHS[case]) <= 1e-6 * (1 + abs(HIGHS[case]))
    assert on["count"] <= off["count"], (on["count"], off["count"])
