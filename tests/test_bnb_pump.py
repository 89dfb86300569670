"""CPU: the feasibility pump (DESIGN.md "Feasibility pump") over the ORACLE's table, so the host twins run: mvx_bnb_pump_obj for the
rounding and the distance objective, set_obj_coef per changed column for the objective apply (the oracle's table has no
set_obj_many), the oracle's simplex for the distance LPs, mvx_bnb_round for the integral ends.

The step twin is checked with == against a plain-Python restatement of the definition built from the test's own arrays; whole
pumps against a restatement written with the oracle's copy / set_obj_coef / simplex; hand-made models pin the tie rule of the
stall move and each way a pump can end; the points the pumps find on the enumerated fixture are feasible and no better than the
pinned optimum; the caller's handle is left as it was; the return codes are pinned."""
import math

import numpy as np
import pytest

from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import CV, DB, FR, FX, IV, LO, MAX, MIN, OPT, UP

from . import lpgen
from .test_bnb_branching import HIGHS
from .test_bnb_dive import COUNTERS as DIVE_COUNTERS
from .test_bnb_dive import TREE_OPTIONS, case_model, col_range, general_model, ilp_model, milp_model, solved_root, tie_model
from .test_bnb_general import INSTANCES, check_pin, failures, instance, run
from .test_bnb_host import same_result

ALPHAS = (0.0, 0.9)
PUMP_COUNTERS = ("pump_calls", "pump_found", "pump_improved", "pump_lps", "pump_pivots")
COUNTERS = DIVE_COUNTERS + PUMP_COUNTERS
ENDS = bnb.PUMP_ENDS
FOUND_MEASURED = 147  # test_fixture_roots, alpha = 0, over the oracle's table
FOUND_FLOOR = int(0.85 * FOUND_MEASURED)


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    assert t.set_obj_coef and not t.set_obj_many and not t.pump_obj_many and not t.round_many  # the host twins run over the oracle
    return t


def py_pump_obj(M, v, lo, hi, xprev, a, q):
    """The definition of the step, one operation at a time on Python floats, arrays 1-based like the twin's:
    ((nfrac, moved, stalled, nnz), xt, c)."""
    n = M.n
    xt, L, U = [0.0] * (n + 1), [0.0] * (n + 1), [0.0] * (n + 1)
    ints = [j for j in range(1, n + 1) if M.isint[j - 1]]
    nfrac = 0
    for j in ints:
        t = float(v[j - 1])
        nfrac += abs(t - float(np.rint(t))) > 1e-9
        L[j], U[j] = float(math.ceil(lo[j - 1])) if math.isfinite(lo[j - 1]) else lo[j - 1], float(math.floor(hi[j - 1])) if math.isfinite(hi[j - 1]) else hi[j - 1]
        xt[j] = min(max(float(math.floor(t + 0.5)), L[j]), U[j])
    moved, stall = 0, xprev is not None and all(xt[j] == xprev[j] for j in ints)
    if stall:
        movable = []
        for j in ints:
            d = float(v[j - 1]) - xt[j]
            s = 1.0 if d > 0 else -1.0
            if abs(d) > 0 and L[j] <= xt[j] + s <= U[j]:
                movable.append((-abs(d), j, s))
        for _key, j, s in sorted(movable)[:10]:  # the largest distances, ties to the lowest column
            xt[j] += s
            moved += 1
    d = [0.0] * (n + 1)
    for j in ints:
        df = float(v[j - 1]) - xt[j]
        d[j] = 0.0 if L[j] == U[j] else 1.0 if xt[j] == L[j] else -1.0 if xt[j] == U[j] else 1.0 if df > 0 else -1.0 if df < 0 else 0.0
    nnz = sum(1 for t in d if t != 0.0)
    b = q * math.sqrt(float(nnz))
    c = [0.0] + [(a * (-M.sg * d[j])) + (b * M.c[j - 1]) for j in range(1, n + 1)]
    return (int(nfrac), moved, int(stall and moved == 0), nnz), xt, c


def node_bounds(orc, node):
    r = [col_range(orc, node, j) for j in range(1, node.n + 1)]
    return [t[0] for t in r], [t[1] for t in r]


def weights(M, alpha_k):
    s = 0.0
    for t in M.c:
        s = s + t * t
    norm = math.sqrt(s)
    return 1.0 - alpha_k, (alpha_k / norm if norm > 0.0 else 0.0)


def check_step(orc, tab, M, root, node, xprev=None, alpha_k=0.0):
    lo, hi = node_bounds(orc, node)
    ab = weights(M, alpha_k)
    want = py_pump_obj(M, node.col_prim(), lo, hi, xprev, *ab)
    rc, info, xt, c = bnb.pump_obj_node(node, root, xprev=xprev, ab=ab, table=tab)
    assert rc == 0 and tuple(int(t) for t in info) == want[0], (info, want[0])
    assert np.array_equal(xt, want[1]) and np.array_equal(c, want[2])
    return want


def check_steps(orc, tab, M, root, node, seen=None):
    """The plain step, the weighted step, and the step against its own rounding (the stall move)."""
    for alpha_k in ALPHAS:
        info, xt, _c = check_step(orc, tab, M, root, node, None, alpha_k)
        again = check_step(orc, tab, M, root, node, xt, alpha_k)
        if seen is not None:
            seen.add(("moved", again[0][1] > 0))
            seen.add(("stalled", again[0][2]))
    return info[0]


def test_step_twin_matches_the_restatement_mixed_rows(orc, tab):
    rng = np.random.default_rng(11)
    seen, checked, fractional, continuous = set(), 0, 0, 0
    for _ in range(120):
        A, row_b, col_b, c, d = lpgen.random_general_lp(rng, 10, 12)
        kinds = [IV if rng.random() < 0.7 else CV for _ in c]
        root = orc.create()
        root.load_general(A, row_b, col_b, c, kinds=kinds, direction=d)
        node = root.copy()
        node.simplex()
        if node.status != OPT:
            continue
        seen |= {("col", t) for t, _, _ in col_b} | {("sense", d)}
        continuous += int(CV in kinds)
        fractional += check_steps(orc, tab, general_model(A, row_b, c, kinds, d), root, node, seen) > 0
        checked += 1
    assert checked > 40 and fractional > 20, (checked, fractional)
    assert {("col", t) for t in (LO, UP, DB, FX, FR)} <= seen and {("sense", MIN), ("sense", MAX)} <= seen
    assert {("moved", True), ("moved", False), ("stalled", 1), ("stalled", 0)} <= seen and continuous > 20


def test_step_twin_matches_the_restatement_on_children(orc, tab):
    """Nodes with tightened column bounds: the bounds are the node's, the flags and the objective the root's."""
    A, b, c, U = synth.dense_ilp(12, 24, 5, 3)
    M = ilp_model(A, b, c)
    root = lpgen.load_ilp(orc, A, b, c, U)
    queue, done = [root.copy()], 0
    while queue and done < 12:
        P = queue.pop(0)
        P.simplex()
        if P.status != OPT:
            continue
        check_steps(orc, tab, M, root, P)
        done += 1
        _st, viol = bnb.print_info(P, quirks=0, table=tab)
        if viol:
            queue += list(bnb.make_children(P, viol[0], quirks=0, table=tab))
    assert done >= 8


def test_the_stall_move_takes_the_lowest_columns_of_a_tie(orc, tab):
    """300 columns at 0.5, every distance 0.5: a repeated rounding moves columns 1..10 and no other.  With 4 x_300 <= 1 the last
    column is at 0.25, rounds down and lies nearer: it does not move either."""
    for last in (2.0, 4.0):
        M, root, node = tie_model(orc, last=last)
        info, xt, _c = check_step(orc, tab, M, root, node)
        assert info == (300, 0, 0, 300) and xt[1:300] == [1.0] * 299 and xt[300] == (1.0 if last == 2.0 else 0.0)
        info2, xt2, c2 = check_step(orc, tab, M, root, node, xt)
        assert info2[:3] == (300, 10, 0) and xt2[1:11] == [0.0] * 10 and xt2[11:] == xt[11:]
        assert c2[1:11] == [-1.0] * 10 and c2[11:300] == [1.0] * 289  # maximising: towards 0 costs, towards 1 pays


# ------------------------------------------------------------------------------------------------ whole pumps

def py_pump(orc, tab, M, root, node, iters, alpha):
    """One pump, written with the oracle's copy / set_obj_coef / simplex: (end, found, obj, x, lps, pivots)."""
    cur, hist, k, alpha_k, lps, piv = node.copy(), [], 0, alpha, 0, 0
    while True:
        lo, hi = node_bounds(orc, cur)
        info, xt, c = py_pump_obj(M, cur.col_prim(), lo, hi, hist[-1] if hist else None, *weights(M, alpha_k))
        if info[0] == 0:
            rc, obj, found, x = bnb.round_node(cur, root, 1, table=tab)
            assert rc == 0
            return "integral", found, obj, x, lps, piv
        if k == iters:
            return "limit", 0, 0.0, None, lps, piv
        if info[2]:
            return "stalled", 0, 0.0, None, lps, piv
        if info[1] > 0 and xt in hist:
            return "cycle", 0, 0.0, None, lps, piv
        hist.append(xt)
        for j in range(M.n + 1):
            if orc.get_obj_coef(cur.h, j) != c[j]:
                orc.set_obj_coef(cur.h, j, c[j])
        before = cur.it_cnt
        cur.simplex()
        lps, piv, k, alpha_k = lps + 1, piv + cur.it_cnt - before, k + 1, alpha_k * 0.9
        if cur.status != OPT:
            return "failed", 0, 0.0, None, lps, piv


def check_pump(orc, tab, M, root, node, iters=30, alpha=0.0, stats=None):
    rc, obj, found, x, lps, piv, end = bnb.pump_node(node, root, iters, alpha, table=tab)
    want = py_pump(orc, tab, M, root, node, iters, alpha)
    assert rc == 0 and (ENDS[end], found, lps, piv) == (want[0], want[1], want[4], want[5]), ((ENDS[end], found, lps, piv), want)
    if found:
        assert obj == want[2] and np.array_equal(x[1:], want[3][1:])
    if stats is not None:
        stats[want[0]] = stats.get(want[0], 0) + 1
    return want[0], found, obj, x, lps


def test_whole_pumps_match_the_restatement_mixed_rows(orc, tab):
    rng = np.random.default_rng(23)
    stats, checked = {}, 0
    for _ in range(80):
        A, row_b, col_b, c, d = lpgen.random_general_lp(rng, 10, 12)
        kinds = [IV if rng.random() < 0.7 else CV for _ in c]
        P = orc.create()
        P.load_general(A, row_b, col_b, c, kinds=kinds, direction=d)
        got = solved_root(orc, tab, P)
        if got is None or got[1].status != OPT:
            continue
        for alpha in ALPHAS:
            check_pump(orc, tab, general_model(A, row_b, c, kinds, d), got[0], got[1], 30, alpha, stats)
        checked += 1
    print("mixed rows", checked, stats)
    assert checked > 30 and stats.get("integral", 0) > 20 and {"cycle", "failed", "limit"} <= set(stats), stats


@pytest.mark.parametrize("case", list(HIGHS), ids=str)
def test_whole_pumps_match_the_restatement_on_children(orc, tab, case):
    root, node = solved_root(orc, tab, lpgen.load_case(orc, case))
    M = case_model(case)
    queue, done, stats = [node], 0, {}
    while queue and done < 5:
        P = queue.pop(0)
        if P.status != OPT:
            continue
        for alpha in ALPHAS:
            check_pump(orc, tab, M, root, P, 30, alpha, stats)
        check_pump(orc, tab, M, root, P, 1, 0.0, stats)
        done += 1
        _st, viol = bnb.print_info(P, quirks=0, table=tab)
        if viol:
            kids = bnb.make_children(P, viol[0], quirks=0, table=tab)
            for k in kids:
                k.simplex()
            queue += list(kids)
    assert done >= 1


def test_whole_pumps_match_the_restatement_on_the_fixture(orc, tab):
    ran, stats = [], {}

    def one(rec):
        inst = instance(rec)
        got = solved_root(orc, tab, lpgen.load_milp(orc, inst))
        if got is None or got[1].status != OPT:
            return
        for alpha in ALPHAS:
            check_pump(orc, tab, milp_model(inst), got[0], got[1], 30, alpha, stats)
        ran.append(rec["index"])

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)
    assert len(ran) >= 20


# ------------------------------------------------------------------------------------------------ how a pump ends

def load(orc, A, row_b, col_b, c, kinds, direction):
    root = orc.create()
    root.load_general(np.array(A, dtype=float), row_b, col_b, c, kinds=kinds, direction=direction)
    node = root.copy()
    node.simplex()
    assert node.status == OPT
    return general_model(np.array(A, dtype=float), row_b, c, kinds, direction), root, node


def test_a_pump_that_ends_integral(orc, tab):
    M, root, node = load(orc, [[1.0, 1.0]], [(UP, 0.0, 3.0)], [(DB, 0.0, 2.0)] * 2, [2.0, 1.0], [IV, IV], MAX)
    end, found, obj, x, lps = check_pump(orc, tab, M, root, node)
    assert (end, found, obj, lps) == ("integral", 1, 5.0, 0) and list(x[1:]) == [2.0, 1.0]


def test_a_pump_that_stalls(orc, tab):
    """max x, x <= 1.5 an integer column with its bound unrounded: the rounding is 1 (clamped), the distance LP leads back to
    1.5, the rounding repeats and 1 + 1 lies outside the clamped bounds: nothing to move."""
    M, root, node = load(orc, [[1.0]], [(UP, 0.0, 10.0)], [(DB, 0.0, 1.5)], [1.0], [IV], MAX)
    end, found, _obj, _x, lps = check_pump(orc, tab, M, root, node)
    assert (end, found, lps) == ("stalled", 0, 1)


def test_a_pump_that_cycles(orc, tab):
    """max 3 x1 + 2 x2 + 2 x3, 3 x1 + 2 x2 + 2 x3 <= 9, 5 x1 + 2 x2 + x3 <= 7, x in {0..3}: after two distance LPs a
    repeated rounding is moved onto a rounding the pump has already tried."""
    M, root, node = load(orc, [[3.0, 2.0, 2.0], [5.0, 2.0, 1.0]], [(UP, 0.0, 9.0), (UP, 0.0, 7.0)], [(DB, 0.0, 3.0)] * 3, [3.0, 2.0, 2.0],
                         [IV] * 3, MAX)
    end, found, _obj, _x, lps = check_pump(orc, tab, M, root, node)
    assert (end, found, lps) == ("cycle", 0, 2)


def test_a_pump_whose_distance_lp_is_unbounded(orc, tab):
    """min x over x >= 0.6, x a free integer column: the rounding is 1, the distance objective pushes x up for ever."""
    M, root, node = load(orc, [[1.0]], [(LO, 0.6, 0.0)], [(FR, 0.0, 0.0)], [1.0], [IV], MIN)
    end, found, _obj, _x, lps = check_pump(orc, tab, M, root, node)
    assert (end, found, lps) == ("failed", 0, 1)


def test_a_pump_that_reaches_its_limit(orc, tab):
    A, b, c, U = synth.dense_ilp(40, 80, 3, 3)
    root, node = solved_root(orc, tab, lpgen.load_ilp(orc, A, b, c, U))
    M = ilp_model(A, b, c)
    full = check_pump(orc, tab, M, root, node, 30)
    assert full[0] == "integral" and full[1] == 1 and full[4] >= 2
    short = check_pump(orc, tab, M, root, node, full[4] - 1)
    assert short[0] == "limit" and short[1] == 0 and short[4] == full[4] - 1


def test_fixture_roots(orc, tab):
    """Every fixture instance whose integer-rounded root solves OPT, the root pump with alpha 0 and 0.9: nothing, or a point that
    is exactly integral, within the root's rows and bounds, priced with the root's objective and no better than the enumerated
    optimum; nothing on a model without one.  Measured over the oracle's table: 259 roots, 147 points for alpha = 0
    (149 pumps end integral, 95 cycle, 15 limit) and 107 for alpha = 0.9 (109 integral, 145 cycle, 5 limit); the floor asserted for
    alpha = 0 is 0.85 times its count, the margin the dives' fixture test takes."""
    roots, stats = 0, {a: {} for a in ALPHAS}
    found_by = {a: 0 for a in ALPHAS}

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
        for alpha in ALPHAS:
            _end, found, obj, x, _lps = check_pump(orc, tab, M, root, node, 30, alpha, stats[alpha])
            if not found:
                continue
            assert rec["status"] == "optimal", "a point on a model without one"
            found_by[alpha] += 1
            x = x[1:]
            assert np.array_equal(x[isint], np.round(x[isint]))
            act = A @ x
            assert np.all(act >= rlo - 1e-9 * np.maximum(1, np.abs(rlo))) and np.all(act <= rhi + 1e-9 * np.maximum(1, np.abs(rhi)))
            assert np.all(x >= clo) and np.all(x <= chi)
            assert abs(float(c @ x) + c0 - obj) <= 1e-9 * (1 + abs(obj))
            assert M.sg * obj <= M.sg * rec["optimum"] + 1e-6 * (1 + abs(rec["optimum"])), (alpha, obj, rec["optimum"])

    bad = failures(INSTANCES, one)
    assert not bad, "%d fail:\n%s" % (len(bad), "\n".join(bad))
    print("roots", roots, "found", found_by, "ends", stats)
    assert roots >= 240 and found_by[0.0] >= FOUND_FLOOR, (roots, found_by)


# ------------------------------------------------------------------------------------------------ trees

@pytest.mark.parametrize("family", "abcd")
@pytest.mark.parametrize("name", list(TREE_OPTIONS))
def test_trees_close_on_the_enumerated_optimum(orc, tab, name, family):
    recs = [r for r in INSTANCES if r["family"] == family]
    assert len(recs) >= 25
    ran = []

    def one(rec):
        inst = instance(rec)
        r = run(orc, rec, inst, table=tab, pump=30, pump_freq=1, pump_alpha=0.5 if rec["index"] % 2 else 0.0, **TREE_OPTIONS[name])
        check_pin(rec, inst, r)
        ran.append(r["pump_calls"])

    bad = failures(recs, one)
    assert not bad, "%d of %d fail:\n%s" % (len(bad), len(recs), "\n".join(bad))
    if family in "ab":
        assert sum(1 for c in ran if c > 0) >= 20  # the pumps ran


def same_counters(a, b):
    for k in COUNTERS:
        assert a[k] == b[k], k


@pytest.mark.parametrize("extra", [dict(), dict(heur=2), dict(dive=7, dive_freq=3), dict(rc_fix=1), dict(cut_strat=1),
                                   dict(heur=2, dive=7, dive_freq=4, rc_fix=1, cut_strat=1, prop=8)], ids=str)
def test_windows_equal_serial(orc, tab, extra):
    A, b, c, U = synth.dense_ilp(10, 20, 4, 3)
    kw = dict(quirks=0, max_nodes=400, table=tab, pump=30, pump_freq=3, pump_alpha=0.3, **extra)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), window=1, **kw)
    assert ref["rc"] == 0 and ref["count"] > 50 and ref["pump_calls"] > 5 and ref["pump_found"] > 0
    assert ref["pump_lps"] > 0 and ref["pump_pivots"] > 0
    for w in (2, 8, 64):
        got = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), window=w, **kw)
        assert got["rc"] == 0
        same_result(got, ref)
        same_counters(got, ref)


def test_windows_give_the_serial_tree_on_the_fixture(orc, tab):
    recs = INSTANCES[::10]

    def one(rec):
        inst = instance(rec)
        for extra in (dict(), dict(heur=2, rc_fix=1, dive=1), dict(cut_strat=1)):
            ref = run(orc, rec, inst, table=tab, window=1, pump=30, pump_freq=3, **extra)
            for w in (2, 8, 64):
                got = run(orc, rec, inst, table=tab, window=w, pump=30, pump_freq=3, **extra)
                same_result(got, ref)
                same_counters(got, ref)

    bad = failures(recs, one)
    assert not bad, "\n".join(bad)


def test_the_root_pump_gives_the_first_incumbent(orc, tab):
    A, b, c, U = synth.dense_ilp(40, 80, 3, 3)
    r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0, max_nodes=1, pump=30)
    assert r["rc"] == 0 and r["has_incumbent"] and r["incumbent_heur"] == 3
    assert (r["pump_calls"], r["pump_found"], r["pump_improved"]) == (1, 1, 1) and r["pump_lps"] >= 1
    x = np.array(r["x"])
    assert np.array_equal(x, np.round(x)) and (x >= 0).all() and (x <= U).all() and (A @ x <= b).all() and float(c @ x) == r["best_lower"]
    both = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0, max_nodes=1, pump=30, dive=7)
    assert both["incumbent_heur"] == 2 and both["pump_improved"] == 1 and both["best_lower"] > r["best_lower"]  # the dive comes behind


def test_pump_0_is_the_parent(orc, tab):
    for case in [(10, 20, 4, 3), ("setcover", 40, 60, 3)]:
        for kw in (dict(window=1), dict(window=64), dict(node_strat=1), dict(heur=2, cut_strat=1, rc_fix=1, prop=8, dive=7)):
            a = bnb.branch_and_bound(lpgen.load_case(orc, case), table=tab, quirks=0, **kw)
            z = bnb.branch_and_bound(lpgen.load_case(orc, case), table=tab, quirks=0, pump=0, pump_freq=5, pump_alpha=0.7, **kw)
            assert {k: v for k, v in z.items() if k not in PUMP_COUNTERS} == {k: v for k, v in a.items() if k not in PUMP_COUNTERS}
            assert [z[k] for k in PUMP_COUNTERS] == [0] * 5 == [a[k] for k in PUMP_COUNTERS]
    pr = bnb.make_params()
    assert (pr.pump, pr.pump_freq, pr.pump_alpha) == (0, 0, 0.0)
    # bug-compatible mode never sees the new fields
    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    assert bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, pump_freq=3, pump_alpha=1.0)["rc"] == 0


def test_refusals(orc, tab):
    from mvolps_amd import dist_bnb, dist_native

    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    for kw in (dict(pump=1001, quirks=0), dict(pump=-1, quirks=0), dict(pump=30, quirks=1), dict(pump=30), dict(pump=1, quirks=0, pump_freq=-1),
               dict(pump=1, quirks=0, pump_alpha=-0.1), dict(pump=1, quirks=0, pump_alpha=1.1), dict(pump=0, quirks=0, pump_alpha=2.0),
               dict(pump=30, quirks=0, node_strat=1, best_window=8), dict(pump=1, quirks=0, best_window=1)):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, **kw)
        assert r["rc"] == -1 and r["n_nodes"] == 0 and r["count"] == 0, kw
    for p in (1, 1000):
        assert bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0, pump=p, pump_freq=2, pump_alpha=1.0)["rc"] == 0
    assert bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0, pump=30, node_strat=1)["rc"] == 0  # BEST, serial
    P = lpgen.load_ilp(orc, A, b, c, U)
    with pytest.raises(ValueError):
        dist_native.branch_and_bound(P, table=tab, pump=30, quirks=0)
    with pytest.raises(ValueError):
        dist_bnb.branch_and_bound(None, P, pump=30, quirks=0)
    pr = bnb.make_params(quirks=0, pump=30)
    L = dist_native._lib()
    res, st = bnb.BnbResult(), dist_native.DistStats()
    tptr = bnb.C.cast(bnb.C.pointer(tab), bnb.C.c_void_p)
    assert L.mvx_branchAndBound_dist(tptr, None, P.h, bnb.C.byref(pr), None, None, bnb.C.byref(res), bnb.C.byref(st)) == capi.EFAIL
    # a pump that cannot run: an error with the tree so far, not a run without the pumps
    for missing in ("get_mat_row", "set_obj_coef"):
        bare = bnb.table_from(orc)
        setattr(bare, missing, None)
        for kw in (dict(window=1), dict(window=64), dict(node_strat=1)):
            r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bare, pump=30, quirks=0, **kw)
            assert r["rc"] == -2 and r["count"] == 0 and r["has_incumbent"] == 0 and r["n_nodes"] == 1, (missing, kw)


def test_the_callers_handle_is_left_as_it_was(orc, tab):
    A, b, c, U = synth.dense_ilp(10, 20, 4, 3)
    root, node = solved_root(orc, tab, lpgen.load_ilp(orc, A, b, c, U))

    def model(P):
        return [orc.get_obj_coef(P.h, j) for j in range(P.n + 1)], P.status, P.it_cnt, P.obj

    def state(P):
        return model(P), P.tableau().tolist(), [a.tolist() for a in P.basis()]

    before = state(node), model(root)
    rc, _obj, _found, _x, lps, _piv, _end = bnb.pump_node(node, root, 30, 0.5, table=tab)
    assert rc == 0 and lps > 0
    assert bnb.pump_obj_node(node, root, table=tab)[0] == 0
    assert (state(node), model(root)) == before
    before = model(root)
    r = bnb.branch_and_bound(root, quirks=0, table=tab, window=1, pump=30, pump_freq=2)
    assert r["rc"] == 0 and r["pump_lps"] > 0
    assert model(root) == before


def test_return_codes(orc, tab):
    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    P = lpgen.load_ilp(orc, A, b, c, U)
    node = P.copy()
    node.simplex()
    assert node.status == OPT
    assert bnb.pump_obj_node(P, P, table=tab)[0] == -3 and bnb.pump_node(P, P, table=tab)[0] == -3  # never solved
    for iters, alpha in ((0, 0.0), (-1, 0.0), (1001, 0.0), (30, -0.1), (30, 1.5), (30, math.nan)):
        assert bnb.pump_node(node, P, iters, alpha, table=tab)[0] == -1, (iters, alpha)
    assert bnb.pump_node(node, P, 1000, 1.0, table=tab)[0] == 0
    A2, b2, c2, U2 = synth.dense_ilp(8, 15, 3, 2)
    other = lpgen.load_ilp(orc, A2, b2, c2, U2)
    assert bnb.pump_obj_node(node, other, table=tab)[0] == -1 and bnb.pump_node(node, other, table=tab)[0] == -1  # another column count
    for missing in ("get_mat_row", "get_col_kind", "get_row_ub", "get_obj_coef"):
        bare = bnb.table_from(orc)
        setattr(bare, missing, None)
        assert bnb.pump_obj_node(node, P, table=bare)[0] == -2 and bnb.pump_node(node, P, table=bare)[0] == -2
    bare = bnb.table_from(orc)  # no way to change an objective
    bare.set_obj_coef = None
    assert bnb.pump_obj_node(node, P, table=bare)[0] == 0 and bnb.pump_node(node, P, table=bare)[0] == -2
