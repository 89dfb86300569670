"""CPU: whole B&B trees on general mixed-integer models (lpgen.random_general_milp: continuous columns, FR / UP / LO / FX / DB
columns with negative and half-integer bounds, ranged / equality / free rows, a constant term, both directions, LP-infeasible
and integer-infeasible members), driver over the ORACLE's table, repaired mode.

The pins of tests/golden/general_milp.json come from enumeration (tests/milp_enum.py), which shares nothing with the driver,
the oracle's restatement or the host twins.  Every kept instance must close on its pin under every option set; windows must
give the serial tree; and the host twins, the penalties and the repaired GMI cuts are checked once more on tree nodes of
these models instead of solved roots."""
import json
import math
import os

import numpy as np
import pytest

from mvolps_amd import bnb, capi
from mvolps_amd.capi import CV, IV, LO, MAX, MIN, NOFEAS, OPT, UNBND

from . import certify as cf
from . import lpgen
from .test_bnb_branching import check_twin as penalties_twin
from .test_bnb_heuristic import Model as RoundModel
from .test_bnb_heuristic import check_twin as round_twin
from .test_bnb_host import same_result
from .test_bnb_rcfix import check_twin as rc_twin
from .test_bnb_rcfix import forced_beyond, sense

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "general_milp.json")))
HEAD, DRAWN = GOLDEN["header"], GOLDEN["instances"]
INSTANCES = DRAWN + GOLDEN["named_instances"]  # the drawn family, then the members kept by name (other seeds)

# name -> branch_and_bound keywords (quirks=0 and the oracle's table are added by run())
OPTIONS = {
    "serial": dict(window=1),
    "window64": dict(window=64),
    "best": dict(node_strat=1, window=1),
    "best_window8": dict(node_strat=1, best_window=8),
    "heur2": dict(window=1, heur=2),
    "heur2_rcfix": dict(window=1, heur=2, rc_fix=1),
    "heur2_rcfix_window64": dict(window=64, heur=2, rc_fix=1),
    "cuts": dict(window=1, cut_strat=1),
    "cuts_select": dict(window=1, cut_strat=1, cut_select=1),
    "cuts_heur2_rcfix_window64": dict(window=64, cut_strat=1, heur=2, rc_fix=1),
    "var1": dict(window=1, var_strat=1),
    "var2": dict(window=1, var_strat=2),
    "var3": dict(window=1, var_strat=3),
    "var4": dict(window=1, var_strat=4),
}


@pytest.fixture(scope="module")
def tab(orc):
    return bnb.table_from(orc)


def instance(rec):
    """The model of a fixture record, regenerated from the seed; a changed stream fails here."""
    inst = lpgen.random_general_milp(rec.get("seed", HEAD["seed"]), rec["index"])
    assert lpgen.milp_sha256(inst) == rec["sha256"], "instance %d is not the model the fixture pinned" % rec["index"]
    return inst


def max_nodes(rec):
    # every branching splits an integer column's LP range, so a tree that terminates has about twice as many nodes as the
    # box has points at the most; the factor only turns a tree that never closes into a failure instead of a hung test
    return 50 * rec["points"] + 1000


def run(api, rec, inst, table=None, **kw):
    return bnb.branch_and_bound(lpgen.load_milp(api, inst), quirks=0, table=table, max_nodes=max_nodes(rec), **kw)


def check_incumbent(inst, r):
    """The incumbent against the test's own arrays: integer columns integral, rows and columns within bounds, c x + c0 the
    reported value.  A heuristic point meets its tests exactly; an integral node LP's vertex within the LP tolerances."""
    A, rlo, rhi, clo, chi, c, c0, isint, _mx = lpgen.milp_arrays(inst)
    x = np.array(r["x"])
    exact = r["incumbent_heur"] == 1
    if isint.any():
        assert np.abs(x[isint] - np.round(x[isint])).max() <= (0.0 if exact else 1e-9)
    act = A @ x
    e = 1e-9 if exact else 1e-7
    assert np.all(act >= rlo - e * np.maximum(1, np.abs(rlo))) and np.all(act <= rhi + e * np.maximum(1, np.abs(rhi)))
    e = 0.0 if exact else 1e-9
    assert np.all(x >= clo - e) and np.all(x <= chi + e)
    obj = float(c @ x) + c0
    assert abs(obj - r["best_lower"]) <= 1e-9 * (1 + abs(obj))


def check_pin(rec, inst, r):
    assert r["rc"] == 0 and r["hit_limit"] == 0, (r["rc"], r["hit_limit"], r["count"])
    if rec["status"] == "optimal":
        pin = rec["optimum"]
        assert r["has_incumbent"], "no incumbent; the optimum is %r" % pin
        assert abs(r["best_lower"] - pin) <= 1e-6 * (1 + abs(pin)), (r["best_lower"], pin)
        check_incumbent(inst, r)
    else:
        assert not r["has_incumbent"], "incumbent %r on an infeasible model" % r["best_lower"]


def failures(recs, fn):
    """fn on every record; the failures by index (all of them are shown, none is tolerated)."""
    bad = []
    for rec in recs:
        try:
            fn(rec)
        except AssertionError as e:  # noqa: PERF203
            bad.append("instance %d (%s, %dx%d): %s" % (rec["index"], rec["family"], rec["m"], rec["n"], str(e).splitlines()[0][:200]))
    return bad


# ------------------------------------------------------------------------------------------------ the fixture itself


def test_fixture_meets_its_conditions():
    kept = HEAD["kept"]
    assert kept == len(DRAWN) >= 240 and HEAD["named"] == len(GOLDEN["named_instances"]) == 2
    assert all(HEAD["kept_by_family"][f] >= 25 for f in "bcd")
    assert HEAD["kept_d_with_feasible_relaxation"] >= 25
    assert all(HEAD["kept_by_direction"][d] >= 0.4 * kept for d in ("min", "max"))
    assert HEAD["kept_pure"] >= 60 and HEAD["kept_mixed"] >= 100
    for t in ("LO", "UP", "DB", "FX", "FR"):
        assert HEAD["kept_with_col_type"][t] >= 30 and HEAD["kept_with_row_type"][t] >= 30
    dropped_a = sum(v for k, v in HEAD["dropped_by_family_and_reason"].items() if k.startswith("a:"))
    assert dropped_a <= 0.5 * HEAD["drawn_by_family"]["a"]
    # the header counts are those of the records
    assert sum(r["n_int"] == r["n"] for r in DRAWN) == HEAD["kept_pure"]
    for f in "abcd":
        assert sum(r["family"] == f for r in DRAWN) == HEAD["kept_by_family"][f]
    assert HEAD["kept"] + sum(HEAD["dropped_by_family_and_reason"].values()) == HEAD["drawn"]
    assert HEAD["kept_large_size_class"] >= 60


def test_pinned_points_are_feasible_and_have_the_pinned_value():
    """Every enumerated optimum comes with a point: feasible in the regenerated model, integral, with the pinned value; and
    wherever HiGHS disagrees about an optimum, the enumerated point is the better one (a certificate, not an opinion)."""
    for rec in INSTANCES:
        inst = instance(rec)
        A, rlo, rhi, clo, chi, c, c0, isint, mx = lpgen.milp_arrays(inst)
        assert (rec["m"], rec["n"], rec["n_int"]) == (A.shape[0], A.shape[1], int(isint.sum()))
        if rec["status"] != "optimal":
            assert rec["x"] is None and rec["optimum"] is None
            continue
        x = np.array(rec["x"])
        assert np.array_equal(x[isint], np.round(x[isint]))
        act = A @ x
        assert np.all(act >= rlo - 1e-9) and np.all(act <= rhi + 1e-9) and np.all(x >= clo - 1e-9) and np.all(x <= chi + 1e-9)
        assert abs(float(c @ x) + c0 - rec["optimum"]) <= 1e-9 * (1 + abs(rec["optimum"]))
        for st, val in (rec["highs_presolve_on"], rec["highs_presolve_off"]):
            if st == "optimal":
                sg = 1.0 if mx else -1.0
                assert sg * rec["optimum"] >= sg * val - 1e-6 * (1 + abs(val)), (rec["index"], val, rec["optimum"])
    listed = {(d["index"], d["highs"]) for d in HEAD["highs_disagreements"]}
    assert len(listed) == len(HEAD["highs_disagreements"]) and {i for i, _ in listed} <= {r["index"] for r in DRAWN}


# ------------------------------------------------------------------------------------------------ whole trees


@pytest.mark.parametrize("family", "abcd")
@pytest.mark.parametrize("name", list(OPTIONS))
def test_trees_close_on_the_enumerated_optimum(orc, tab, name, family):
    recs = [r for r in INSTANCES if r["family"] == family]
    assert len(recs) >= 25

    def one(rec):
        inst = instance(rec)
        check_pin(rec, inst, run(orc, rec, inst, table=tab, **OPTIONS[name]))

    bad = failures(recs, one)
    assert not bad, "%d of %d fail:\n%s" % (len(bad), len(recs), "\n".join(bad))


def test_some_trees_have_tens_to_hundreds_of_nodes():
    """A guard on the family, not on the driver's answers: most of these trees are a handful of nodes (the median serial
    tree has 3), so the family must keep the members that branch for real -- at least 30 trees of 10 nodes or more and one
    of a hundred or more."""
    from oracle import oracle

    orc = oracle.api()
    tab = bnb.table_from(orc)
    counts = []
    for rec in INSTANCES:
        if rec["relaxation"] == "optimal":  # sub-family d included: a tree that must exhaust its box to prove infeasibility
            counts.append(run(orc, rec, instance(rec), table=tab, window=1)["count"])
    assert sum(c >= 10 for c in counts) >= 30 and max(counts) >= 100, sorted(counts)[-10:]


def test_windows_give_the_serial_tree(orc, tab):
    recs = INSTANCES[::10]
    assert len({r["family"] for r in recs}) == 4

    def one(rec):
        inst = instance(rec)
        for extra in (dict(), dict(heur=2, rc_fix=1), dict(cut_strat=1)):
            ref = run(orc, rec, inst, table=tab, window=1, **extra)
            for w in (2, 8, 64):
                same_result(run(orc, rec, inst, table=tab, window=w, **extra), ref)
        for extra in (dict(), dict(heur=2), dict(cut_strat=1)):
            ref = run(orc, rec, inst, table=tab, node_strat=1, window=1, **extra)
            for w in (2, 8, 64):
                same_result(run(orc, rec, inst, table=tab, node_strat=1, best_window=w, **extra), ref)

    bad = failures(recs, one)
    assert not bad, "\n".join(bad)


def test_the_callers_handle_is_left_as_it_was(orc, tab):
    """The driver rounds the bounds of a copy: the caller's fractional bounds are still there after the run."""
    rec = next(r for r in INSTANCES if r["family"] == "b" and r["status"] == "optimal")
    inst = instance(rec)
    P = lpgen.load_milp(orc, inst)
    before = [(orc.get_col_type(P.h, j), orc.get_col_lb(P.h, j), orc.get_col_ub(P.h, j)) for j in range(1, P.n + 1)]
    assert any(l != math.floor(l) or u != math.floor(u) for _, l, u in before)
    r = bnb.branch_and_bound(P, quirks=0, table=tab, window=1)
    check_pin(rec, inst, r)
    assert before == [(orc.get_col_type(P.h, j), orc.get_col_lb(P.h, j), orc.get_col_ub(P.h, j)) for j in range(1, P.n + 1)]


def test_oracle_restatement_follows_the_rule(orc, tab):
    """orc_branchAndBound (the oracle's own restatement of the serial loop) applies the same rule for fractional bounds: the
    driver over the oracle's table and the restatement give one tree on sub-family b, and an integer column fixed at or
    boxed around a fraction makes the root infeasible without a solve in both."""
    from oracle import oracle

    done = 0
    for rec in [r for r in INSTANCES if r["family"] == "b"][:30]:
        inst = instance(rec)
        a = run(orc, rec, inst, table=tab, window=1)
        b = oracle.branch_and_bound(lpgen.load_milp(orc, inst), quirks=0, max_nodes=max_nodes(rec))
        same_result(a, b)
        done += 1
    assert done == 30
    A = np.array([[1.0, 1.0]])
    for col in ((capi.FX, 1.5, 1.5), (capi.DB, 1.25, 1.75)):
        P = orc.create()
        P.load_general(A, [(capi.UP, 0.0, 9.0)], [col, (capi.DB, 0.0, 3.0)], [1.0, 1.0], kinds=[IV, IV], direction=MIN)
        a = bnb.branch_and_bound(P, quirks=0, table=tab, window=1)
        b = oracle.branch_and_bound(P, quirks=0)
        same_result(a, b)
        assert (a["rc"], a["count"], a["has_incumbent"], a["n_nodes"], a["prune"], a["total_pivots"]) == (0, 0, 0, 1, [1], 0)
        assert a["best_lower"] == math.inf
        for kw in (dict(window=64), dict(node_strat=1, best_window=8)):
            same_result(bnb.branch_and_bound(P, quirks=0, table=tab, **kw), a)


def test_distributed_coordinators_follow_the_rule(orc, tab):
    """One rank, no communicator: mvx_branchAndBound_dist and the Python coordinator give the serial driver's tree on
    sub-family b, and book an integer column boxed around a fraction as an infeasible root."""
    from mvolps_amd import dist_bnb, dist_native

    from . import dist_helpers

    api, table, image = dist_helpers.oracle_tables()
    engine = dist_helpers.OracleNodeEngine()
    recs = [r for r in INSTANCES if r["family"] == "b"][:20]
    for rec in recs:
        inst = instance(rec)
        ref = run(orc, rec, inst, table=tab, window=1)
        check_pin(rec, inst, ref)
        nat = dist_native.branch_and_bound(lpgen.load_milp(api, inst), table=table, image=image, quirks=0, per_rank=4, max_nodes=max_nodes(rec))
        py = dist_bnb.branch_and_bound(engine, lpgen.load_milp(engine.api, inst), quirks=0, per_rank=4, max_nodes=max_nodes(rec))
        same_result(nat, ref)
        same_result(py, ref)
    P = orc.create()
    P.load_general(np.array([[1.0, 1.0]]), [(capi.UP, 0.0, 9.0)], [(capi.DB, 1.25, 1.75), (capi.DB, 0.0, 3.0)], [1.0, 1.0], kinds=[IV, IV],
                   direction=MAX)
    ref = bnb.branch_and_bound(P, quirks=0, table=tab, window=1)
    assert (ref["count"], ref["has_incumbent"], ref["prune"], ref["best_lower"]) == (0, 0, [1], -math.inf)
    same_result(dist_native.branch_and_bound(P, table=table, image=image, quirks=0), ref)
    same_result(dist_bnb.branch_and_bound(engine, P, quirks=0), ref)


def test_unbounded_root_relaxation(orc, tab):
    """What the family leaves out (the fixture drops it): max x1 + x2 with x1 - x2 <= 5 only.  The driver books the root as
    it books an infeasible one and returns without an incumbent; it does not tell unbounded from infeasible."""
    for direction, c, inf in ((MAX, [1.0, 1.0], -math.inf), (MIN, [-1.0, -1.0], math.inf)):
        P = orc.create()
        P.load_general(np.array([[1.0, -1.0]]), [(capi.UP, 0.0, 5.0)], [(LO, 0.0, 0.0)] * 2, c, kinds=[IV, IV], direction=direction)
        Q = P.copy()
        Q.simplex()
        assert Q.status == UNBND
        for kw in (dict(window=1), dict(window=64), dict(node_strat=1, best_window=8)):
            r = bnb.branch_and_bound(P, quirks=0, table=tab, **kw)
            assert (r["rc"], r["count"], r["has_incumbent"], r["hit_limit"]) == (0, 0, 0, 0)
            assert r["best_lower"] == inf


# ------------------------------------------------------------------------------------------------ twins and cuts on tree nodes


def sampled(recs, count):
    step = max(1, len(recs) // count)
    return recs[::step][:count]


def tree_nodes(api, inst, tab, count=12):
    """Solved OPT nodes below the root as the driver sees it: the rounding rule first, then bnb.node_sample."""
    root = lpgen.load_milp(api, inst)
    if bnb.integral_bounds(root, table=tab) == 2:
        return root, []
    return root, bnb.node_sample(root, count, quirks=0, table=tab)


def node_box(api, P):
    lo = np.array([api.get_col_lb(P.h, j) for j in range(1, P.n + 1)])
    hi = np.array([api.get_col_ub(P.h, j) for j in range(1, P.n + 1)])
    return lo, hi


def node_cut_rows(api, P, tab, **kw):
    """The rows the driver's cut step appends to a clone of the solved node P: [(coef over the n columns, rhs)], cut
    coef . x >= rhs."""
    Q = P.copy()
    m0 = Q.m
    bnb.node_cuts(Q, dict(cut_strat=1, quirks=0, **kw), table=tab)
    out = []
    for i in range(m0 + 1, api.get_num_rows(Q.h) + 1):
        ind, val = Q.get_mat_row(i)
        coef = np.zeros(P.n)
        coef[np.asarray(ind) - 1] = val
        out.append((coef, api.get_row_lb(Q.h, i)))
    return out


def col_bounds(api, P):
    return [(api.get_col_type(P.h, j), api.get_col_lb(P.h, j), api.get_col_ub(P.h, j)) for j in range(1, P.n + 1)]


def test_children_bounds_for_every_column_type(orc, tab):
    """mvx_bnb_make_children (child_bounds, which strong branching shares) on tree nodes, every violated column of each: the
    down child is the node with x_j <= floor(v), the up child with x_j >= ceil(v), each keeping the node's other bound (so a
    LO column with a negative lower bound keeps it), FX where the two meet; no other column changes, no bounds cross."""
    has_lo, has_up = (capi.LO, capi.DB, capi.FX), (capi.UP, capi.DB, capi.FX)
    seen, negative, fixed = set(), 0, 0
    for rec in sampled([r for r in INSTANCES if r["relaxation"] == "optimal"], 120):
        _root, sample = tree_nodes(orc, instance(rec), tab, count=6)
        for P in sample:
            before = col_bounds(orc, P)
            x = P.col_prim()
            for j in bnb.print_info(P, quirks=0, table=tab)[1]:
                t, l, u = before[j - 1]
                v = float(x[j - 1])
                dn, up = math.floor(v), math.ceil(v)
                S2, S3 = bnb.make_children(P, j, quirks=0, table=tab)
                want2 = (capi.FX if l == dn else capi.DB, l, dn) if t in has_lo else (capi.UP, None, dn)
                want3 = (capi.FX if u == up else capi.DB, up, u) if t in has_up else (capi.LO, up, None)
                for S, want in ((S2, want2), (S3, want3)):
                    after = col_bounds(orc, S)
                    assert after[: j - 1] == before[: j - 1] and after[j:] == before[j:]
                    gt, gl, gu = after[j - 1]
                    assert gt == want[0] and (want[1] is None or gl == want[1]) and (want[2] is None or gu == want[2] or gt == capi.FX), (
                        rec["index"], j, before[j - 1], v, after[j - 1], want)
                    assert gt not in (capi.DB,) or gl < gu
                    fixed += gt == capi.FX
                seen.add(t)
                negative += t in has_lo and l < 0
    assert seen >= {capi.LO, capi.UP, capi.DB, capi.FR} and negative >= 20 and fixed >= 20, (seen, negative, fixed)


def test_twins_on_tree_nodes(orc, tab):
    """rc_tighten_node, round_node and penalties against their definitions on B&B nodes of 30 instances (sub-family b
    included), and no rc entry cuts off a point better than the cutoff."""
    recs = sampled([r for r in INSTANCES if r["status"] == "optimal" and r["family"] in "ab"], 30)
    assert len(recs) == 30 and {r["family"] for r in recs} == {"a", "b"}
    nodes = entries = forced = found = cands = 0
    seen = set()
    for rec in recs:
        inst = instance(rec)
        root, sample = tree_nodes(orc, inst, tab)
        M = RoundModel(inst["A"], inst["row_b"], inst["col_b"], inst["c"], inst["c0"], inst["kinds"], inst["direction"])
        sg = sense(orc, root)
        for P in sample:
            nodes += 1
            found += sum(round_twin(M, root, P, tab))
            cands += len(penalties_twin(P, tab)[0])
            for B in (rec["optimum"], P.obj - sg * 0.25, P.obj - sg * 2.0, P.obj - sg * 9.0):
                got = rc_twin(orc, tab, P, B, seen)
                entries += len(got)
                for (j, lb, ub) in got:
                    Q = forced_beyond(orc, P, j, lb, ub)
                    assert Q.status == NOFEAS or (Q.status == OPT and sg * Q.obj <= sg * B + 1e-9 * max(1.0, abs(B)) + 1e-7), (
                        rec["index"], j, Q.status, Q.obj, B)
                    forced += 1
    # 30 instances whose median tree has 3 nodes: at least two nodes each on average
    assert nodes >= 60 and entries >= 100 and forced == entries and found > 20 and cands >= 60, (nodes, entries, found, cands)
    assert seen >= {"NL", "NU", "continuous"}, seen


@pytest.mark.parametrize("family", "abd")
def test_repaired_cuts_on_tree_nodes_keep_the_optimum(orc, tab, family):
    """Every cut row the driver's cut step adds on a tree node keeps the enumerated optimal point whenever that point lies in
    the node's box; on sub-family d (no integer point at all) the step must still run."""
    recs = sampled([r for r in INSTANCES if r["family"] == family and r["relaxation"] == "optimal"], 30)
    cuts = inside = 0
    bad = []
    for rec in recs:
        inst = instance(rec)
        _root, sample = tree_nodes(orc, inst, tab)
        for P in sample:
            lo, hi = node_box(orc, P)
            for kw in (dict(), dict(cut_select=1)):
                rows = node_cut_rows(orc, P, tab, **kw)
                cuts += len(rows)
                if rec["status"] != "optimal":
                    continue
                x = np.array(rec["x"])
                if not (np.all(x >= lo - 1e-9) and np.all(x <= hi + 1e-9)):
                    continue
                for coef, rhs in rows:
                    inside += 1
                    if len(cf.cut_cuts_off(coef, rhs, [x])):
                        bad.append("instance %d: a cut excludes the optimum %s (%.6g < %.6g)" % (rec["index"], rec["x"], coef @ x, rhs))
    assert not bad, "\n".join(bad[:20])
    assert cuts >= 30, cuts
    if family != "d":
        assert inside >= 20, inside
