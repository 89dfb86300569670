"""CPU: reduced-cost bound tightening (mvx_bnb_params.rc_fix, DESIGN.md "Reduced-cost tightening"), driver over the ORACLE's
table, so the host twins run (mvx_bnb_rc_tighten for the lists, set_col_bnds per entry for the apply).

The twin is checked with == against a plain-Python restatement of the definition built from the test's own view of the
handle; no list entry may cut off a point better than the incumbent; the trees close on the HiGHS optima; the FIFO window
gives the serial tree for every window size; rc_fix = 0 is the parent's driver; the refusals are pinned."""
import math
import sys

import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import CV, DB, FX, IV, LO, MAX, MIN, NL, NOFEAS, NU, OPT, UP

from . import lpgen
from .test_bnb_branching import HIGHS
from .test_bnb_heuristic import incumbent_ok
from .test_bnb_host import same_result

DBLMAX = sys.float_info.max
TOL = 1e-9
DENSE = [(10, 20, 4, 3), (16, 32, 5, 2), (20, 40, 7, 3)]
# node counts of the plain-Python restatement of the rule over the oracle's table (repaired, FIFO, VO, no cuts, no heuristic)
RESTATED_COUNT = {(10, 20, 4, 3): 563, (16, 32, 5, 2): 4319, (20, 40, 7, 3): 12605, ("setcover", 40, 60, 3): 15}


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    assert not t.rc_tighten_many and not t.tighten_cols_many  # the host twins are what runs over the oracle
    return t


def sense(orc, P):
    return -1.0 if orc.get_obj_dir(P.h) == MIN else 1.0


def restate(orc, P, B, tol=TOL, seen=None):
    """The definition, one operation at a time on Python floats, from the handle's exported tableau and basis."""
    m, n = P.m, P.n
    T0 = P.tableau()[0]
    _head, nb, flag = P.basis()
    sg = sense(orc, P)
    gap = sg * P.obj - sg * B
    gap2 = gap + 1e-9 * max(1.0, abs(B))
    out = []
    if not gap2 > 0:
        return out
    for q in range(1, n + 1):
        v = int(nb[q])
        if v <= m:
            continue
        j = v - m
        f = int(flag[q])
        d = abs(float(T0[q]))
        if orc.get_col_kind(P.h, j) == CV:
            if seen is not None and f in (NL, NU) and d > tol:
                seen.add("continuous")
            continue
        if f not in (NL, NU) or not d > tol:
            continue
        lb, ub = orc.get_col_lb(P.h, j), orc.get_col_ub(P.h, j)
        at = lb if f == NL else ub
        if at != float(np.rint(at)):
            if seen is not None:
                seen.add("fractional bound")
            continue
        r = gap2 / d
        t = float(math.ceil(r)) - 1.0 if math.isfinite(r) else r
        if f == NL:
            nu = at + t
            if nu < ub:
                out.append((j, lb, nu))
                if seen is not None:
                    seen.add("NL")
                    if ub >= DBLMAX:
                        seen.add("absent far bound")
        else:
            nl = at - t
            if nl > lb:
                out.append((j, nl, ub))
                if seen is not None:
                    seen.add("NU")
                    if lb <= -DBLMAX:
                        seen.add("absent far bound")
    return sorted(out)


def check_twin(orc, tab, P, B, seen=None):
    rc, got = bnb.rc_tighten_node(P, B, TOL, table=tab)
    assert rc == 0
    want = restate(orc, P, B, seen=seen)
    assert got == want, (B, got, want)
    return got


def test_twin_matches_definition_general_bounds(orc, tab):
    rng = np.random.default_rng(23)
    seen, dirs, entries, checked = set(), set(), 0, 0
    for _ in range(400):
        A, row_b, col_b, c, d = lpgen.random_general_lp(rng, 10, 12)
        if rng.random() < 0.3:  # some integer columns rest on a fractional bound
            k = int(rng.integers(len(col_b)))
            t, l, u = col_b[k]
            col_b[k] = (t, l - 0.5, u + 0.5)
        kinds = [IV if rng.random() < 0.7 else CV for _ in c]
        P = orc.create()
        P.load_general(A, row_b, col_b, c, c0=float(rng.integers(-3, 4)), kinds=kinds, direction=d)
        P.simplex()
        if P.status != OPT:
            continue
        sg = sense(orc, P)
        for delta in (0.25, 1.5, 6.0, 40.0):
            entries += len(check_twin(orc, tab, P, P.obj - sg * delta, seen))
        dirs.add(d)
        checked += 1
    assert checked > 150 and entries > 200
    assert dirs == {MIN, MAX}
    assert seen >= {"NL", "NU", "fractional bound", "absent far bound", "continuous"}, seen


def test_twin_matches_definition_on_children_and_empty_lists(orc, tab):
    A, b, c, U = synth.dense_ilp(12, 24, 5, 3)
    root = lpgen.load_ilp(orc, A, b, c, U)
    queue, done, entries = [root.copy()], 0, 0
    while queue and done < 30:
        P = queue.pop(0)
        P.simplex()
        if P.status != OPT:
            continue
        for delta in (0.5, 3.0, 11.0):
            entries += len(check_twin(orc, tab, P, P.obj - delta))
        # nothing to gain: the cutoff at or above the LP value; no incumbent: -inf for this maximisation
        assert check_twin(orc, tab, P, P.obj + 1.0) == []
        assert check_twin(orc, tab, P, P.obj + 1e-6) == []
        assert check_twin(orc, tab, P, -math.inf) == []
        assert check_twin(orc, tab, P, math.nan) == []
        done += 1
        _st, viol = bnb.print_info(P, quirks=0, table=tab)
        if viol:
            queue += list(bnb.make_children(P, viol[0], quirks=0, table=tab))
    assert done >= 20 and entries > 50
    Ac, cc = lpgen.setcover_ilp(40, 60, 3)
    S = lpgen.load_setcover(orc, Ac, cc)
    S.simplex()
    assert check_twin(orc, tab, S, S.obj + 2.0)  # a minimisation: the cutoff lies above
    assert check_twin(orc, tab, S, math.inf) == [] and check_twin(orc, tab, S, S.obj - 1.0) == []


@pytest.mark.parametrize("var_strat", [0, 2, 3])
@pytest.mark.parametrize("cut_strat", [0, 1])
@pytest.mark.parametrize("heur", [0, 2])
@pytest.mark.parametrize("case", list(HIGHS), ids=str)
def test_trees_close_on_the_optimum(orc, tab, case, heur, cut_strat, var_strat):
    r = bnb.branch_and_bound(lpgen.load_case(orc, case), table=tab, quirks=0, rc_fix=1, heur=heur, cut_strat=cut_strat, var_strat=var_strat)
    assert r["rc"] == 0 and r["hit_limit"] == 0 and r["has_incumbent"]
    assert abs(r["best_lower"] - HIGHS[case]) <= 1e-6 * (1 + abs(HIGHS[case]))
    incumbent_ok(orc, case, r)


def forced_beyond(orc, P, j, lb, ub):
    """A clone of the solved node P with column j forced one unit beyond the tightened bound of entry (j, lb, ub)."""
    olb, oub = orc.get_col_lb(P.h, j), orc.get_col_ub(P.h, j)
    Q = P.copy()
    if ub < oub:  # the upper bound came down: x_j >= ub + 1
        lo = ub + 1.0
        if oub >= DBLMAX:
            orc.set_col_bnds(Q.h, j, LO, lo, 0.0)
        else:
            assert lo <= oub
            orc.set_col_bnds(Q.h, j, FX if lo == oub else DB, lo, oub)
    else:  # the lower bound went up: x_j <= lb - 1
        assert lb > olb
        hi = lb - 1.0
        if olb <= -DBLMAX:
            orc.set_col_bnds(Q.h, j, UP, 0.0, hi)
        else:
            assert hi >= olb
            orc.set_col_bnds(Q.h, j, FX if hi == olb else DB, olb, hi)
    Q.simplex()
    return Q


@pytest.mark.parametrize("case", DENSE, ids=str)
def test_no_entry_cuts_off_a_better_point(orc, tab, case):
    """A FIFO tree with the rule, restated in Python over the twin: for every entry of every node's list the node LP with
    the column forced one unit beyond its new bound is infeasible or no better than the incumbent (within the slack of the
    definition plus the LP's own 1e-7 on z').  The restated tree has the node count the driver must reproduce."""
    root = lpgen.load_case(orc, case)
    sg = sense(orc, root)
    B = -sg * math.inf
    queue, count, entries = [root.copy()], 0, 0
    while queue:
        P = queue.pop(0)
        P.simplex()
        count += 1
        st, viol = bnb.print_info(P, quirks=0, table=tab)
        if st == -1:
            continue
        z = P.obj
        if st == 1:
            if sg * z > sg * B:
                B = z
            continue
        if sg * z <= sg * B:
            continue
        edits = []
        if math.isfinite(B) and P.status == OPT:
            rc, edits = bnb.rc_tighten_node(P, B, TOL, table=tab)
            assert rc == 0
            for (j, lb, ub) in edits:
                Q = forced_beyond(orc, P, j, lb, ub)
                assert Q.status == NOFEAS or (Q.status == OPT and sg * Q.obj <= sg * B + 1e-9 * max(1.0, abs(B)) + 1e-7), (
                    count, j, Q.status, Q.obj, B)
                entries += 1
        S2, S3 = bnb.make_children(P, viol[0], quirks=0, table=tab)
        for S in (S2, S3):
            for (j, lb, ub) in edits:
                orc.set_col_bnds(S.h, j, FX if lb == ub else DB, lb, ub)
        queue += [S2, S3]
    assert count == RESTATED_COUNT[case] and entries > 500
    assert abs(B - HIGHS[case]) <= 1e-6 * (1 + abs(HIGHS[case]))


def test_it_acts_and_counts_match_the_restatement(orc, tab):
    total_on = total_off = 0
    for case in DENSE + [("setcover", 40, 60, 3)]:
        off = bnb.branch_and_bound(lpgen.load_case(orc, case), table=tab, quirks=0)
        on = bnb.branch_and_bound(lpgen.load_case(orc, case), table=tab, quirks=0, rc_fix=1)
        assert on["rc"] == off["rc"] == 0 and on["hit_limit"] == 0
        assert on["rc_fixed"] > 0 and on["rc_calls"] > 0 and on["rc_tightened"] >= 0, case
        assert on["count"] == RESTATED_COUNT[case], (case, on["count"])
        assert abs(on["best_lower"] - HIGHS[case]) <= 1e-6 * (1 + abs(HIGHS[case]))
        assert abs(off["best_lower"] - HIGHS[case]) <= 1e-6 * (1 + abs(HIGHS[case]))
        if case in DENSE:
            total_on += on["count"]
            total_off += off["count"]
    assert total_off == 19073 and total_on <= total_off


def same_counters(a, b):
    for k in ("rc_calls", "rc_fixed", "rc_tightened", "heur_calls", "heur_found", "heur_improved", "incumbent_heur"):
        assert a[k] == b[k], k


def incumbent_moves_inside_a_window(r, window):
    """From the serial event stream of a heur = 0 maximisation run: does an integral node improve the incumbent in the middle
    of a FIFO window of `window` nodes, with a node behind it in the same window that branches (the recompute path)?"""
    order = [e for e in r["events"] if e[0] in (1, 2, 3, 4)]  # one decision event per popped node, in pop order
    best = -math.inf
    queue_len, pos, hit = 1, 0, False
    while pos < len(order):
        chunk = order[pos:pos + min(queue_len, window)]
        moved = False
        for e in chunk:
            if e[0] == 1 and e[4] > best:
                best = e[4]
                moved = True
            elif e[0] == 4 and moved:
                hit = True
        queue_len += 2 * sum(1 for e in chunk if e[0] == 4) - len(chunk)
        pos += len(chunk)
    return hit


@pytest.mark.parametrize("cut_strat", [0, 1])
@pytest.mark.parametrize("var_strat", [0, 2, 3])
@pytest.mark.parametrize("heur", [0, 2])
def test_windows_equal_serial(orc, tab, heur, var_strat, cut_strat):
    A, b, c, U = synth.dense_ilp(10, 20, 4, 3)
    kw = dict(var_strat=var_strat, quirks=0, cut_strat=cut_strat, max_nodes=400, table=tab, heur=heur, rc_fix=1)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), window=1, **kw)
    assert ref["rc"] == 0 and ref["count"] > 50 and ref["rc_calls"] > 0 and ref["rc_fixed"] > 0
    for w in (2, 8, 64):
        got = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), window=w, **kw)
        assert got["rc"] == 0
        same_result(got, ref)
        same_counters(got, ref)
    kw["max_nodes"] = 0
    best = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), node_strat=1, best_window=0, **kw)
    assert best["rc"] == 0 and best["hit_limit"] == 0 and best["has_incumbent"]
    if heur:  # without the heuristic best-bound order has its first incumbent when nothing is left to branch
        assert best["rc_calls"] > 0
    assert abs(best["best_lower"] - HIGHS[(10, 20, 4, 3)]) <= 1e-6 * (1 + HIGHS[(10, 20, 4, 3)])


def test_some_window_run_recomputes_its_lists(orc, tab):
    A, b, c, U = synth.dense_ilp(10, 20, 4, 3)
    hits = []
    for var_strat in (0, 2, 3):
        for cut_strat in (0, 1):
            r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), window=1, var_strat=var_strat, cut_strat=cut_strat, quirks=0,
                                     max_nodes=400, table=tab, rc_fix=1)
            hits += [incumbent_moves_inside_a_window(r, w) for w in (2, 8, 64)]
    assert any(hits)


def test_rc_fix_0_is_the_parent(orc, tab):
    for case in [(10, 20, 4, 3), ("setcover", 40, 60, 3)]:
        for kw in (dict(window=1), dict(window=64), dict(node_strat=1), dict(heur=2, cut_strat=1)):
            a = bnb.branch_and_bound(lpgen.load_case(orc, case), table=tab, quirks=0, **kw)
            z = bnb.branch_and_bound(lpgen.load_case(orc, case), table=tab, quirks=0, rc_fix=0, **kw)
            same_result(z, a)
            same_counters(z, a)
            assert (z["rc_calls"], z["rc_fixed"], z["rc_tightened"]) == (0, 0, 0)


def test_refusals_and_return_codes(orc, tab):
    from mvolps_amd import dist_bnb, dist_native

    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    for kw in (dict(rc_fix=2, quirks=0), dict(rc_fix=-1, quirks=0), dict(rc_fix=1, quirks=1), dict(rc_fix=1),
               dict(rc_fix=1, quirks=0, node_strat=1, best_window=8), dict(rc_fix=1, quirks=0, best_window=1)):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, **kw)
        assert r["rc"] == -1 and r["n_nodes"] == 0 and r["count"] == 0, kw
    P = lpgen.load_ilp(orc, A, b, c, U)
    with pytest.raises(ValueError):
        dist_native.branch_and_bound(P, table=tab, rc_fix=1, quirks=0)
    with pytest.raises(ValueError):
        dist_bnb.branch_and_bound(None, P, rc_fix=1, quirks=0)
    # the C++ coordinator refuses it too (MVX_EFAIL), in front of any engine call
    from mvolps_amd import capi

    pr = bnb.make_params(quirks=0, rc_fix=1)
    L = dist_native._lib()
    res, st = bnb.BnbResult(), dist_native.DistStats()
    tptr = bnb.C.cast(bnb.C.pointer(tab), bnb.C.c_void_p)
    assert L.mvx_branchAndBound_dist(tptr, None, P.h, bnb.C.byref(pr), None, None, bnb.C.byref(res), bnb.C.byref(st)) == capi.EFAIL
    # neither rc_tighten_many nor the twin's tableau export: an error once an incumbent exists, not a run without the rule
    bare = bnb.table_from(orc)
    bare.get_tableau = None
    # (best-bound order meets its first integral node late: the heuristic gives it an incumbent while nodes still branch)
    for kw in (dict(window=1), dict(window=64), dict(node_strat=1, best_window=0, heur=2)):
        full = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, rc_fix=1, quirks=0, **kw)
        assert full["rc"] == 0 and full["rc_calls"] > 0, kw
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bare, rc_fix=1, quirks=0, **kw)
        assert r["rc"] == -2 and r["has_incumbent"] == 1 and r["count"] < full["count"], kw
    # mvx_bnb_rc_tighten's own codes
    node = P.copy()
    node.simplex()
    assert bnb.rc_tighten_node(node, node.obj - 3.0, TOL, table=tab)[0] == 0
    assert bnb.rc_tighten_node(P, 0.0, TOL, table=tab)[0] == -3  # never solved
    assert bnb.rc_tighten_node(node, node.obj - 3.0, TOL, table=bare)[0] == -5
    nobasis = bnb.table_from(orc)
    nobasis.get_basis = None
    assert bnb.rc_tighten_node(node, node.obj - 3.0, TOL, table=nobasis)[0] == -5
