"""CPU, oracle alone: every instance of test_gpu_general_at_size.py has the property its GPU test relies on, the shape table
lies on both sides of every limit it names, and the certificates of tests/certify.py hold on the oracle's own end states
-- which is where a wrong NOFEAS of the oracle is caught without a GPU."""
import time

import numpy as np
import pytest

from mvolps_amd import capi
from mvolps_amd.capi import DB, FR, FX, LO, UP, NF, NL, NS, NU, EITLIM, INFEAS, NOFEAS, OPT, UNBND

from . import general_at_size as ga
from . import thresholds as th

PHASE1 = [c for c in ga.CASES if c.family == "general"]
COLD = [c for c in ga.CASES if c.family == "cold"]


def shapes(cases):
    return {(c.m, c.n) for c in cases}


def test_shape_table_lies_on_both_sides_of_every_limit():
    ms, ns = {c.m for c in PHASE1}, {c.n for c in PHASE1}
    assert {63, 64, 65} <= ms  # the wave edge of k_p1_head's count and scan
    assert [ga.p1_chunk(m) for m in (1024, 1025, 2049)] == [1, 2, 3] and {1024, 1025} <= ms  # rows per lane (2049: the stepwise case)
    assert -(-1025 // ga.p1_chunk(1025)) == 513  # R = 2: lanes 0..512 hold rows, lanes 513.. idle
    assert {255, 256} <= ns and {1023, 1024, 1025} <= ns  # k_p1_fix's block edge, dev_price's stride in k_p1_select
    assert (62 + 1) % 4 == 3 and (63 + 1) % 4 == 0 and {62, 63} <= ms  # the cost row m + 1 closes a 4-row tile / opens one
    depth = {c.name: th.update_tile_rows(c.m + 1, c.n) for c in PHASE1}
    assert depth["p1-1025x8192"] == 8 and depth["p1-2048x8192"] == 16
    assert all(d == 4 for k, d in depth.items() if "8192" not in k) and set(depth.values()) == {4, 8, 16}
    assert sum(ga.P1_BATCHES[:3]) < 40 < sum(ga.P1_BATCHES[:4])  # 40 pivots: the 4, 8, 16 and 32 batches of phase 1
    for m, n in ((300, 700), (700, 300), (1100, 1030)):  # k_chain with more than one workgroup
        assert (m, n) in shapes(PHASE1) and -(-max(m, n) // ga.CHAIN_WG) >= 3
    assert th.persist_plan(300, 700, 256)[0] >= 3  # k_persist at three columns per workgroup
    cold = shapes(COLD)
    assert {(300, 600), (1024, 1024), (1025, 300), (1100, 2000)} <= cold
    assert max(1024, 1024) <= th.DSEL_MAX < 1025
    assert ga.DUAL_FUSED_MIN <= 1101 * 2001 < ga.DUAL_FUSED_MAX
    assert all((c.m + 1) * (c.n + 1) < ga.DUAL_FUSED_MIN for c in COLD if c.n != 2000)


def test_end_statuses_of_the_table():
    ends = {c.stops[-1][1] for c in ga.CASES}
    assert {OPT, UNBND, NOFEAS} <= ends
    assert all(c.stops[-1][1] != NOFEAS for c in ga.CASES if c.feasible)
    assert all(c.stops[-1][1] == NOFEAS for c in ga.CASES if not c.feasible)


@pytest.mark.parametrize("case", ga.CASES + [ga.STEPWISE], ids=ga.case_id)
def test_slack_basis_has_the_properties_relied_on(case):
    inst = case.instance()
    g = ga.slack_signs(inst)
    rows = 1 + np.nonzero(g)[0]
    assert len(rows) > 0  # primal infeasible
    dinf = ga.slack_dual_infeasibilities(inst)
    _, flag = ga.slack_point(inst)
    if case.family == "cold":
        assert dinf == 0  # dual feasible: select_step goes to the dual simplex from pivot 0
        assert {NL, NU, NF} <= set(flag.tolist()) and {t for t, _, _ in inst["row_b"]} >= {LO, DB, FX}
        return
    assert dinf > 0  # neither: phase 1
    assert {NL, NU, NF, NS} <= set(flag.tolist()) and {t for t, _, _ in inst["row_b"]} >= {LO, UP, DB, FX, FR}
    # the first change list is every infeasible row: past one unrolled group of k_p1_fix, with a tail
    assert len(rows) >= 9 and len(rows) % ga.P1_FIX_UNROLL != 0
    R = ga.p1_chunk(case.rows)
    lanes = {(i - 1) // R for i in rows}
    if case.m in (63, 64, 65, 1024, 1025, 2049) and case.feasible:
        assert g[case.m - 1] != 0  # the last row, the one the edge is about, is in the list
    if case.rows > ga.WAVE:
        assert len({t // ga.WAVE for t in lanes}) >= 2  # infeasible rows in two waves' row ranges
    if R >= 2:
        assert len(lanes) >= 2 and any(sum((i - 1) // R == t for i in rows) >= 2 for t in lanes)


@pytest.fixture(scope="module")
def ended(orc):
    """name -> (instance, the oracle's handle after the case's schedule, its stops, seconds, a copy of the handle in
    front of the call that leaves phase 1)"""
    out = {}

    def get(case):
        if case.name not in out:
            inst = case.instance()
            P = ga.load(orc, inst)
            t = time.time()
            stops, before = [], None
            for lim in case.calls:
                keep = P.copy() if case.p1 is not None and before is None else None
                rc = P.simplex(it_lim=lim)
                stops.append((rc, P.status, P.it_cnt))
                if keep is not None and P.status != INFEAS:
                    before = keep
                if rc != EITLIM:
                    break
            out[case.name] = (inst, P, stops, time.time() - t, before)
        return out[case.name]

    return get


@pytest.mark.parametrize("case", ga.CASES, ids=ga.case_id)
def test_schedule_stops_where_the_table_says(ended, case):
    """The first call ends on its pivot limit with status INFEAS -- the oracle reports that from phase 1 and the dual only,
    so phase 1 (the dual) ran that many pivots; where a second limited call follows it ends past phase 1 (FEAS).  The
    table's p1 is the pivot at which phase 1 ended: from the stop in front of the crossing call, a limit one short of it
    still ends INFEAS and a limit that reaches it does not."""
    inst, P, stops, secs, before = ended(case)
    print("%s: %s, %.1f s on the oracle (table: %s)" % (case.name, stops, secs, case.secs))
    assert stops == case.stops
    assert stops[0] == (EITLIM, INFEAS, case.calls[0])
    assert (case.p1 is not None) == (case.family == "general" and len(case.stops) == 3)
    if case.p1 is not None:
        for lim, inside in ((case.p1 - before.it_cnt - 1, True), (case.p1 - before.it_cnt, False)):
            Q = before.copy()
            Q.simplex(it_lim=lim)
            assert (Q.status == INFEAS) == inside, (case.name, lim, Q.status)


@pytest.mark.parametrize("case", ga.CASES, ids=ga.case_id)
def test_oracle_end_state_is_certified(ended, case):
    inst, P, stops, _, _ = ended(case)
    ga.certify_end(case, inst, P, stops[-1][0])


# ------------------------------------------------------------------------------------------------ the wrong NOFEAS
# general_lp(2049, 256, 5) has the point x0.  Solved in calls of 500 pivots the oracle used to end NOFEAS at pivot 7698,
# and in calls of 20 from pivot 7500 at 7749: by then the basis is ill-conditioned (tableau entries of 2e5), column 0 is
# off by up to 1e-7 on hundreds of rows while A x = x_R holds to 2e-12, and the dual simplex stops on a row 1e-8 out of
# bounds that no column can move back.  The NOFEAS_RECHECK rule rebuilds the tableau for the same basis and solves on.
STEPWISE = ga.STEPWISE


@pytest.fixture(scope="module")
def stepwise(orc):
    inst = STEPWISE.instance()
    P = ga.load(orc, inst)
    trace = []
    while P.it_cnt < 7500:
        if P.it_cnt == 6500:  # in front of the call that leaves phase 1 at pivot STEPWISE.p1
            for lim, inside in ((STEPWISE.p1 - 6500 - 1, True), (STEPWISE.p1 - 6500, False)):
                Q = P.copy()
                Q.simplex(it_lim=lim)
                assert (Q.status == INFEAS) == inside, (lim, Q.status)
        rc = P.simplex(it_lim=500)
        trace.append((rc, P.status, P.it_cnt))
    return inst, P, trace


def test_stepwise_calls_of_500_end_optimal(orc, stepwise):
    inst, P, trace = stepwise
    assert trace[0] == (EITLIM, INFEAS, 500) and [t[1] for t in trace[-2:]] == [capi.FEAS, capi.FEAS]
    Q = P.copy()
    rc = EITLIM
    while rc == EITLIM:
        rc = Q.simplex(it_lim=500)
    assert orc.get_refresh_cnt(Q.h) >= 1  # the verdict was NOFEAS on the pivoted tableau: the rebuild is what this is about
    assert rc == 0 and Q.status == OPT
    ga.certify_end(STEPWISE, inst, Q, rc)


def test_stepwise_calls_of_20_from_7500_end_optimal(orc, stepwise):
    inst, P, trace = stepwise
    Q = P.copy()
    rc = EITLIM
    while rc == EITLIM:
        rc = Q.simplex(it_lim=20)
        assert Q.it_cnt < 9000
    assert rc == 0 and Q.status == OPT
    ga.certify_end(STEPWISE, inst, Q, rc)


@pytest.mark.parametrize("lim", [None, 2000, 7000])
def test_stepwise_other_call_patterns_end_optimal(orc, lim):
    inst = STEPWISE.instance()
    P = ga.load(orc, inst)
    rc = EITLIM
    while rc == EITLIM:
        rc = P.simplex(it_lim=lim)
    assert rc == 0 and P.status == OPT
    ga.certify_end(STEPWISE, inst, P, rc)
