"""CPU, oracle alone: every instance of test_gpu_dual_fused.py contains the event its GPU test relies on, at a pivot the
engine's schedule (dual_fused.generic_indices) hands to k_da + k_fb<DUAL>; the figures of the case table are the oracle's;
the schedule's restatement does what its text says on hand-made inputs."""
import time

import pytest

from mvolps_amd import capi
from mvolps_amd.capi import NL, NS, NU, EITLIM, OPT

from . import dual_fused as df
from . import general_at_size as ga

_LOGS = {}


@pytest.fixture(scope="module")
def logs(orc):
    """case -> (pivot log, the oracle's end handle); cases that differ only in their call schedule share one"""

    def get(case):
        key = (case.m, case.n, case.seed, tuple(case.moves), case.infeasible_seed, case.stall_limit)
        if key not in _LOGS:
            t = time.time()
            _LOGS[key] = df.case_log(orc, case)
            print("%s: log of %d pivots in %.1f s" % (case.name, len(_LOGS[key][0]), time.time() - t))
        return _LOGS[key]

    return get


def fused_of(case, log):
    g = set(df.case_generic(case, log))
    return [k for k in range(len(log)) if k not in g]


# ------------------------------------------------------------------------------------------------ the schedule
def test_schedule_of_a_cold_start():
    # call to the end: the opening batch is one generic pivot; batches of 16, 32, 64 follow, their first pivot generic
    assert df.generic_indices(120, False, (None,)) == [0, 1, 17, 49, 113]
    assert df.generic_indices(1, False, (None,)) == [0] and df.generic_indices(2, False, (None,)) == [0, 1]
    # batches stop doubling at 256: 8 (opening), 16, 32, 64, 128, 256, 256
    assert df.generic_indices(800, False, (None,)) == [0, 1, 17, 49, 113, 241, 497, 753]


def test_schedule_of_a_warm_start():
    assert df.generic_indices(1, True, (None,)) == [0]
    assert df.generic_indices(30, True, (None,)) == [0, 8, 24]
    assert [df.warm_fused(t) for t in (1, 2, 8, 9, 24, 25)] == [0, 1, 7, 7, 22, 22]
    # the hint is the first call's only
    assert df.generic_indices(30, True, (4, None)) == [0, 4, 5, 21]


def test_schedule_under_pivot_limits():
    # (12, 1, 2, 7, None): call 1 opens with batch 12 (one generic pivot) and a batch of 24 cut to the 11 pivots left: the limit
    # falls on the last fused pivot queued; call 2 is the opening pivot alone; call 3 the opening pivot and a batch of one
    # (generic); call 4 the opening pivot, then 1 + 5; call 5 runs to the end
    g = df.generic_indices(99, False, df.LIMIT_CALLS)
    assert g == [0, 1, 12, 13, 14, 15, 16, 22, 23, 39, 71]
    assert df.generic_indices(20, False, (12, 1, 2, 7, None)) == [0, 1, 12, 13, 14, 15, 16]  # the solve ends inside call 4
    assert df.generic_indices(10, False, (12, None)) == [0, 1]  # the limit is never reached: the second call does nothing


def test_schedule_under_a_stall_limit():
    D, N = True, False
    # limit 1: the opening pivot is degenerate, so the batch of 16 behind it is generic throughout (1..16); the count is
    # back to 0 at its end and the batch of 32 is fused again
    deg = [D, D, D, N] + [N] * 96
    assert df.generic_indices(100, False, (None,), degenerate=deg, stall_limit=1) == list(range(0, 17)) + [17, 49]
    # the same with the count still at the limit where that batch ends: one more generic batch
    deg = [D] * 17 + [N] * 83
    assert df.generic_indices(100, False, (None,), degenerate=deg, stall_limit=1) == list(range(0, 49)) + [49]
    # limit 3: pivots 0, 1 generic, pivot 2 fused (count 2), count 3 after it: the fused run stops, 3..34 generic
    deg = [D, D, D, D, N] + [N] * 95
    assert df.generic_indices(100, False, (None,), degenerate=deg, stall_limit=3) == [0, 1] + list(range(3, 35)) + [35, 99]
    # a count that never reaches the limit changes nothing
    assert df.generic_indices(100, False, (None,), degenerate=[D, D, N] * 34, stall_limit=3) == df.generic_indices(100, False, (None,))


def test_the_table_covers_every_edge():
    assert [c.n for c in df.COLUMNS] == [df.DA_THREADS - 2, df.DA_THREADS - 1, df.DA_THREADS, df.DA_THREADS + 1]
    assert [c.m for c in df.ROWS] == [df.DA_THREADS - 1, df.DA_THREADS, df.DA_THREADS + 1]
    assert [c.n for c in df.COLUMN_TILES] == [df.FB_COLS - 2, df.FB_COLS - 1, df.FB_COLS, df.FB_COLS + 1]
    assert [c.m for c in df.ROW_TILES] == [df.ROW_TILE - 1, df.ROW_TILE, df.ROW_TILE + 1] and df.ROW_TILE in df.FB_TR
    assert all(df.RAGGED.m % tr != 0 for tr in df.FB_TR) and df.RAGGED.m % 4 == 1  # every depth's last block ends early; row 61 alone at depth 4
    # below the size rule, so that mode 1 leaves every case to the generic path
    assert all((c.m + 3) * (c.n + 1) < ga.DUAL_FUSED_MIN for c in df.CASES + df.ROW_TILES)


# ------------------------------------------------------------------------------------------------ the instances
@pytest.mark.parametrize("case", [c for c in df.CASES + df.ROW_TILES if c not in df.LIMITS], ids=df.case_id)
def test_instance_has_its_events_at_fused_pivots(logs, case):
    log, end = logs(case)
    inst = case.instance()
    assert ga.slack_dual_infeasibilities(inst) == 0 and ga.slack_signs(inst).any()  # the dual simplex from pivot 0
    assert (end.rc, end.status, len(log), end.pert_cnt) == (0, case.status, case.total, 0)
    assert end.bland_cnt == (case.bland or 0) and sum(x.bland for x in log) == end.bland_cnt
    if case.stall_limit is None:  # the default limit, 64 + (m + n) / 8 consecutive degenerate pivots, is never reached
        run = longest = 0
        for x in log:
            run = run + 1 if x.degenerate else 0
            longest = max(longest, run)
        assert longest < 64 + (len(inst["row_b"]) + case.n) // 8
    fused = fused_of(case, log)
    print("%s: %d pivots, %d of them fused" % (case.name, len(log), len(fused)))
    assert len(fused) == df.expected_fused(case)
    for kind, idx in case.events:
        hits = [k for k in fused if (log[k].p if kind == "p" else log[k].q) == idx]
        print("%s: %s == %d at fused pivots %s" % (case.name, kind, idx, hits))
        assert hits, (case.name, kind, idx)
    assert len(df.repeats_at(log, fused)) >= case.repeats
    # the end is the fused pair's to find: the last pivot is fused and k_da runs once more behind it (no leaving row: the
    # phase is over; no entering column: NOFEAS) -- the pivot after the last would have been a fused one
    if case.calls == (None,) and case.stall_limit is None:
        assert case.total - 1 in fused and case.total not in df.generic_indices(case.total + 1, False, case.calls)
    if case.stall_limit is not None:
        # Bland's rule takes pivots the schedule alone would have given the fused pair; at 1025x60 it hands the solve back
        # (fused pivots behind the last Bland pivot), at 60x513 it keeps most of it
        openers = df.generic_indices(case.total, False, case.calls)
        last_bland = max(k for k, x in enumerate(log) if x.bland)
        assert len(fused) < case.total - len(openers)
        if case.m > case.n:
            assert any(k > last_bland for k in fused) and 2 * len(fused) > case.total
        else:
            assert 2 * case.bland > case.total and len(fused) <= 1
        # the recomputed degeneracy flags reproduce the oracle's own Bland pivots: the rule is in force exactly while the
        # count of consecutive degenerate pivots in front of a pivot is at or above the limit
        stall, mine = 0, []
        for x in log:
            mine.append(stall >= case.stall_limit)
            stall = stall + 1 if x.degenerate else 0
        assert mine == [x.bland for x in log]


def test_row_cases_cover_the_flags(logs):
    for case in df.ROWS:
        log, _ = logs(case)
        fl = [log[k] for k in fused_of(case, log)]
        assert {NL, NU} <= {x.enter for x in fl} and {NL, NU, NS} <= {x.leave for x in fl}, case.name


def test_column_tile_cases_enter_on_both_sides_of_the_tile_edge(logs):
    sides = set()
    for case in df.COLUMN_TILES:
        log, _ = logs(case)
        fl = [log[k] for k in fused_of(case, log)]
        sides |= {(x.q >= df.FB_COLS, x.q % 2) for x in fl}
        assert {x.q % 2 for x in fl if x.q < df.FB_COLS} == {0, 1}, case.name
        if case.n >= df.FB_COLS:
            assert any(x.q >= df.FB_COLS for x in fl), case.name
    assert sides == {(False, 0), (False, 1), (True, 0), (True, 1)}


def test_limit_cases_stop_inside_and_at_the_end_of_fused_runs(orc):
    """The stops of (12, 1, 2, 7, None) against the schedule: after call 1 the last pivot made was fused and the last one
    queued; call 3 ends on a generic pivot that opened a batch; call 4 ends behind five fused pivots."""
    for case in df.LIMITS:
        g = set(df.case_generic(case))
        assert 11 not in g and 10 not in g and {12, 13, 14, 15, 16} <= g and not (set(range(17, 22)) & g) and 22 in g
        stops = ga.run_calls(ga.load(orc, case.instance()), case.calls)
        assert stops == [(EITLIM, capi.INFEAS, 12), (EITLIM, capi.INFEAS, 13), (EITLIM, capi.INFEAS, 15), (EITLIM, capi.INFEAS, 22), (0, OPT, case.total)]
        assert df.expected_fused(case) == case.total - len(g) and case.total < 64 + (case.m + case.n) // 8


# ------------------------------------------------------------------------------------------------ warm starts
def test_warm_starts_take_the_pivots_the_table_says(orc):
    root = df.warm_root(orc)
    assert root.status == OPT and root.m == df.WARM_ILP[0]
    branches = df.warm_branches(root)
    assert len(branches) == 2 * df.WARM_COLUMNS

    def children(parent):
        out = []
        for br in branches:
            k = df.warm_child(orc, parent, br)
            assert k.simplex() == 0 and k.status == OPT and k.bland_cnt == parent.bland_cnt
            out.append(k.it_cnt - parent.it_cnt)
        return out

    assert children(root) == df.WARM_PIVOTS["children"]
    assert 1 in df.WARM_PIVOTS["children"]  # k_dboot finds the solve over behind the generic pivot
    assert max(df.WARM_PIVOTS["children"]) > df.BATCH_FIRST  # a second batch
    cut_root, taken = root.copy(), []
    from . import thresholds as th

    for vals, rhs in df.warm_cuts(orc, root):
        before = cut_root.it_cnt
        assert th.append_cut(orc, cut_root, vals, rhs) == 0 and cut_root.status == OPT
        taken.append(cut_root.it_cnt - before)
    assert taken == df.WARM_PIVOTS["cuts"] and min(taken) > 0
    assert cut_root.m == df.WARM_ILP[0] + df.WARM_CUTS == 65  # past the 64 | 65 edge of every tile depth
    # the same columns are still fractional, so the same branches apply
    assert [b[:2] for b in df.warm_branches(cut_root)] == [b[:2] for b in branches]
    branches = df.warm_branches(cut_root)
    assert children(cut_root) == df.WARM_PIVOTS["cut-children"]
