"""GPU: general-bound LPs at kernel scale -- phase 1 past one wave, one lane chunk, one k_p1_fix block and one pricing
stride, primal phase 2 on free / fixed / upper-bounded non-basic columns behind it, cold dual starts on and past k_dsel and
on the fused dual pair.  Every case (general_at_size.CASES) is solved in limited calls on the engine and the oracle side by
side: the state is compared bitwise at every stop (inside phase 1 or the cold dual, past the phase boundary, at the end),
twice over (the second time on the slab the first handle gave back); the end state then gets the independent certificate
of its status and, where the instance was built around a point, that point is checked exactly and NOFEAS is a failure.
test_general_at_size_inputs.py proves on the oracle alone that each instance has the property relied on here."""
import ctypes as C

import pytest

from mvolps_amd import synth
from mvolps_amd.capi import EITLIM, OPT

from . import general_at_size as ga
from . import thresholds as th
from .test_gpu_certify import batch, paths  # noqa: F401  (fixture)
from .test_gpu_chain import cluster_counts
from .test_gpu_parity import assert_same_state
from .test_gpu_thresholds import dsel_chains, persist_counts, round_stats
from .general_at_size import STEPWISE

pytestmark = pytest.mark.gpu


class Frozen:
    """What assert_same_state reads from a handle, copied: the oracle's state at one stop, kept for the second run"""

    def __init__(self, P, rc):
        self.rc = rc
        self.status, self.it_cnt, self.obj, self.pert_cnt, self.bland_cnt = P.status, P.it_cnt, P.obj, P.pert_cnt, P.bland_cnt
        self._v = dict(basis=P.basis(), tableau=P.tableau(), col_prim=P.col_prim(), row_prim=P.row_prim(), col_stat=P.col_stat(),
                       row_stat=P.row_stat())

    def __getattr__(self, name):
        v = self.__dict__["_v"][name]
        return lambda: v


def same(g, o, what):
    assert_same_state(g, o, what)
    assert g.pert_cnt == o.pert_cnt and g.bland_cnt == o.bland_cnt, what


def side_by_side(api, orc, case, inst):
    """The schedule on both sides, compared at every stop, then the engine alone a second time on the recycled slab.
    Returns the engine's last handle and the stops."""
    o = ga.load(orc, inst)
    frozen, stops = [], []
    g = ga.load(api, inst)
    for k, lim in enumerate(case.calls):
        rcs = [P.simplex(it_lim=lim) for P in (g, o)]
        assert rcs[0] == rcs[1], (case.name, k, rcs)
        same(g, o, "%s stop %d" % (case.name, k))
        stops.append((rcs[1], o.status, o.it_cnt))
        frozen.append(Frozen(o, rcs[1]))
        if rcs[1] != EITLIM:
            break
    del g
    g = ga.load(api, inst)
    for k, fz in enumerate(frozen):
        assert g.simplex(it_lim=case.calls[k]) == fz.rc, (case.name, k)
        same(g, fz, "%s stop %d, second run" % (case.name, k))
    return g, stops


def dual_fused_pivots(api):
    boots, pivots = C.c_longlong(0), C.c_longlong(0)
    api.dual_fused_stats(C.byref(boots), C.byref(pivots))
    return pivots.value


@pytest.mark.parametrize("case", ga.CASES, ids=ga.case_id)
def test_general_bounds_at_size(gpu, orc, case):
    """Path counters: k_chain's launches are read from cluster_stats wherever a limited call starts in primal phase 2, k_dsel's
    chains from the round histogram on the cold dual starts.  Phase 1 has no counter: that its kernels ran follows from the
    INFEAS stop after the first call.  dual-1100x2000 lies inside the entry-count rule of dual_fused_worth_it: that k_da +
    k_fb<DUAL> took pivots of it is read from mvx_dual_fused_stats, counted on the device, and no smaller case moves it."""
    inst = case.instance()
    before, fused_before = cluster_counts(gpu), dual_fused_pivots(gpu)
    with round_stats(gpu) as since:
        g, stops = side_by_side(gpu, orc, case, inst)
        d = since()
    after, fused = cluster_counts(gpu), dual_fused_pivots(gpu) - fused_before
    print("%s: stops %s, k_chain launches +%d aborts +%d, round histogram moved by %s, fused dual pivots +%d"
          % (case.name, stops, after[0] - before[0], after[1] - before[1], d.tolist(), fused))
    assert stops == case.stops
    in_rule = ga.DUAL_FUSED_MIN <= (case.rows + 1) * (case.n + 1) < ga.DUAL_FUSED_MAX
    assert (fused > 0) == (case.family == "cold" and in_rule), (case.name, fused)
    assert after[1] == before[1], "a k_chain launch gave up"
    if len(stops) == 3:  # a limited call that starts in primal phase 2: the chained path, chosen by k_chain
        assert after[0] > before[0], "no k_chain launch was made"
    if case.family == "cold":
        chains, long_chains, passed = dsel_chains(d)
        if case.m <= th.DSEL_MAX and case.n <= th.DSEL_MAX:
            assert long_chains > 0, d.tolist()
        elif case.m > th.DSEL_MAX:
            assert not d[1:th.DCH_MAX + 3].any(), d.tolist()
    ga.certify_end(case, inst, g, stops[-1][0])


@pytest.mark.parametrize("name", ["p2-300x700", "p1-65x40"])
def test_phase_two_on_general_flags_with_the_cluster_off(paths, orc, name):
    """k_persist (300x700: three columns per workgroup) and k_pc / k_pr choose the steps of phase 2 instead of k_chain."""
    case = ga.by_name(name)
    inst = case.instance()
    for persist in (1, 0):
        paths.set_cluster(0)
        paths.set_persist(persist)
        before, cb = persist_counts(paths), cluster_counts(paths)
        g, stops = side_by_side(paths, orc, case, inst)
        after, ca = persist_counts(paths), cluster_counts(paths)
        assert stops == case.stops and ca[0] == cb[0]
        assert after[1] == before[1], "a k_persist launch gave up"
        if persist and th.persist_plan(case.m, case.n, 256) is not None:
            assert after[0] > before[0], "k_persist was not launched"
        if not persist:
            assert after[0] == before[0]
        ga.certify_end(case, inst, g, stops[-1][0])


def debug_counters(api):
    out = (C.c_longlong * 8)()
    api.lib.mvx_debug_counters(out, 0)
    return list(out)


def test_one_batch_window_with_three_kinds_of_start(gpu, orc):
    """A phase-1 start, a cold dual start and a primal feasible LP of three shapes in one mvx_simplex_batch call: the
    phase-1 one is handed to the single-handle path; each result equals its one-by-one solve and the oracle's."""
    insts = [ga.by_name("p1-300x255").instance(), ga.by_name("dual-300x600").instance()]
    A, b, c = synth.dense_lp(320, 500, 17)

    def load_all(api):
        P = [ga.load(api, i) for i in insts] + [api.create()]
        P[2].load_dense(A, b, c)
        return P

    alone, ref = load_all(gpu), load_all(orc)
    for P in alone + ref:
        assert P.simplex() == 0
    before = debug_counters(gpu)
    window = load_all(gpu)
    assert batch(gpu, window) == [0, 0, 0]
    assert debug_counters(gpu)[4] == before[4] + 1  # one job handed to the single-handle path: the phase-1 start
    for k in range(3):
        same(window[k], alone[k], "batch job %d against its own solve" % k)
        same(window[k], ref[k], "batch job %d against the oracle" % k)
    assert [P.status for P in window] == [OPT, OPT, OPT]


def test_stepwise_2049x256_ends_optimal_under_both_call_patterns(gpu, orc):
    """general_lp(2049, 256, 5) in calls of 500 (the oracle used to end NOFEAS at 7698, the engine with it), and in calls
    of 20 from 7500 (NOFEAS at 7749): bitwise at every stop, rows per lane R = 3 in k_p1_head, OPT and certified at the
    end, the NOFEAS recheck's rebuild counted on both sides."""
    inst = STEPWISE.instance()
    g, o = ga.load(gpu, inst), ga.load(orc, inst)
    forks = None
    rcs = [EITLIM, EITLIM]
    while rcs[1] == EITLIM:
        rcs = [P.simplex(it_lim=500) for P in (g, o)]
        assert rcs[0] == rcs[1]
        same(g, o, "calls of 500, at %d" % o.it_cnt)
        if o.it_cnt == 7500:
            forks = (g.copy(), o.copy())
    assert rcs[1] == 0 and o.status == OPT
    assert gpu.get_refresh_cnt(g.h) == orc.get_refresh_cnt(o.h) >= 1
    ga.certify_end(STEPWISE, inst, g, 0)
    g, o = forks
    rcs = [EITLIM, EITLIM]
    while rcs[1] == EITLIM:
        rcs = [P.simplex(it_lim=20) for P in (g, o)]
        assert rcs[0] == rcs[1] and o.it_cnt < 9000
    same(g, o, "calls of 20 from 7500")
    assert rcs[1] == 0 and o.status == OPT
    ga.certify_end(STEPWISE, inst, g, 0)
