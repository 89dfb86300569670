"""GPU: the fused dual path -- k_dboot, k_da and the twelve k_fb<TR, 1, NT, 1> -- at its block edges, forced by
mvx_set_dual_fused(2) at shapes far below the size rule.  Every case of dual_fused.py is solved on the engine and held
against the oracle bit for bit at every stop of its call schedule; mvx_dual_fused_stats, counted on the device, must have
moved by exactly the pivots the schedule (dual_fused.generic_indices) leaves to the fused pair; the end state gets the
independent certificate of tests/certify.py.  Each case runs again with the path off (mode 0) and under the size rule
(mode 1): the same bits, and a counter that stands still.  test_dual_fused_inputs.py proves on the oracle alone that each
instance has its event -- the last column entering, the last row leaving, the same row twice -- at a fused pivot.  No
pivot log is computed here."""
import ctypes as C

import pytest

from mvolps_amd import capi
from mvolps_amd.capi import EITLIM, OPT

from . import certify as cf
from . import dual_fused as df
from . import general_at_size as ga
from . import thresholds as th
from .test_gpu_certify import batch
from .test_gpu_general_at_size import Frozen, same

pytestmark = pytest.mark.gpu

MODES = [2, 0, 1]  # always, never, the size rule
EXACT_ROWS = 33


def fused_stats(api):
    boots, pivots = C.c_longlong(0), C.c_longlong(0)
    api.dual_fused_stats(C.byref(boots), C.byref(pivots))
    return boots.value, pivots.value


@pytest.fixture(scope="module", autouse=True)
def forced(gpu, orc):
    """Mode 2 for the whole file; dual chains off, so that a generic step is one pivot and the schedule can be counted"""
    gpu.set_dual_fused(2)
    gpu.set_dual_chain(1)
    gpu.set_cluster(1)
    yield gpu
    gpu.set_dual_fused(-1)
    gpu.set_tuning(0, 1, -1)
    gpu.set_stall_limit(0)
    orc.set_stall_limit(0)
    gpu.set_dual_chain(0)


_REF = {}


def reference(orc, case):
    """The oracle's state at every stop of the case's schedule, computed once and shared by every mode and variant"""
    if case.name not in _REF:
        orc.set_stall_limit(case.stall_limit or 0)
        try:
            o = ga.load(orc, case.instance())
            out = []
            for lim in case.calls:
                rc = o.simplex(it_lim=lim)
                out.append(Frozen(o, rc))
                if rc != EITLIM:
                    break
        finally:
            orc.set_stall_limit(0)
        _REF[case.name] = out
    return _REF[case.name]


def run_case(gpu, orc, case, mode, tuning=None):
    ref = reference(orc, case)
    inst = case.instance()
    gpu.set_stall_limit(case.stall_limit or 0)
    gpu.set_dual_fused(mode)
    if tuning is not None:
        gpu.set_tuning(*tuning)
    try:
        g = ga.load(gpu, inst)
        before = fused_stats(gpu)
        for k, fz in enumerate(ref):
            assert g.simplex(it_lim=case.calls[k]) == fz.rc, (case.name, k)
            same(g, fz, "%s mode %d stop %d" % (case.name, mode, k))
        after = fused_stats(gpu)
    finally:
        gpu.set_stall_limit(0)
        gpu.set_dual_fused(2)
        if tuning is not None:
            gpu.set_tuning(0, 1, -1)
    boots, pivots = after[0] - before[0], after[1] - before[1]
    want = df.expected_fused(case) if mode == 2 else 0
    print("%s mode %d tuning %s: %d pivots, fused %d (schedule: %d), k_dboot started %d runs" % (case.name, mode, tuning, g.it_cnt, pivots, want, boots))
    assert (g.it_cnt, g.status, ref[-1].rc) == (case.total, case.status, 0)
    assert g.bland_cnt == (case.bland or 0)
    assert pivots == want, (case.name, mode, pivots, want)
    assert (boots > 0) if want > 0 else (mode == 2 or boots == 0)
    # exact fractions where they take about a second (the 31..33-row cases, once); with 500 and more columns and 40..61 rows
    # they take 6 to 10 s per state, so the certificate is certify.py's long double one there, as above 64 rows
    ga.certify_end(case, inst, g, 0, exact=(case.m <= EXACT_ROWS and mode == 2))
    return g


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", df.CASES, ids=df.case_id)
def test_case_at_a_block_edge(gpu, orc, case, mode):
    run_case(gpu, orc, case, mode)


@pytest.mark.parametrize("mode", [2, 0])
@pytest.mark.parametrize("case", df.ROW_TILES, ids=df.case_id)
def test_row_tiles_of_32(gpu, orc, case, mode):
    """m = 31, 32, 33 under 32-row tiles: one partial block, one full block, a second block of one row; row m leaves and
    column 513 -- the lower half of a double2 whose upper half lies behind the last column -- enters at fused pivots"""
    run_case(gpu, orc, case, mode, tuning=(df.ROW_TILE, 1, -1))


@pytest.mark.parametrize("nt", df.FB_NT)
@pytest.mark.parametrize("tr", df.FB_TR)
def test_every_variant_of_the_dual_update(gpu, orc, tr, nt):
    """All twelve k_fb<TR, 1, NT, 1> of launch_db on 61x513; the counter shows that its pivots were theirs"""
    run_case(gpu, orc, df.RAGGED, 2, tuning=(tr, 1, nt))


# ------------------------------------------------------------------------------------------------ warm starts
@pytest.fixture(scope="module")
def warm(orc):
    """The oracle's side, once: root, branches, the solved children, the root with its cuts and its children"""
    from mvolps_amd import synth

    A, b, c, U = synth.dense_ilp(*df.WARM_ILP)
    root = df.warm_root(orc)
    branches = df.warm_branches(root)
    cuts = df.warm_cuts(orc, root)
    cut_root, cut_stops = root.copy(), []
    for vals, rhs in cuts:
        assert th.append_cut(orc, cut_root, vals, rhs) == 0
        cut_stops.append(Frozen(cut_root, 0))
    cut_branches = df.warm_branches(cut_root)

    def solved(parent, brs):
        out = []
        for br in brs:
            k = df.warm_child(orc, parent, br)
            assert k.simplex() == 0
            out.append(k)
        return out

    return dict(model=cf.Model.ilp(A, b, c, U), root=root, branches=branches, kids=solved(root, branches), cuts=cuts, cut_stops=cut_stops,
                cut_root=cut_root, cut_branches=cut_branches, cut_kids=solved(cut_root, cut_branches))


def child_model(M, branch):
    j, _, (lo, hi) = branch
    Mc = M.copy()
    Mc.set_col_bnds(j, capi.DB, lo, hi)
    return Mc


def resolve(gpu, g, o, mode, pivots, what):
    """One warm re-solve of an engine handle against the oracle's solved one: bits, pivots of the table, the counter"""
    it0, before = g.it_cnt, fused_stats(gpu)
    assert g.simplex() == 0
    moved = fused_stats(gpu)[1] - before[1]
    same(g, o, what)
    assert g.it_cnt - it0 == pivots, (what, g.it_cnt - it0, pivots)
    assert moved == (df.warm_fused(pivots) if mode == 2 else 0), (what, mode, moved, pivots)
    return moved


@pytest.mark.parametrize("mode", MODES)
def test_warm_started_children(gpu, orc, warm, mode):
    """Both branches of six fractional columns of the 61x513 root: every batch of a start with the dual hint gives its first
    pivot to the generic step and the rest to the fused pair; a one-pivot child is the run that k_dboot starts and k_da
    finds over.  Then the root's repaired GMI cuts, one re-solve each, take m from 61 to 65 -- past a block edge of every
    tile depth -- and the same branches are solved from there."""
    gpu.set_dual_fused(mode)
    try:
        root = df.warm_root(gpu)
        same(root, warm["root"], "root")
        M = warm["model"]
        boots0 = fused_stats(gpu)[0]
        for k, br in enumerate(warm["branches"]):
            g = df.warm_child(gpu, root, br)
            resolve(gpu, g, warm["kids"][k], mode, df.WARM_PIVOTS["children"][k], "child %s" % (br[:2],))
            cf.certify(child_model(M, br), g, exact=False, what="child %s" % (br[:2],))
        assert (fused_stats(gpu)[0] - boots0 >= len(warm["branches"])) if mode == 2 else (fused_stats(gpu)[0] == boots0)
        Mc, cut_root = M.copy(), root.copy()
        for k, (vals, rhs) in enumerate(warm["cuts"]):
            it0, before = cut_root.it_cnt, fused_stats(gpu)
            assert th.append_cut(gpu, cut_root, vals, rhs) == 0
            moved = fused_stats(gpu)[1] - before[1]
            same(cut_root, warm["cut_stops"][k], "cut %d" % k)
            pivots = df.WARM_PIVOTS["cuts"][k]
            assert cut_root.it_cnt - it0 == pivots and moved == (df.warm_fused(pivots) if mode == 2 else 0), (k, moved)
            Mc.add_row(vals[1:], capi.LO, float(rhs), 0.0)
        assert cut_root.m == 65
        cf.certify(Mc, cut_root, exact=False, what="root with cuts")
        for k, br in enumerate(warm["cut_branches"]):
            g = df.warm_child(gpu, cut_root, br)
            resolve(gpu, g, warm["cut_kids"][k], mode, df.WARM_PIVOTS["cut-children"][k], "cut child %s" % (br[:2],))
            cf.certify(child_model(Mc, br), g, exact=False, what="cut child %s" % (br[:2],))
    finally:
        gpu.set_dual_fused(2)


def test_a_batch_does_not_take_the_fused_path(gpu, orc, warm):
    """mvx_simplex_batch over eight of the children under mode 2: the oracle's bits, and a counter that stands still"""
    root = df.warm_root(gpu)
    kids = [df.warm_child(gpu, root, br) for br in warm["branches"][:8]]
    before = fused_stats(gpu)
    assert batch(gpu, kids) == [0] * 8
    assert fused_stats(gpu) == before
    for k, g in enumerate(kids):
        same(g, warm["kids"][k], "batch child %d" % k)
        assert g.status == OPT
