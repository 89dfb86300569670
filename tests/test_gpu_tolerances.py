"""GPU: the three simplex tolerances of mvx_smcp on every selection path, bitwise against the oracle under the same `parm`.

Every path re-implements the comparisons that use tol_bnd, tol_dj and tol_piv and reads the values from another place (Ctl,
ChainArgs filled in job_begin, the batch's own Ctl fill); on the data of the rest of the suite a kernel that hard-coded
1e-9, or compared with >= where the definition is >, would pass.  Here each path runs, at the smallest shape at which it is
the path taken, the instances of tolerances.py under every tolerance set of the table -- test_tolerances_inputs.py proves on
the oracle alone that each single coarse field changes the pivot count or the final basis there -- and is compared at
every stop of a call schedule (status, return code, it_cnt, pert_cnt, bland_cnt, tableau, basis, values); end states that
are OPT get certify.py's certificate under the call's tolerances; the engine's own counters show that the path under test
ran.  The boundary models put a value exactly on each threshold and one double past it, at a lane tail, in a second wave
and in a second workgroup; their outcomes are written down by hand.  The last section holds the tolerances as state of the
handle (last_tol / already_solved, clones, the defaults behind a NULL parm) and a B&B prefix under coarse defaults (admitted
by the CPU companion: the oracle's tree differs from the default one and costs fewer pivots).

The case table, with the oracle's figures (rc, status, pivots at every stop; E = EITLIM, F = FEAS, I = INFEAS):

    default-96x160     sensitive_lp(96, 160, 3)    calls (7, 20, end)   DEFAULT 44  BND 52   DJ 42   PIV 45 NOFEAS  ALL 46
    chain-300x700      sensitive_lp(300, 700, 37)  calls (7, end)       DEFAULT 172 BND 239  DJ 161  PIV 391        ALL 250
    persist-200x300    sensitive_lp(200, 300, 1)   calls (7, 50, end)   DEFAULT 193 BND 150  DJ 186  PIV 282        ALL 57 NOFEAS
    phase1-62x40       general_lp(62, 40, 4)       calls (10, 110, end) DEFAULT 128 BND 135  DJ 127  PIV 127        ALL 128 (another basis)
    children-128x256   dense_ilp(128, 256, 7, 3)   root under the set   DEFAULT 117 BND 117  DJ 109  PIV 129        ALL 127, eight children each
    children-1000x2001 dense_ilp(1000, 2001, 7, 3) root under DEFAULT   1436, six children of 0 to 57 dual pivots under each set

NOFEAS under PIV / ALL: rows the coarse ratio test skipped end up violated; recorded, no certificate expected.  No (case,
set) pair is dropped: the seeds are those at which every set ends within four times the DEFAULT pivots (tolerances.py says
which seeds were passed over and why).  At 1000x2001 tol_dj is not asserted to matter (k_dboot / k_da do not read it and a
DEFAULT root leaves it nothing to decide); roots under PIV / ALL run past the 4x rule there, so the root is DEFAULT's.
That k_dboot / k_da take the 1000x2001 children is read from mvx_dual_fused_stats, counted on the device.

Oracle seconds (CPU companion): 0.01 per solve up to 128x256, 0.03 at 300x700, 0.7 for the 1000x2001 root.  First device
run (MI355X, all six positions in the boundary loop): the file 10.5 s for 24 tests, of which 1.6 s is the session's set-up;
the 1000x2001 leg 1.27 s, the longest; every other test 0.55 s or less.  test_gpu_thresholds.py took 8.5 s on the same run,
so the boundary loop on the device was thinned by index to positions 1, 65 and last (the CPU companion keeps all six):
7.9 s on the next run.

Mutation check (scratch copies, never committed).  (i) job_begin filling ChainArgs.tol_piv with 1e-9: fails the primal rows
default, k_chain-5, k_chain-by-size and two-launch under PIV, the pivot model on those paths, and everything whose root is
a primal solve under PIV (the dual rows, the batch, the B&B leg) -- the default 96x160 row with them, because the chained
pipeline takes every primal call; k_persist, phase 1, the 1000x2001 leg and the handle-state tests pass.  (ii) ratio_row
with aa >= tp: fails the pivot model on all four primal paths, both leads, and nothing else.  The suite as it was before
this file passes under both."""
import ctypes as C

import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import EITLIM, OPT

from . import certify as cf
from . import lpgen
from . import tolerances as tl
from .test_gpu_certify import paths  # noqa: F401  (fixture)
from .test_gpu_chain import cluster_counts
from .test_gpu_parity import assert_same_state
from .test_gpu_thresholds import dsel_chains, persist_counts, round_stats

pytestmark = pytest.mark.gpu


def same(g, o, what):
    assert_same_state(g, o, what)
    assert g.pert_cnt == o.pert_cnt and g.bland_cnt == o.bland_cnt, what


# ------------------------------------------------------------------------------------------------ the path matrix
# path -> (case, persist, cluster, chain, cluster launches expected, persist launches expected).  "default" is the small
# shape under the default settings: job_enqueue hands every primal call to the chained pipeline, so k_chain (length by
# size) chooses the steps there too and the generic k_select step only closes each batch; on its own k_select chooses in
# phase 1 ("phase1"), in the dual simplex (the dual rows below with one pivot a pass) and under Bland's rule.
PRIMAL_PATHS = {
    "default": ("default-96x160", 1, 1, 0, True, False),
    "k_chain-5": ("chain-300x700", 0, 1, 5, True, False),
    "k_chain-by-size": ("chain-300x700", 0, 1, 0, True, False),
    "two-launch": ("chain-300x700", 0, 0, 5, False, False),
    "k_persist": ("persist-200x300", 1, 0, 0, False, True),
    "phase1": ("phase1-62x40", 1, 1, 0, None, None),
}
BOUNDARY_PATHS = ("default", "k_chain-5", "two-launch", "k_persist")


class forced:
    """with forced(api, path) as moved: ...; moved() -> (cluster launches, cluster aborts, persist launches, persist aborts)
    since the start.  The `paths` fixture puts the settings back."""

    def __init__(self, api, path):
        self.api, self.path = api, path

    def __enter__(self):
        _, persist, cluster, chain, _, _ = PRIMAL_PATHS[self.path]
        self.api.set_persist(persist)
        self.api.set_cluster(cluster)
        self.api.set_chain(chain)
        base = cluster_counts(self.api) + persist_counts(self.api)
        return lambda: tuple(a - b for a, b in zip(cluster_counts(self.api) + persist_counts(self.api), base))

    def __exit__(self, *exc):
        return False


def assert_path_ran(path, moved, what):
    _, _, _, _, cluster, persist = PRIMAL_PATHS[path]
    cl, cl_abort, pe, pe_abort = moved
    assert cl_abort == 0 and pe_abort == 0, (what, "a k_chain or k_persist launch gave up", moved)
    if cluster is not None:
        assert (cl > 0) == cluster, (what, "k_chain launches", moved)
    if persist is not None:
        assert (pe > 0) == persist, (what, "k_persist launches", moved)


@pytest.mark.parametrize("path", list(PRIMAL_PATHS))
def test_primal_paths_under_every_tolerance_set(paths, orc, path):
    case = tl.by_name(PRIMAL_PATHS[path][0])
    inst = case.instance()
    M = tl.model(inst)
    for name in case.sets:
        tol = tl.SETS[name]
        with forced(paths, path) as moved:
            g, o = tl.load(paths, inst), tl.load(orc, inst)
            stops = []
            for k, lim in enumerate(case.calls):
                rcs = [P.simplex(it_lim=-1 if lim is None else lim, tol=tol) for P in (g, o)]
                assert rcs[0] == rcs[1], (path, name, k, rcs)
                same(g, o, "%s under %s, stop %d" % (path, name, k))
                stops.append((rcs[1], o.status, o.it_cnt))
                if rcs[1] != EITLIM:
                    break
            d = moved()
        print("%s under %s: stops %s, k_chain +%d (aborts +%d), k_persist +%d (aborts +%d)" % ((path, name, stops) + d))
        assert stops == case.figures[name]
        assert_path_ran(path, d, (path, name))
        if g.status == OPT:
            tl.certify_end(M, g, tol, "%s under %s" % (path, name))


@pytest.mark.parametrize("lead", tl.LEADS)
@pytest.mark.parametrize("path", BOUNDARY_PATHS)
def test_boundary_models_on_every_primal_path(paths, orc, path, lead):
    """A value exactly on each threshold and one double past it, the special row / column at a lane tail, in a second wave,
    in a second workgroup and last: the hand-derived outcome, and the oracle's bits.  lead = 3: the decision is the fourth
    step of the call (inside the first chain of five on the chained paths)."""
    case = tl.by_name(PRIMAL_PATHS[path][0])
    m, n = case.m, case.n
    with forced(paths, path) as moved:
        for pos in tl.POSITIONS_ON_DEVICE:
            for name, inst, tol, lim, expected in tl.boundary_outcomes(m, n, pos, lead):
                what = "%s on %s at %d, lead %d" % (name, path, pos, lead)
                g, o = tl.load(paths, inst), tl.load(orc, inst)
                rcs = [P.simplex(it_lim=lim, tol=tol) for P in (g, o)]
                tl.assert_outcome(g, rcs[0], expected, what)
                assert rcs[0] == rcs[1], what
                same(g, o, what)
        d = moved()
    assert d[1] == 0 and d[3] == 0, d
    if lead and path in ("default", "k_chain-5"):
        assert d[0] > 0, "no k_chain launch was made"
    if lead and path == "k_persist":
        assert d[2] > 0, "k_persist was not launched"
    if path == "two-launch":
        assert d[0] == 0 and d[2] == 0, d


# ------------------------------------------------------------------------------------------------ dual paths
def children_side_by_side(api, orc, case, name, batch_slots=None):
    """Root and near_children on both sides under a set; the engine's children one by one, or through one
    mvx_simplex_batch call with a non-NULL parm.  Returns the figures and the engine's handles."""
    tol = tl.SETS[name]
    root_tol = tol if case.own_root else tl.DEFAULT
    A, b, c, U = case.data()
    g, o = synth.load_ilp(api, A, b, c, U), synth.load_ilp(orc, A, b, c, U)
    rcs = [P.simplex(tol=root_tol) for P in (g, o)]
    assert rcs[0] == rcs[1]
    same(g, o, "%s root under %s" % (case.name, name))
    ko = tl.near_children(orc, o, tol, case.count)
    kg = tl.near_children(api, g, tol, case.count, solve=batch_slots is None)
    if batch_slots is not None:
        arr = (C.c_void_p * len(kg))(*[k[3].h for k in kg])
        out = (C.c_int * len(kg))()
        parm = tl.smcp(api, tol)
        assert api.simplex_batch(arr, len(kg), C.byref(parm), out) == 0
        kg = [k[:4] + (rc,) for k, rc in zip(kg, out)]
    for a, r in zip(kg, ko):
        assert a[:3] == r[:3] and a[4] == r[4], (case.name, name, a[:3], a[4], r[4])
        same(a[3], r[3], "%s child %d/%s under %s" % (case.name, a[0], a[1], name))
    return (rcs[1], o.status, o.it_cnt), [(k[4], k[3].status, k[3].it_cnt) for k in ko], g, kg


def certify_children(case, name, g, kg):
    M = cf.Model.ilp(*case.data())
    tol = tl.SETS[name]
    tl.certify_end(M, g, tol if case.own_root else tl.DEFAULT, "%s root under %s" % (case.name, name))
    for Mc, k in zip(tl.child_models(M, kg), kg):
        if k[3].status == OPT:
            tl.certify_end(Mc, k[3], tol, "%s child %d/%s under %s" % (case.name, k[0], k[1], name))


@pytest.mark.parametrize("dchain", [8, 0, 1], ids=["k_dsel-chains-of-8", "default-setting", "one-pivot-a-pass"])
def test_dual_paths_at_128x256_under_every_tolerance_set(paths, orc, dchain):
    case = tl.by_name("children-128x256")
    paths.set_dual_chain(dchain)
    for name in case.sets:
        with round_stats(paths) as since:
            rf, kf, g, kg = children_side_by_side(paths, orc, case, name)
            d = since()
        print("128x256 dual chain %d under %s: root %s children %s, round histogram moved by %s" % (dchain, name, rf, kf, d.tolist()))
        assert (rf, kf) == case.figures[name]
        if dchain == 8:
            assert dsel_chains(d)[0] > 0, ("k_dsel took no chain", d.tolist())
        certify_children(case, name, g, kg)


def test_fused_dual_pair_at_1000x2001_under_every_tolerance_set(gpu, orc):
    """2.0 M entries: k_dboot / k_da by the size rule.  One root (DEFAULT's), three near and three down children under each
    set; the fused pair's pivot counter must have moved."""
    case = tl.by_name("children-1000x2001")
    assert 2000000 <= (case.m + 1) * (case.n + 1) < 12000000
    boots0, fused0 = C.c_longlong(0), C.c_longlong(0)
    gpu.dual_fused_stats(C.byref(boots0), C.byref(fused0))
    A, b, c, U = case.data()
    g, o = synth.load_ilp(gpu, A, b, c, U), synth.load_ilp(orc, A, b, c, U)
    for P in (g, o):
        assert P.simplex(tol=tl.DEFAULT) == 0
    same(g, o, "1000x2001 root")
    M = cf.Model.ilp(A, b, c, U)
    for name in case.sets:
        tol = tl.SETS[name]
        ko, kg = tl.near_children(orc, o, tol, case.count), tl.near_children(gpu, g, tol, case.count)
        for a, r in zip(kg, ko):
            assert a[:3] == r[:3] and a[4] == r[4], (name, a[:3], a[4], r[4])
            same(a[3], r[3], "1000x2001 child %d/%s under %s" % (a[0], a[1], name))
        assert ((0, o.status, o.it_cnt), [(k[4], k[3].status, k[3].it_cnt) for k in ko]) == case.figures[name]
        for Mc, k in list(zip(tl.child_models(M, kg), kg))[2:4]:  # one near and one down child: the fp64 certificate costs a factor each
            tl.certify_end(Mc, k[3], tol, "1000x2001 child %d/%s under %s" % (k[0], k[1], name))
    boots, fused = C.c_longlong(0), C.c_longlong(0)
    gpu.dual_fused_stats(C.byref(boots), C.byref(fused))
    assert fused.value > fused0.value and boots.value > boots0.value, "k_da + k_fb<DUAL> took no pivot"


def test_batched_queue_with_a_non_null_parm(paths, orc):
    """Eight children in three slots through mvx_simplex_batch, the tolerances in the call's parm (the batch fills its own
    control blocks from it)."""
    case = tl.by_name("children-128x256")
    paths.set_batch_slots(3)
    try:
        for name in case.sets:
            rf, kf, g, kg = children_side_by_side(paths, orc, case, name, batch_slots=3)
            assert (rf, kf) == case.figures[name] and len(kg) == 8
            certify_children(case, name, g, kg)
    finally:
        paths.set_batch_slots(64)


# ------------------------------------------------------------------------------------------------ state of the handle
STATE_CASES = ["default-96x160", "persist-200x300"]


@pytest.mark.parametrize("name", STATE_CASES)
def test_a_tolerance_change_is_no_short_cut_for_the_handle_or_its_clone(gpu, orc, name):
    """(a) OPT under DJ, cloned, then both solved under DEFAULT: both pivot on to the default optimum -- the oracle's bits,
    the vertex and (to the certificate's own bound) the objective of a fresh default solve.  (b) The other way round costs no
    pivot, but is a solve.  (c) The same tolerances again: answered from the state at hand (last_solve_ms == 0)."""
    case = tl.by_name(name)
    inst = case.instance()
    M = tl.model(inst)
    g, o = tl.load(gpu, inst), tl.load(orc, inst)
    for P in (g, o):
        assert P.simplex(tol=tl.DJ) == 0 and P.status == OPT
        P.clone = P.copy()
    same(g, o, "under DJ")
    at_dj = o.it_cnt
    assert g.simplex(tol=tl.DJ) == 0 and gpu.last_solve_ms(g.h) == 0.0 and g.it_cnt == at_dj  # (c)
    for P in (g, o):
        assert P.simplex(tol=tl.DEFAULT) == 0 and P.clone.simplex(tol=tl.DEFAULT) == 0
    assert o.it_cnt > at_dj and o.clone.it_cnt > at_dj  # what makes (a) a test: the default optimum lies further on
    same(g, o, "DJ then DEFAULT")
    same(g.clone, o.clone, "clone of a DJ optimum under DEFAULT")
    fresh = tl.load(gpu, inst)
    assert fresh.simplex(tol=tl.DEFAULT) == 0 and fresh.status == OPT
    for P in (g, g.clone):
        ref = tl.certify_end(M, P, tl.DEFAULT, "DJ then DEFAULT")
        assert sorted(P.basis()[0][1:].tolist()) == sorted(fresh.basis()[0][1:].tolist())
        assert abs(P.obj - fresh.obj) <= 2 * cf.RTOL * ref.growth * (1.0 + abs(float(ref.z)) + np.abs(M.c) @ np.abs(P.col_prim()))
    # (b) DEFAULT then DJ: zero pivots, through a real solve; (c) again
    o2 = tl.load(orc, inst)
    for P in (fresh, o2):
        if P is o2:
            assert P.simplex(tol=tl.DEFAULT) == 0
        before = P.it_cnt
        assert P.simplex(tol=tl.DJ) == 0 and P.status == OPT and P.it_cnt == before
    assert gpu.last_solve_ms(fresh.h) > 0.0
    same(fresh, o2, "DEFAULT then DJ")
    assert fresh.simplex(tol=tl.DJ) == 0 and gpu.last_solve_ms(fresh.h) == 0.0
    same(fresh, o2, "DJ again")


def test_default_tolerances_behind_a_null_parm_equal_an_explicit_parm(paths, orc):
    """(d) set_default_tolerances(GLPK) and parm == NULL on the k_chain and k_dsel shapes: the bits of an explicit parm with
    the same values, which are the oracle's."""
    paths.set_persist(0)
    paths.set_cluster(1)
    paths.set_chain(5)
    paths.set_dual_chain(8)
    lp = tl.by_name("chain-300x700").instance()
    kids = tl.by_name("children-128x256")
    A, b, c, U = kids.data()

    def run(api, tol):
        """tol None: NULL parm everywhere"""
        P = tl.load(api, lp)
        P.rc = P.simplex(tol=tol)
        root = synth.load_ilp(api, A, b, c, U)
        root.rc = root.simplex(tol=tol)
        x = root.col_prim()
        out = [P, root]
        for j in tl.fractional_columns(x)[:2]:
            k = root.copy()
            api.set_col_bnds(k.h, j, tl.DB, 0.0, float(np.floor(x[j - 1])))
            k.rc = k.simplex(tol=tol)
            out.append(k)
        return out

    explicit, ref = run(paths, tl.GLPK), run(orc, tl.GLPK)
    before = cluster_counts(paths)
    with round_stats(paths) as since:
        try:
            paths.set_default_tolerances(*tl.GLPK)
            null = run(paths, None)
        finally:
            paths.set_default_tolerances(*tl.DEFAULT)
        d = since()
    after = cluster_counts(paths)
    assert after[0] > before[0] and after[1] == before[1] and dsel_chains(d)[0] > 0, (before, after, d.tolist())
    for k, (a, e, r) in enumerate(zip(null, explicit, ref)):
        assert a.rc == e.rc == r.rc == 0
        same(a, e, "NULL parm against explicit, handle %d" % k)
        same(a, r, "NULL parm against the oracle, handle %d" % k)
    parm = tl.smcp(paths, tl.DEFAULT)
    paths.init_smcp(C.byref(parm))
    assert (parm.tol_bnd, parm.tol_dj, parm.tol_piv) == tl.DEFAULT


@pytest.mark.parametrize("window", [1, 64])
def test_branch_and_bound_prefix_under_coarse_defaults(gpu, orc, window):
    """200 nodes of the 128x256 ILP with (2^-10, 2^-5, 2^-6) behind every NULL-parameter node solve, node at a time and in
    windows of 64: the oracle's record."""
    from oracle import oracle

    A, b, c, U = synth.dense_ilp(*tl.BNB_CASE)
    with tl.default_tolerances([gpu, orc], tl.ALL):
        for quirks in (0, 1):
            ref = oracle.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), quirks=quirks, max_nodes=tl.BNB_NODES)
            got = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), quirks=quirks, max_nodes=tl.BNB_NODES, window=window)
            for k in ("events", "prune", "parent", "node_bound", "total_pivots", "x"):
                assert got[k] == ref[k], (quirks, window, k)
