"""GPU: the kernels at their built-in size limits and dispatch thresholds, bitwise against the oracle -- k_gmi_work past
one pass of 1024 positions and k_gmi_backsub at its group / lane / block tails, k_dsel at 1024 rows and across that
limit, k_persist at three and four columns per workgroup, at its LDS ceiling and on both sides of its area thresholds,
clones in every copy regime of engine_copy, k_rowcomb at its 64-row chunk edges.  test_thresholds_inputs.py proves on
the oracle alone that each instance has the property relied on here; every test about a path reads the engine's own
counter to prove the path ran (or did not)."""
import ctypes as C

import numpy as np
import pytest

from mvolps_amd import capi, synth

from . import certify as cf
from . import lpgen
from . import thresholds as th
from .test_gpu_certify import paths  # noqa: F401  (fixture)
from .test_gpu_chain import dual_chained  # noqa: F401  (fixture)
from .test_gpu_gmi import device_cuts
from .test_gpu_parity import assert_same_state
from .thresholds import same_bits

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ counters
def persist_counts(api):
    a, b = C.c_longlong(0), C.c_longlong(0)
    api.persist_stats(C.byref(a), C.byref(b))
    return a.value, b.value


def round_hist(api):
    """g_round_hist: [0] k_dsel not applicable, [1..DCH_MAX] k_dsel chains of that length, [DCH_MAX + 1] applicable but
    no plain dual pivot, [DCH_MAX + 2] k_select passing a step k_dsel prepared through, then k_select's own"""
    out = (C.c_ulonglong * (th.DCH_MAX + 10))()
    api.lib.mvx_debug_round_hist(out, 0)
    return np.array(list(out), dtype=np.int64)


class round_stats:
    """with round_stats(api) as since: ...; since() is what the counters moved by so far.  Off again on the way out."""

    def __init__(self, api):
        self.api = api

    def __enter__(self):
        self.api.lib.mvx_debug_stats(1)
        self.base = round_hist(self.api)
        return lambda: round_hist(self.api) - self.base

    def __exit__(self, *exc):
        self.api.lib.mvx_debug_stats(0)
        return False


def dsel_chains(d):
    """(chains k_dsel took, those of two pivots or more, steps k_select passed through)"""
    return int(d[1:th.DCH_MAX + 1].sum()), int(d[2:th.DCH_MAX + 1].sum()), int(d[th.DCH_MAX + 2])


# ------------------------------------------------------------------------------------------------ A: GMI cuts
@pytest.mark.parametrize("case", th.GMI_CASES, ids=th.gmi_id)
def test_gmi_cuts_past_one_pass_and_at_the_backsubstitution_edges(gpu, orc, case):
    """Three rounds, both modes, every basic column, against the oracle's one-column restatements; the last
    bug-compatible cut appended and re-solved between rounds."""
    P, Q = th.load_gmi_case(gpu, case), th.load_gmi_case(orc, case)
    for H in (P, Q):
        assert H.simplex() == 0
    assert_same_state(P, Q, "root")
    for rnd in range(th.GMI_ROUNDS):
        basic, cuts = th.oracle_round(orc, Q)
        for mode in (0, 1):
            vals, rhs, ok = device_cuts(gpu, P, basic, mode)
            done = 0
            for t, j in enumerate(basic):
                rc, rv, rl = cuts[mode][t]
                if mode and rc != 0:
                    continue  # declined for its fractional part or its norm on the host side of the driver
                assert rc == 0 and ok[t] == 1
                assert same_bits(rhs[t], rl) and same_bits(vals[t, 0], rl), (rnd, mode, j, rhs[t], rl)
                assert same_bits(vals[t, 1:], rv[1:]), (rnd, mode, j)
                done += 1
            assert 4 * done >= 3 * len(basic)
        for api, H in ((gpu, P), (orc, Q)):
            assert th.append_cut(api, H, cuts[0][-1][1], cuts[0][-1][2]) == 0
        assert_same_state(P, Q, "round %d" % rnd)


def test_gmi_cut_counts_at_the_lane_tails(gpu, orc):
    """1, 3, 4 and 5 columns (GMI_CT = 4 cuts per lane): each call equals the first rows of the full call."""
    P, Q = th.load_gmi_case(gpu, th.GMI_TAIL_CASE), th.load_gmi_case(orc, th.GMI_TAIL_CASE)
    for H in (P, Q):
        assert H.simplex() == 0
    basic = th.basic_columns(Q)
    for mode in (0, 1):
        full = device_cuts(gpu, P, basic, mode)
        for k in (1, 3, 4, 5):
            part = device_cuts(gpu, P, basic[:k], mode)
            assert same_bits(part[0], full[0][:k]) and same_bits(part[1], full[1][:k]) and np.array_equal(part[2], full[2][:k]), (mode, k)


def test_gmi_temp_is_carried_into_a_pass_that_opens_on_a_binary_position(gpu, orc):
    """Every third column boxed to [0, 1] (GLP_BV to generateCut3, which then re-uses `temp`), one of them at position
    1025: the first coefficient of the second pass is the `temp` the first pass ended on."""
    P, Q = th.load_mixed(gpu), th.load_mixed(orc)
    for H in (P, Q):
        assert H.simplex() == 0
    assert_same_state(P, Q, "mixed root")
    basic = [j for j in th.basic_columns(Q) if orc.get_col_kind(Q.h, j) == capi.IV]
    for mode in (0, 1):
        vals, rhs, ok = device_cuts(gpu, P, basic, mode)
        for t, j in enumerate(basic):
            rc, rv, rl = th.oracle_cut(orc, Q, j, mode)
            assert rc == 0 and ok[t] == 1
            assert same_bits(rhs[t], rl) and same_bits(vals[t, 1:], rv[1:]), (mode, j)


def test_gmi_free_nonbasic_flag_is_carried_across_passes(gpu, orc):
    """ok[t] = 0 exactly where a free non-basic position holds a non-zero: in the first pass (the flag has to survive
    the second), only after it, or nowhere -- computed here from the oracle's tableau rows and statuses."""
    P, Q = th.load_free(gpu), th.load_free(orc)
    for H in (P, Q):
        assert H.simplex(it_lim=th.FREE_LIMIT) == capi.EITLIM
    assert_same_state(P, Q, "free model at its pivot limit")
    kinds = th.free_model()[4]
    basic = [j for j in th.basic_columns(Q) if kinds[j - 1] == capi.IV]
    pos = th.free_positions(Q, basic)
    expect = np.array([0 if p else 1 for p in pos], dtype=np.int32)
    assert 0 < expect.sum() < len(expect)
    vals, rhs, ok = device_cuts(gpu, P, basic, 1)
    assert np.array_equal(ok, expect), (basic, pos, ok.tolist())
    same = 0
    for t, j in enumerate(basic):
        rc, rv, rl = th.oracle_cut(orc, Q, j, 1)
        if ok[t] == 1 and rc == 0:
            assert same_bits(rhs[t], rl) and same_bits(vals[t, 1:], rv[1:]), j
            same += 1
    assert same >= 1
    # each column on its own (its own launch, a grid of one) reports the same flag
    for t, j in enumerate(basic):
        assert device_cuts(gpu, P, [j], 1)[2][0] == expect[t], j


@pytest.mark.parametrize("case", th.GMI_CERT_CASES, ids=th.gmi_id)
def test_gmi_repaired_cuts_past_one_pass_are_certified(gpu, case):
    """The repaired root cuts of the two- and three-pass instances against the formula on the recomputed row."""
    A, b, c, U = synth.dense_ilp(*case)
    P, M = synth.load_ilp(gpu, A, b, c, U), cf.Model.ilp(A, b, c, U)
    assert P.simplex() == 0
    ref = cf.certify(M, P, what="gmi root %s" % th.gmi_id(case))
    cols = [int(k) - M.m for k in ref.head if k > M.m and cf.gmi_ref(ref, int(k) - M.m) is not None]
    assert len(cols) >= 20
    vals, rhs, ok = device_cuts(gpu, P, cols, 1)
    for t, j in enumerate(cols):
        assert ok[t] == 1
        cf.certify_gmi(ref, j, vals[t, 1:], rhs[t], (), what="root %s" % th.gmi_id(case))


# ------------------------------------------------------------------------------------------------ B: k_dsel
@pytest.mark.parametrize("case", th.DSEL_CASES, ids=th.dsel_id)
def test_dual_chains_at_the_row_limit_of_k_dsel(dual_chained, orc, case):
    """Root and both children of its first two fractional columns, each child solved twice (the second time on the
    slab the first gave back), dual chain forced to 8.  Up to 1024 rows k_dsel takes chains of two pivots and more;
    one row past it none of its counters moves (the launch is not even made)."""
    m, n, seed, U = case
    o, x, ref = th.dsel_children(orc, case)
    dual_chained.set_dual_chain(th.DSEL_CHAIN)
    A, b, c, U = synth.dense_ilp(*case)
    g = synth.load_ilp(dual_chained, A, b, c, U)
    assert g.simplex() == 0
    assert_same_state(g, o, "root")
    with round_stats(dual_chained) as since:
        for rep in range(2):
            for (j, up), k_ref in ref.items():
                k = g.copy()
                dual_chained.set_col_bnds(k.h, j, capi.DB, *th.child_bounds(x, j, up, U))
                assert k.simplex() == 0
                assert_same_state(k, k_ref, "child %d/%d rep %d" % (j, up, rep))
                del k
        d = since()
    chains, long_chains, passed = dsel_chains(d)
    print("k_dsel %s: round histogram moved by %s" % (th.dsel_id(case), d.tolist()))
    if m <= th.DSEL_MAX:
        assert long_chains > 0 and passed >= chains, d.tolist()
    else:
        assert not d[1:th.DCH_MAX + 3].any(), d.tolist()


def test_cut_rows_take_a_handle_across_the_row_limit_of_k_dsel(dual_chained, orc):
    """1020 rows, one bug-compatible cut row and one down branch per round for eight rounds: m = 1021 .. 1028.  State
    bitwise after every round; k_dsel's chains are counted while m <= 1024 and never after, where k_select and its
    dual_chain carry on alone."""
    dual_chained.set_dual_chain(th.DSEL_CHAIN)
    P, Q = th.load_gmi_case(dual_chained, th.DSEL_GROW), th.load_gmi_case(orc, th.DSEL_GROW)
    for H in (P, Q):
        assert H.simplex() == 0
    assert_same_state(P, Q, "root")
    moved = []
    with round_stats(dual_chained) as since:
        last = since()
        for rnd in range(th.DSEL_GROW_ROUNDS):
            plan = th.grow_plan(orc, Q)
            for api, H in ((dual_chained, P), (orc, Q)):
                assert th.grow_apply(api, H, plan) == 0
            assert_same_state(P, Q, "round %d, m = %d" % (rnd, Q.m))
            now = since()
            moved.append((Q.m, now - last))
            last = now
    for m, d in moved:
        print("k_dsel growth m = %d: round histogram moved by %s" % (m, d.tolist()))
        if m <= th.DSEL_MAX:
            assert dsel_chains(d)[0] > 0, (m, d.tolist())
        else:
            assert not d[1:th.DCH_MAX + 3].any(), (m, d.tolist())
    assert [m for m, _ in moved] == list(range(1021, 1029))


# ------------------------------------------------------------------------------------------------ C: k_persist
def compute_units():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


PERSIST_NAMES = list(th.persist_shapes(256))


@pytest.mark.parametrize("name", PERSIST_NAMES)
def test_resident_tableau_geometry_and_thresholds(paths, orc, name):
    """Degenerate boxed LPs with the cluster chain off: three and four columns per workgroup (a last strip of one
    column; just under the area cap), the tallest strip the LDS admits and one row more, both area thresholds from both
    sides, sixteen columns per workgroup and a shape that would need seventeen (those two stopped by a pivot limit).  The shapes follow from the device's compute-unit count; k_persist is launched exactly where its plan
    admits the shape, never gives up, and the bits are the oracle's either way."""
    cus = compute_units()
    m, n, seed, taken = th.persist_shapes(cus)[name]
    assert (th.persist_plan(m, n, cus) is not None) == taken
    A, b, c = lpgen.degenerate_lp(m, n, seed)
    paths.set_cluster(0)
    paths.set_persist(1)
    before = persist_counts(paths)
    g, o = lpgen.load_degenerate(paths, A, b, c), lpgen.load_degenerate(orc, A, b, c)
    for P in (g, o):
        P.rc = P.simplex(it_lim=th.PERSIST_LIMITS.get(name))
    after = persist_counts(paths)
    print("k_persist %s %dx%d (%d units, plan %s): launches +%d, aborts +%d, %d pivots"
          % (name, m, n, cus, th.persist_plan(m, n, cus), after[0] - before[0], after[1] - before[1], o.it_cnt))
    assert g.rc == o.rc and g.pert_cnt == o.pert_cnt and g.bland_cnt == o.bland_cnt
    assert_same_state(g, o, "%s %dx%d" % (name, m, n))
    assert after[1] == before[1], "a k_persist launch gave up"
    if taken:
        assert after[0] > before[0], "k_persist was not launched"
    else:
        assert after[0] == before[0], "k_persist was launched on a shape its plan declines"


# ------------------------------------------------------------------------------------------------ D: clones
def assert_same_copy(a, b, what):
    """Two handles of one engine: tableau, basis arrays, values, statuses and column bounds, bitwise"""
    assert a.status == b.status and a.it_cnt == b.it_cnt, what
    assert same_bits(a.tableau(), b.tableau()), what
    for u, v in zip(a.basis(), b.basis()):
        assert np.array_equal(u, v), what
    for u, v in zip(th.column_bounds(a), th.column_bounds(b)):
        assert same_bits(u, v), what


@pytest.mark.parametrize("case", th.CLONE_CASES, ids=th.clone_id)
def test_clones_in_every_copy_regime(gpu, orc, case):
    """A source stopped by a pivot limit, cloned twice in a row, then a clone of the first clone (a source that is itself
    a recorded destination): every copy reads like the source and like the oracle's; the source and the clone of a clone
    then carry on to a second limit -- a clone with a stale tail (bounds, statuses, basis arrays) goes another way."""
    m, n, seed, lim1, lim2, regime = case
    assert th.copy_regime(m, n) == regime
    g, o = th.load_clone_case(gpu, case), th.load_clone_case(orc, case)
    for P in (g, o):
        assert P.simplex(it_lim=lim1) == capi.EITLIM
    for P in (g, o):
        P.c1 = P.copy()
        P.c2 = P.copy()
        P.c3 = P.c1.copy()
    assert_same_state(g, o, "source")
    for name in ("c1", "c2", "c3"):
        assert_same_copy(getattr(g, name), g, "%s against its source" % name)
    assert_same_state(g.c3, o.c3, "clone of a clone")
    assert_same_state(g.c2, o.c2, "second clone")
    for P in (g, o):
        assert P.simplex(it_lim=lim2) == capi.EITLIM
        assert P.c3.simplex(it_lim=lim2) == capi.EITLIM
    assert_same_state(g, o, "source, carried on")
    assert_same_state(g.c3, o.c3, "clone of a clone, carried on")
    assert_same_state(g.c1, o.c1, "first clone, untouched by its own clone's solve")


# ------------------------------------------------------------------------------------------------ E: objective row
@pytest.mark.parametrize("m,n,seed", th.ROWCOMB_CASES)
def test_objective_change_at_the_chunk_edges(gpu, orc, m, n, seed):
    A, b, c = synth.dense_lp(m, n, seed)
    g, o = gpu.create(), orc.create()
    for P in (g, o):
        P.load_dense(A, b, c)
        assert P.simplex() == 0
        th.change_objective(P)
    assert same_bits(g.tableau(), o.tableau())
    for P in (g, o):
        assert P.simplex() == 0
    assert_same_state(g, o, "%dx%d after the objective change" % (m, n))
