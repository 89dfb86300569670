"""GPU: the speculative best-bound window (mvx_bnb_params.best_window) over the gfx950 engine against the oracle's
node-at-a-time restatement of bs.cpp in best-bound order, and the device classification it uses
(mvx_classify_many / k_classify) against the host printInfo, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from mvolps_amd import bnb, capi, synth

from . import lpgen
from .test_gpu_bnb import same_result

pytestmark = pytest.mark.gpu


def hip_table():
    return bnb.LpApiTable.from_address(bnb.lib().mvx_hip_lp_api())


def test_engine_table_has_the_classification_entry(gpu):
    assert hip_table().classify_many  # the driver's rounds go through k_classify


@pytest.mark.parametrize("W", [8, 64])
@pytest.mark.parametrize("quirks", [0, 1])
@pytest.mark.parametrize("case", [(16, 32, 5, 2), (40, 80, 7, 2)], ids=lambda c: "%dx%d" % (c[0], c[1]))
def test_best_window_bit_exact_vs_oracle(gpu, orc, case, quirks, W):
    from oracle import oracle

    A, b, c, U = synth.dense_ilp(*case)
    ref = oracle.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), node_strat=1, quirks=quirks, max_nodes=1500)
    got = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), node_strat=1, quirks=quirks, max_nodes=1500, best_window=W)
    same_result(got, ref)
    assert 0 < got["rounds"] < got["count"]


@pytest.mark.parametrize("kw", [dict(quirks=1, cut_strat=1), dict(quirks=0, cut_strat=1), dict(quirks=0, cut_strat=1, cut_select=1, cut_chance=0.5),
                                dict(quirks=0, var_strat=1), dict(quirks=1, var_strat=2)],
                         ids=["quirks-cuts", "repaired-cuts", "repaired-select", "vfp", "vgo"])
def test_best_window_modes_vs_oracle(gpu, orc, kw):
    from oracle import oracle

    A, b, c, U = synth.dense_ilp(16, 32, 5, 2)
    ref = oracle.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), node_strat=1, max_nodes=800, **kw)
    got = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), node_strat=1, max_nodes=800, best_window=32, **kw)
    same_result(got, ref)
    assert got["rounds"] > 0


def test_best_window_minimisation_vs_oracle(gpu, orc):
    from oracle import oracle

    A, c = lpgen.setcover_ilp(40, 60, 3)
    ref = oracle.branch_and_bound(lpgen.load_setcover(orc, A, c), node_strat=1, quirks=0, max_nodes=5000)
    got = bnb.branch_and_bound(lpgen.load_setcover(gpu, A, c), node_strat=1, quirks=0, max_nodes=5000, best_window=64)
    same_result(got, ref)


def test_best_window_deep_cut_dive_vs_oracle(gpu, orc):
    """test_gpu_bnb.test_deep_cut_rows_cross_the_spare_rows's setup (2500 best-bound nodes of a 128x256 ILP, bug-compatible
    cuts, depth > 40: slabs grow under the driver) through the window: the oracle's tree."""
    from oracle import oracle

    A, b, c, U = synth.dense_ilp(128, 256, 7, 3)
    kw = dict(quirks=1, cut_strat=1, node_strat=1, max_nodes=2500)
    ref = oracle.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), **kw)
    got = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), best_window=64, **kw)
    same_result(got, ref)
    assert got["rounds"] < got["count"]


# ---------------------------------------------------------------- mvx_classify_many against the host printInfo

def host_classify(P, quirks):
    st, viol = bnb.print_info(P, quirks=quirks)
    x = P.col_prim()
    return st, viol, [float(x[j - 1]) for j in viol]


def assert_same_bits(got, want):
    assert got[0] == want[0] and got[1] == want[1]
    assert np.array(got[2], dtype=np.float64).view(np.int64).tolist() == np.array(want[2], dtype=np.float64).view(np.int64).tolist()


def tree_nodes(api, A, b, c, U, quirks, want, cuts=False):
    """Handles of a small breadth-first tree grown with the driver's own helpers: solved nodes, infeasible children,
    integral leaves; with cuts=True every branched node gets its cut row(s) (mvx_bnb_node_cuts) before it is cloned."""
    root = lpgen.load_ilp(api, A, b, c, U)
    root.simplex()
    out, queue = [root], [root]
    params = dict(quirks=quirks, cut_strat=1)
    while queue and len(out) < want:
        a = queue.pop(0)
        if a.status != capi.OPT:
            continue
        st, viol = bnb.print_info(a, quirks=quirks)
        if st != 0:
            continue
        pick = viol[0]
        if cuts:
            a = a.copy()
            bnb.node_cuts(a, params)
            a.simplex()
            out.append(a)
        S2, S3 = bnb.make_children(a, pick, quirks=quirks)
        for ch in (S2, S3):
            ch.simplex()
            out.append(ch)
            queue.append(ch)
    return out


@pytest.mark.parametrize("quirks", [1, 0])
def test_classify_many_matches_host_print_info(gpu, quirks):
    A, b, c, U = synth.dense_ilp(16, 32, 5, 2)
    nodes = tree_nodes(gpu, A, b, c, U, quirks, 120)
    # an infeasible node for sure: x_1 >= 1e6 against A > 0, b finite
    bad = nodes[0].copy()
    bad.api.set_col_bnds(bad.h, 1, capi.LO, 1e6, 0.0)
    bad.simplex()
    assert bad.status == capi.NOFEAS
    nodes.append(bad)
    # an integral node for sure: every column fixed at the floor of the root's value (feasible: A > 0, b >= 0)
    whole = nodes[0].copy()
    for j, v in enumerate(nodes[0].col_prim(), start=1):
        whole.api.set_col_bnds(whole.h, j, capi.FX, float(np.floor(v)), float(np.floor(v)))
    whole.simplex()
    assert whole.status == capi.OPT
    nodes.append(whole)
    rc, got = bnb.classify_many(nodes, quirks=quirks)
    assert rc == 0
    seen = set()
    for P, g in zip(nodes, got):
        want = host_classify(P, quirks)
        assert_same_bits(g, want)
        seen.add(want[0])
    assert seen == {-1, 0, 1}  # infeasible, fractional and integral nodes were all in the batch


@pytest.mark.parametrize("quirks", [1, 0])
def test_classify_many_with_cut_rows(gpu, quirks):
    A, b, c, U = synth.dense_ilp(24, 48, 3, 2)
    nodes = tree_nodes(gpu, A, b, c, U, quirks, 60, cuts=True)
    assert max(P.m for P in nodes) > 24
    # a cut row appended and not yet solved: the values are the tableau's as it stands
    fresh = nodes[0].copy()
    bnb.node_cuts(fresh, dict(quirks=quirks, cut_strat=1))
    nodes.append(fresh)
    rc, got = bnb.classify_many(nodes, quirks=quirks)
    assert rc == 0
    for P, g in zip(nodes, got):
        assert_same_bits(g, host_classify(P, quirks))


def test_classify_many_unbounded(gpu):
    """UNBND maps to -1 (util.cpp:424); a bounded copy of the same model classifies by its values."""
    A = np.array([[1.0, -1.0, 0.0], [0.0, 0.0, 1.0]])
    rows = [(capi.UP, 0.0, 1.0), (capi.UP, 0.0, 2.5)]
    cols = [(capi.LO, 0.0, 0.0)] * 3
    P = gpu.create()
    P.load_general(A, rows, cols, np.array([1.0, 1.0, 1.0]), kinds=[capi.IV] * 3, direction=capi.MAX)
    P.simplex()
    assert P.status == capi.UNBND
    Q = P.copy()
    Q.api.set_col_bnds(Q.h, 2, capi.DB, 0.0, 2.5)
    Q.simplex()
    assert Q.status == capi.OPT
    for quirks in (1, 0):
        rc, got = bnb.classify_many([P, Q], quirks=quirks)
        assert rc == 0
        assert got[0] == (-1, [], [])
        assert_same_bits(got[1], host_classify(Q, quirks))
        assert got[1][0] == 0  # x_1 = 3.5


def test_classify_many_at_size_and_cap_overflow(gpu):
    """512x1024 nodes with over a hundred fractional columns each (U = 50); a `cap` below the largest count returns -3."""
    A, b, c, U = synth.dense_ilp(512, 1024, 12345, 50)
    nodes = tree_nodes(gpu, A, b, c, U, 0, 9)
    for quirks in (1, 0):
        rc, got = bnb.classify_many(nodes, quirks=quirks)
        assert rc == 0
        for P, g in zip(nodes, got):
            assert_same_bits(g, host_classify(P, quirks))
        most = max(len(g[1]) for g in got)
        assert most >= 100, most
        rc, _ = bnb.classify_many(nodes, quirks=quirks, cap=most - 1)
        assert rc == -3
        rc, again = bnb.classify_many(nodes, quirks=quirks, cap=most)
        assert rc == 0 and again == got


def test_classify_many_rejects_bad_arguments(gpu):
    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    P = lpgen.load_ilp(gpu, A, b, c, U)
    assert bnb.classify_many([P])[0] == -1  # never solved: no tableau
    P.simplex()
    A2, b2, c2, U2 = synth.dense_ilp(8, 20, 3, 2)
    Q = lpgen.load_ilp(gpu, A2, b2, c2, U2)
    Q.simplex()
    assert bnb.classify_many([P, Q])[0] == -1  # different columns
    assert bnb.lib().mvx_classify_many(None, 0, 1, None, None, None, None, 1) == -1
