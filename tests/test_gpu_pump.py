"""GPU: the feasibility pump's device entries.  mvx_set_obj_many (k_objrow) against n + 1 mvx_set_obj_coef calls on a clone and
against the oracle doing the same, tableaux bit for bit and the next solve too; mvx_pump_obj_many (k_pumpobj) against the host
twin (mvx_bnb_pump_obj through the engine's own table); whole pumps on the HIP engine against the same call over the oracle's
table."""
import ctypes as C

import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import CV, DB, IV, OPT, UNDEF, UP

from . import lpgen
from .test_bnb_dive import tie_model
from .test_bnb_host import same_result
from .test_bnb_pump import COUNTERS
from .test_bnb_general import INSTANCES, failures, instance
from .test_gpu_parity import assert_same_state

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ mvx_set_obj_many

def objectives(rng, k, n):
    """k objectives of n + 1 entries: small integers, a third of them zero, some negative; entry 0 a constant."""
    c = rng.integers(-9, 10, size=(k, n + 1)).astype(float)
    c[rng.random((k, n + 1)) < 0.33] = 0.0
    c[:, 0] = rng.integers(-3, 4, size=k)
    return c


def per_coefficient(api, P, c):
    Q = P.copy()
    for j in range(len(c)):
        api.set_obj_coef(Q.h, j, float(c[j]))
    return Q


def check_set_obj(gpu, orc, gs, os_, c, solve=True):
    """gs[t] / os_[t]: the same handle on the engine and on the oracle (os_ may be None).  One call for all of gs against the
    per-coefficient path on clones and on the oracle; then one more solve of each."""
    refs = [per_coefficient(gpu, G, c[t]) for t, G in enumerate(gs)]
    orefs = [per_coefficient(orc, O, c[t]) for t, O in enumerate(os_)] if os_ is not None else None
    assert bnb.set_obj_many(gs, c) == 0
    for t, (G, R) in enumerate(zip(gs, refs)):
        assert G.status == R.status == UNDEF
        assert [gpu.get_obj_coef(G.h, j) for j in range(G.n + 1)] == list(c[t])
        assert np.array_equal(G.tableau(), R.tableau()), t
        if orefs is not None:
            assert np.array_equal(G.tableau(), orefs[t].tableau()), t
            assert all(np.array_equal(x, y) for x, y in zip(G.basis(), orefs[t].basis()))
    if not solve:
        return
    for t, (G, R) in enumerate(zip(gs, refs)):
        G.simplex()
        R.simplex()
        assert_same_state(G, R, t)
        if orefs is not None:
            orefs[t].simplex()
            assert_same_state(G, orefs[t], t)


def solved_pair(gpu, orc, m, n, seed):
    A, b, c = synth.dense_lp(m, n, seed)
    g, o = gpu.create(), orc.create()
    for P in (g, o):
        P.load_dense(A, b, c)
        assert P.simplex() == 0 and P.status == OPT
    return g, o


@pytest.mark.parametrize("n1", [255, 256, 257, 1030])
@pytest.mark.parametrize("m", [63, 64, 65, 129])
def test_set_obj_many_at_the_chunk_and_tile_edges(gpu, orc, m, n1):
    """Rows: one fewer than a 64-row chunk, one chunk, one more, two chunks and a row.  Entries of row 0: one fewer than four
    64-column workgroups, as many, one more, sixteen and a bit."""
    g, o = solved_pair(gpu, orc, m, n1 - 1, 7)
    c = objectives(np.random.default_rng(m * 10000 + n1), 2, n1 - 1)
    check_set_obj(gpu, orc, [g.copy(), g.copy()], [o.copy(), o.copy()], c)


def test_set_obj_many_tall(gpu, orc):
    g, o = solved_pair(gpu, orc, 1200, 300, 9)
    check_set_obj(gpu, orc, [g.copy()], [o.copy()], objectives(np.random.default_rng(3), 1, 300))


@pytest.fixture(scope="module")
def base129(gpu, orc):
    return solved_pair(gpu, orc, 129, 256, 12345)


@pytest.mark.parametrize("k", [1, 7, 64])
def test_set_obj_many_batches(gpu, orc, base129, k):
    g, o = base129
    c = objectives(np.random.default_rng(k), k, 256)
    check_set_obj(gpu, orc, [g.copy() for _ in range(k)], [o.copy() for _ in range(k)], c, solve=k <= 7)


def cut_nodes(api, table, count):
    """Solved nodes of one tree, every second one with a GMI cut row appended and solved again."""
    A, b, c, U = synth.dense_ilp(40, 80, 3, 3)
    root = lpgen.load_ilp(api, A, b, c, U)
    out = []
    for k, P in enumerate(bnb.node_sample(root, count, table=table)):
        if k % 2:
            assert bnb.node_cuts(P, dict(cut_strat=1, quirks=0), table=table) >= 1
            P.simplex()
        out.append(P)
    return root, out


def test_set_obj_many_mixes_row_counts_an_unsolved_handle_and_a_pending_edit(gpu, orc):
    groot, gs = cut_nodes(gpu, None, 6)
    oroot, os_ = cut_nodes(orc, bnb.table_from(orc), 6)
    assert [P.m for P in gs] == [P.m for P in os_] and len({P.m for P in gs}) > 1  # different m in one launch
    # a handle that was never solved: it only takes its objective
    gs.append(groot.copy())
    os_.append(oroot.copy())
    # a pending bound edit: the bound of a basic column waits for the next solve
    for api, nodes in ((gpu, gs), (orc, os_)):
        P = nodes[0].copy()
        x = P.col_prim()
        j = int(np.argmax(np.abs(x - np.round(x)))) + 1
        assert abs(x[j - 1] - round(x[j - 1])) > 1e-6  # fractional, hence basic
        api.set_col_bnds(P.h, j, DB, 0.0, float(np.floor(x[j - 1])))
        nodes.append(P)
    c = objectives(np.random.default_rng(17), len(gs), 80)
    refs = [per_coefficient(gpu, G, c[t]) for t, G in enumerate(gs)]
    orefs = [per_coefficient(orc, O, c[t]) for t, O in enumerate(os_)]
    assert bnb.set_obj_many(gs, c) == 0
    for t, (G, R, O) in enumerate(zip(gs, refs, orefs)):
        assert [gpu.get_obj_coef(G.h, j) for j in range(81)] == list(c[t]) and G.status == UNDEF
        if t != 6:
            assert np.array_equal(G.tableau(), R.tableau()) and np.array_equal(G.tableau(), O.tableau()), t
        for P in (G, R, O):
            P.simplex()
        assert_same_state(G, R, t)
        assert_same_state(G, O, t)


def test_set_obj_many_return_codes(gpu):
    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    P = lpgen.load_ilp(gpu, A, b, c, U)
    P.simplex()
    Q = P.copy()
    before = P.tableau()
    other = lpgen.load_ilp(gpu, *synth.dense_ilp(8, 15, 3, 2))
    L = bnb.lib()
    cc = np.zeros(2 * 17)
    hs = (C.c_void_p * 2)(P.h, Q.h)
    DP = C.POINTER(C.c_double)
    assert L.mvx_set_obj_many(hs, 0, cc.ctypes.data_as(DP)) == 0  # nothing to do
    assert L.mvx_set_obj_many(hs, -1, cc.ctypes.data_as(DP)) == -1
    assert L.mvx_set_obj_many(None, 2, cc.ctypes.data_as(DP)) == -1
    assert L.mvx_set_obj_many(hs, 2, None) == -1
    assert L.mvx_set_obj_many((C.c_void_p * 2)(P.h, None), 2, cc.ctypes.data_as(DP)) == -1
    assert bnb.set_obj_many([P, other], np.zeros((2, 17))) == -1  # another column count
    assert bnb.set_obj_many([P, P], np.zeros((2, 17))) == -1  # one handle twice
    assert P.status == OPT and np.array_equal(P.tableau(), before)  # a refused call changes nothing


# ------------------------------------------------------------------------------------------------ mvx_pump_obj_many

WEIGHTS = ((1.0, 0.0), (1.0 - 0.9, 0.9 / 37.5))


def tree_nodes(gpu, case, count):
    A, b, c, U = synth.dense_ilp(*case)
    root = lpgen.load_ilp(gpu, A, b, c, U)
    return root, bnb.node_sample(root, count)


def device_vs_host(root, nodes):
    """All nodes in one launch against the twin per node, under both weightings, then again against each node's own rounding
    (the stall move).  Returns (handles with fractional columns, columns moved)."""
    frac = moved = 0
    for ab in WEIGHTS:
        prev = None
        for _again in range(2):
            rc, info, xt, c = bnb.pump_obj_many(root, nodes, prev, [ab] * len(nodes))
            assert rc == 0
            for t, P in enumerate(nodes):
                hrc, hinfo, hxt, hc = bnb.pump_obj_node(P, root, None if prev is None else prev[t], ab)
                assert hrc == 0 and np.array_equal(info[t], hinfo), (t, info[t], hinfo)
                assert np.array_equal(xt[t], hxt) and np.array_equal(c[t], hc), t
            frac += int((info[:, 0] > 0).sum())
            moved += int(info[:, 1].sum())
            prev = [x.copy() for x in xt]
    return frac, moved


@pytest.fixture(scope="module")
def sample64(gpu):
    root, nodes = tree_nodes(gpu, (128, 256, 7, 1, 0.01), 64)
    assert len(nodes) == 64
    return root, nodes


@pytest.mark.parametrize("k", [1, 7, 64])
def test_pump_obj_batches_match_host_twin(sample64, k):
    root, nodes = sample64
    frac, moved = device_vs_host(root, nodes[:k])
    assert frac > 0 and moved > 0


def test_pump_obj_mixes_first_steps_and_repeats(sample64):
    """has_prev differs within one launch, and so do the weights."""
    root, nodes = sample64
    nodes = nodes[:8]
    first = bnb.pump_obj_many(root, nodes)
    prev = [first[2][t] if t % 2 else None for t in range(8)]
    ab = [WEIGHTS[t % 2] for t in range(8)]
    rc, info, xt, c = bnb.pump_obj_many(root, nodes, prev, ab)
    assert rc == 0
    for t, P in enumerate(nodes):
        hrc, hinfo, hxt, hc = bnb.pump_obj_node(P, root, prev[t], ab[t])
        assert hrc == 0 and np.array_equal(info[t], hinfo) and np.array_equal(xt[t], hxt) and np.array_equal(c[t], hc), t
        assert (info[t][1] > 0 or info[t][2] == 1) == (t % 2 == 1)  # a repeated rounding moves columns or reports the stall


@pytest.mark.parametrize("case", [(12, 255, 3, 2), (12, 256, 3, 2), (12, 257, 3, 2), (12, 1030, 3, 2), (1200, 300, 3, 2)], ids=str)
def test_pump_obj_column_counts_and_a_tall_model(gpu, case):
    """One column fewer than a workgroup's lanes, as many, one more, four strides and a bit; more rows than columns."""
    root, nodes = tree_nodes(gpu, case, 6)
    assert len(nodes) >= 3
    frac, moved = device_vs_host(root, nodes)
    assert frac > 0 and moved > 0


def test_pump_obj_ties_go_to_the_lowest_columns(gpu):
    for last in (2.0, 4.0):
        _M, root, node = tie_model(gpu, last)
        device_vs_host(root, [node])
        rc, info, xt, _c = bnb.pump_obj_many(root, [node])
        assert rc == 0 and list(info[0]) == [300, 0, 0, 300]
        rc, info, xt2, _c = bnb.pump_obj_many(root, [node], [xt[0]])
        assert rc == 0 and list(info[0][:3]) == [300, 10, 0]
        assert np.array_equal(xt2[0][1:11], np.zeros(10)) and np.array_equal(xt2[0][11:], xt[0][11:])


def test_pump_obj_mixed_rows_lp(gpu):
    rng = np.random.default_rng(5)
    checked = fractional = 0
    for _ in range(80):
        A, row_b, col_b, c, d = lpgen.random_general_lp(rng, 10, 12)
        root = gpu.create()
        root.load_general(A, row_b, col_b, c, c0=1.5, kinds=[IV if rng.random() < 0.7 else CV for _ in c], direction=d)
        node = root.copy()
        node.simplex()
        if node.status != OPT:
            continue
        fractional += device_vs_host(root, [node])[0] > 0
        checked += 1
    assert checked > 30 and fractional > 10


def test_pump_obj_cut_rows_are_ignored_and_return_codes(gpu):
    root, nodes = cut_nodes(gpu, None, 8)
    ok = [P for P in nodes if P.status == OPT]
    assert any(P.m > root.m for P in ok) and any(P.m == root.m for P in ok)
    assert device_vs_host(root, ok)[0] > 0
    E = ok[0].copy()
    gpu.set_col_bnds(E.h, 1, UP, 0.0, 0.0)  # an edit: not solved
    assert bnb.pump_obj_many(root, [ok[0], E])[0] == -3
    other, _ = tree_nodes(gpu, (40, 81, 3, 3), 1)
    assert bnb.pump_obj_many(other, ok[:1])[0] == -1  # another column count
    L, DP, IP = bnb.lib(), C.POINTER(C.c_double), C.POINTER(C.c_int)
    hs = (C.c_void_p * 1)(ok[0].h)
    hp, info, ab, xt, c = np.ones(1, dtype=np.int32), np.zeros(4, dtype=np.int32), np.array([1.0, 0.0]), np.zeros(81), np.zeros(81)
    args = (ab.ctypes.data_as(DP), info.ctypes.data_as(IP), xt.ctypes.data_as(DP), c.ctypes.data_as(DP))
    assert L.mvx_pump_obj_many(root.h, hs, 1, None, hp.ctypes.data_as(IP), *args) == -1  # has_prev without xprev
    assert L.mvx_pump_obj_many(root.h, hs, 0, None, hp.ctypes.data_as(IP), *args) == -1
    assert L.mvx_pump_obj_many(None, hs, 1, None, hp.ctypes.data_as(IP), *args) == -1


def same_pump(a, b):
    assert a[0] == b[0] == 0 and a[1:3] == b[1:3] and a[4:] == b[4:], (a[:3] + a[4:], b[:3] + b[4:])
    if a[2]:
        assert np.array_equal(a[3][1:], b[3][1:])


def test_as_many_columns_as_the_kernel_holds_and_more(gpu, orc):
    """n = 4 096 is accepted; n = 4 200: mvx_pump_obj_many refuses with -5 and the pump runs the twin -- the oracle's pump."""
    root, nodes = tree_nodes(gpu, (12, 4096, 3, 2), 2)
    assert device_vs_host(root, nodes)[0] > 0
    A, b, c, U = synth.dense_ilp(12, 4200, 3, 2)
    root = lpgen.load_ilp(gpu, A, b, c, U)
    nodes = bnb.node_sample(root, 2)
    assert bnb.pump_obj_many(root, nodes)[0] == -5
    tab = bnb.table_from(orc)
    oroot = lpgen.load_ilp(orc, A, b, c, U)
    onodes = bnb.node_sample(oroot, 2, table=tab)
    for G, O in zip(nodes, onodes):
        g = bnb.pump_node(G, root, 6, 0.5)
        same_pump(g, bnb.pump_node(O, oroot, 6, 0.5, table=tab))
        assert g[4] > 0
    kw = dict(quirks=0, pump=6, pump_freq=4, pump_alpha=0.5, max_nodes=24)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, **kw)
    got = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), **kw)
    assert got["rc"] == ref["rc"] == 0 and got["pump_calls"] > 1 and got["pump_lps"] > 0
    same_result(got, ref)
    for k in COUNTERS:
        assert got[k] == ref[k], k


# ------------------------------------------------------------------------------------------------ whole pumps

def test_whole_pumps_match_the_oracle_table(gpu, orc):
    tab = bnb.table_from(orc)
    A, b, c, U = synth.dense_ilp(40, 80, 3, 3)
    groot, oroot = lpgen.load_ilp(gpu, A, b, c, U), lpgen.load_ilp(orc, A, b, c, U)
    gnodes = bnb.node_sample(groot, 8)
    onodes = bnb.node_sample(oroot, 8, table=tab)
    assert len(gnodes) == len(onodes) == 8
    found = lps = 0
    for G, O in zip(gnodes, onodes):
        for alpha in (0.0, 0.9):
            g = bnb.pump_node(G, groot, 30, alpha)
            same_pump(g, bnb.pump_node(O, oroot, 30, alpha, table=tab))
            found += g[2]
            lps += g[4]
    assert found > 0 and lps > 0

    def one(rec):
        inst = instance(rec)
        for alpha in (0.0, 0.9):
            pair = []
            for api, t in ((gpu, None), (orc, tab)):
                root = lpgen.load_milp(api, inst)
                if bnb.integral_bounds(root, table=t) == 2:
                    return
                node = root.copy()
                node.simplex()
                if node.status != OPT:
                    return
                pair.append(bnb.pump_node(node, root, 30, alpha, table=t))
            same_pump(*pair)

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kw", [dict(window=1), dict(window=64), dict(window=64, cut_strat=1),
                                dict(window=64, heur=2, dive=7, rc_fix=1, prop=8)], ids=str)
def test_tree_matches_oracle_table(gpu, orc, kw):
    from .test_gpu_chain import cluster_counts

    aborts0 = cluster_counts(gpu)[1]
    A, b, c, U = synth.dense_ilp(40, 80, 3, 3)
    opts = dict(quirks=0, pump=30, pump_freq=8, max_nodes=400, **kw)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bnb.table_from(orc), **opts)
    got = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), **opts)
    assert got["rc"] == ref["rc"] == 0
    same_result(got, ref)
    for k in COUNTERS:
        assert got[k] == ref[k], k
    assert got["pump_calls"] > 10 and got["pump_found"] > 0 and got["pump_lps"] > 0
    assert cluster_counts(gpu)[1] == aborts0


# The root pumps of the two 512 x 1024 instances, pump = 30, max_nodes = 1, window 64, as the same call over the oracle's table
# gives them on the CPU: (pump_alpha) -> best_lower, pump_lps, pump_pivots.
SIZED = {
    ((512, 1024, 12345, 3, 0.4), 0.0): (7149.0, 3, 942),
    ((512, 1024, 12345, 3, 0.4), 0.9): (7191.0, 11, 1283),
    ((512, 1024, 12345, 1, 0.002), 0.0): (0.0, 1, 1167),
}


@pytest.mark.parametrize("case,alpha", list(SIZED), ids=str)
def test_root_pumps_at_size(gpu, case, alpha):
    A, b, c, U = synth.dense_ilp(*case)
    r = bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), quirks=0, pump=30, pump_alpha=alpha, window=64, max_nodes=1)
    print(case, alpha, r["best_lower"], r["pump_lps"], r["pump_pivots"], r["incumbent_heur"])
    assert r["rc"] == 0 and r["has_incumbent"] == 1 and r["count"] == 1
    assert (r["best_lower"], r["pump_lps"], r["pump_pivots"], r["incumbent_heur"]) == SIZED[(case, alpha)] + (3,)
    assert (r["pump_calls"], r["pump_found"], r["pump_improved"]) == (1, 1, 1)
    x = np.array(r["x"])
    assert np.array_equal(x, np.round(x))
    assert (x >= 0).all() and (x <= U).all()
    assert (A @ x <= b + 1e-9 * np.maximum(1.0, np.abs(b))).all()
    assert abs(float(c @ x) - r["best_lower"]) <= 1e-9 * (1 + abs(r["best_lower"]))
