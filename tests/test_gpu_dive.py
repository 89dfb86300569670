"""GPU: the LP diving heuristic on the device (k_divepick through mvx_dive_pick_many) against the host twin (mvx_bnb_dive_pick
through the engine's own table), whole dives and dive trees on the HIP engine against the same calls over the oracle's table."""
import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import CV, IV, OPT, UP

from . import lpgen
from .test_bnb_dive import COUNTERS, RULES, tie_model
from .test_bnb_general import INSTANCES, failures, instance
from .test_bnb_host import same_result

pytestmark = pytest.mark.gpu


def tree_nodes(gpu, case, count):
    A, b, c, U = synth.dense_ilp(*case)
    root = lpgen.load_ilp(gpu, A, b, c, U)
    return root, bnb.node_sample(root, count)


def device_vs_host(root, nodes):
    """Every (node, rule) pair in one launch against the twin per pair; returns the number of pairs with a candidate."""
    hs = [P for P in nodes for _ in RULES]
    rules = [r for _ in nodes for r in RULES]
    rc, got = bnb.dive_pick_many(root, hs, rules)
    assert rc == 0
    for k, (P, r) in enumerate(zip(hs, rules)):
        hrc, want = bnb.dive_pick_node(P, root, r)
        assert hrc == 0 and got[k] == want, (k, r, got[k], want)
    return sum(1 for g in got if g[0] > 0)


@pytest.fixture(scope="module")
def sample64(gpu):
    root, nodes = tree_nodes(gpu, (128, 256, 7, 1, 0.01), 64)
    assert len(nodes) == 64
    return root, nodes


@pytest.mark.parametrize("k", [1, 7, 64])
def test_batches_match_host_twin(sample64, k):
    root, nodes = sample64
    assert device_vs_host(root, nodes[:k]) > 0


@pytest.mark.parametrize("case", [(12, 255, 3, 2), (12, 256, 3, 2), (12, 257, 3, 2), (12, 1030, 3, 2), (1200, 300, 3, 2)], ids=str)
def test_column_counts_and_a_tall_model(gpu, case):
    """One column fewer than a workgroup's lanes, as many, one more, four strides and a bit; more rows than columns."""
    root, nodes = tree_nodes(gpu, case, 6)
    assert len(nodes) >= 3
    assert device_vs_host(root, nodes) > 0
    assert device_vs_host(root, nodes[:2]) > 0  # the model stays with the root: the same bits again


def test_ties_go_to_the_lowest_column(gpu):
    for last in (2.0, 4.0):
        _M, root, node = tie_model(gpu, last)
        assert device_vs_host(root, [node]) == 3
        rc, got = bnb.dive_pick_many(root, [node] * 3, RULES)
        assert rc == 0 and [g[1] for g in got] == ([1, 1, 1] if last == 2.0 else [300, 300, 300])
        assert all(g[0] == 300 and g[2] == 0 for g in got)


def test_mixed_rows_lp(gpu):
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
        fractional += device_vs_host(root, [node]) > 0
        checked += 1
    assert checked > 30 and fractional > 10


def test_cut_rows_are_ignored_and_return_codes(gpu):
    root, nodes = tree_nodes(gpu, (40, 80, 3, 3), 6)
    cut = []
    for P in nodes[:4]:
        Q = P.copy()
        assert bnb.node_cuts(Q, dict(cut_strat=1, quirks=0)) >= 1
        Q.simplex()
        if Q.status == OPT:
            assert Q.m > root.m
            cut.append(Q)
    assert cut
    assert device_vs_host(root, cut + nodes) > 0
    E = nodes[0].copy()
    gpu.set_col_bnds(E.h, 1, UP, 0.0, 0.0)  # an edit: not solved
    assert bnb.dive_pick_many(root, [nodes[0], E], [1, 1])[0] == -3
    for rule in (0, 3, 7, 8):
        assert bnb.dive_pick_many(root, nodes[:2], [1, rule])[0] == -1
    other, _ = tree_nodes(gpu, (40, 81, 3, 3), 1)
    assert bnb.dive_pick_many(other, nodes[:1], [1])[0] == -1  # another column count


def test_as_many_columns_as_the_kernel_holds_and_more(gpu, orc):
    """n = 4 096 is accepted; n = 4 200: mvx_dive_pick_many refuses with -5 and the driver runs the twin -- the oracle's tree."""
    root, nodes = tree_nodes(gpu, (12, 4096, 3, 2), 2)
    assert device_vs_host(root, nodes) > 0
    A, b, c, U = synth.dense_ilp(12, 4200, 3, 2)
    root = lpgen.load_ilp(gpu, A, b, c, U)
    nodes = bnb.node_sample(root, 2)
    assert bnb.dive_pick_many(root, nodes, [1, 2])[0] == -5
    kw = dict(quirks=0, dive=7, dive_freq=4, dive_depth=6, max_nodes=24)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bnb.table_from(orc), **kw)
    got = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), **kw)
    assert got["rc"] == ref["rc"] == 0 and got["dive_calls"] > 1 and got["dive_lps"] > 0
    same_result(got, ref)
    for k in COUNTERS:
        assert got[k] == ref[k], k


def same_dive(a, b):
    assert a[0] == b[0] == 0 and a[1:3] == b[1:3] and a[4:] == b[4:], (a[:3] + a[4:], b[:3] + b[4:])
    if a[2]:
        assert np.array_equal(a[3][1:], b[3][1:])


def test_whole_dives_match_the_oracle_table(gpu, orc):
    tab = bnb.table_from(orc)
    A, b, c, U = synth.dense_ilp(40, 80, 3, 3)
    groot, oroot = lpgen.load_ilp(gpu, A, b, c, U), lpgen.load_ilp(orc, A, b, c, U)
    gnodes = bnb.node_sample(groot, 8)
    onodes = bnb.node_sample(oroot, 8, table=tab)
    assert len(gnodes) == len(onodes) == 8
    found = 0
    for G, O in zip(gnodes, onodes):
        g = bnb.dive_node(G, groot, 7)
        same_dive(g, bnb.dive_node(O, oroot, 7, table=tab))
        found += g[2]
    assert found > 0

    def one(rec):
        inst = instance(rec)
        pair = []
        for api, t in ((gpu, None), (orc, tab)):
            root = lpgen.load_milp(api, inst)
            if bnb.integral_bounds(root, table=t) == 2:
                return
            node = root.copy()
            node.simplex()
            if node.status != OPT:
                return
            pair.append(bnb.dive_node(node, root, 7, table=t))
        same_dive(*pair)

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kw", [dict(window=1), dict(window=64), dict(window=64, cut_strat=1), dict(window=64, heur=2, rc_fix=1, prop=8)],
                         ids=str)
def test_tree_matches_oracle_table(gpu, orc, kw):
    from .test_gpu_chain import cluster_counts

    aborts0 = cluster_counts(gpu)[1]
    A, b, c, U = synth.dense_ilp(40, 80, 3, 3)
    opts = dict(quirks=0, dive=7, dive_freq=8, max_nodes=400, **kw)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bnb.table_from(orc), **opts)
    got = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), **opts)
    assert got["rc"] == ref["rc"] == 0
    same_result(got, ref)
    for k in COUNTERS:
        assert got[k] == ref[k], k
    assert got["dive_calls"] > 10 and got["dive_found"] > 0 and got["dive_lps"] > got["dive_calls"]
    assert cluster_counts(gpu)[1] == aborts0


# The root dives of the two 512 x 1024 instances, dive = 7, max_nodes = 1, window 64, as the same call over the oracle's table
# gives them on the CPU (about 20 s each there): best_lower, dive_lps, dive_pivots.
SIZED = {
    (512, 1024, 12345, 3, 0.4): (7344.0, 2940, 9008),
    (512, 1024, 12345, 1, 0.002): (20.0, 2390, 12267),
}


@pytest.mark.parametrize("case", list(SIZED), ids=str)
def test_root_dives_at_size(gpu, case):
    A, b, c, U = synth.dense_ilp(*case)
    r = bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), quirks=0, dive=7, window=64, max_nodes=1)
    print(case, r["best_lower"], r["dive_lps"], r["dive_pivots"], r["incumbent_heur"])
    assert r["rc"] == 0 and r["has_incumbent"] == 1 and r["count"] == 1
    assert (r["best_lower"], r["dive_lps"], r["dive_pivots"], r["incumbent_heur"]) == SIZED[case] + (2,)
    assert (r["dive_calls"], r["dive_found"], r["dive_improved"]) == (1, 1, 1)
    x = np.array(r["x"])
    assert np.array_equal(x, np.round(x))
    assert (x >= 0).all() and (x <= U).all()
    assert (A @ x <= b + 1e-9 * np.maximum(1.0, np.abs(b))).all()
    assert abs(float(c @ x) - r["best_lower"]) <= 1e-9 * (1 + abs(r["best_lower"]))
