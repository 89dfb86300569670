"""GPU: the primal rounding heuristic on the device (k_round through mvx_round_many) against the host twin (mvx_bnb_round
through the engine's own table), and heur 1 / 2 trees on the HIP engine against the same driver over the oracle's table."""
import json
import os

import numpy as np
import pytest

from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import CV, IV, OPT, UP

from . import lpgen
from .test_bnb_host import same_result

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tree_nodes(gpu, case, count):
    """The root of an ILP and solved OPT node LPs below it, breadth first (bnb.node_sample)."""
    A, b, c, U = synth.dense_ilp(*case)
    root = lpgen.load_ilp(gpu, A, b, c, U)
    return root, bnb.node_sample(root, count)


def device_vs_host(root, nodes, expect_found=False):
    found = 0
    for mode in (1, 2):
        rc, obj, fnd, x = bnb.round_many(root, nodes, mode)
        assert rc == 0
        for t, P in enumerate(nodes):
            hrc, hobj, hf, hx = bnb.round_node(P, root, mode)
            assert hrc == 0
            assert obj[t] == hobj and fnd[t] == hf, (mode, t, obj[t], hobj, fnd[t], hf)
            assert np.array_equal(x[t, 1:], hx[1:]), (mode, t)
        found += int(fnd.sum())
    if expect_found:
        assert found > 0
    return found


@pytest.mark.parametrize("k", [1, 7, 64])
def test_batches_match_host_twin(gpu, k):
    root, nodes = tree_nodes(gpu, (128, 256, 7, 1, 0.01), 64)
    assert len(nodes) == 64
    device_vs_host(root, nodes[:k])


@pytest.mark.parametrize("case", [(128, 256, 9, 2, 0.01), (512, 1024, 12345, 3, 0.4), (512, 1024, 12345, 1, 0.002), (1024, 2048, 5, 2)],
                         ids=str)
def test_tree_nodes_match_host_twin(gpu, case):
    root, nodes = tree_nodes(gpu, case, 64 if case[0] < 1024 else 16)
    device_vs_host(root, nodes, expect_found=case[4:] == (0.4,))
    # the model stays with the root: a second call reuses it, the same bits again
    device_vs_host(root, nodes[:3])


@pytest.mark.parametrize("case", [(1200, 300, 3, 2), (4200, 64, 3, 2)], ids=str)
def test_tall_models(gpu, case):
    """More rows than the fill keeps in registers (1024): activities in LDS; more than RND_NMAX (4096): in global scratch."""
    root, nodes = tree_nodes(gpu, case, 8)
    assert len(nodes) >= 3
    device_vs_host(root, nodes)


def test_zero_cost_integer_columns(gpu):
    """Integer columns with c_j = 0 (every fifth, and a block of 200): the fill skips them, every wave alike, and the
    device still gives the host twin's bits on many-wave 512 x 1024 nodes."""
    A, b, c, U = synth.dense_ilp(512, 1024, 12345, 3, 0.4)
    c = c.copy()
    c[::5] = 0.0
    c[300:500] = 0.0
    root = lpgen.load_ilp(gpu, A, b, c, U)
    nodes = bnb.node_sample(root, 64)
    assert len(nodes) == 64
    assert device_vs_host(root, nodes) > 0


def test_more_columns_than_the_kernel_holds(gpu, orc):
    """n = 4 200 > 4 096: mvx_round_many refuses with -5 and the driver runs the host twin -- the tree of the oracle's."""
    A, b, c, U = synth.dense_ilp(12, 4200, 3, 2)
    root = lpgen.load_ilp(gpu, A, b, c, U)
    nodes = bnb.node_sample(root, 2)
    assert bnb.round_many(root, nodes, 2)[0] == -5
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bnb.table_from(orc), quirks=0, heur=2, max_nodes=40)
    got = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), quirks=0, heur=2, max_nodes=40)
    assert got["rc"] == ref["rc"] == 0 and got["heur_calls"] > 0
    same_result(got, ref)
    for k in ("heur_calls", "heur_found", "heur_improved", "incumbent_heur"):
        assert got[k] == ref[k], k


def test_mixed_rows_lp(gpu):
    """Every row and column bound type, continuous columns, both directions: lpgen's general LPs on the engine."""
    rng = np.random.default_rng(5)
    checked = 0
    for _ in range(80):
        A, row_b, col_b, c, d = lpgen.random_general_lp(rng, 10, 12)
        root = gpu.create()
        root.load_general(A, row_b, col_b, c, c0=1.5, kinds=[IV if rng.random() < 0.7 else CV for _ in c], direction=d)
        node = root.copy()
        node.simplex()
        if node.status != OPT:
            continue
        device_vs_host(root, [node])
        checked += 1
    assert checked > 30


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
    device_vs_host(root, cut + nodes)
    # a handle that is not OPT: -3; a mode outside 1..2: -1
    E = nodes[0].copy()
    gpu.set_col_bnds(E.h, 1, UP, 0.0, 0.0)  # an edit: not solved
    assert bnb.round_many(root, [nodes[0], E], 2)[0] == -3
    assert bnb.round_many(root, nodes[:1], 0)[0] == -1
    assert bnb.round_many(root, nodes[:1], 3)[0] == -1


@pytest.mark.parametrize("kw", [dict(window=1), dict(window=64), dict(window=64, cut_strat=1), dict(node_strat=1, best_window=8)], ids=str)
def test_tree_matches_oracle_table(gpu, orc, kw):
    A, b, c, U = synth.dense_ilp(40, 80, 3, 3)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bnb.table_from(orc), quirks=0, heur=2, max_nodes=400, **kw)
    got = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), quirks=0, heur=2, max_nodes=400, **kw)
    assert got["rc"] == ref["rc"] == 0
    same_result(got, ref)
    for k in ("heur_calls", "heur_found", "heur_improved", "incumbent_heur"):
        assert got[k] == ref[k], k
    assert got["heur_calls"] > 20


# recorded on one MI355X (scripts/heur_profile.py --part trees, profiles/heuristic_trees.jsonl): config 5 with heur 2, FIFO
# window 64.  The heuristic's points never beat the node LPs' incumbent here, so the tree is heur 0's.
CONFIG5_HEUR2 = {"count": 15697, "total_pivots": 704037}


def test_config5_closes_with_heur2(gpu):
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "config5.json")))
    A, b, c, U = synth.dense_ilp(fx["m"], fx["n"], fx["seed"], fx["U"], fx["cap"])
    r = bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), quirks=0, heur=2, window=64)
    assert r["rc"] == 0 and r["hit_limit"] == 0 and r["has_incumbent"]
    assert abs(r["best_lower"] - 20.0) <= 1e-6 * 21
    assert r["count"] <= 15697
    assert r["count"] == CONFIG5_HEUR2["count"] and r["total_pivots"] == CONFIG5_HEUR2["total_pivots"], (r["count"], r["total_pivots"])


def test_wide_instance_gets_an_incumbent(gpu):
    A, b, c, U = synth.dense_ilp(512, 1024, 12345, 3, 0.4)
    r = bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), quirks=0, heur=2, window=64, max_nodes=20000)
    assert r["rc"] == 0 and r["has_incumbent"] == 1
    x = np.array(r["x"])
    if r["incumbent_heur"]:
        assert np.array_equal(x, np.round(x))
    assert np.abs(x - np.round(x)).max() <= 1e-9
    assert (x >= -1e-9).all() and (x <= U + 1e-9).all()
    act = A @ x
    assert (act <= b + 1e-9 * np.maximum(1.0, np.abs(b))).all()
    assert abs(float(c @ x) - r["best_lower"]) <= 1e-9 * (1 + abs(r["best_lower"]))
