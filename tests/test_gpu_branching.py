"""GPU: the branching penalties on the device (k_penalty through mvx_branch_penalties_many) against the host twin
(mvx_bnb_penalties, which exports each tableau), and var_strat 3 / 4 trees on the HIP engine against the same driver over
the oracle's table."""
import json
import os

import numpy as np
import pytest

from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import OPT, UP

from . import lpgen
from .test_bnb_branching import basic_fractional, certify_node, np_penalties
from .test_bnb_host import same_result

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9


def node_set(gpu, case, count, quirks=0):
    """Breadth-first solved node LPs of an ILP (root, children, grandchildren ...) that still have candidates."""
    A, b, c, U = synth.dense_ilp(*case)
    root = lpgen.load_ilp(gpu, A, b, c, U)
    root.simplex()
    out, queue, keep = [], [root], []
    while queue and len(out) < count:
        P = queue.pop(0)
        cols = basic_fractional(P, None)
        if P.status != OPT or not cols:
            continue
        out.append((P, cols))
        S2, S3 = bnb.make_children(P, cols[len(out) % len(cols)], quirks=quirks)
        S2.simplex()
        S3.simplex()
        queue += [S2, S3]
        keep += [S2, S3]
    return out, keep


def same_bits(dev, host):
    for d, h in zip(dev, host):
        assert np.array_equal(d, h), (d, h)


def device_vs_host(nodes):
    rc, got = bnb.branch_penalties_many([P for P, _ in nodes], [c for _, c in nodes], TOL)
    assert rc == 0
    for (P, cols), dev in zip(nodes, got):
        hrc, host = bnb.penalties(P, cols, TOL)
        assert hrc == 0
        same_bits(dev, host)
    return got


@pytest.mark.parametrize("k", [1, 2, 7, 33, 64])
def test_batches_match_host_twin(gpu, k):
    nodes, _keep = node_set(gpu, (40, 80, 3, 3), 64)
    assert len(nodes) == 64
    got = device_vs_host(nodes[:k])
    # and the definition itself, on a few of them
    for (P, cols), dev in list(zip(nodes, got))[:3]:
        ref = np_penalties(P, cols)
        assert [tuple(r[:2]) for r in ref] == [(d, u) for d, u in zip(dev[0], dev[1])]


def test_wide_nodes_512x1024(gpu):
    nodes, _keep = node_set(gpu, (512, 1024, 12345, 3, 0.4), 6)
    assert len(nodes) == 6
    device_vs_host(nodes)


def test_lp_optimum_1024x2048_many_rows(gpu):
    A, b, c, U = synth.dense_ilp(1024, 2048, 7, 3, 0.4)
    P = lpgen.load_ilp(gpu, A, b, c, U)
    P.simplex()
    assert P.status == OPT
    cols = basic_fractional(P, None)
    assert len(cols) >= 100
    device_vs_host([(P, cols)])
    head = P.basis()[0]
    every = [int(k) - P.m for k in head[1:] if k > P.m]  # every basic column, integral ones too
    device_vs_host([(P, every), (P, cols[:5])])


def test_clones_pending_edits_and_cut_rows(gpu):
    nodes, _keep = node_set(gpu, (40, 80, 5, 3), 4)
    P, cols = nodes[1]
    Q = P.copy()  # a clone of a solved node: same tableau, recorded device-to-device copy
    got = device_vs_host([(Q, cols), (P, cols)])
    same_bits(got[0], got[1])
    # children whose bound edits are still pending are not solved LPs
    S2, S3 = bnb.make_children(P, cols[0], quirks=0)
    assert bnb.branch_penalties_many([S2], [basic_fractional(P, None)[:1]], TOL)[0] == -3
    assert bnb.branch_penalties_many([P, S3], [cols, cols[:1]], TOL)[0] == -3
    for S in (S2, S3):
        S.simplex()
    kids = [(S, basic_fractional(S, None)) for S in (S2, S3) if S.status == OPT]
    kids = [(S, c) for S, c in kids if c]
    assert kids
    device_vs_host(kids)
    # a node with an appended cut row, solved again
    R = P.copy()
    m0 = R.m
    assert bnb.node_cuts(R, dict(cut_strat=1, quirks=0)) >= 1
    R.simplex()
    assert R.m > m0 and R.status == OPT
    device_vs_host([(R, basic_fractional(R, None)), (P, cols)])


def test_return_codes(gpu):
    nodes, _keep = node_set(gpu, (40, 80, 3, 3), 2)
    P, cols = nodes[0]
    assert bnb.branch_penalties_many([P], [[0]], TOL)[0] == -1
    assert bnb.branch_penalties_many([P], [[P.n + 1]], TOL)[0] == -1
    nonbasic = [j for j in range(1, P.n + 1) if P.col_stat()[j - 1] != capi.BS]
    assert bnb.branch_penalties_many([P], [nonbasic[:1]], TOL)[0] == -4
    Q = P.copy()
    gpu.set_col_bnds(Q.h, cols[0], UP, 0.0, 0.0)
    assert bnb.branch_penalties_many([Q], [cols[:1]], TOL)[0] == -3
    assert bnb.branch_penalties_many([P], [[]], TOL)[0] == 0  # nothing asked, nothing launched


@pytest.mark.parametrize("kw", [dict(var_strat=3, quirks=0), dict(var_strat=4, quirks=0), dict(var_strat=4, quirks=1, cut_strat=1),
                                dict(var_strat=3, quirks=1, cut_strat=1)], ids=str)
@pytest.mark.parametrize("case", [(40, 80, 3, 3, 400), (128, 256, 11, 3, 200)], ids=lambda c: "%dx%d" % (c[0], c[1]))
@pytest.mark.parametrize("window", [1, 64])
def test_trees_match_oracle_table(gpu, orc, case, kw, window):
    m, n, seed, U, mx = case
    A, b, c, U = synth.dense_ilp(m, n, seed, U)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bnb.table_from(orc), window=window, max_nodes=mx, **kw)
    got = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), window=window, max_nodes=mx, **kw)
    assert got["rc"] == ref["rc"] == 0
    same_result(got, ref)
    assert (got["sb_lps"], got["sb_pivots"]) == (ref["sb_lps"], ref["sb_pivots"])
    assert got["count"] > 50


@pytest.mark.parametrize("quirks", [1, 0])
def test_certificate_on_gpu_children(gpu, quirks):
    nodes, _keep = node_set(gpu, (40, 80, 5, 3), 4, quirks=quirks)
    assert sum(certify_node(P, None, quirks) for P, _ in nodes) > 20


@pytest.mark.parametrize("var_strat", [3, 4])
def test_pinned_cut_ilp_closes_on_the_highs_optimum(gpu, var_strat):
    pin = json.load(open(os.path.join(ROOT, "tests", "golden", "milp_pins.json")))["cut_ilps"][0]
    A, b, c, U = synth.dense_ilp(pin["m"], pin["n"], pin["seed"], pin["U"], pin["cap"])
    r = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), var_strat=var_strat, quirks=0)
    assert r["rc"] == 0 and r["hit_limit"] == 0 and r["has_incumbent"]
    assert abs(r["best_lower"] - pin["milp_obj"]) <= 1e-6 * (1 + abs(pin["milp_obj"]))
