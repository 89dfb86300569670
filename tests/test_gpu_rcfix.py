"""GPU: reduced-cost bound tightening on the device (k_rcfix through mvx_rc_tighten_many, k_setbnds through
mvx_tighten_cols_many) against the host twins through the engine's own table (mvx_bnb_rc_tighten, mvx_set_col_bnds per entry),
and rc_fix = 1 trees on the HIP engine against the same driver over the oracle's table."""
import json
import os

import numpy as np
import pytest

from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import CV, DB, FX, IV, OPT, UP

from . import lpgen
from .test_bnb_host import same_result

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9


def config5():
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "config5.json")))
    return synth.dense_ilp(fx["m"], fx["n"], fx["seed"], fx["U"], fx["cap"])


def tree_nodes(gpu, case, count):
    A, b, c, U = synth.dense_ilp(*case)
    return bnb.node_sample(lpgen.load_ilp(gpu, A, b, c, U), count)


def device_vs_twin(nodes, cutoffs):
    rc, lists = bnb.rc_tighten_many(nodes, cutoffs, TOL)
    assert rc == 0
    total = 0
    for t, P in enumerate(nodes):
        hrc, want = bnb.rc_tighten_node(P, cutoffs[t], TOL)
        assert hrc == 0
        assert lists[t] == want, (t, cutoffs[t], lists[t][:4], want[:4])
        assert [e[0] for e in want] == sorted(e[0] for e in want)
        total += len(want)
    return total


def spread_cutoffs(nodes, deltas):
    """A cutoff per handle: the node's LP value less one of `deltas` (maximisation), in turn."""
    return [P.obj - deltas[t % len(deltas)] for t, P in enumerate(nodes)]


@pytest.mark.parametrize("k", [1, 7, 64])
def test_batches_match_host_twin(gpu, k):
    nodes = tree_nodes(gpu, (128, 256, 7, 1, 0.01), 64)
    assert len(nodes) == 64
    assert device_vs_twin(nodes[:k], spread_cutoffs(nodes[:k], (0.5, 2.0, 7.5, -1.0))) > 0


@pytest.mark.parametrize("case", [(512, 1024, 12345, 3, 0.4), (1024, 2048, 5, 2)], ids=str)
def test_tree_nodes_match_host_twin(gpu, case):
    nodes = tree_nodes(gpu, case, 16)
    assert device_vs_twin(nodes, spread_cutoffs(nodes, (3.0, 25.0, 70.0, 400.0))) > 0
    assert device_vs_twin(nodes, [float("-inf")] * len(nodes)) == 0
    assert device_vs_twin(nodes, [P.obj + 1.0 for P in nodes]) == 0


def test_config5_root_fixes_75_columns(gpu):
    A, b, c, U = config5()
    nodes = bnb.node_sample(synth.load_ilp(gpu, A, b, c, U), 16)
    device_vs_twin(nodes, [20.0] * len(nodes))
    rc, lists = bnb.rc_tighten_many(nodes[:1], [20.0], TOL)
    assert rc == 0 and len(lists[0]) == 75 and all(lb == ub for _j, lb, ub in lists[0]), len(lists[0])


def test_mixed_kinds_general_lps(gpu):
    rng = np.random.default_rng(5)
    checked = entries = 0
    for _ in range(80):
        A, row_b, col_b, c, d = lpgen.random_general_lp(rng, 10, 12)
        P = gpu.create()
        P.load_general(A, row_b, col_b, c, c0=1.5, kinds=[IV if rng.random() < 0.7 else CV for _ in c], direction=d)
        P.simplex()
        if P.status != OPT:
            continue
        sg = -1.0 if d == capi.MIN else 1.0
        for delta in (0.25, 1.5, 6.0, 40.0):
            entries += device_vs_twin([P], [P.obj - sg * delta])
        checked += 1
    assert checked > 30 and entries > 30


def cut_nodes(nodes):
    out = []
    for P in nodes:
        Q = P.copy()
        assert bnb.node_cuts(Q, dict(cut_strat=1, quirks=0)) >= 1
        Q.simplex()
        if Q.status == OPT:
            out.append(Q)
    return out


def test_cut_rows_and_return_codes(gpu):
    nodes = tree_nodes(gpu, (40, 80, 3, 3), 8)
    cut = cut_nodes(nodes[:4])
    assert cut and cut[0].m > nodes[0].m
    both = cut + nodes
    assert device_vs_twin(both, spread_cutoffs(both, (1.0, 5.0, 20.0))) > 0
    E = nodes[0].copy()
    gpu.set_col_bnds(E.h, 1, UP, 0.0, 0.0)  # an edit: not solved
    assert bnb.rc_tighten_many([nodes[0], E], [0.0, 0.0])[0] == -3
    other = tree_nodes(gpu, (12, 24, 5, 3), 1)
    assert bnb.rc_tighten_many([nodes[0], other[0]], [0.0, 0.0])[0] == -1  # another column count


def state(P):
    n = P.n
    api = P.api
    return ([api.get_col_lb(P.h, j) for j in range(1, n + 1)], [api.get_col_ub(P.h, j) for j in range(1, n + 1)],
            [api.get_col_type(P.h, j) for j in range(1, n + 1)], [a.tolist() for a in P.basis()], P.status)


def assert_same_handles(X, Y):
    assert state(X) == state(Y)
    assert np.array_equal(X.tableau(), Y.tableau())
    X.simplex()
    Y.simplex()
    assert (X.status, X.obj, X.it_cnt) == (Y.status, Y.obj, Y.it_cnt)
    assert np.array_equal(X.tableau(), Y.tableau()) and state(X) == state(Y)


@pytest.mark.parametrize("case", [(128, 256, 7, 1, 0.01), (40, 80, 3, 3)], ids=str)
def test_batched_apply_equals_one_by_one(gpu, case):
    nodes = tree_nodes(gpu, case, 12)
    if case == (40, 80, 3, 3):
        nodes = cut_nodes(nodes[:4]) + nodes
    rc, lists = bnb.rc_tighten_many(nodes, spread_cutoffs(nodes, (0.5, 2.0, 7.5)), TOL)
    assert rc == 0 and sum(len(l) for l in lists) > 0
    # both children of every branching, with their pending branching edit, in ONE call
    kids, kid_lists, twins = [], [], []
    for P, l in zip(nodes, lists):
        _st, viol = bnb.print_info(P, quirks=0)
        if not viol:
            continue
        for S, R in zip(bnb.make_children(P, viol[0], quirks=0), bnb.make_children(P, viol[0], quirks=0)):
            kids.append(S)
            kid_lists.append(l)
            for (j, lb, ub) in l:
                gpu.set_col_bnds(R.h, j, FX if lb == ub else DB, lb, ub)
            twins.append(R)
    assert len(kids) >= 8
    assert bnb.tighten_cols_many(kids, kid_lists) == 0
    for S, R in zip(kids, twins):
        assert_same_handles(S, R)


def test_one_call_over_empty_short_unsolved_and_fixing_lists(gpu):
    """One mvx_tighten_cols_many call over four handles: an empty list, a one-entry list, a handle that was loaded and never
    solved (a model edit only: no device entry) and a list that fixes a column (lb == ub: MVX_NS)."""
    A, b, c, U = synth.dense_ilp(40, 80, 3, 3)
    nodes = bnb.node_sample(lpgen.load_ilp(gpu, A, b, c, U), 8)
    rc, lists = bnb.rc_tighten_many(nodes, spread_cutoffs(nodes, (1.0, 5.0, 20.0)), TOL)
    assert rc == 0
    one = next((P, [e]) for P, l in zip(nodes, lists) for e in l)
    stat = nodes[1].col_stat()
    j = next(j for j in range(1, nodes[1].n + 1) if stat[j - 1] in (capi.NL, capi.NU)
             and gpu.get_col_lb(nodes[1].h, j) < gpu.get_col_ub(nodes[1].h, j))
    at = gpu.get_col_lb(nodes[1].h, j) if stat[j - 1] == capi.NL else gpu.get_col_ub(nodes[1].h, j)
    cases = [(nodes[0], []), one, (lpgen.load_ilp(gpu, A, b, c, U), [(3, 0.0, 1.0), (7, 2.0, 2.0)]), (nodes[1], [(j, at, at)])]
    kids, twins = [P.copy() for P, _l in cases], [P.copy() for P, _l in cases]
    assert bnb.tighten_cols_many(kids, [l for _P, l in cases]) == 0
    for R, (_P, l) in zip(twins, cases):
        for (col, lb, ub) in l:
            gpu.set_col_bnds(R.h, col, FX if lb == ub else DB, lb, ub)
    assert kids[0].status == OPT and kids[3].col_stat()[j - 1] == capi.NS
    S, R = kids[2], twins[2]  # no basis, no tableau: the model, then what a solve makes of it
    cols = range(1, S.n + 1)
    assert [(gpu.get_col_lb(S.h, q), gpu.get_col_ub(S.h, q), gpu.get_col_type(S.h, q)) for q in cols] == \
        [(gpu.get_col_lb(R.h, q), gpu.get_col_ub(R.h, q), gpu.get_col_type(R.h, q)) for q in cols]
    assert (gpu.get_col_lb(S.h, 7), gpu.get_col_ub(S.h, 7), gpu.get_col_type(S.h, 7), S.status) == (2.0, 2.0, FX, R.status)
    S.simplex()
    R.simplex()
    assert (S.status, S.obj, S.it_cnt) == (R.status, R.obj, R.it_cnt) and np.array_equal(S.tableau(), R.tableau())
    for S, R in ((kids[0], twins[0]), (kids[1], twins[1]), (kids[3], twins[3])):
        assert_same_handles(S, R)


def test_apply_refuses_what_would_move_a_column(gpu):
    P = tree_nodes(gpu, (40, 80, 3, 3), 1)[0]
    stat = P.col_stat()
    basic = int(np.nonzero(stat == capi.BS)[0][0]) + 1
    at_lower = int(np.nonzero(stat == capi.NL)[0][0]) + 1
    Q, R = P.copy(), P.copy()
    before = state(Q)
    lo, hi = gpu.get_col_lb(Q.h, at_lower), gpu.get_col_ub(Q.h, at_lower)
    assert bnb.tighten_cols_many([Q], [[(basic, 0.0, 1.0)]]) == -4
    assert bnb.tighten_cols_many([R, Q], [[], [(at_lower, lo + 1.0, hi)]]) == -4  # the resting value would move
    assert bnb.tighten_cols_many([Q], [[(at_lower, lo, hi), (at_lower, lo, hi)]]) == -1  # not ascending
    assert bnb.tighten_cols_many([Q], [[(Q.n + 1, 0.0, 1.0)]]) == -1
    assert state(Q) == before and Q.status == OPT and np.array_equal(Q.tableau(), P.tableau())


def same_tree(got, ref):
    assert got["rc"] == ref["rc"] == 0
    same_result(got, ref)
    for k in ("rc_calls", "rc_fixed", "rc_tightened", "heur_calls", "heur_found", "heur_improved", "incumbent_heur"):
        assert got[k] == ref[k], k


@pytest.mark.parametrize("kw", [dict(window=1), dict(window=64), dict(window=64, cut_strat=1, heur=2), dict(node_strat=1)], ids=str)
@pytest.mark.parametrize("case", [(10, 20, 4, 3), (16, 32, 5, 2), ("setcover", 40, 60, 3)], ids=str)
def test_small_trees_match_oracle_table(gpu, orc, case, kw):
    ref = bnb.branch_and_bound(lpgen.load_case(orc, case), table=bnb.table_from(orc), quirks=0, rc_fix=1, **kw)
    got = bnb.branch_and_bound(lpgen.load_case(gpu, case), quirks=0, rc_fix=1, **kw)
    same_tree(got, ref)
    assert got["hit_limit"] == 0
    if "node_strat" not in kw:  # best-bound order meets its incumbent late: the rule need not find anything to fix there
        assert got["rc_fixed"] > 0


def test_config5_prefix_matches_oracle_table(gpu, orc):
    A, b, c, U = config5()
    kw = dict(quirks=0, heur=2, rc_fix=1, window=64, max_nodes=300)
    ref = bnb.branch_and_bound(synth.load_ilp(orc, A, b, c, U), table=bnb.table_from(orc), **kw)
    got = bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), **kw)
    same_tree(got, ref)
    assert got["rc_fixed"] >= 75


def test_config5_closes_on_20_same_tree_at_window_1_and_64(gpu):
    A, b, c, U = config5()
    from .test_gpu_chain import cluster_counts

    aborts0 = cluster_counts(gpu)[1]
    r64 = bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), quirks=0, heur=2, rc_fix=1, window=64)
    r1 = bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), quirks=0, heur=2, rc_fix=1, window=1)
    print("config-5 heur 2 + rc_fix: nodes %d pivots %d rc_calls %d fixed %d tightened %d" % (
        r64["count"], r64["total_pivots"], r64["rc_calls"], r64["rc_fixed"], r64["rc_tightened"]))
    same_tree(r64, r1)
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "milp_pins.json")))
    assert pins["config5"]["milp_obj"] == 20.0
    assert r64["hit_limit"] == 0 and abs(r64["best_lower"] - 20.0) <= 1e-6 * 21
    assert cluster_counts(gpu)[1] == aborts0
