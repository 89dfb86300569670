"""GPU: node bound propagation on the device (k_prop through mvx_propagate_many, k_setbnds through mvx_set_col_bnds_many)
against the host twins through the engine's own table (mvx_bnb_propagate, mvx_set_col_bnds per entry), and prop trees on the
HIP engine against the same driver over the oracle's table and the enumerated pins."""
import json
import math
import os

import numpy as np
import pytest

from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import CV, DB, FR, FX, IV, LO, OPT, UP

from . import lpgen
from .test_bnb_general import INSTANCES, check_pin, failures, instance, run
from .test_bnb_host import same_result
from .test_bnb_prop import COUNTERS, set_bounds
from .test_gpu_rcfix import assert_same_handles, config5, cut_nodes, tree_nodes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf
RND_NMAX = 4096  # mvx_internal.hpp: the columns (and the rows' activities) a k_prop workgroup holds in LDS


def device_vs_twin(root, handles, K=8):
    """One mvx_propagate_many call against mvx_bnb_propagate per handle: lists, infeasible and rounds.  Returns the results."""
    rc, got = bnb.propagate_many(root, handles, K)
    assert rc == 0
    for t, P in enumerate(handles):
        hrc, want = bnb.propagate_node(P, root, K)
        assert hrc == 0
        assert got[t] == want, (t, got[t][:2], want[:2], got[t][2][:4], want[2][:4])
        assert [e[0] for e in want[2]] == sorted(e[0] for e in want[2])
    return got


def unsolved_children(nodes):
    kids = []
    for P in nodes:
        _st, viol = bnb.print_info(P, quirks=0)
        if viol:
            kids += list(bnb.make_children(P, viol[0], quirks=0))
    return kids


@pytest.fixture(scope="module")
def sample(gpu):
    A, b, c, U = synth.dense_ilp(128, 256, 7, 1, 0.01)
    root = lpgen.load_ilp(gpu, A, b, c, U)
    kids = unsolved_children(bnb.node_sample(root, 40))
    assert len(kids) >= 64 and all(S.status != OPT for S in kids)  # a pending branching edit each
    return root, kids[:64]


@pytest.mark.parametrize("k", [1, 7, 64])
def test_batches_of_unsolved_children_match_the_twin(sample, k):
    root, kids = sample
    got = device_vs_twin(root, kids[:k])
    if k == 64:
        assert sum(len(g[2]) for g in got) > 0
        for K in (1, 2):
            device_vs_twin(root, kids, K)


def test_mixed_kinds_general_models(gpu):
    rng = np.random.default_rng(7)
    entries = proved = 0
    for _ in range(80):
        A, row_b, col_b, c, d = lpgen.random_general_lp(rng, 10, 12)
        root = gpu.create()
        root.load_general(A, row_b, col_b, c, kinds=[IV if rng.random() < 0.7 else CV for _ in c], direction=d)
        clo, chi = lpgen.bounds_arrays(col_b)
        handles = [root]
        for variant in (1, 2):
            P = root.copy()
            for j in rng.choice(len(c), size=min(len(c), variant), replace=False):
                j = int(j)
                mid = float(rng.integers(-2, 5))
                l, u = float(clo[j]), float(chi[j])
                if rng.random() < 0.5:
                    u = min(u, mid) if l <= mid else u
                else:
                    l = max(l, mid) if mid <= u else l
                set_bounds(gpu, P, j + 1, l, u)
            handles.append(P)
        for inf, _rounds, lst in device_vs_twin(root, handles):
            entries += len(lst)
            proved += inf
    assert entries > 100 and proved > 5, (entries, proved)


def sized_model(gpu, rng, m, n, dens, boxed=0.5):
    """random_general_lp's recipe at a given size: integer data, rows bounded around the activity of an integer point x0
    (which therefore no propagation may cut off); `boxed` of the columns have both bounds."""
    A = np.round(rng.normal(size=(m, n)) * 3)
    A[rng.random((m, n)) >= dens] = 0
    x0 = rng.integers(0, 4, size=n).astype(float)
    act = A @ x0
    row_b = []
    for i in range(m):
        t = int(rng.choice([LO, UP, DB, FX, FR], p=[0.25, 0.35, 0.2, 0.1, 0.1]))
        row_b.append((t, float(act[i] - (0 if t == FX else rng.integers(0, 3))), float(act[i] + rng.integers(1, 4))))
    col_b = []
    for j in range(n):
        t = DB if rng.random() < boxed else int(rng.choice([LO, UP, FR], p=[0.6, 0.2, 0.2]))
        col_b.append((t, float(x0[j] - rng.integers(0, 3)), float(x0[j] + rng.integers(1, 4))))
    P = gpu.create()
    P.load_general(A, row_b, col_b, np.ones(n), kinds=[IV if rng.random() < 0.8 else CV for _ in range(n)])
    return P, x0


@pytest.mark.parametrize("shape", [(1100, 48, 0.2, 0.5), (4200, 24, 0.3, 0.5), (6, RND_NMAX, 0.002, 1.0)], ids=str)
def test_sizes_around_the_kernels_limits(gpu, shape):
    """More rows than one pass of the workgroup, more rows than the LDS holds (the global slice), and the widest model."""
    m, n, dens, boxed = shape
    rng = np.random.default_rng(m)
    root, x0 = sized_model(gpu, rng, m, n, dens, boxed)
    kid, deep = root.copy(), root.copy()
    j = int(np.argmax([gpu.get_col_kind(root.h, k) != CV for k in range(1, n + 1)])) + 1
    set_bounds(gpu, kid, j, x0[j - 1], x0[j - 1])
    for k in range(1, n + 1):  # deep in a tree: most columns fixed, so the rows say much about the others
        if k % 16:
            set_bounds(gpu, deep, k, x0[k - 1], x0[k - 1])
    got = device_vs_twin(root, [root, kid, deep])
    # x0 is a point of every one of them: never infeasible, never cut off; and something is learnt
    assert not any(inf for inf, _rounds, _lst in got) and sum(len(lst) for _inf, _rounds, lst in got) > 0
    for _inf, _rounds, lst in got:
        assert all(lb <= x0[c - 1] <= ub for c, lb, ub in lst)


def test_more_columns_than_the_kernel_holds(gpu):
    root, _x0 = sized_model(gpu, np.random.default_rng(3), 6, RND_NMAX + 1, 0.002)
    assert bnb.propagate_many(root, [root], 8) == (-5, None)
    assert bnb.propagate_node(root, root, 8)[0] == 0
    assert bnb.propagate_many(root, [root], 0)[0] == -1
    other, _ = sized_model(gpu, np.random.default_rng(3), 6, 12, 0.5)
    assert bnb.propagate_many(root, [other], 8)[0] == -1  # another column count


def test_config5_up_child_is_decided_in_one_round(gpu):
    A, b, c, U = config5()
    root = synth.load_ilp(gpu, A, b, c, U)
    assert device_vs_twin(root, [root])[0] == (0, 1, [])  # at the root nothing can be fixed
    kids = []
    for j in (1, 98, 195):
        P = root.copy()
        gpu.set_col_bnds(P.h, j, FX, 1.0, 1.0)
        kids.append(P)
    for j, (inf, rounds, lst) in zip((1, 98, 195), device_vs_twin(root, kids)):
        assert (inf, rounds, len(lst)) == (0, 2, 1023)
        assert all((lb, ub) == (0.0, 0.0) for _c, lb, ub in lst) and j not in [e[0] for e in lst]


def per_entry(gpu, R, lst):
    for (j, lb, ub) in lst:
        set_bounds(gpu, R, j, lb, ub)


def mixed_list(gpu, S, rng):
    """A bound list over a solved-then-branched child S: every basic column (tightened where its range allows; more than 8 of
    them overflow the pending edits), non-basic columns whose resting value moves (NU with a lowered ub, NL with a raised lb),
    and columns that lose a bound (+-inf)."""
    stat = S.col_stat()
    lst = []
    for j in range(1, S.n + 1):
        lb, ub = gpu.get_col_lb(S.h, j), gpu.get_col_ub(S.h, j)
        if lb <= -1e300 or ub >= 1e300 or lb == ub:
            continue
        r = rng.random()
        if stat[j - 1] == capi.BS:
            lst.append((j, lb + 1.0, ub) if r < 0.5 and ub - lb >= 2.0 else (j, lb, ub - 1.0) if ub - lb >= 1.0 else (j, lb, ub))
        elif stat[j - 1] == capi.NU and r < 0.4:
            lst.append((j, lb, ub - 1.0))
        elif stat[j - 1] == capi.NL and r < 0.4:
            lst.append((j, lb + 1.0, ub))
        elif r < 0.5:
            lst.append((j, -INF, ub))
        elif r < 0.6:
            lst.append((j, lb, INF))
        elif r < 0.65:
            lst.append((j, -INF, INF))
    return lst


@pytest.mark.parametrize("case", [(128, 256, 7, 1, 0.01), (40, 80, 3, 3)], ids=str)
def test_batched_apply_equals_one_by_one(gpu, case):
    rng = np.random.default_rng(11)
    nodes = tree_nodes(gpu, case, 8)
    if case == (40, 80, 3, 3):
        nodes = cut_nodes(nodes[:4]) + nodes  # tableau rows beyond the model's: the shifts cover them
        assert nodes[0].m > nodes[-1].m
    kids, twins, lists = [], [], []
    basic_most = moved = absent = 0
    for P in nodes:
        _st, viol = bnb.print_info(P, quirks=0)
        if not viol:
            continue
        for S, R in zip(bnb.make_children(P, viol[0], quirks=0), bnb.make_children(P, viol[0], quirks=0)):
            lst = mixed_list(gpu, S, rng)
            stat = S.col_stat()
            basic_most = max(basic_most, sum(1 for e in lst if stat[e[0] - 1] == capi.BS))
            moved += sum(1 for (j, lb, ub) in lst if (stat[j - 1] == capi.NU and ub < gpu.get_col_ub(S.h, j))
                         or (stat[j - 1] == capi.NL and lb > gpu.get_col_lb(S.h, j)))
            absent += sum(1 for e in lst if math.isinf(e[1]) or math.isinf(e[2]))
            kids.append(S)
            twins.append(R)
            lists.append(lst)
    kids.append(nodes[-1].copy())  # a handle with an empty list stays as it is
    twins.append(nodes[-1].copy())
    lists.append([])
    assert len(kids) >= 8 and basic_most > 8 and moved > 10 and absent > 10, (len(kids), basic_most, moved, absent)
    assert bnb.set_col_bnds_many(kids, lists) == 0
    for R, lst in zip(twins, lists):
        per_entry(gpu, R, lst)
    assert kids[-1].status == OPT
    for S, R in zip(kids, twins):
        assert_same_handles(S, R)


def test_a_row_sent_twice_takes_the_later_bounds(gpu):
    """A pending edit of column j's row, then a list with at least 8 basic columns before j, j itself with other bounds, and at
    least 8 behind it: the pending edits overflow twice and the row of j goes to the device both times.  The per-entry path's
    launches are ordered, so the later bounds stand; the one launch must leave the same."""
    done = 0
    for P in tree_nodes(gpu, (80, 160, 3, 3), 4):
        stat = P.col_stat()
        basic = [j for j in range(1, P.n + 1) if stat[j - 1] == capi.BS and gpu.get_col_ub(P.h, j) - gpu.get_col_lb(P.h, j) >= 2.0]
        if len(basic) < 17:
            continue
        j = basic[8]
        assert len([b for b in basic if b < j]) >= 8 and len([b for b in basic if b > j]) >= 8
        S, R = P.copy(), P.copy()
        lo, hi = gpu.get_col_lb(P.h, j), gpu.get_col_ub(P.h, j)
        for Q in (S, R):
            gpu.set_col_bnds(Q.h, j, DB, lo, hi - 1.0)  # the branching edit: pending on the row of j
        lst = [(b, lo + 1.0, hi - 1.0) if b == j else (b, gpu.get_col_lb(P.h, b), gpu.get_col_ub(P.h, b) - 1.0) for b in basic]
        assert bnb.set_col_bnds_many([S], [lst]) == 0
        per_entry(gpu, R, lst)
        assert_same_handles(S, R)
        assert (gpu.get_col_lb(S.h, j), gpu.get_col_ub(S.h, j)) == (lo + 1.0, hi - 1.0)
        done += 1
    assert done >= 2, done


def test_the_1023_entry_list_and_bad_lists(gpu):
    A, b, c, U = config5()
    root = synth.load_ilp(gpu, A, b, c, U)
    X = root.copy()
    X.simplex()
    gpu.set_col_bnds(X.h, 98, FX, 1.0, 1.0)
    Y = X.copy()
    rc, [(inf, _rounds, lst)] = bnb.propagate_many(root, [X], 8)
    assert rc == 0 and not inf and len(lst) == 1023
    assert bnb.set_col_bnds_many([X], [lst]) == 0
    per_entry(gpu, Y, lst)
    assert_same_handles(X, Y)
    # a bad list changes nothing
    P = tree_nodes(gpu, (40, 80, 3, 3), 1)[0]
    Q = P.copy()
    for bad in ([(2, 0.0, 1.0), (2, 0.0, 1.0)], [(3, 0.0, 1.0), (2, 0.0, 1.0)], [(1, 2.0, 1.0)], [(1, math.nan, 1.0)], [(Q.n + 1, 0.0, 1.0)],
                [(1, INF, INF)]):
        assert bnb.set_col_bnds_many([Q], [bad]) == -1, bad
        assert bnb.set_col_bnds_many([P.copy(), Q], [[(1, 0.0, 1.0)], bad]) == -1, bad
    assert bnb.set_col_bnds_many([Q, Q], [[(1, 0.0, 1.0)], [(2, 0.0, 1.0)]]) == -1  # a handle listed twice
    assert_same_handles(Q, P.copy())


def same_tree(got, ref):
    assert got["rc"] == ref["rc"] == 0
    same_result(got, ref)
    for k in COUNTERS:
        assert got[k] == ref[k], k


@pytest.mark.parametrize("kw", [dict(window=1), dict(window=64), dict(window=64, cut_strat=1, heur=2, rc_fix=1)], ids=str)
@pytest.mark.parametrize("case", [(10, 20, 4, 3), (16, 32, 5, 2), ("setcover", 40, 60, 3)], ids=str)
def test_small_trees_match_oracle_table(gpu, orc, case, kw):
    ref = bnb.branch_and_bound(lpgen.load_case(orc, case), table=bnb.table_from(orc), quirks=0, prop=8, **kw)
    got = bnb.branch_and_bound(lpgen.load_case(gpu, case), quirks=0, prop=8, **kw)
    same_tree(got, ref)
    assert got["hit_limit"] == 0 and got["prop_calls"] == got["n_nodes"]


@pytest.mark.parametrize("window", [1, 64])
def test_fixture_trees_match_oracle_table_and_pins(gpu, orc, window):
    tab = bnb.table_from(orc)
    recs = INSTANCES[::4]

    def one(rec):
        inst = instance(rec)
        r = run(gpu, rec, inst, window=window, prop=8)
        check_pin(rec, inst, r)
        same_tree(r, run(orc, rec, inst, table=tab, window=window, prop=8))

    bad = failures(recs, one)
    assert not bad, "%d of %d fail:\n%s" % (len(bad), len(recs), "\n".join(bad))


def test_without_the_batched_apply_the_tree_is_the_same(gpu):
    """A table without set_col_bnds_many: set_col_bnds per entry, the same tree."""
    case = (16, 32, 5, 2)
    L = bnb.lib()
    full = bnb.LpApiTable.from_address(L.mvx_hip_lp_api())
    assert full.propagate_many and full.set_col_bnds_many
    part = bnb.LpApiTable()
    bnb.C.memmove(bnb.C.byref(part), bnb.C.byref(full), bnb.C.sizeof(part))
    part.set_col_bnds_many = None
    ref = bnb.branch_and_bound(lpgen.load_case(gpu, case), quirks=0, prop=8, window=64)
    got = bnb.branch_and_bound(lpgen.load_case(gpu, case), quirks=0, prop=8, window=64, table=part)
    same_tree(got, ref)


def test_wider_than_the_kernel_the_tree_runs_on_the_twin(gpu, orc):
    """n = RND_NMAX + 1: mvx_propagate_many answers -5 and the driver goes on with the host twin -- the oracle-table tree."""
    case = (4, RND_NMAX + 1, 2, 1, 0.0005)  # b_i about 21: an up-branch fixes the rest
    for window in (1, 64):
        kw = dict(quirks=0, prop=8, window=window, max_nodes=40)
        ref = bnb.branch_and_bound(lpgen.load_case(orc, case), table=bnb.table_from(orc), **kw)
        got = bnb.branch_and_bound(lpgen.load_case(gpu, case), **kw)
        same_tree(got, ref)
        assert got["prop_calls"] > 1 and got["prop_fixed"] > 0


@pytest.mark.parametrize("extra", [dict(), dict(heur=2, rc_fix=1)], ids=["prop", "heur2_rcfix_prop"])
def test_config5_closes_on_20_same_tree_at_window_1_and_64(gpu, extra):
    A, b, c, U = config5()
    from .test_gpu_chain import cluster_counts

    aborts0 = cluster_counts(gpu)[1]
    r64 = bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), quirks=0, prop=8, window=64, **extra)
    r1 = bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), quirks=0, prop=8, window=1, **extra)
    print("config-5 prop 8 %s: nodes %d pivots %d prop_calls %d fixed %d tightened %d infeasible %d" % (
        extra, r64["count"], r64["total_pivots"], r64["prop_calls"], r64["prop_fixed"], r64["prop_tightened"], r64["prop_infeasible"]))
    same_tree(r64, r1)
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "milp_pins.json")))
    assert pins["config5"]["milp_obj"] == 20.0
    assert r64["hit_limit"] == 0 and abs(r64["best_lower"] - 20.0) <= 1e-6 * 21
    assert cluster_counts(gpu)[1] == aborts0
    plain = 15697 if not extra else 1349  # the tree without prop (DESIGN.md "Reduced-cost tightening")
    assert r64["count"] < plain
