"""GPU: row deletion on many live tableaux in one launch and the purge of cut rows in the tree (DESIGN.md "Cut purging in the tree
(node_purge)").  k_delrows_many through mvx_del_rows_many against k_delrows through mvx_del_rows, handle by handle, as 64-bit
patterns: handles of different row counts (one past its spare rows) with different delete sets in one batch, batches of one and
two, a batch that mixes a given-up tableau, an untouched handle and a never-solved one, children with their branching bounds
pending, refusals.  Then whole trees with the purge on the device table, on a copy without del_rows_many and on one without
del_rows either, and one deeper tree with efficacy-selected cuts."""
import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import BS, DB, FX, LO, OPT, UNDEF, UP

from . import general_at_size as gs
from .test_bnb_general import INSTANCES, check_pin, failures, instance, run
from .test_bnb_host import same_result
from .test_gpu_purge import SHAPES, aborts, bits, cut_rows, delete_sets, solved, state

pytestmark = pytest.mark.gpu

SET_NAMES = ["one", "first", "every second", "all", "last tableau row", "two adjacent"]
EXTRA = {3: 5, 7: 40, 11: 5}  # copy -> cut rows appended to it first; 40 is more than the 32 rows every slab keeps spare


def same_state(a, b, what):
    assert a.m == b.m and a.status == b.status, what
    for x, y in zip(state(a), state(b)):
        assert np.array_equal(bits(x) if x.dtype == np.float64 else x, bits(y) if y.dtype == np.float64 else y), what
    assert np.array_equal(bits(a.col_prim()), bits(b.col_prim())), what


def sources(gpu, name):
    """13 solved handles out of one base, three of them with more rows: [(handle, delete set)], every set name used."""
    inst, base = solved(gpu, name)
    out = []
    for i in range(13):
        X = base.copy()
        if i in EXTRA:
            vals, rhs = cut_rows(inst, X.col_prim(), EXTRA[i], 900 + i)
            assert bnb.add_cut_rows(X, vals, rhs) == 0
            assert X.simplex(it_lim=20000) == 0 and X.status == OPT, (name, i, X.status)
            assert X.m == base.m + EXTRA[i]
        sets = delete_sets(X.basis()[0], X.m)
        assert set(SET_NAMES) <= set(sets) or i in EXTRA, (name, i, sorted(sets))
        names = [s for s in SET_NAMES if s in sets]
        out.append((X, sets[names[i % len(names)]]))
    assert base.m + 40 > SHAPES[name][0] + 32
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_del_rows_many_equals_del_rows(gpu, name):
    src = sources(gpu, name)
    assert len({X.m for X, _ in src}) == 3
    for count in (13, 1, 2):
        many = [X.copy() for X, _ in src[:count]]
        twins = [X.copy() for X, _ in src[:count]]
        lists = [d for _, d in src[:count]]
        assert bnb.del_rows_many(many, lists) == 0
        for k, (H, Tw, (X, d)) in enumerate(zip(many, twins, src)):
            assert Tw.del_rows(d) == 0
            assert H.m == X.m - len(d) and H.status == UNDEF, (name, count, k)
            same_state(H, Tw, (name, count, k))
        for k, (H, Tw, (X, d)) in enumerate(zip(many, twins, src)):
            for P in (H, Tw):
                assert P.simplex() == 0 and P.status == OPT and P.it_cnt == X.it_cnt, (name, count, k, P.status, P.it_cnt, X.it_cnt)
                assert bits(P.obj) == bits(X.obj), (name, count, k)
            same_state(H, Tw, (name, count, k, "solved"))
    # the sources were not touched by their copies' deletions
    for X, _ in src:
        assert X.status == OPT


def test_mixed_batch(gpu):
    """One call: a handle that loses a non-basic row (its tableau is given up), one with an empty list (not touched at all), one
    that was never solved (the model edit only), and handles whose rows leave in place."""
    name = "33x130"
    inst, base = solved(gpu, name)
    stat = base.row_stat()
    nonbasic = [i + 1 for i in range(base.m) if stat[i] != BS]
    assert nonbasic
    sets = delete_sets(base.basis()[0], base.m)
    fresh, fresh_twin = gs.load(gpu, inst), gs.load(gpu, inst)
    hs = [base.copy(), base.copy(), base.copy(), fresh, base.copy()]
    twins = [base.copy(), base.copy(), base.copy(), fresh_twin, base.copy()]
    lists = [sets["every second"], [nonbasic[len(nonbasic) // 2]], [], [2, 5], sets["two adjacent"]]
    untouched = state(hs[2])
    assert bnb.del_rows_many(hs, lists) == 0
    for Tw, l in zip(twins, lists):
        if l:
            assert Tw.del_rows(l) == 0
    # in place
    for k in (0, 4):
        same_state(hs[k], twins[k], k)
    # given up: no tableau, the next solve starts from the slack basis and reaches the twin's objective
    with pytest.raises(RuntimeError):
        hs[1].tableau()
    assert hs[1].m == base.m - 1 and hs[1].status == UNDEF
    for P in (hs[1], twins[1]):
        assert P.simplex() == 0 and P.status == OPT and P.it_cnt > 0
    assert abs(hs[1].obj - twins[1].obj) <= 1e-9 * max(1.0, abs(twins[1].obj)), (hs[1].obj, twins[1].obj)
    # not touched: still OPT, the same bits
    assert hs[2].status == OPT and hs[2].m == base.m
    for x, y in zip(state(hs[2]), untouched):
        assert np.array_equal(bits(x) if x.dtype == np.float64 else x, bits(y) if y.dtype == np.float64 else y)
    # never solved: the model edit only; its first solve is the twin's
    assert fresh.m == fresh_twin.m == SHAPES[name][0] - 2
    for P in (fresh, fresh_twin):
        assert P.simplex(it_lim=20000) == 0 and P.status == OPT
    assert fresh.it_cnt == fresh_twin.it_cnt
    same_state(fresh, fresh_twin, "never solved")
    for k in (0, 4):
        for P in (hs[k], twins[k]):
            assert P.simplex() == 0 and P.status == OPT and P.it_cnt == base.it_cnt and bits(P.obj) == bits(base.obj), k


@pytest.mark.parametrize("name", ["24x48", "70x200"])
def test_children_with_pending_branching_bounds(gpu, name):
    """The tree's own case: both children of a solved node carry their branching bound on a basic column as a pending edit when
    their rows leave.  del_rows_many against del_rows on twins: the same pivots and the same bits after the solve."""
    _inst, base = solved(gpu, name)
    head = base.basis()[0]
    m = base.m
    x = base.col_prim()
    pick = None
    for i in range(1, m + 1):  # a basic structural column with a fractional value strictly inside its bounds
        j = int(head[i]) - m
        if j < 1:
            continue
        v = x[j - 1]
        lo, hi = gpu.get_col_lb(base.h, j), gpu.get_col_ub(base.h, j)
        if abs(v - round(v)) > 1e-3 and lo < np.floor(v) and np.ceil(v) < hi:
            pick = (j, v, lo, hi)
            break
    assert pick, "no basic column to branch on"
    j, v, lo, hi = pick
    dele = delete_sets(head, m)["every second"]

    def children():
        down, up = base.copy(), base.copy()
        if lo > -1e300:
            gpu.set_col_bnds(down.h, j, FX if lo == np.floor(v) else DB, lo, float(np.floor(v)))
        else:
            gpu.set_col_bnds(down.h, j, UP, 0.0, float(np.floor(v)))
        if hi < 1e300:
            gpu.set_col_bnds(up.h, j, FX if hi == np.ceil(v) else DB, float(np.ceil(v)), hi)
        else:
            gpu.set_col_bnds(up.h, j, LO, float(np.ceil(v)), 0.0)
        return [down, up]

    many, twins = children(), children()
    assert bnb.del_rows_many(many, [dele, dele]) == 0
    for Tw in twins:
        assert Tw.del_rows(dele) == 0
    moved = 0
    for H, Tw in zip(many, twins):
        same_state(H, Tw, name)
        for P in (H, Tw):
            assert P.simplex(it_lim=20000) == 0
        assert H.it_cnt == Tw.it_cnt and H.status == Tw.status, (name, H.it_cnt, Tw.it_cnt, H.status, Tw.status)
        same_state(H, Tw, (name, "solved"))
        moved += H.it_cnt > base.it_cnt
    assert moved >= 1  # a branching bound cut the vertex off: the pending edit was applied behind the deletion


def test_refusals_change_nothing(gpu):
    _inst, base = solved(gpu, "24x48")
    _inst2, other = solved(gpu, "6x5")
    hs = [base.copy() for _ in range(3)]
    before = [[a.tolist() for a in state(H)] for H in hs]

    def untouched():
        return all(H.status == OPT and H.m == base.m and [a.tolist() for a in state(H)] == b for H, b in zip(hs, before))

    m = base.m
    for lists in ([[1], [2], [2, 2]], [[1], [2], [m + 1]], [[1], [2], [0]], [[0], [2], [3]], [[1], [3, 1, 3], [2]]):
        assert bnb.del_rows_many(hs, lists) == -1 and untouched(), lists
    assert bnb.del_rows_many([hs[0], hs[1], hs[0]], [[1], [2], [3]]) == -1 and untouched()
    O = other.copy()
    assert bnb.del_rows_many([hs[0], O], [[1], [2]]) == -1 and untouched() and O.status == OPT and O.m == other.m
    L = bnb.lib()
    IP = bnb.C.POINTER(bnb.C.c_int)
    arr = (bnb.C.c_void_p * 3)(*[H.h for H in hs])
    rows = np.array([1, 2, 3], dtype=np.int32)
    for off in ([0, 2, 1, 3], [1, 2, 3, 3]):  # descending; off[0] is not 0
        o = np.array(off, dtype=np.int32)
        assert L.mvx_del_rows_many(arr, 3, o.ctypes.data_as(IP), rows.ctypes.data_as(IP)) == -1 and untouched(), off
    o = np.array([0, 1, 2, 3], dtype=np.int32)
    assert L.mvx_del_rows_many(arr, 0, o.ctypes.data_as(IP), rows.ctypes.data_as(IP)) == -1 and untouched()
    assert L.mvx_del_rows_many(None, 3, o.ctypes.data_as(IP), rows.ctypes.data_as(IP)) == -1 and untouched()
    # all lists empty: 0, and still nothing is touched
    assert bnb.del_rows_many(hs, [[], [], []]) == 0 and untouched()


# ------------------------------------------------------------------------------------------------ trees

PATHS = ["del_rows_many", "del_rows", "free rows"]
_TREES = {}


def fixture_trees(gpu, path):
    if path not in _TREES:
        table = None
        if path != "del_rows_many":
            table = bnb.table_from(gpu)
            assert table.del_rows_many and table.del_rows
            table.del_rows_many = None
            if path == "free rows":
                table.del_rows = None
        out = {}

        def one(rec):
            inst = instance(rec)
            r = run(gpu, rec, inst, table=table, cut_strat=1, node_purge=1, window=64)
            check_pin(rec, inst, r)
            assert 0 <= r["node_purge_calls"] <= r["node_purge_rows"]
            out[rec["index"], rec.get("seed")] = r

        a0 = aborts(gpu)
        bad = failures(INSTANCES[::10], one)
        assert not bad, "\n".join(bad)
        assert aborts(gpu) == a0
        _TREES[path] = out
    return _TREES[path]


@pytest.mark.parametrize("path", PATHS)
def test_fixture_trees_with_the_purge_close_on_the_pins(gpu, path):
    trees = fixture_trees(gpu, path)
    assert sum(r["node_purge_rows"] for r in trees.values()) >= 1  # the path under test ran


def test_batched_and_per_handle_deletion_give_one_tree(gpu):
    a, b = fixture_trees(gpu, "del_rows_many"), fixture_trees(gpu, "del_rows")
    assert a.keys() == b.keys()
    for key in a:
        same_result(a[key], b[key])
        for k in bnb.NODE_PURGE_COUNTERS:
            assert a[key][k] == b[key][k], (key, k)


def test_deeper_tree_with_selected_cuts(gpu):
    A, b, c, U = synth.dense_ilp(64, 128, 7, 1, 0.025)
    a0 = aborts(gpu)
    res = {}
    for purge in (1, 0):
        r = bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), quirks=0, cut_strat=1, cut_select=1, window=64, node_purge=purge)
        assert r["rc"] == 0 and r["hit_limit"] == 0 and r["has_incumbent"], (purge, r["rc"], r["hit_limit"])
        res[purge] = r
    # both trees are exact: the same optimum, within the tolerance the fixture pins are held to
    assert abs(res[1]["best_lower"] - res[0]["best_lower"]) <= 1e-6 * (1 + abs(res[0]["best_lower"])), (res[1]["best_lower"], res[0]["best_lower"])
    assert res[1]["node_purge_rows"] > 0 and res[1]["node_purge_calls"] > 0
    assert res[0]["node_purge_rows"] == 0 and res[0]["node_purge_calls"] == 0
    assert 0 < res[1]["node_cut_rows_peak"] and 0 < res[0]["node_cut_rows_peak"]
    assert aborts(gpu) == a0
