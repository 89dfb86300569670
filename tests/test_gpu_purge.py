"""GPU: row deletion on a live tableau and the purge of the root cut rounds (DESIGN.md "Cut purging (cut_purge)").  k_delrows through
mvx_del_rows against numpy: the tableau and the basis are read before the call, the rows are taken out with np.delete, the
variable numbers are remapped by the rule of the definition, and everything is compared as 64-bit patterns.  Then the edges: a
non-basic row (the tableau is given up), pending bound edits behind a deleted row, clones, appends behind a deletion; the loop
and whole trees with the purge on the device table, and on a copy of it without del_rows (the free-row path)."""
import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import BS, DB, LO, OPT, UNDEF, UP

from . import general_at_size as gs
from . import lpgen
from .test_bnb_general import INSTANCES, check_pin, failures, instance, run

pytestmark = pytest.mark.gpu

# (m, n, seed, cut rows) of general_at_size.cold_dual_lp, the general-bound family that is bounded by construction.  33 x 130 has
# n + 1 = 131 columns: two 64-column tiles of k_delrows and a ragged third; 70 x 200 moves more rows than a lane holds in flight
# (DEL_BATCH = 8), and not a multiple of it.  A seed is the first from 1 on at which the oracle, which needs no device, solves the LP
# to OPT before and after the cut rows and leaves an auxiliary basic in the last tableau row, two basic auxiliaries in adjacent
# tableau rows, a non-basic auxiliary and, from 24 x 48 on, twelve basic auxiliaries (the flushed-edit case needs ten).
SHAPES = {"6x5": (6, 5, 1, 3), "24x48": (24, 48, 8, 7), "33x130": (33, 130, 1, 9), "70x200": (70, 200, 1, 13)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def cut_rows(inst, x, k, seed):
    """k dense rows v . y >= rhs that cut the vertex x off and keep the instance's own point x0: (vals (k, n + 1), rhs)."""
    rng = np.random.default_rng(seed)
    x0, n = inst["x0"], len(x)
    vals, rhs = np.zeros((k, n + 1)), np.zeros(k)
    assert np.abs(np.asarray(x) - x0).max() > 1e-2, "the vertex is the instance's own point: nothing to cut off"
    t = 0
    for _draw in range(100 * k):
        if t == k:
            break
        v = np.round(rng.uniform(-2.0, 2.0, n), 3) * (rng.random(n) >= 0.3)
        s, s0 = float(v @ x), float(v @ x0)
        if abs(s - s0) < 1e-3:
            continue
        if s > s0:
            v, s, s0 = -v, -s, -s0
        vals[t, 1:] = v
        rhs[t] = s + 0.75 * (s0 - s)
        t += 1
    assert t == k
    return vals, rhs


def build(api, name, batched=True):
    """The shape's LP solved to OPT, its cut rows appended and solved again: (instance, handle)."""
    m, n, seed, k = SHAPES[name]
    inst = gs.cold_dual_lp(m, n, seed)
    P = gs.load(api, inst)
    assert P.simplex(it_lim=20000) == 0 and P.status == OPT, (name, P.status)
    vals, rhs = cut_rows(inst, P.col_prim(), k, seed + 100)
    if batched:
        assert bnb.add_cut_rows(P, vals, rhs) == 0
    else:
        from .test_gpu_cutloop import append_per_row

        append_per_row(P, vals, rhs)
    assert P.simplex(it_lim=20000) == 0 and P.status == OPT, (name, P.status)
    return inst, P


_CACHE = {}


def solved(gpu, name):
    """Built once per shape and never edited: every test works on copies."""
    if name not in _CACHE:
        _CACHE[name] = build(gpu, name)
    return _CACHE[name]


def state(P):
    head, nb, flag = P.basis()
    return P.tableau(), head, nb, flag


def basic_rows(head, m):
    """{model row: tableau row} of the rows whose auxiliary variable is basic."""
    return {int(k): i for i, k in enumerate(head) if i >= 1 and 1 <= k <= m}


def delete_sets(head, m):
    pos = basic_rows(head, m)
    B = sorted(pos)
    sets = {"one": [B[len(B) // 2]], "first": [B[0]], "every second": B[::2], "all": B}
    if 1 <= head[m] <= m:
        sets["last tableau row"] = [int(head[m])]
    adj = [(int(head[i]), int(head[i + 1])) for i in range(1, m) if 1 <= head[i] <= m and 1 <= head[i + 1] <= m]
    if adj:
        sets["two adjacent"] = list(adj[len(adj) // 2])
    return sets


def expected(T, head, nb, flag, m, dele):
    """The definition in numpy: tableau rows out, variable numbers remapped."""
    pos = basic_rows(head, m)
    gone = sorted(pos[i] for i in dele)
    dl = np.array(sorted(dele))

    def renum(k):
        k = np.asarray(k)
        return np.where(k > m, k - len(dl), k - np.searchsorted(dl, k, side="left")).astype(np.int32)

    h = renum(np.delete(head, gone))
    h[0] = 0
    q = renum(nb)
    q[0] = 0
    return np.delete(T, gone, axis=0), h, q, flag.copy()


@pytest.mark.parametrize("name", list(SHAPES))
def test_del_rows_equals_numpy(gpu, name):
    _inst, base = solved(gpu, name)
    T, head, nb, flag = state(base)
    m = base.m
    sets = delete_sets(head, m)
    assert {"one", "first", "every second", "all", "last tableau row", "two adjacent"} <= set(sets), sorted(sets)
    res0, it0, obj0 = gpu.row_residual(base.h), base.it_cnt, base.obj
    for what, dele in sets.items():
        P = base.copy()
        assert P.del_rows(dele) == 0, what
        eT, eh, eq, ef = expected(T, head, nb, flag, m, dele)
        assert P.m == m - len(dele) and P.status == UNDEF, what
        gT, gh, gq, gf = state(P)
        assert np.array_equal(bits(gT), bits(eT)), (name, what, int((bits(gT) != bits(eT)).sum()))
        assert np.array_equal(gh, eh) and np.array_equal(gq, eq) and np.array_equal(gf, ef), (name, what)
        assert P.obj == obj0  # the mirror of row 0 is still the tableau's
        assert np.array_equal(bits(P.col_prim()), bits(base.col_prim())), (name, what)
        assert P.simplex() == 0 and P.status == OPT and P.it_cnt == it0, (name, what, P.status, P.it_cnt, it0)
        assert bits(P.obj) == bits(obj0), (name, what)
        assert gpu.row_residual(P.h) <= res0, (name, what, gpu.row_residual(P.h), res0)
        # nothing was left behind in the solve either: the tableau is still the expected one
        assert np.array_equal(bits(P.tableau()), bits(eT)), (name, what)


@pytest.mark.parametrize("name", list(SHAPES))
def test_del_rows_on_a_clone_leaves_the_parent(gpu, name):
    _inst, base = solved(gpu, name)
    parent = base.copy()
    T, head, nb, flag = state(parent)
    clone = parent.copy()
    assert clone.del_rows(delete_sets(head, parent.m)["every second"]) == 0
    gT, gh, gq, gf = state(parent)
    assert np.array_equal(bits(gT), bits(T)) and np.array_equal(gh, head) and np.array_equal(gq, nb) and np.array_equal(gf, flag)
    assert parent.status == OPT and parent.m == base.m
    # and a clone of the handle that lost rows is that handle
    again = clone.copy()
    for a, b in zip(state(again), state(clone)):
        assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b)


@pytest.mark.parametrize("name", list(SHAPES))
def test_del_rows_of_a_nonbasic_row_gives_the_tableau_up(gpu, name):
    """The call returns 0, the next solve starts from the slack basis and reaches the objective of a handle that never had the
    row, within the 1e-9 relative tolerance of the goldens."""
    inst, base = solved(gpu, name)
    m, n, seed, k = SHAPES[name]
    stat = base.row_stat()
    nonbasic = [i + 1 for i in range(base.m) if stat[i] != BS]
    assert nonbasic
    row = nonbasic[len(nonbasic) // 2]
    P = base.copy()
    assert P.del_rows([row]) == 0 and P.m == base.m - 1 and P.status == UNDEF
    with pytest.raises(RuntimeError):  # no tableau any more: the solve below builds the slack basis
        P.tableau()
    assert P.simplex() == 0 and P.status == OPT and P.it_cnt > 0
    # the same model built without the row: the instance's rows and the cut rows, as model rows from the start
    vals, rhs = cut_rows(inst, first_vertex(gpu, inst), k, seed + 100)
    A = np.vstack([inst["A"], vals[:, 1:]])
    row_b = list(inst["row_b"]) + [(LO, float(r), 0.0) for r in rhs]
    keep = [i for i in range(m + k) if i != row - 1]
    Q = gpu.create()
    Q.load_general(A[keep], [row_b[i] for i in keep], inst["col_b"], inst["c"], direction=inst["direction"])
    assert Q.simplex() == 0 and Q.status == OPT
    assert abs(P.obj - Q.obj) <= 1e-9 * max(1.0, abs(Q.obj)), (P.obj, Q.obj)


def first_vertex(gpu, inst):
    P = gs.load(gpu, inst)
    P.simplex()
    return P.col_prim()


def tighter_bounds(api, inst, P, row):
    """Bounds for the basic row `row` that its current value violates and the instance's point x0 keeps: (type, lb, ub)."""
    ind, val = P.get_mat_row(row)
    act0 = float(np.dot(val, inst["x0"][np.asarray(ind, dtype=int) - 1]))
    v = api.get_row_prim(P.h, row)
    if abs(v - act0) < 1e-6:
        return None
    lo, hi = api.get_row_lb(P.h, row), api.get_row_ub(P.h, row)
    big = 1e300
    if act0 < v:
        return (DB, lo, (v + act0) / 2) if lo > -big else (UP, 0.0, (v + act0) / 2)
    return (DB, (v + act0) / 2, hi) if hi < big else (LO, (v + act0) / 2, 0.0)


@pytest.mark.parametrize("name", list(SHAPES))
def test_pending_edit_behind_a_deleted_row_is_applied(gpu, name):
    """A bound edit of a basic row waits on the handle (no launch) when the row in front of it is deleted: the next solve
    applies it to the row's new place.  Against the edit made after the deletion, under the row's new number, and -- where the
    shape has the rows for it -- against a handle whose edit had been flushed to the device before the deletion (eight more edits
    that change nothing overflow the pending list).  Tableaux by bits."""
    inst, base = solved(gpu, name)
    head = base.basis()[0]
    pos = basic_rows(head, base.m)
    order = sorted(pos, key=lambda i: pos[i])  # basic rows by tableau row
    pick = None
    for a in range(len(order) - 1):
        for r in order[a + 1:]:
            bnds = tighter_bounds(gpu, inst, base, r)
            if bnds is not None and r != order[a]:
                pick = (order[a], r, bnds)
                break
        if pick:
            break
    assert pick, "no basic row behind another whose value can be cut off"
    d, r, (t, lb, ub) = pick
    r_new = r - (1 if d < r else 0)
    P1, P2 = base.copy(), base.copy()
    gpu.set_row_bnds(P1.h, r, t, lb, ub)  # pending
    assert P1.del_rows([d]) == 0
    assert P2.del_rows([d]) == 0
    gpu.set_row_bnds(P2.h, r_new, t, lb, ub)
    handles = [P1, P2]
    others = [i for i in order if i not in (d, r)]
    if len(others) >= 8:
        P3 = base.copy()
        gpu.set_row_bnds(P3.h, r, t, lb, ub)
        for i in others[:8]:  # the ninth edit sends the first eight to the device
            gpu.set_row_bnds(P3.h, i, gpu.get_row_type(P3.h, i), max(gpu.get_row_lb(P3.h, i), -1e300), min(gpu.get_row_ub(P3.h, i), 1e300))
        assert P3.del_rows([d]) == 0
        handles.append(P3)
    else:
        assert name == "6x5"
    it0 = base.it_cnt
    for H in handles:
        assert H.simplex() == 0 and H.status == OPT, (name, H.status)
    assert P1.it_cnt > it0  # the edit cut the vertex off: it was applied
    lo, hi = gpu.get_row_lb(P1.h, r_new), gpu.get_row_ub(P1.h, r_new)
    assert lo - 1e-7 * max(1, abs(lo)) <= gpu.get_row_prim(P1.h, r_new) <= hi + 1e-7 * max(1, abs(hi))
    for H in handles[1:]:
        assert H.it_cnt == P1.it_cnt
        for a, b in zip(state(P1), state(H)):
            assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b), name


@pytest.mark.parametrize("name,extra", [("24x48", 1), ("33x130", 40), ("70x200", 40)])
def test_appends_behind_a_deletion_equal_the_per_row_path(gpu, name, extra):
    """mvx_add_cut_rows of more rows than the deletion freed, against add_rows / set_mat_row / set_row_bnds on a clone, as
    test_gpu_cutloop.py compares them; 40 more rows than the handle was built with cross its spare rows (grow_rows)."""
    from .test_gpu_cutloop import append_per_row, assert_same_unsolved
    from .test_gpu_parity import assert_same_state

    inst, base = solved(gpu, name)
    head = base.basis()[0]
    dele = delete_sets(head, base.m)["every second"]
    X = base.copy()
    assert X.del_rows(dele) == 0
    k = len(dele) + extra
    if extra == 40:
        assert X.m + k > SHAPES[name][0] + 32  # behind the rows every slab keeps spare
    x = X.col_prim()
    vals, rhs = cut_rows(inst, x, k, 4242)
    Y = X.copy()
    m0 = X.m
    assert bnb.add_cut_rows(X, vals, rhs) == 0
    append_per_row(Y, vals, rhs)
    assert_same_unsolved(X, Y, m0, name)
    for H in (X, Y):
        assert H.simplex() == 0
    assert_same_state(X, Y, name)
    assert X.status == OPT and X.it_cnt > base.it_cnt
    # and rows leave again, out of the grown slab
    T, head, nb, flag = state(X)
    dele = delete_sets(head, X.m)["all"]
    assert X.del_rows(dele) == 0
    eT, eh, eq, ef = expected(T, head, nb, flag, m0 + k, dele)
    gT, gh, gq, gf = state(X)
    assert np.array_equal(bits(gT), bits(eT)) and np.array_equal(gh, eh) and np.array_equal(gq, eq) and np.array_equal(gf, ef)


def test_del_rows_refusals_change_nothing(gpu):
    _inst, base = solved(gpu, "24x48")
    P = base.copy()
    before = [a.tolist() for a in state(P)]
    for bad in ([2, 2], [0], [P.m + 1], []):
        assert P.del_rows(bad) == -1
        assert [a.tolist() for a in state(P)] == before and P.status == OPT and P.m == base.m


# ------------------------------------------------------------------------------------------------ the loop, trees


def aborts(gpu):
    from .test_gpu_chain import cluster_counts
    from .test_gpu_thresholds import persist_counts

    return cluster_counts(gpu)[1], persist_counts(gpu)[1]


def test_cut_loop_with_the_purge_on_the_device(gpu):
    a0 = aborts(gpu)
    purged = []

    def one(rec):
        P = lpgen.load_milp(gpu, instance(rec))
        assert bnb.integral_bounds(P) != 2
        m0 = P.m
        rc, out = bnb.cut_loop(P, rounds=5, purge=1)
        assert rc == 0 and out["cutloop_live_rows"] == out["cutloop_rows"] - out["cutloop_purged"]
        assert P.m == m0 + out["cutloop_live_rows"] and P.status == OPT, (P.m, m0, out, P.status)
        assert out["cutloop_lps"] == 1 + out["cutloop_rounds"]
        purged.append(out["cutloop_purged"])

    bad = failures([r for r in INSTANCES if r["status"] == "optimal"][::10], one)
    assert not bad, "\n".join(bad)
    assert sum(purged) >= 1, purged  # rows did leave: the purge ran
    A, b, c, U = synth.dense_ilp(24, 48, 5, 1, 0.06)
    P = synth.load_ilp(gpu, A, b, c, U)
    m0 = P.m
    rc, out = bnb.cut_loop(P, rounds=5, families=3, purge=2)
    assert rc == 0 and P.m == m0 + out["cutloop_live_rows"] and P.status == OPT and out["cutloop_purged"] >= 1, out
    assert P.obj == out["cutloop_bound"]
    assert aborts(gpu) == a0


@pytest.mark.parametrize("path", ["del_rows", "free rows"])
def test_fixture_trees_behind_the_purge_close_on_the_pins(gpu, path):
    a0 = aborts(gpu)
    table = None
    if path == "free rows":  # the device engine without the entry: a purged row becomes a free row
        table = bnb.table_from(gpu)
        assert table.del_rows and table.add_cut_rows
        table.del_rows = None
    purged = []

    def one(rec):
        inst = instance(rec)
        r = run(gpu, rec, inst, table=table, cut_rounds=5, cut_purge=1, window=64)
        check_pin(rec, inst, r)
        assert r["cutloop_live_rows"] == r["cutloop_rows"] - r["cutloop_purged"] and r["cutloop_lps"] in (0, 1 + r["cutloop_rounds"])
        purged.append(r["cutloop_purged"])

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)
    assert sum(purged) >= 1, purged  # the path under test ran
    assert aborts(gpu) == a0
