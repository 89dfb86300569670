"""CPU: column append (DESIGN.md "Column append (add_cols)") without a device.

The model layer of mvx_add_dense_cols / mvx_set_mat_col / mvx_get_mat_col runs on handles that have no tableau, so it is checked
here against a second handle built with add_cols + set_mat_col + set_col_bnds + set_obj_coef + set_col_kind.  The arithmetic of
the device pass is checked through its host twin mvx_bnb_price_cols over the ORACLE's table: bit for bit against a restatement
of the written definition (64 chains, the tree, the base added last; fma emulated exactly in fractions), and against the
independent reference of tests/certify.py, which recomputes the extended tableau from the extended model and the basis with the
new variables appended to nb."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import mvolps_amd
from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import CV, DB, FR, FX, IV, LO, MAX, MIN, NF, NL, NS, NU, OPT, UP

from . import certify as cf
from . import general_at_size as gs

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
STD_FLAG = {FR: NF, LO: NL, UP: NU, DB: NL, FX: NS}


def fma(a, b, c):
    """round(a * b + c), one rounding (finite operands; the chains never hold -0.0, so the sign of a zero is +)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def resting(t, lb, ub):
    return {NL: lb, NU: ub, NS: lb, NF: 0.0}[STD_FLAG[t]]


def np_price(T, head, nb, cols, obj):
    """The definition, restated: img[t][p] = base + S with S in 64 chains and the tree."""
    m, n = T.shape[0] - 1, T.shape[1] - 1
    k = len(obj)
    img = np.zeros((k, m + 1))
    for t in range(k):
        w = [0.0] * (n + 1)
        for q in range(1, n + 1):
            if nb[q] <= m:
                w[q] = -float(cols[t, nb[q]])
        for p in range(m + 1):
            s = [0.0] * 64
            for l in range(64):
                acc = 0.0
                for q in range(l + 1, n + 1, 64):
                    if w[q] != 0.0:
                        acc = fma(w[q], float(T[p, q]), acc)
                s[l] = acc
            h = 32
            while h >= 1:
                for l in range(h):
                    s[l] = s[l] + s[l + h]
                h //= 2
            if p == 0:
                base = float(obj[t])
            else:
                base = float(cols[t, head[p]]) if head[p] <= m else 0.0
            img[t, p] = base + s[0]
    return img


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    assert t.get_tableau and t.get_basis
    return t


def draw_cols(rng, k, m, zeros=0.3):
    cols = np.round(rng.normal(size=(k, m + 1)) * 3)
    cols[rng.random((k, m + 1)) < zeros] = 0.0
    cols[:, 0] = 0.0
    return cols, np.round(rng.normal(size=k) * 5)


# ------------------------------------------------------------------------------------------------ 1. the model layer


def general_handle(api, seed=5, m=6, n=9):
    inst = gs.general_lp(m, n, seed)
    kinds = [IV if j % 3 == 0 else CV for j in range(n)]
    P = api.create()
    P.load_general(inst["A"], inst["row_b"], inst["col_b"], inst["c"], kinds=kinds, direction=inst["direction"])
    return P, inst


NEW_COLS = [(LO, 0.0, 0.0, CV), (DB, -1.5, 2.0, IV), (UP, 0.0, 3.0, CV), (FR, 0.0, 0.0, CV), (FX, 2.0, 7.0, IV), (DB, 0.0, 1.0, IV)]


def columns_of(P):
    api = P.api
    out = []
    for j in range(1, P.n + 1):
        ind, val = P.get_mat_col(j)
        out.append((list(ind), list(val), api.get_col_type(P.h, j), api.get_col_lb(P.h, j), api.get_col_ub(P.h, j), api.get_col_kind(P.h, j),
                    api.get_obj_coef(P.h, j)))
    return out


def rows_of(P):
    return [tuple(map(list, P.get_mat_row(i))) for i in range(1, P.m + 1)]


def test_model_edit_equals_add_cols_and_setters():
    api = mvolps_amd.api()
    P, inst = general_handle(api)
    Q, _ = general_handle(api)
    m, n = P.m, P.n
    api.set_col_name(P.h, 2, b"second")
    clone = P.copy()
    rows_before = rows_of(P)
    rng = np.random.default_rng(11)
    k = len(NEW_COLS)
    cols, obj = draw_cols(rng, k, m)
    types = [t for t, _, _, _ in NEW_COLS]
    lb = [l for _, l, _, _ in NEW_COLS]
    ub = [u for _, _, u, _ in NEW_COLS]
    kinds = [kd for _, _, _, kd in NEW_COLS]
    assert P.add_dense_cols(cols, obj, types, lb, ub, kinds) == 0
    first = api.add_cols(Q.h, k)
    assert first == n + 1
    for t in range(k):
        nz = np.nonzero(cols[t])[0]
        Q.set_mat_col(n + 1 + t, np.concatenate([[0], nz]), np.concatenate([[0.0], cols[t, nz]]))
        api.set_col_bnds(Q.h, n + 1 + t, types[t], lb[t], ub[t])
        api.set_obj_coef(Q.h, n + 1 + t, float(obj[t]))
        api.set_col_kind(Q.h, n + 1 + t, kinds[t])
    assert (P.m, P.n) == (Q.m, Q.n) == (m, n + k)
    assert rows_of(P) == rows_of(Q)
    assert columns_of(P) == columns_of(Q)
    assert api.get_num_int(P.h) == api.get_num_int(Q.h) == 3 + 3
    assert api.get_col_kind(P.h, n + k) == capi.BV  # integer with bounds [0, 1]
    assert api.get_status(P.h) == capi.UNDEF and api.get_obj_dir(P.h) == inst["direction"]
    for t in range(k):  # what went in comes out, and the old part of every row is what it was
        ind, val = P.get_mat_col(n + 1 + t)
        nz = np.nonzero(cols[t])[0]
        assert list(ind) == list(nz) and list(val) == list(cols[t, nz])
    for i in range(m):
        ind, val = P.get_mat_row(i + 1)
        old = [(a, b) for a, b in zip(ind, val) if a <= n]
        assert old == list(zip(*rows_before[i]))
    # the clone taken before the append keeps its rows and its n; names of old columns survive, new ones have none
    assert clone.n == n and rows_of(clone) == rows_before
    assert api.get_col_name(P.h, 2) == b"second" and api.get_col_name(P.h, n + 1) is None
    assert api.get_col_name(clone.h, 2) == b"second"
    # kinds omitted: all continuous
    R, _ = general_handle(api)
    assert R.add_dense_cols(cols[:2], obj[:2], types[:2], lb[:2], ub[:2]) == 0
    assert [api.get_col_kind(R.h, n + 1 + t) for t in range(2)] == [CV, CV]


def test_set_mat_col_rewrites_a_column_and_leaves_clones_alone():
    api = mvolps_amd.api()
    P, inst = general_handle(api, seed=8)
    A = np.array(inst["A"])
    m = P.m
    clone = P.copy()
    ind, val = P.get_mat_col(3)
    assert list(ind) == [i + 1 for i in np.nonzero(A[:, 2])[0]] and list(val) == list(A[np.nonzero(A[:, 2])[0], 2])
    P.set_mat_col(3, [0, m, 1], [0.0, 4.5, -2.0])  # any order of rows
    ind, val = P.get_mat_col(3)
    assert list(ind) == [1, m] and list(val) == [-2.0, 4.5]
    B = A.copy()
    B[:, 2] = 0.0
    B[0, 2], B[m - 1, 2] = -2.0, 4.5
    for i in range(m):
        ind, val = P.get_mat_row(i + 1)
        assert list(ind) == [j + 1 for j in np.nonzero(B[i])[0]] and list(val) == list(B[i, np.nonzero(B[i])[0]])
    ind, val = clone.get_mat_col(3)
    assert list(val) == list(A[np.nonzero(A[:, 2])[0], 2])
    P.set_mat_col(3, [0], [0.0])
    assert list(P.get_mat_col(3)[0]) == []


def test_every_refusal_leaves_the_model_alone():
    api = mvolps_amd.api()
    P, _ = general_handle(api, seed=9)
    m, n = P.m, P.n
    before = rows_of(P), columns_of(P)
    cols, obj = draw_cols(np.random.default_rng(2), 2, m)
    good = dict(cols=cols, obj=obj, type=np.array([LO, DB], dtype=np.int32), lb=np.array([0.0, 1.0]), ub=np.array([0.0, 2.0]),
                kind=np.array([CV, IV], dtype=np.int32))

    def call(k=2, **over):
        a = dict(good)
        a.update(over)
        ptr = lambda v, T: None if v is None else np.ascontiguousarray(v).ctypes.data_as(T)  # noqa: E731
        keep = [None if a[x] is None else np.ascontiguousarray(a[x]) for x in ("cols", "obj", "type", "lb", "ub", "kind")]
        return api.add_dense_cols(P.h, k, ptr(keep[0], DP), ptr(keep[1], DP), ptr(keep[2], IP), ptr(keep[3], DP), ptr(keep[4], DP),
                                  ptr(keep[5], IP))

    nan_cols = cols.copy()
    nan_cols[1, m] = math.nan
    refusals = [
        dict(cols=None), dict(obj=None), dict(type=None), dict(lb=None), dict(ub=None), dict(k=0), dict(k=-3),
        dict(cols=nan_cols), dict(obj=np.array([1.0, math.nan])), dict(lb=np.array([math.nan, 1.0])), dict(ub=np.array([0.0, math.nan])),
        dict(type=np.array([LO, 0], dtype=np.int32)), dict(type=np.array([6, DB], dtype=np.int32)),
        dict(lb=np.array([0.0, 3.0])),  # lb > ub on the DB column
        dict(kind=np.array([CV, capi.BV], dtype=np.int32)), dict(kind=np.array([0, IV], dtype=np.int32)),
    ]
    for over in refusals:
        assert call(**over) == -1, over
        assert (P.m, P.n) == (m, n) and (rows_of(P), columns_of(P)) == before, over
    nan_unread = cols.copy()
    nan_unread[:, 0] = math.nan  # entry 0 of a column is not read
    assert call(cols=nan_unread, kind=None) == 0 and P.n == n + 2
    assert api.price_cols(P.h, 1, None, None, None, None) == -1
    dj = np.zeros(2)
    assert api.price_cols(P.h, 2, good["cols"].ctypes.data_as(DP), good["obj"].ctypes.data_as(DP), dj.ctypes.data_as(DP), None) == -3  # no tableau


# ------------------------------------------------------------------------------------------------ 2. twin = restatement


def solved(P):
    P.simplex()
    return P


def with_cut_row(P, rng):
    """One more LO row that the current vertex violates, then a re-solve: a handle that carries an appended row."""
    n = P.n
    x = P.col_prim()
    coef = np.round(rng.normal(size=n) * 2)
    coef[0] = coef[0] or 1.0
    r = P.api.add_rows(P.h, 1)
    P.set_mat_row(r, np.arange(n + 1), np.concatenate([[0.0], coef]))
    P.api.set_row_bnds(P.h, r, UP, 0.0, float(coef @ x) - 0.25)
    P.simplex()
    return coef, float(coef @ x) - 0.25


def twin_handles(orc):
    """(name, handle, certify model or None): solved oracle handles of the existing generators, MIN and MAX."""
    out = []
    for m, n, seed in ((5, 7, 3), (24, 96, 5), (12, 130, 9)):
        A, b, c = synth.dense_lp(m, n, seed)
        P = orc.create()
        P.load_dense(A, b, c)
        out.append(("dense_lp %dx%d" % (m, n), solved(P), cf.Model.dense(A, b, c)))
    dirs = set()
    for m, n, seed in ((6, 9, 1), (6, 9, 2), (9, 70, 3), (9, 70, 4), (14, 20, 6), (14, 20, 7)):
        inst = gs.general_lp(m, n, seed)
        P = solved(gs.load(orc, inst))
        dirs.add(inst["direction"])
        out.append(("general %dx%d seed %d dir %d status %d" % (m, n, seed, inst["direction"], P.status), P, gs.model(inst)))
    assert dirs == {MIN, MAX}
    # a handle that carries an appended row
    A, b, c = synth.dense_lp(10, 40, 4)
    P = orc.create()
    P.load_dense(A, b, c)
    P.simplex()
    M = cf.Model.dense(A, b, c)
    coef, rhs = with_cut_row(P, np.random.default_rng(3))
    M.add_row(coef, UP, 0.0, rhs)
    assert P.status == OPT and P.m == 11
    out.append(("dense_lp 10x40 + row", P, M))
    # a basis without a non-basic auxiliary: no column is worth entering, the slack basis is optimal
    A, b, c = synth.dense_lp(7, 66, 2)
    P = orc.create()
    P.load_dense(A, b, -np.abs(c) - 1.0)
    P.simplex()
    assert P.status == OPT and P.it_cnt == 0
    out.append(("slack basis 7x66", P, cf.Model.dense(A, b, -np.abs(c) - 1.0)))
    return out


@pytest.fixture(scope="module")
def handles(orc):
    return twin_handles(orc)


def test_twin_equals_the_restatement(handles, tab):
    rng = np.random.default_rng(17)
    seen_aux = {True: 0, False: 0}
    for name, P, _ in handles:
        m = P.m
        T = P.tableau()
        head, nb, _flag = P.basis()
        k = 5
        cols, obj = draw_cols(rng, k, m)
        cols[:, 0] = 99.0  # entry 0 is not read
        rc, dj, img = bnb.price_cols(P, cols, obj, table=tab)
        assert rc == 0, name
        want = np_price(T, head, nb, cols, obj)
        assert same_bits(img, want), (name, np.argwhere(img != want)[:4])
        assert same_bits(dj, want[:, 0]), name
        has_aux = bool((nb[1:] <= m).any())
        seen_aux[has_aux] += 1
        if not has_aux:  # S is +0.0 exactly: the image is the base
            base = np.zeros((k, m + 1))
            base[:, 0] = obj
            for p in range(1, m + 1):
                base[:, p] = cols[:, head[p]] if head[p] <= m else 0.0
            assert same_bits(img, base + 0.0), name
    assert seen_aux[True] >= 5 and seen_aux[False] >= 1


def test_twin_without_images_gives_the_same_reduced_costs(handles, tab):
    name, P, _ = handles[1]
    cols, obj = draw_cols(np.random.default_rng(23), 3, P.m)
    rc, dj, _img = bnb.price_cols(P, cols, obj, table=tab)
    dj2 = np.zeros(3)
    tptr = C.cast(C.pointer(tab), C.c_void_p)
    rc2 = bnb.lib().mvx_bnb_price_cols(tptr, P.h, 3, cols.ctypes.data_as(DP), obj.ctypes.data_as(DP), dj2.ctypes.data_as(DP), None)
    assert rc == 0 and rc2 == 0 and same_bits(dj, dj2)


# ------------------------------------------------------------------------------------------------ 3. twin against the reference

COL_TYPES = [(LO, 0.0, 0.0), (DB, -2.0, 3.0), (UP, 0.0, 1.5), (FR, 0.0, 0.0), (FX, 2.0, 2.0)]


def extended(M, P, tab, cols, obj, types):
    """The extended model, basis and tableau: the old tableau, the twin's images, column 0 shifted by the resting values."""
    m, n, k = P.m, P.n, len(obj)
    T = P.tableau()
    head, nb, flag = P.basis()
    rc, _dj, img = bnb.price_cols(P, cols, obj, table=tab)
    assert rc == 0
    Tx = np.hstack([T, img.T])
    Mx = M.copy()
    for t, (ty, l, u) in enumerate(types):
        Mx.add_col(cols[t, 1:], ty, l, u, cost=obj[t])
        x = resting(ty, l, u)
        if x != 0.0:
            for p in range(m + 1):
                Tx[p, 0] = fma(Tx[p, n + 1 + t], x, Tx[p, 0])
    nbx = np.concatenate([nb, m + n + 1 + np.arange(k)]).astype(np.int32)
    flagx = np.concatenate([flag, [STD_FLAG[ty] for ty, _, _ in types]]).astype(np.int32)
    return Mx, (head, nbx, flagx), Tx


def test_twin_images_are_the_columns_of_the_extended_tableau(handles, tab):
    rng = np.random.default_rng(29)
    worst = 0.0
    for name, P, M in handles:
        cols, obj = draw_cols(rng, len(COL_TYPES), P.m)
        obj[0] = 3.0
        Mx, basis, Tx = extended(M, P, tab, cols, obj, COL_TYPES)
        ref = cf.Ref(Mx, basis, exact=P.m <= 12)
        worst = max(worst, cf.certify_tableau(ref, Tx, name))
        # the reference notices the other sign of the cost in row 0, under MIN and under MAX
        bad = Tx.copy()
        bad[0, P.n + 1] -= 2.0 * obj[0]
        with pytest.raises(cf.CertError):
            cf.certify_tableau(ref, bad, name)
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 4. refusals of the twin


def test_twin_refuses_a_table_without_tableau_or_basis(orc, handles):
    name, P, _ = handles[0]
    cols, obj = draw_cols(np.random.default_rng(1), 2, P.m)
    for gone in ("get_basis", "get_tableau"):
        t = bnb.table_from(orc)
        setattr(t, gone, None)
        rc, _dj, _img = bnb.price_cols(P, cols, obj, table=t)
        assert rc == -2, gone
    t = bnb.table_from(orc)
    dj = np.zeros(2)
    tptr = C.cast(C.pointer(t), C.c_void_p)
    f = bnb.lib().mvx_bnb_price_cols
    assert f(tptr, P.h, 0, cols.ctypes.data_as(DP), obj.ctypes.data_as(DP), dj.ctypes.data_as(DP), None) == -1
    assert f(tptr, P.h, 2, None, obj.ctypes.data_as(DP), dj.ctypes.data_as(DP), None) == -1
    assert f(tptr, None, 2, cols.ctypes.data_as(DP), obj.ctypes.data_as(DP), dj.ctypes.data_as(DP), None) == -1
