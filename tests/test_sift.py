"""CPU: sifting (DESIGN.md "Sifting (sift)") without a device.

The column pool's model layer (mvx_pool_create / add_cols / num / get_col / delete and every refusal) runs on the host alone.  The
two loops mvx_pool_price is defined by are checked through their host twins: mvx_bnb_pool_price_values bit for bit against a
restatement of the written chain order with fma emulated exactly in fractions, and against the exact value within a derived bound;
the attractive rule per type, direction and sign; mvx_bnb_pool_select on ties, limits, skips and the order of zeros and denormals."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import mvolps_amd
from mvolps_amd import bnb, capi
from mvolps_amd.capi import CV, DB, FR, FX, IV, LO, MAX, MIN, UP

from .test_addcols import draw_cols, fma, same_bits

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
ZERO_REST = [(LO, 0.0, 9.0), (UP, 5.0, 0.0), (DB, 0.0, 2.5), (FR, 1.0, -1.0), (FX, 0.0, 7.0), (DB, -0.0, 0.0)]
NON_ZERO_REST = [(LO, 1.0, 0.0), (UP, 0.0, -2.0), (DB, 1.0, 4.0), (FX, 3.0, 3.0)]


def pool_of(m, k, seed, types=None):
    rng = np.random.default_rng(seed)
    cols, obj = draw_cols(rng, k, m)
    types = types or [ZERO_REST[t % len(ZERO_REST)] for t in range(k)]
    S = mvolps_amd.create_pool(m)
    kinds = [IV if t % 2 else CV for t in range(k)]
    assert S.add_cols(cols, obj, [t for t, _, _ in types], [l for _, l, _ in types], [u for _, _, u in types], kinds) == 0
    return S, cols, obj, types, kinds


def contents(S):
    return [(c.tobytes(), np.float64(o).tobytes(), t, np.float64(l).tobytes(), np.float64(u).tobytes(), kd)
            for _, c, o, t, l, u, kd in (S.get_col(j) for j in range(1, S.n + 1))]


# ------------------------------------------------------------------------------------------------ 1. the pool's model layer


def test_pool_round_trip_by_bits_without_a_device():
    S, cols, obj, types, kinds = pool_of(7, 9, 1)
    assert (S.m, S.n) == (7, 9)
    cols[2, 3] = -0.0  # a signed zero keeps its sign
    S2 = mvolps_amd.create_pool(7)
    assert S2.add_cols(cols[:4], obj[:4], [t for t, _, _ in types[:4]], [l for _, l, _ in types[:4]], [u for _, _, u in types[:4]],
                       kinds[:4]) == 0
    assert S2.add_cols(cols[4:], obj[4:], [t for t, _, _ in types[4:]], [l for _, l, _ in types[4:]], [u for _, _, u in types[4:]],
                       kinds[4:]) == 0  # a second call extends the numbering
    assert S2.n == 9
    for j in range(1, 10):
        rc, col, o, t, l, u, kd = S2.get_col(j)
        assert rc == 0 and same_bits(col[1:], cols[j - 1, 1:]) and col[0] == 0.0
        assert same_bits([o, l, u], [obj[j - 1], types[j - 1][1], types[j - 1][2]]) and (t, kd) == (types[j - 1][0], kinds[j - 1])
    assert S2.get_col(0)[0] == -1 and S2.get_col(10)[0] == -1
    # kinds default to continuous; outputs are optional
    S3 = mvolps_amd.create_pool(7)
    assert S3.add_cols(cols[:1], obj[:1], [LO], [0.0], [0.0]) == 0 and S3.get_col(1)[6] == CV
    assert S3.api.pool_get_col(S3.h, 1, None, None, None, None, None, None) == 0
    # a pool over no rows, and no pool at all
    S0 = mvolps_amd.create_pool(0)
    assert S0.add_cols(np.zeros((2, 1)), [1.0, 2.0], [LO, FR], [0.0, 0.0], [0.0, 0.0]) == 0 and S0.n == 2
    api = mvolps_amd.api()
    assert not api.pool_create(-1)
    assert api.pool_num_cols(None) == 0 and api.pool_num_rows(None) == 0
    api.pool_delete(None)
    if api.device_count() == 0:  # nothing above may have needed one
        assert S2.n == 9


@pytest.mark.parametrize("bad", NON_ZERO_REST, ids=["LO-lb1", "UP-ub-2", "DB-lb1", "FX-3"])
def test_a_column_that_cannot_rest_at_zero_is_refused(bad):
    S, cols, obj, types, kinds = pool_of(5, 4, 2)
    before = contents(S)
    rng = np.random.default_rng(3)
    c2, o2 = draw_cols(rng, 3, 5)
    ty = [(LO, 0.0, 0.0), bad, (FR, 0.0, 0.0)]  # the good columns around it do not enter either
    assert S.add_cols(c2, o2, [t for t, _, _ in ty], [l for _, l, _ in ty], [u for _, _, u in ty]) == -1
    assert S.n == 4 and contents(S) == before


def test_every_zero_rest_type_is_admitted():
    S = mvolps_amd.create_pool(3)
    for t, l, u in ZERO_REST:
        assert S.add_cols(np.ones((1, 3)), [1.0], [t], [l], [u]) == 0
    assert S.n == len(ZERO_REST)


def test_the_refusals_of_add_dense_cols_change_nothing():
    S, cols, obj, types, kinds = pool_of(5, 4, 4)
    before = contents(S)
    api = S.api
    rng = np.random.default_rng(5)
    c2, o2 = draw_cols(rng, 2, 5)
    good = dict(cols=c2, obj=o2, type=np.array([LO, FR], dtype=np.int32), lb=np.zeros(2), ub=np.zeros(2), kind=np.array([CV, IV], dtype=np.int32))

    def call(k=2, **over):
        a = dict(good)
        a.update(over)
        keep = [None if a[key] is None else np.ascontiguousarray(a[key], dtype=dt)
                for key, dt in (("cols", np.float64), ("obj", np.float64), ("type", np.int32), ("lb", np.float64), ("ub", np.float64), ("kind", np.int32))]
        ptr = lambda v, T: None if v is None else v.ctypes.data_as(T)
        return api.pool_add_cols(S.h, k, ptr(keep[0], DP), ptr(keep[1], DP), ptr(keep[2], IP), ptr(keep[3], DP), ptr(keep[4], DP), ptr(keep[5], IP))

    nan_col = c2.copy()
    nan_col[1, 5] = math.nan
    nan_col0 = c2.copy()
    nan_col0[1, 0] = math.nan  # entry 0 is not read
    assert call(k=0) == -1 and call(k=-3) == -1
    for key in ("cols", "obj", "type", "lb", "ub"):
        assert call(**{key: None}) == -1
    assert call(type=[LO, 0]) == -1 and call(type=[6, LO]) == -1
    assert call(obj=[1.0, math.nan]) == -1 and call(lb=[math.nan, 0.0]) == -1 and call(ub=[0.0, math.nan]) == -1
    assert call(type=[DB, LO], lb=[0.0, 0.0], ub=[-1.0, 0.0]) == -1  # lb > ub on a DB column
    assert call(kind=[CV, 3]) == -1
    assert call(cols=nan_col) == -1
    assert api.pool_add_cols(None, 2, None, None, None, None, None, None) == -1
    assert S.n == 4 and contents(S) == before
    assert call(cols=nan_col0) == 0 and call(kind=None) == 0 and S.n == 8
    assert contents(S)[:4] == before


# ------------------------------------------------------------------------------------------------ 2. the pricing twin


def py_price(cols, obj, y):
    """The definition, restated: 64 chains over the rows, the tree, obj last; fma exact."""
    N, m = len(obj), len(y) - 1
    out = [0.0]
    for t in range(N):
        s = [0.0] * 64
        for l in range(64):
            acc = 0.0
            for i in range(l + 1, m + 1, 64):
                if y[i] != 0.0:
                    acc = fma(-float(cols[t, i]), float(y[i]), acc)
            s[l] = acc
        h = 32
        while h >= 1:
            for l in range(h):
                s[l] = s[l] + s[l + h]
            h //= 2
        out.append(float(obj[t]) + s[0])
    return np.array(out)


def draw_y(rng, m):
    y = rng.normal(size=m + 1) * 2
    y[rng.random(m + 1) < 0.3] = 0.0
    y[rng.random(m + 1) < 0.1] = -0.0
    y[0] = math.nan  # not read
    return y


@pytest.mark.parametrize("m", [1, 63, 64, 65, 130])
def test_price_values_equal_the_written_order_and_the_exact_value(m):
    rng = np.random.default_rng(100 + m)
    N = 7
    cols = rng.normal(size=(N, m + 1)) * 3  # full mantissas: the order of the additions shows in the bits
    cols[rng.random((N, m + 1)) < 0.2] = 0.0
    cols[:, 0] = math.nan  # not read
    obj = rng.normal(size=N) * 5
    y = draw_y(rng, m)
    if m >= 63:
        assert np.any(y[1:] == 0.0) and np.any(np.signbit(y[1:]) & (y[1:] == 0.0))
    types = [[LO, UP, DB, FR, FX][t % 5] for t in range(N)]
    rc, dj, att = bnb.pool_price_values(cols, obj, types, y, MAX, 1e-9)
    assert rc == 0 and dj[0] == 0.0 and att[0] == 0
    assert same_bits(dj, py_price(cols, obj, y))
    for t in range(N):
        exact = Fraction(float(obj[t])) - sum(Fraction(float(cols[t, i])) * Fraction(float(y[i])) for i in range(1, m + 1))
        mag = abs(float(obj[t])) + sum(abs(float(cols[t, i]) * float(y[i])) for i in range(1, m + 1))
        # chain length + six tree levels + the last add, one to spare
        bound = (math.ceil(m / 64) + 8) * 2.0 ** -53 * mag
        assert abs(Fraction(float(dj[t + 1])) - exact) <= Fraction(bound), (t, float(dj[t + 1]), float(exact))


def test_price_values_refusals():
    f = bnb.lib().mvx_bnb_pool_price_values
    UPT = C.POINTER(C.c_ubyte)
    cols, obj, ty, y, dj = np.zeros((1, 3)), np.zeros(1), np.array([LO], dtype=np.int32), np.zeros(3), np.zeros(2)
    a = lambda v, T=DP: v.ctypes.data_as(T)
    assert f(2, 1, a(cols), a(obj), a(ty, IP), a(y), MAX, 1e-9, a(dj), None) == 0
    assert f(2, 1, a(cols), a(obj), a(ty, IP), a(y), MAX, 1e-9, None, None) == -1
    assert f(2, 1, None, a(obj), a(ty, IP), a(y), MAX, 1e-9, a(dj), None) == -1
    assert f(2, 1, a(cols), a(obj), a(ty, IP), None, MAX, 1e-9, a(dj), None) == -1
    assert f(2, 1, a(cols), a(obj), a(ty, IP), a(y), 0, 1e-9, a(dj), None) == -1
    assert f(-1, 1, a(cols), a(obj), a(ty, IP), a(y), MAX, 1e-9, a(dj), None) == -1
    g = bnb.lib().mvx_bnb_pool_select
    att, pick, n = np.zeros(2, dtype=np.uint8), np.zeros(1, dtype=np.int32), C.c_int(0)
    assert g(1, a(dj), a(att, UPT), None, 1, a(pick, IP), C.byref(n)) == 0
    assert g(1, a(dj), a(att, UPT), None, -1, a(pick, IP), C.byref(n)) == -1
    assert g(1, None, a(att, UPT), None, 1, a(pick, IP), C.byref(n)) == -1
    assert g(1, a(dj), a(att, UPT), None, 1, None, C.byref(n)) == -1
    assert g(1, a(dj), a(att, UPT), None, 0, None, C.byref(n)) == 0  # K = 0 needs no pick


TOL = 1e-9
# (type, direction) -> for d in (2 tol, tol, 0.5 tol, 0, -0.5 tol, -tol, -2 tol): attractive?
RULE = {
    (LO, MAX): [1, 0, 0, 0, 0, 0, 0], (LO, MIN): [0, 0, 0, 0, 0, 0, 1], (DB, MAX): [1, 0, 0, 0, 0, 0, 0], (DB, MIN): [0, 0, 0, 0, 0, 0, 1],
    (UP, MAX): [0, 0, 0, 0, 0, 0, 1], (UP, MIN): [1, 0, 0, 0, 0, 0, 0], (FR, MAX): [1, 0, 0, 0, 0, 0, 1], (FR, MIN): [1, 0, 0, 0, 0, 0, 1],
    (FX, MAX): [0] * 7, (FX, MIN): [0] * 7,
}


@pytest.mark.parametrize("ty,direction", sorted(RULE))
def test_the_attractive_rule(ty, direction):
    ds = [2 * TOL, TOL, 0.5 * TOL, 0.0, -0.5 * TOL, -TOL, -2 * TOL]  # |d| == tol exactly is not attractive
    # m = 1, y = 1, a = 0: d = obj exactly
    rc, dj, att = bnb.pool_price_values(np.zeros((len(ds), 2)), ds, [ty] * len(ds), [0.0, 1.0], direction, TOL)
    assert rc == 0 and same_bits(dj[1:], ds)
    assert list(att[1:]) == RULE[(ty, direction)]


# ------------------------------------------------------------------------------------------------ 3. the selection twin


def test_select_orders_by_magnitude_and_breaks_ties_by_column():
    #            1     2     3    4     5     6    7     8
    dj = [0.0, 3.0, -5.0, 3.0, 1.0, -3.0, 5.0, 0.5, -5.0]
    att = [0, 1, 1, 1, 1, 1, 1, 0, 1]
    order = [2, 6, 8, 1, 3, 5, 4]  # |5| at 2, 6, 8; |3| at 1, 3, 5; then 4; column 7 is not attractive
    for K in range(0, 10):
        rc, pick = bnb.pool_select(dj, att, K)
        assert rc == 0 and list(pick) == order[:K]
    rc, pick = bnb.pool_select(dj, att, 100)  # K larger than the attractive count
    assert list(pick) == order
    skip = [1, 0, 1, 0, 0, 0, 1, 0, 0]  # skip[0] is not read
    rc, pick = bnb.pool_select(dj, att, 4, skip)
    assert list(pick) == [8, 1, 3, 5]
    rc, pick = bnb.pool_select(dj, [0] * 9, 5)  # all unattractive
    assert rc == 0 and len(pick) == 0
    rc, pick = bnb.pool_select(dj, att, 5, [1] * 9)  # all skipped
    assert rc == 0 and len(pick) == 0
    rc, pick = bnb.pool_select([0.0], [0], 3)  # an empty pool
    assert rc == 0 and len(pick) == 0


def test_select_orders_zeros_and_denormals_by_their_bits():
    tiny = 5e-324
    #          1     2      3         4      5     6
    dj = [0.0, 0.0, -0.0, 3 * tiny, -tiny, 1e-300, -0.0]
    att = [0, 1, 1, 1, 1, 1, 1]
    rc, pick = bnb.pool_select(dj, att, 6)
    assert list(pick) == [5, 3, 4, 1, 2, 6]  # +0.0 and -0.0 tie: the lower column first
