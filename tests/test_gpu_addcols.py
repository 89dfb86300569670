"""GPU: column append on a live tableau (mvx_add_dense_cols, mvx_price_cols, k_addcols; DESIGN.md "Column append (add_cols)").

mvx_price_cols is held bit for bit to its host twin over the engine's own table at the shape boundaries of the kernel (one
position, 63 / 64 / 65 positions around a wave, 127 / 129 around two; 1, CT, CT+1, 2 CT+3 columns around the tile).  The append is
checked against the images priced just before, the shift rule of column 0, the untouched old entries, the extended basis, and the
independent reference of tests/certify.py before any solve -- in place and across one or two multiples of the row stride, on
plain handles, handles that carry cut rows and handles after a row deletion.  Then the solves that follow: unattractive columns
cost no pivot, attractive ones lead to the optimum the oracle finds cold, pending bound edits and clones survive, and a column
generation loop ends in the optimum of the full model."""
import ctypes as C
import math

import numpy as np
import pytest

from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import CV, DB, FR, FX, LO, MAX, NL, OPT, UNDEF, UP

from . import certify as cf
from . import general_at_size as gs
from .test_addcols import COL_TYPES, STD_FLAG, draw_cols, fma, resting, same_bits

pytestmark = pytest.mark.gpu

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


def dense(api, m, n, seed, c_sign=1.0):
    A, b, c = synth.dense_lp(m, n, seed)
    c = c if c_sign > 0 else -np.abs(c) - 1.0
    P = api.create()
    P.load_dense(A, b, c)
    assert P.simplex() == 0 and P.status == OPT
    return P, cf.Model.dense(A, b, c)


def ld_of(n):
    return (n + 1 + 31) // 32 * 32


# ------------------------------------------------------------------------------------------------ 1. pricing = twin


@pytest.mark.parametrize("m,n", [(1, 1), (5, 63), (7, 64), (9, 65), (40, 127), (33, 129)])
def test_price_cols_equals_the_twin_at_the_shape_boundaries(gpu, m, n):
    P, _ = dense(gpu, m, n, 3 + m)
    CT = gpu.price_cols_tile()
    assert CT in (4, 8)
    head, nb, _ = P.basis()
    assert (nb[1:] <= m).any()  # some auxiliary is non-basic: S is not empty
    rng = np.random.default_rng(100 * m + n)
    T = P.tableau()
    for k in (1, CT, CT + 1, 2 * CT + 3):
        cols, obj = draw_cols(rng, k, m)
        rc, dj, img = P.price_cols(cols, obj, images=True)
        rc2, tdj, timg = bnb.price_cols(P, cols, obj, table=None)
        assert rc == 0 and rc2 == 0
        assert same_bits(img, timg), (k, np.argwhere(img != timg)[:4])
        assert same_bits(dj, tdj) and same_bits(dj, img[:, 0])
        rc3, dj_only = P.price_cols(cols, obj)  # img == NULL: only row 0 is read
        assert rc3 == 0 and same_bits(dj_only, dj)
    assert np.array_equal(P.tableau(), T) and P.status == OPT  # pure


def test_price_cols_on_general_bases_and_without_a_nonbasic_auxiliary(gpu):
    for seed in (3, 4):
        inst = gs.general_lp(9, 70, seed)
        P = gs.load(gpu, inst)
        P.simplex()
        cols, obj = draw_cols(np.random.default_rng(seed), 6, P.m)
        rc, dj, img = P.price_cols(cols, obj, images=True)
        rc2, tdj, timg = bnb.price_cols(P, cols, obj, table=None)
        assert rc == 0 and rc2 == 0 and same_bits(img, timg) and same_bits(dj, tdj)
    P, _ = dense(gpu, 7, 66, 2, c_sign=-1.0)  # the slack basis is optimal: every auxiliary is basic
    head, nb, _ = P.basis()
    m = P.m
    assert P.it_cnt == 0 and not (nb[1:] <= m).any()
    cols, obj = draw_cols(np.random.default_rng(5), 6, m)
    rc, dj, img = P.price_cols(cols, obj, images=True)
    base = np.zeros((6, m + 1))
    base[:, 0] = obj
    for p in range(1, m + 1):
        base[:, p] = cols[:, head[p]]
    assert rc == 0 and same_bits(img, base + 0.0)  # S is +0.0 exactly
    rc2, tdj, timg = bnb.price_cols(P, cols, obj, table=None)
    assert rc2 == 0 and same_bits(img, timg)


# ------------------------------------------------------------------------------------------------ 2. the append


def with_cut_rows(P, M, violated):
    """Two rows through mvx_add_cut_rows; violated: the vertex breaks them and the handle is solved again."""
    n = P.n
    rng = np.random.default_rng(7)
    x = P.col_prim()
    vals = np.zeros((2, n + 1))
    vals[:, 1:] = -np.abs(np.round(rng.normal(size=(2, n)) * 2)) - 1.0
    rhs = vals[:, 1:] @ x + (0.25 if violated else -5.0)
    assert bnb.add_cut_rows(P, vals, rhs) == 0
    for t in range(2):
        M.add_row(vals[t, 1:], LO, float(rhs[t]), 0.0)
    assert P.simplex() == 0 and P.status == OPT


def check_append(P, M, k, rng, types=None):
    """Appends k columns to the solved handle P (model M) and checks everything the definition says; returns the extended model."""
    m, n = P.m, P.n
    types = types or [COL_TYPES[t % len(COL_TYPES)] for t in range(k)]
    cols, obj = draw_cols(rng, k, m)
    T0 = P.tableau()
    head0, nb0, flag0 = P.basis()
    rc, dj, img = P.price_cols(cols, obj, images=True)
    assert rc == 0
    assert P.add_dense_cols(cols, obj, [t for t, _, _ in types], [l for _, l, _ in types], [u for _, _, u in types]) == 0
    assert (P.m, P.n) == (m, n + k) and P.status == UNDEF
    assert P.api.get_tableau_ld(P.h) == ld_of(n + k)
    T1 = P.tableau()
    head1, nb1, flag1 = P.basis()
    assert same_bits(T1[:, 1 : n + 1], T0[:, 1 : n + 1])  # old body entries, bit for bit
    assert same_bits(T1[:, n + 1 :], img.T)  # the images priced just before
    col0 = T0[:, 0].copy()
    Mx = M.copy()
    for t, (ty, l, u) in enumerate(types):
        Mx.add_col(cols[t, 1:], ty, l, u, cost=obj[t])
        x = resting(ty, l, u)
        if x != 0.0:
            for p in range(m + 1):
                col0[p] = fma(float(img[t, p]), x, float(col0[p]))
    assert same_bits(T1[:, 0], col0)  # the shift rule
    assert np.array_equal(head1, head0)
    assert np.array_equal(nb1, np.concatenate([nb0, m + n + 1 + np.arange(k)]))
    assert np.array_equal(flag1, np.concatenate([flag0, [STD_FLAG[ty] for ty, _, _ in types]]))
    ref = cf.Ref(Mx, (head1, nb1, flag1))
    assert cf.certify_tableau(ref, T1, "append n=%d k=%d" % (n, k)) <= 1.0
    for t, (ty, l, u) in enumerate(types):
        lo, hi = cf._bounds(ty, l, u)
        assert P.api.get_col_lb(P.h, n + 1 + t) == (lo if lo > -math.inf else -np.finfo(float).max)
        assert P.api.get_col_ub(P.h, n + 1 + t) == (hi if hi < math.inf else np.finfo(float).max)
        assert P.api.get_col_prim(P.h, n + 1 + t) == resting(ty, l, u)
    return Mx


@pytest.mark.parametrize("variant", ["plain", "cut rows", "after del_rows"])
@pytest.mark.parametrize("n,k", [(30, 1), (31, 1), (62, 2), (20, 50)])
def test_append_in_place_and_with_relayout(gpu, n, k, variant):
    P, M = dense(gpu, 12, n, 5 + n)
    if variant == "cut rows":
        with_cut_rows(P, M, violated=True)
    elif variant == "after del_rows":
        with_cut_rows(P, M, violated=False)
        assert P.row_stat()[12] == capi.BS and P.del_rows([13]) == 0 and P.m == 13
        M.A = np.delete(M.A, 12, axis=0)
        del M.rows[12]
    assert (ld_of(n + k) == ld_of(n)) == ((n, k) == (30, 1))
    Mx = check_append(P, M, k, np.random.default_rng(n + k))
    P.simplex()  # whatever the new columns make of the LP, the state certifies against the extended model
    cf.certify(Mx, P, what="%s n=%d k=%d" % (variant, n, k))
    # and again on the handle that has moved once: an in-place append behind a relayout
    if ld_of(n + k + 1) == ld_of(n + k):
        assert P.status in (OPT, capi.UNBND, capi.NOFEAS)
        Mx2 = check_append(P, Mx, 1, np.random.default_rng(1), types=[(LO, 0.0, 0.0)])
        P.simplex()
        cf.certify(Mx2, P, what="second append")


# ------------------------------------------------------------------------------------------------ 3. the solve that follows


def priced_out(P, cols, types, margin, attractive):
    """obj[t] from the twin's reduced cost at obj = 0, `margin` on the attractive or the unattractive side of the column's
    status under the handle's direction."""
    sgn = 1.0 if P.api.get_obj_dir(P.h) == MAX else -1.0
    rc, dj0, _ = bnb.price_cols(P, cols, np.zeros(len(cols)), table=None)
    assert rc == 0
    obj = np.zeros(len(cols))
    for t, (ty, _, _) in enumerate(types):
        want = margin if STD_FLAG[ty] == NL else -margin  # sgn * d > 0 improves from a lower bound, < 0 from an upper one
        if not attractive:
            want = 0.0 if STD_FLAG[ty] == capi.NF else -want  # a free column rests only on a zero reduced cost
        obj[t] = sgn * want - dj0[t]
    return obj


def test_unattractive_columns_cost_no_pivot(gpu):
    for inst in (None, gs.general_lp(14, 20, 6), gs.general_lp(14, 20, 7)):
        if inst is None:
            P, M = dense(gpu, 20, 40, 8)
        else:
            P, M = gs.load(gpu, inst), gs.model(inst)
            P.simplex()
            if P.status != OPT:
                continue
        # every type, resting at 0: the basic values do not move, so the basis stays primal feasible as well
        types = [(LO, 0.0, 0.0), (UP, 0.0, 0.0), (DB, 0.0, 4.0), (FR, 0.0, 0.0), (FX, 0.0, 0.0), (LO, 0.0, 0.0)]
        cols, _ = draw_cols(np.random.default_rng(4), len(types), P.m)
        obj = priced_out(P, cols, types, 1.0, attractive=False)
        before, z = P.it_cnt, P.obj
        assert P.add_dense_cols(cols, obj, [t for t, _, _ in types], [l for _, l, _ in types], [u for _, _, u in types]) == 0
        assert P.simplex() == 0 and P.status == OPT and P.it_cnt == before
        Mx = M.copy()
        for t, (ty, l, u) in enumerate(types):
            Mx.add_col(cols[t, 1:], ty, l, u, cost=obj[t])
        cf.certify(Mx, P, what="unattractive")
        assert P.obj == z


def test_attractive_columns_end_in_the_optimum_of_the_extended_model(gpu, orc):
    A, b, c = synth.dense_lp(20, 40, 8)
    P, M = dense(gpu, 20, 40, 8)
    k = 6
    rng = np.random.default_rng(6)
    cols = np.zeros((k, 21))
    cols[:, 1:] = np.abs(np.round(rng.normal(size=(k, 20)) * 3)) / 4.0
    cols[:, 1] += 0.5  # every column meets a row: the LP stays bounded
    types = [(LO, 0.0, 0.0)] * k
    obj = priced_out(P, cols, types, 1.0, attractive=True)
    before = P.it_cnt
    assert P.add_dense_cols(cols, obj, [LO] * k, [0.0] * k, [0.0] * k) == 0
    assert P.simplex() == 0 and P.status == OPT and P.it_cnt > before
    Mx = M.copy()
    for t in range(k):
        Mx.add_col(cols[t, 1:], LO, 0.0, 0.0, cost=obj[t])
    cf.certify(Mx, P, what="attractive")
    O = orc.create()
    O.load_dense(np.hstack([A, cols[:, 1:].T]), b, np.concatenate([c, obj]))
    assert O.simplex() == 0 and O.status == OPT
    assert abs(P.obj - O.obj) <= 1e-9 * abs(O.obj)


# ------------------------------------------------------------------------------------------------ 4. state that survives


def test_pending_bound_edit_and_clones_survive_the_append(gpu):
    P, M = dense(gpu, 16, 30, 11)
    T0 = P.tableau()
    stat, x = P.col_stat(), P.col_prim()
    j = next(j + 1 for j in range(30) if stat[j] == capi.BS and x[j] > 1.0)
    rng = np.random.default_rng(12)
    cols, obj = draw_cols(rng, 3, 16)
    cols[:, 1:] = np.abs(cols[:, 1:])
    cols[:, 1] += 1.0
    types = [(LO, 0.0, 0.0), (DB, 1.0, 2.0), (LO, 0.0, 0.0)]
    args = ([t for t, _, _ in types], [l for _, l, _ in types], [u for _, _, u in types])
    # a clone, a pending branching bound on a basic column, the append (31 -> 34 columns: a relayout), the solve
    Q = P.copy()
    ub = float(np.floor(x[j - 1]))
    Q.api.set_col_bnds(Q.h, j, DB, 0.0, ub)
    assert Q.add_dense_cols(cols, obj, *args) == 0 and Q.api.get_tableau_ld(Q.h) == 64
    assert Q.simplex() == 0
    Mq = M.copy()
    Mq.set_col_bnds(j, DB, 0.0, ub)
    for t, (ty, l, u) in enumerate(types):
        Mq.add_col(cols[t, 1:], ty, l, u, cost=obj[t])
    ref = cf.certify(Mq, Q, what="pending edit + append")
    assert float(ref.x[16 + j - 1]) <= ub + 1e-9
    # the source of the clone is untouched by the append to the clone
    assert P.n == 30 and P.status == OPT and same_bits(P.tableau(), T0)
    before = P.it_cnt
    assert P.simplex() == 0 and P.it_cnt == before
    # a clone that is only recorded when the append moves its source: it receives the bits from before the append
    R = P.copy()
    assert P.add_dense_cols(cols, obj, *args) == 0 and P.api.get_tableau_ld(P.h) == 64
    assert R.n == 30 and same_bits(R.tableau(), T0)
    assert R.simplex() == 0 and R.status == OPT and R.it_cnt == before
    assert P.simplex() == 0
    Mp = M.copy()
    for t, (ty, l, u) in enumerate(types):
        Mp.add_col(cols[t, 1:], ty, l, u, cost=obj[t])
    cf.certify(Mp, P, what="source after the append")


# ------------------------------------------------------------------------------------------------ 5. column generation


def test_column_generation_ends_in_the_optimum_of_the_full_model(gpu):
    A, b, c = synth.dense_lp(24, 96, 7)
    P = gpu.create()
    P.load_dense(A[:, :24], b, c[:24])
    assert P.simplex() == 0 and P.status == OPT
    order = list(range(24))
    rest = list(range(24, 96))
    rounds = 0
    while rest:
        rc, dj = P.price_cols(A[:, rest].T, c[rest])  # one call prices every column that is still outside
        assert rc == 0
        pick = [i for i in np.argsort(-dj, kind="stable")[:8] if dj[i] > cf.TOL_DJ]
        if not pick:
            break
        take = [rest[i] for i in pick]
        assert P.add_dense_cols(A[:, take].T, c[take], [LO] * len(take), [0.0] * len(take), [0.0] * len(take)) == 0
        assert P.simplex() == 0 and P.status == OPT
        order += take
        rest = [j for j in rest if j not in take]
        rounds += 1
    assert rounds >= 2 and rest  # the restricted master found the optimum without seeing every column
    before = P.it_cnt
    assert P.add_dense_cols(A[:, rest].T, c[rest], [LO] * len(rest), [0.0] * len(rest), [0.0] * len(rest)) == 0
    order += rest
    assert P.simplex() == 0 and P.status == OPT and P.it_cnt == before and P.n == 96
    cf.certify(cf.Model.dense(A[:, order], b, c[order]), P, what="column generation")


# ------------------------------------------------------------------------------------------------ 6. refusals, set_mat_col


def test_refusals_leave_the_live_handle_alone(gpu):
    P, _ = dense(gpu, 10, 30, 13)
    T0 = P.tableau()
    cols, obj = draw_cols(np.random.default_rng(2), 2, 10)
    ty = np.array([LO, DB], dtype=np.int32)
    lb, ub = np.array([0.0, 1.0]), np.array([0.0, 2.0])
    f = gpu.add_dense_cols
    p = lambda a, T=DP: a.ctypes.data_as(T)  # noqa: E731
    nan_cols = cols.copy()
    nan_cols[0, 3] = math.nan
    bad_ty, bad_lb, nan_obj = np.array([LO, 7], dtype=np.int32), np.array([0.0, 3.0]), np.array([math.nan, 0.0])
    bad_kind = np.array([CV, 9], dtype=np.int32)
    calls = [
        (P.h, 0, p(cols), p(obj), p(ty, IP), p(lb), p(ub), None), (P.h, 2, None, p(obj), p(ty, IP), p(lb), p(ub), None),
        (P.h, 2, p(nan_cols), p(obj), p(ty, IP), p(lb), p(ub), None), (P.h, 2, p(cols), p(nan_obj), p(ty, IP), p(lb), p(ub), None),
        (P.h, 2, p(cols), p(obj), p(bad_ty, IP), p(lb), p(ub), None), (P.h, 2, p(cols), p(obj), p(ty, IP), p(bad_lb), p(ub), None),
        (P.h, 2, p(cols), p(obj), p(ty, IP), p(lb), p(ub), p(bad_kind, IP)),
    ]
    for a in calls:
        assert f(*a) == -1
        assert P.n == 30 and P.status == OPT and same_bits(P.tableau(), T0)
    dj = np.zeros(2)
    assert gpu.price_cols(P.h, 0, p(cols), p(obj), p(dj), None) == -1
    assert gpu.price_cols(P.h, 2, p(cols), p(obj), None, None) == -1
    assert f(P.h, 2, p(cols), p(obj), p(ty, IP), p(lb), p(ub), None) == 0 and P.n == 32


def test_set_mat_col_on_a_solved_handle_gives_the_tableau_up(gpu):
    A, b, c = synth.dense_lp(10, 30, 13)
    P = gpu.create()
    P.load_dense(A, b, c)
    assert P.simplex() == 0
    first = P.it_cnt
    newcol = np.linspace(0.1, 1.0, 10)
    P.set_mat_col(4, np.arange(11), np.concatenate([[0.0], newcol]))
    assert P.status == UNDEF
    with pytest.raises(RuntimeError):
        P.tableau()
    assert P.simplex() == 0
    B = A.copy()
    B[:, 3] = newcol
    R = gpu.create()
    R.load_dense(B, b, c)
    for i in range(10):  # the parent's only way to fill a column: every row rewritten
        R.set_mat_row(i + 1, np.arange(31), np.concatenate([[0.0], B[i]]))
    assert R.simplex() == 0
    assert (P.status, P.obj, P.it_cnt - first) == (R.status, R.obj, R.it_cnt)
    assert np.array_equal(P.tableau(), R.tableau())
