"""GPU: sifting over a device column pool (mvx_pool_price, mvx_pool_append, mvx_sift; DESIGN.md "Sifting (sift)").

mvx_pool_price is held bit for bit to its two host twins -- the reduced costs by bits, the picks by equality -- at the shape
boundaries of k_poolprice (1 row, 63 / 64 / 65 rows around a wave of chains, 130 rows; 1, 63 / 64 / 65, 255 / 256 / 257 and 1000
columns around a wave, a selection workgroup and several of them), for K = 0, 1, 7 and N, with and without skip masks, on a slack
basis, on duplicated columns and on a pool that grew after its first pricing; and, independently, against mvx_price_cols within
the sum of the two derived error bounds.  mvx_pool_append is held bit for bit to mvx_add_dense_cols on a clone.  The loop is held
to the direct solve of the full-width LP, to certify.py on its working model, to its own pricing, and to its contract on `where`,
purging, the round limit, unboundedness and clones."""
import ctypes as C
import math

import numpy as np
import pytest

import mvolps_amd
from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import CV, DB, FR, FX, IV, LO, MAX, MIN, OPT, UNBND, UNDEF, UP

from . import certify as cf
from . import general_at_size as gs
from .test_addcols import columns_of, same_bits
from .test_gpu_addcols import dense, ld_of, with_cut_rows

pytestmark = pytest.mark.gpu

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
TOL = 1e-9  # mvx_init_smcp's tol_dj
ZERO_REST = [(LO, 0.0, 0.0), (UP, 0.0, 0.0), (DB, 0.0, 2.5), (FR, 0.0, 0.0), (FX, 0.0, 0.0), (LO, 0.0, 0.0), (DB, 0.0, 1.0)]


def draw_pool(rng, N, m, scale=1.0):
    """N columns with full mantissas (the order of the additions shows in the bits), a third of the entries zero."""
    cols = rng.normal(size=(N, m + 1)) * 3
    cols[rng.random((N, m + 1)) < 0.3] = 0.0
    cols[:, 0] = 0.0
    return cols, rng.normal(size=N) * scale


def make_pool(m, cols, obj, types):
    S = mvolps_amd.create_pool(m)
    assert S.add_cols(cols, obj, [t for t, _, _ in types], [l for _, l, _ in types], [u for _, _, u in types]) == 0
    return S


def y_of(P):
    """y_i: row 0 at the non-basic position of auxiliary i, +0.0 where it is basic."""
    T = P.tableau()
    _, nb, _ = P.basis()
    y = np.zeros(P.m + 1)
    for q in range(1, P.n + 1):
        if nb[q] <= P.m:
            y[nb[q]] = T[0, q]
    return y


def twins(P, cols, obj, types, K, skip=None):
    rc, dj, att = bnb.pool_price_values(cols, obj, [t for t, _, _ in types], y_of(P), P.api.get_obj_dir(P.h), TOL)
    assert rc == 0
    rc, pick = bnb.pool_select(dj, att, K, skip)
    assert rc == 0
    return dj, att, pick


def root(gpu, kind, m, n, seed):
    if kind == "dense":  # MAX
        return dense(gpu, m, n, seed)[0]
    inst = gs.general_lp(m, n, seed)
    inst["direction"] = MIN
    P = gs.load(gpu, inst)
    P.simplex()
    assert P.status != UNDEF
    return P


def check_against_twins(P, S, cols, obj, types, rng):
    N = S.n
    T0 = P.tableau()
    for K in (0, 1, 7, N):
        for masked in (False, True):
            skip = None
            if masked:
                skip = (rng.random(N + 1) < 0.4).astype(np.uint8)
                skip[0] = 1  # not read
            rc, dj, pick = P.pool_price(S, K, skip)
            tdj, att, tpick = twins(P, cols, obj, types, K, skip)
            assert rc == 0 and same_bits(dj, tdj), (K, masked, np.argwhere(dj != tdj)[:4])
            assert list(pick) == list(tpick), (K, masked)
    rc, none, pick = P.pool_price(S, 3, want_dj=False)  # dj == NULL
    assert rc == 0 and none is None and list(pick) == list(twins(P, cols, obj, types, 3)[2])
    assert same_bits(P.tableau(), T0)  # pure
    return att


# ------------------------------------------------------------------------------------------------ 1. pricing and selection = twins


@pytest.mark.parametrize("kind", ["dense", "general"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1000])
@pytest.mark.parametrize("m", [1, 5, 63, 64, 65, 130])
def test_pool_price_equals_the_twins_at_the_shape_boundaries(gpu, m, N, kind):
    P = root(gpu, kind, m, 24, 3 + m)
    status = P.status
    rng = np.random.default_rng(1000 * m + N)
    cols, obj = draw_pool(rng, N, m)
    types = [ZERO_REST[t % len(ZERO_REST)] for t in range(N)]
    S = make_pool(m, cols, obj, types)
    check_against_twins(P, S, cols, obj, types, rng)
    assert P.status == status


def test_pool_price_on_a_slack_basis_is_the_objective(gpu):
    P, _ = dense(gpu, 7, 66, 2, c_sign=-1.0)  # the slack basis is optimal: every auxiliary is basic, all y = 0
    assert P.it_cnt == 0 and not y_of(P).any()
    rng = np.random.default_rng(8)
    cols, obj = draw_pool(rng, 300, 7)
    obj[5] = -0.0
    types = [ZERO_REST[t % len(ZERO_REST)] for t in range(300)]
    S = make_pool(7, cols, obj, types)
    rc, dj, pick = P.pool_price(S, 300)
    assert rc == 0 and same_bits(dj[1:], obj + 0.0)
    check_against_twins(P, S, cols, obj, types, rng)


def test_pool_price_breaks_ties_between_duplicates_by_column(gpu):
    P, _ = dense(gpu, 65, 30, 4)
    rng = np.random.default_rng(9)
    base, bobj = draw_pool(rng, 40, 65)
    rep = rng.integers(0, 40, size=700)  # 700 columns drawn from 40: every reduced cost many times over
    cols, obj = base[rep], bobj[rep]
    types = [(LO, 0.0, 0.0)] * 700
    S = make_pool(65, cols, obj, types)
    att = check_against_twins(P, S, cols, obj, types, rng)
    assert att.sum() > 100
    rc, dj, pick = P.pool_price(S, 700)
    mag = np.abs(dj[pick])
    assert np.all(mag[:-1] >= mag[1:])
    assert all(pick[t] < pick[t + 1] for t in range(len(pick) - 1) if mag[t] == mag[t + 1])  # ties: the lower column first
    assert len(set(pick.tolist())) == len(pick) == att.sum()


def test_pool_price_after_the_pool_grew(gpu):
    P, _ = dense(gpu, 64, 30, 6)
    rng = np.random.default_rng(10)
    cols, obj = draw_pool(rng, 900, 64)
    types = [ZERO_REST[t % len(ZERO_REST)] for t in range(900)]
    S = make_pool(64, cols[:200], obj[:200], types[:200])
    check_against_twins(P, S, cols[:200], obj[:200], types[:200], rng)  # the device copy holds 200 columns
    for lo, hi in ((200, 230), (230, 900)):  # within the copy's spare room, then beyond it
        assert S.add_cols(cols[lo:hi], obj[lo:hi], [t for t, _, _ in types[lo:hi]], [l for _, l, _ in types[lo:hi]],
                          [u for _, _, u in types[lo:hi]]) == 0
        check_against_twins(P, S, cols[:hi], obj[:hi], types[:hi], rng)


@pytest.mark.parametrize("m,n", [(5, 63), (65, 130), (130, 40)])
def test_pool_price_agrees_with_price_cols_within_the_derived_bounds(gpu, m, n):
    """An independent path: k_addcols sums the same products over the non-basic positions, not over the rows."""
    P, _ = dense(gpu, m, n, 11 + m)
    rng = np.random.default_rng(m + n)
    cols, obj = draw_pool(rng, 200, m)
    S = make_pool(m, cols, obj, [(LO, 0.0, 0.0)] * 200)
    rc, dj, _ = P.pool_price(S, 0)
    rc2, pdj = P.price_cols(cols, obj)
    assert rc == 0 and rc2 == 0
    y = y_of(P)
    mag = np.abs(obj) + np.abs(cols[:, 1:] * y[1:]).sum(axis=1)
    u = 2.0 ** -53
    bound = ((math.ceil(m / 64) + 8) + (math.ceil(n / 64) + 8)) * u * mag
    assert np.all(np.abs(dj[1:] - pdj) <= bound), float((np.abs(dj[1:] - pdj) / np.maximum(bound, 1e-300)).max())


# ------------------------------------------------------------------------------------------------ 2. the append = add_dense_cols


def state_of(P):
    head, nb, flag = P.basis()
    return P.tableau(), head, nb, flag, P.api.get_tableau_ld(P.h), P.status, P.col_prim(), P.row_prim()


def check_pool_append(P, k, seed):
    m, n = P.m, P.n
    rng = np.random.default_rng(seed)
    N = k + 9
    cols, obj = draw_pool(rng, N, m, scale=0.01)
    types = [ZERO_REST[t % len(ZERO_REST)] for t in range(N)]
    kinds = [IV if t % 3 == 0 else CV for t in range(N)]
    S = mvolps_amd.create_pool(m)
    assert S.add_cols(cols, obj, [t for t, _, _ in types], [l for _, l, _ in types], [u for _, _, u in types], kinds) == 0
    idx = rng.permutation(N)[:k] + 1  # distinct, in no order
    Q = P.copy()
    sel = idx - 1
    assert Q.add_dense_cols(cols[sel], obj[sel], [types[t][0] for t in sel], [types[t][1] for t in sel], [types[t][2] for t in sel],
                            [kinds[t] for t in sel]) == 0
    assert P.pool_append(S, idx) == 0
    assert (P.m, P.n) == (m, n + k) and P.status == UNDEF
    a, b = state_of(P), state_of(Q)
    assert same_bits(a[0], b[0]), np.argwhere(a[0] != b[0])[:4]
    assert all(np.array_equal(a[i], b[i]) for i in (1, 2, 3)) and a[4] == b[4] == ld_of(n + k) and a[5] == b[5]
    assert same_bits(a[6], b[6]) and same_bits(a[7], b[7])
    assert columns_of(P) == columns_of(Q)
    assert P.simplex() == Q.simplex() and P.status == Q.status and P.it_cnt == Q.it_cnt and same_bits(P.tableau(), Q.tableau())


@pytest.mark.parametrize("variant", ["plain", "cut rows"])
@pytest.mark.parametrize("n,k", [(30, 1), (31, 1), (62, 2), (20, 50)])
def test_pool_append_equals_add_dense_cols(gpu, n, k, variant):
    P, M = dense(gpu, 12, n, 5 + n)
    if variant == "cut rows":
        with_cut_rows(P, M, violated=True)
    assert (ld_of(n + k) == ld_of(n)) == ((n, k) == (30, 1))  # in place once, a relayout otherwise
    check_pool_append(P, k, n + k)
    if ld_of(P.n + 1) == ld_of(P.n):  # and in place on the handle that has moved
        P.simplex()
        check_pool_append(P, 1, 1)


def test_pool_append_without_a_tableau_edits_the_model_only(gpu):
    A, b, c = synth.dense_lp(9, 14, 3)
    P, Q = gpu.create(), gpu.create()
    P.load_dense(A, b, c)
    Q.load_dense(A, b, c)
    rng = np.random.default_rng(2)
    cols, obj = draw_pool(rng, 6, 9)
    types = ZERO_REST[:6]
    S = make_pool(9, cols, obj, types)
    idx = np.array([5, 2, 6], dtype=np.int32)
    assert P.pool_append(S, idx) == 0
    sel = idx - 1
    assert Q.add_dense_cols(cols[sel], obj[sel], [types[t][0] for t in sel], [types[t][1] for t in sel], [types[t][2] for t in sel]) == 0
    assert P.n == 17 and columns_of(P) == columns_of(Q) and P.status == UNDEF
    with pytest.raises(RuntimeError):
        P.tableau()
    assert P.simplex() == Q.simplex() and same_bits(P.tableau(), Q.tableau())


# ------------------------------------------------------------------------------------------------ 3. the loop

OWN = 8  # columns of the working set the loop starts from


def dense_instance(m, N, seed):
    """max c x, A x <= b, x >= 0 over OWN + N columns: the first OWN are the working set, the others the pool (MVX_LO at 0)."""
    A, b, c = synth.dense_lp(m, OWN + N, seed)
    rows = [(UP, 0.0, float(v)) for v in b]
    colb = [(LO, 0.0, 0.0)] * (OWN + N)
    return dict(A=A, row_b=rows, col_b=colb, c=c, direction=MAX)


def general_instance(m, N, seed):
    """The same LP with its columns turned into every zero-rest type, minimised: a column with an upper bound of 0 is the
    mirror image of one with a lower bound of 0, a double-bounded one gains an upper bound, and one column in 250 is free (a
    free column turns a dual inequality into an equation: a handful of them, all with the same gain of 2 -- above every other
    column's -- leave the dual feasible, so the optimum is finite, which the direct solve of `instance` asserts).  The slack basis is feasible."""
    inst = dense_instance(m, N, seed)
    rng = np.random.default_rng(seed)
    A, c = inst["A"].copy(), -inst["c"]  # min -c x
    colb = list(inst["col_b"])
    for j in range(OWN + N):
        t = FR if j % 250 == 3 else (LO, UP, DB)[j % 3]
        if t == UP:
            A[:, j], c[j] = -A[:, j], -c[j]
            colb[j] = (UP, 0.0, 0.0)
        elif t == DB:
            colb[j] = (DB, 0.0, float(rng.integers(1, 4)))
        elif t == FR:
            colb[j], c[j] = (FR, 0.0, 0.0), -2.0
    inst.update(A=A, c=c, col_b=colb, direction=MIN)
    return inst


INSTANCES = {
    "dense-24x600": lambda: dense_instance(24, 600, 7),
    "dense-40x1500": lambda: dense_instance(40, 1500, 8),
    "general-24x600": lambda: general_instance(24, 600, 9),
    "general-40x1500": lambda: general_instance(40, 1500, 10),
}
_CACHE = {}


def instance(name):
    """The instance with the objective of the direct solve on all columns, computed once and left unchanged."""
    if name not in _CACHE:
        inst = INSTANCES[name]()
        F = gs.load(mvolps_amd.api(), inst)
        assert F.simplex() == 0 and F.status == OPT
        inst["z"] = F.obj
        _CACHE[name] = inst
    return _CACHE[name]


def sub_instance(inst, order):
    order = list(order)
    return dict(A=inst["A"][:, order], row_b=inst["row_b"], col_b=[inst["col_b"][j] for j in order], c=inst["c"][order],
                direction=inst["direction"])


def start(gpu, inst):
    """The working LP over the first OWN columns and the pool of the others."""
    P = gs.load(gpu, sub_instance(inst, range(OWN)))
    n = inst["A"].shape[1]
    S = make_pool(P.m, inst["A"][:, OWN:].T, inst["c"][OWN:], inst["col_b"][OWN:])
    assert S.n == n - OWN
    return P, S


def columns_in(P, where):
    """The columns of the full LP that P holds, in P's order; checks `where` against P through mvx_get_mat_col."""
    inv = {int(w): j for j, w in enumerate(where) if j >= 1 and w != 0}
    assert len(inv) == int(np.count_nonzero(where[1:])) == P.n - OWN and all(OWN < w <= P.n for w in inv)
    return list(range(OWN)) + [OWN + inv[w] - 1 for w in range(OWN + 1, P.n + 1)]


def check_end(P, S, inst, where, info):
    order = columns_in(P, where)
    for w in range(1, P.n + 1):
        ind, val = P.get_mat_col(w)
        col = inst["A"][:, order[w - 1]]
        assert list(ind) == list(np.nonzero(col)[0] + 1) and same_bits(val, col[col != 0.0])
        assert P.api.get_obj_coef(P.h, w) == inst["c"][order[w - 1]]
    assert info.end == OPT and P.status == OPT and info.n_final == P.n
    cf.certify(gs.model(sub_instance(inst, order)), P, what="working LP")  # (b)
    skip = (np.asarray(where) != 0).astype(np.uint8)
    rc, _, pick = P.pool_price(S, S.n, skip)
    assert rc == 0 and len(pick) == 0  # (c)
    assert abs(P.obj - inst["z"]) <= 1e-9 * abs(inst["z"])  # (d)


@pytest.mark.parametrize("purge", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_sift_meets_the_direct_solve(gpu, name, purge):
    inst = instance(name)
    P, S = start(gpu, inst)
    rc, where, info = P.sift(S, purge=purge)
    assert rc == 0, (rc, info.end, info.rounds)
    check_end(P, S, inst, where, info)
    assert info.rounds == info.lps >= 2 and info.priced == info.rounds * S.n
    assert info.appended - info.purged == P.n - OWN and (purge > 0 or info.purged == 0)
    assert P.n < inst["A"].shape[1]  # the optimum was found without every column


@pytest.mark.parametrize("name", ["dense-24x600", "general-24x600"])
def test_a_second_call_continues_warm_after_a_bound_edit(gpu, name):
    inst = instance(name)
    P, S = start(gpu, inst)
    rc, where, info = P.sift(S)
    assert rc == 0
    order = columns_in(P, where)
    x = P.col_prim()
    w = next(w for w in range(1, P.n + 1) if inst["col_b"][order[w - 1]][0] in (LO, DB) and x[w - 1] > 1e-3)  # a column in use
    ub = 0.5 * float(x[w - 1])
    P.api.set_col_bnds(P.h, w, DB, 0.0, ub)
    edited = dict(inst)
    edited["col_b"] = list(inst["col_b"])
    edited["col_b"][order[w - 1]] = (DB, 0.0, ub)
    F = gs.load(gpu, edited)
    assert F.simplex() == 0 and F.status == OPT
    edited["z"] = F.obj
    assert abs(F.obj - inst["z"]) > 1e-9 * abs(inst["z"])  # the edit matters
    n1 = P.n
    P.tableau()  # the edit left the tableau in place
    rc, where2, info2 = P.sift(S, where=where)
    assert rc == 0 and np.array_equal(where2[where != 0], where[where != 0]) and P.n >= n1
    check_end(P, S, edited, where2, info2)
    assert info2.pivots <= info.pivots  # warm: the first call's work is not done again


def test_the_round_limit_leaves_a_solved_working_lp(gpu):
    inst = instance("dense-24x600")
    P, S = start(gpu, inst)
    rc, where, info = P.sift(S, max_rounds=1)
    assert rc == -4 and info.end == 0 and info.rounds == 1 and info.appended == 0 and not where.any()
    assert P.status == OPT and P.n == OWN
    cf.certify(gs.model(sub_instance(inst, range(OWN))), P, what="round limit")
    rc, where, info = P.sift(S, where=where, K=5, max_rounds=2)  # one append, then the limit again
    assert rc == -4 and info.appended == 5 and P.n == OWN + 5 and P.status == OPT
    cf.certify(gs.model(sub_instance(inst, columns_in(P, where))), P, what="round limit after an append")


def test_an_unbounded_pool_column_ends_the_loop(gpu):
    inst = instance("dense-24x600")
    P = gs.load(gpu, sub_instance(inst, range(OWN)))
    A, c = inst["A"][:, OWN:].T.copy(), inst["c"][OWN:].copy()
    A[17], c[17] = -1.0, 2.0  # a ray: every row lets it grow
    S = make_pool(P.m, A, c, inst["col_b"][OWN:])
    rc, where, info = P.sift(S)
    assert rc == 0 and info.end == UNBND and P.status == UNBND and where[18] != 0


def test_a_clone_taken_before_the_call_keeps_its_bits(gpu):
    inst = instance("dense-24x600")
    P, S = start(gpu, inst)
    assert P.simplex() == 0
    Q = P.copy()
    T0, z0 = Q.tableau(), Q.obj
    rc, where, info = P.sift(S)
    assert rc == 0 and P.n > OWN
    assert Q.n == OWN and Q.status == OPT and Q.obj == z0 and same_bits(Q.tableau(), T0)
    before = Q.it_cnt
    assert Q.simplex() == 0 and Q.it_cnt == before


# ------------------------------------------------------------------------------------------------ 4. refusals


def test_refusals(gpu):
    inst = instance("dense-24x600")
    P, S = start(gpu, inst)
    N = S.n
    api = gpu
    pick, npick, dj = np.zeros(N, dtype=np.int32), C.c_int(0), np.zeros(N + 1)
    p = lambda a, T=IP: a.ctypes.data_as(T)  # noqa: E731
    # no tableau yet / a status of MVX_UNDEF
    assert api.pool_price(P.h, S.h, None, 3, None, p(pick), C.byref(npick)) == -3
    assert P.simplex() == 0
    T0 = P.tableau()
    assert api.pool_price(None, S.h, None, 3, None, p(pick), C.byref(npick)) == -1
    assert api.pool_price(P.h, None, None, 3, None, p(pick), C.byref(npick)) == -1
    assert api.pool_price(P.h, S.h, None, -1, None, p(pick), C.byref(npick)) == -1
    assert api.pool_price(P.h, S.h, None, 3, None, None, C.byref(npick)) == -1
    assert api.pool_price(P.h, S.h, None, 3, None, p(pick), None) == -1
    S5 = make_pool(5, np.ones((1, 5)), [1.0], [(LO, 0.0, 0.0)])  # another row count
    assert api.pool_price(P.h, S5.h, None, 1, None, p(pick), C.byref(npick)) == -1
    assert api.pool_append(P.h, S5.h, 1, p(np.array([1], dtype=np.int32))) == -1
    for idx in ([0], [N + 1], [3, 3], []):
        a = np.array(idx + [0], dtype=np.int32)
        assert api.pool_append(P.h, S.h, len(idx), p(a)) == -1
    assert api.pool_append(None, S.h, 1, p(pick)) == -1 and api.pool_append(P.h, None, 1, p(pick)) == -1
    assert api.pool_append(P.h, S.h, 1, None) == -1

    def sift(where=None, **kw):
        return P.sift(S, where=where, **kw)[0]

    assert sift(K=0) == -1 and sift(max_rounds=0) == -1 and sift(purge=-1) == -1 and sift(purge=65) == -1
    w = np.zeros(N + 1, dtype=np.int32)
    for j, v in ((3, OWN + 1), (3, -1)):  # out of range
        w[:] = 0
        w[j] = v
        assert sift(w) == -1
    w[:] = 0
    w[3] = w[9] = 2  # a column named twice
    assert sift(w) == -1
    w[:] = 0
    w[3] = 2  # column 2 of P is not pool column 3
    assert sift(w) == -1
    assert api.sift(P.h, S5.h, None, None, p(w), None) == -1 and api.sift(P.h, S.h, None, None, None, None) == -1
    assert P.n == OWN and P.status == OPT and same_bits(P.tableau(), T0)  # nothing changed
    info = capi.SiftInfo()
    w[:] = 0
    assert api.sift(P.h, S.h, None, None, p(w), C.byref(info)) == 0 and info.end == OPT  # sp == NULL: the defaults
    assert abs(P.obj - inst["z"]) <= 1e-9 * abs(inst["z"])


# ------------------------------------------------------------------------------------------------ 5. the command line

WIDE = """\\ three rows, ten columns; x9 and x10 cannot rest at 0 and form the first working set
Maximize
 obj: 3 x1 + 2 x2 + 4 x3 + x4 + 5 x5 + 2 x6 + 3 x7 + x8 + x9 - x10
Subject To
 c1: x1 + 2 x2 + x3 + 3 x5 + x7 + x9 <= 14
 c2: 2 x1 + x3 + x4 + 2 x5 + 2 x6 + x8 + x10 <= 12
 c3: x2 + 3 x3 + x4 + x6 + 2 x7 + x8 + x9 + x10 <= 15
Bounds
 1 <= x9 <= 4
 2 <= x10 <= 6
 x8 <= 3
End
"""


def test_cli_sift_solves_the_relaxation(gpu, tmp_path):
    import os
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mvolps_amd", "bin", "mvolps")
    lp = str(tmp_path / "wide.lp")
    open(lp, "w").write(WIDE)
    L = bnb.lib()
    L.mvx_read_lp.restype = C.c_int
    L.mvx_read_lp.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p]
    P = gpu.create()
    assert L.mvx_read_lp(P.h, None, lp.encode()) == 0
    assert P.simplex() == 0 and P.status == OPT
    for extra, K in (([], None), (["2"], 2)):
        r = subprocess.run([exe, "-f", lp, "--sift"] + extra, capture_output=True, text=True)
        out = dict(line.split(" ", 1) for line in r.stdout.splitlines() if line.startswith("SIFT."))
        assert r.returncode == 0 and out["SIFT.RC"] == "0" and out["SIFT.STATUS"] == "OPTIMAL", (r.stdout, r.stderr)
        assert abs(float(out["SIFT.OBJ"]) - P.obj) <= 1e-9 * abs(P.obj)
        assert int(out["SIFT.ROUNDS"]) >= 2 and int(out["SIFT.APPENDED"]) >= 1 and out["SIFT.PURGED"] == "0"
        assert out["SIFT.N_FINAL"] == "%d of 10" % (2 + int(out["SIFT.APPENDED"]))
    bad = subprocess.run([exe, "-f", lp, "--sift", "0"], capture_output=True, text=True)
    assert bad.returncode != 0 and "--sift" in bad.stderr
