"""GPU: column deletion on a live tableau (mvx_del_cols, k_delcols; DESIGN.md "Column deletion (del_cols)").

check_delete restates the definition in numpy -- the fma chain on column 0 over the deleted positions with a non-zero resting
value, in ascending position order, then the compaction by position and the renumbering by column -- and holds the handle to
it bit for bit, and to the independent reference of tests/certify.py on the reduced model before any solve.  The sweep places
the deletion in place and across one and two multiples of the row stride, at the first and the last position, on adjacent
positions, on all non-basic structurals but one, and with moved spans around the kernel's batch (mvx_del_cols_span), each on
plain handles, handles that carry cut rows and handles after a row deletion.  Then the shift of column 0 on general bounds, the
solves that follow, the state that survives, a column generation loop with a purge, and the refusals."""
import bisect
import ctypes as C

import numpy as np
import pytest

from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import DB, FR, FX, LO, NF, NL, NS, NU, OPT, UNDEF, UP

from . import certify as cf
from . import general_at_size as gs
from .test_addcols import draw_cols, fma, same_bits

pytestmark = pytest.mark.gpu

IP = C.POINTER(C.c_int)
VARIANTS = ["plain", "cut rows", "after del_rows"]


def ld_of(n):
    return (n + 1 + 31) // 32 * 32


def dense(api, m, n, seed):
    A, b, c = synth.dense_lp(m, n, seed)
    P = api.create()
    P.load_dense(A, b, c)
    assert P.simplex() == 0 and P.status == OPT
    return P, cf.Model.dense(A, b, c)


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


def prepared(api, m, n, seed, variant):
    P, M = dense(api, m, n, seed)
    if variant == "cut rows":
        with_cut_rows(P, M, violated=True)
    elif variant == "after del_rows":
        with_cut_rows(P, M, violated=False)
        assert P.row_stat()[m] == capi.BS and P.del_rows([m + 1]) == 0 and P.m == m + 1
        M.A = np.delete(M.A, m, axis=0)
        del M.rows[m]
    return P, M


def structural_positions(P):
    """The non-basic positions that hold a structural variable, ascending."""
    _, nb, _ = P.basis()
    return [q for q in range(1, P.n + 1) if nb[q] > P.m]


def cols_at(P, positions):
    _, nb, _ = P.basis()
    return [int(nb[q]) - P.m for q in positions]


def reduced(M, cols):
    """The certify model without the columns `cols` (1-based)."""
    idx = sorted(j - 1 for j in cols)
    R = M.copy()
    R.A = np.delete(R.A, idx, axis=1)
    R.c = np.delete(R.c, idx)
    R.cols = [b for j, b in enumerate(R.cols) if j not in idx]
    R.kinds = [k for j, k in enumerate(R.kinds) if j not in idx]
    return R


def check_delete(P, M, cols, what=""):
    """Deletes the non-basic columns `cols` of the handle P (model M, valid tableau) and checks everything the definition says;
    returns (the reduced model, whether column 0 was shifted)."""
    m, n = P.m, P.n
    cols = [int(j) for j in cols]
    ncs = len(cols)
    T0 = P.tableau()
    head0, nb0, flag0 = P.basis()
    api, h = P.api, P.h
    lb0 = [api.get_col_lb(h, j) for j in range(1, n + 1)]
    ub0 = [api.get_col_ub(h, j) for j in range(1, n + 1)]
    prim0 = P.col_prim()
    pos_of = {int(nb0[q]): q for q in range(1, n + 1)}
    qs = sorted(pos_of[m + j] for j in cols)  # KeyError: a basic column, which check_delete is not for
    lo, hi = M.lo_hi()
    # the restatement: column 0 first, one fma chain per row over the deleted positions, ascending
    col0 = T0[:, 0].copy()
    shifted = False
    for q in qs:
        k, f = int(nb0[q]), int(flag0[q])
        x = {NL: lo[k - 1], NS: lo[k - 1], NU: hi[k - 1], NF: 0.0}[f]
        if x != 0.0:
            shifted = True
            for p in range(m + 1):
                col0[p] = fma(float(T0[p, q]), -float(x), float(col0[p]))
    keep_pos = [q for q in range(1, n + 1) if q not in set(qs)]
    gone = sorted(cols)

    def ren(k):
        return k if k <= m else k - bisect.bisect_left(gone, k - m)

    head_w = np.array([0] + [ren(int(k)) for k in head0[1:]], dtype=np.int32)
    nb_w = np.array([0] + [ren(int(nb0[q])) for q in keep_pos], dtype=np.int32)
    flag_w = np.array([0] + [int(flag0[q]) for q in keep_pos], dtype=np.int32)
    assert P.del_cols(cols) == 0, what
    assert (P.m, P.n) == (m, n - ncs) and P.status == UNDEF, what
    assert api.get_tableau_ld(h) == ld_of(n - ncs), what
    T1 = P.tableau()
    head1, nb1, flag1 = P.basis()
    assert same_bits(T1[:, 1:], T0[:, keep_pos]), (what, np.argwhere(T1[:, 1:] != T0[:, keep_pos])[:4])
    assert same_bits(T1[:, 0], col0), what
    assert np.array_equal(head1, head_w) and np.array_equal(nb1, nb_w) and np.array_equal(flag1, flag_w), what
    R = reduced(M, cols)
    assert cf.certify_tableau(cf.Ref(R, (head1, nb1, flag1)), T1, what or "delete n=%d ncs=%d" % (n, ncs)) <= 1.0
    kept = [j for j in range(1, n + 1) if j not in set(cols)]
    row_of = {int(head1[i]): i for i in range(1, m + 1)}
    prim1 = P.col_prim()
    for w, j in enumerate(kept, start=1):
        assert api.get_col_lb(h, w) == lb0[j - 1] and api.get_col_ub(h, w) == ub0[j - 1], (what, j)
        # a basic column reads its row of column 0, which is the old value unless resting values were shifted out
        want = col0[row_of[m + w]] if m + w in row_of else prim0[j - 1]
        assert prim1[w - 1] == want, (what, j)
        if not shifted:
            assert prim1[w - 1] == prim0[j - 1], (what, j)
    return R, shifted


def solve_and_certify(P, R, what):
    P.simplex()
    cf.certify(R, P, what=what)


# ------------------------------------------------------------------------------------------------ 1. the shape sweep


def pick_middle(P):
    s = structural_positions(P)
    return [s[len(s) // 2]]


def pick_scattered(count):
    def pick(P):
        s = structural_positions(P)
        assert len(s) >= count
        return sorted(int(q) for q in np.random.default_rng(count).choice(s, size=count, replace=False))

    return pick


def pick_last(P):
    s = structural_positions(P)
    return [P.n] if s[-1] == P.n else None


def pick_first(P):
    s = structural_positions(P)
    return [1] if s[0] == 1 else None


def pick_adjacent(P):
    s = structural_positions(P)
    return next(([q, q + 1] for q in s[2:] if q + 1 in s), None)


def pick_all_but_one(P):
    s = structural_positions(P)
    return [q for q in s if q != s[len(s) // 2]]


SWEEP = [
    ("in place", 8, 40, pick_middle, lambda n, k: ld_of(n - k) == ld_of(n) == 64 and k == 1),
    ("one stride down", 9, 32, pick_middle, lambda n, k: (ld_of(n), ld_of(n - k)) == (64, 32) and k == 1),
    ("two strides down", 12, 70, pick_scattered(40), lambda n, k: (ld_of(n), ld_of(n - k)) == (96, 32) and k == 40),
    ("nothing moves", 5, 40, pick_last, lambda n, k: k == 1),
    ("everything moves", 6, 40, pick_first, lambda n, k: k == 1),
    ("adjacent", 7, 45, pick_adjacent, lambda n, k: k == 2),
    ("all but one", 10, 50, pick_all_but_one, lambda n, k: k >= 38),
]


def find_handle(api, m, n, variant, pick):
    """The first seed whose solved basis offers the positions the case asks for (the generator is deterministic)."""
    for seed in range(1, 13):
        P, M = prepared(api, m, n, seed, variant)
        positions = pick(P)
        if positions:
            return P, M, positions
    raise AssertionError("no seed gives the case its positions")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_delete_in_place_and_with_relayout(gpu, case, variant):
    name, m, n, pick, shape_ok = case
    P, M, positions = find_handle(gpu, m, n, variant, pick)
    assert shape_ok(n, len(positions)), (n, len(positions))
    what = "%s, %s" % (name, variant)
    R, shifted = check_delete(P, M, cols_at(P, positions), what)
    assert not shifted  # load_dense columns rest at 0
    # a second deletion, in place, on the handle that may have moved once
    s = structural_positions(P)
    if len(s) >= 2 and ld_of(P.n - 1) == ld_of(P.n):
        R, _ = check_delete(P, R, cols_at(P, [s[0]]), what + ", second")
    solve_and_certify(P, R, what)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("over", [-1, 0, 1, None], ids=["S-1", "S", "S+1", "2S+3"])
def test_moved_spans_around_the_batch(gpu, over, variant):
    S = gpu.del_cols_span()
    assert S == bnb.del_cols_span() and S % 64 == 0
    span = 2 * S + 3 if over is None else S + over
    n = span + 10
    P, M = prepared(gpu, 4, n, 3, variant)
    s = structural_positions(P)
    first = s[0]
    ncs = n - span - first + 1  # nmove = (n - ncs) - first + 1 == span
    assert 1 <= ncs <= 10
    rest = sorted(int(q) for q in np.random.default_rng(span).choice(s[1:], size=ncs - 1, replace=False))
    positions = [first] + rest
    assert (n - ncs) - first + 1 == span
    what = "span %d, %s" % (span, variant)
    R, _ = check_delete(P, M, cols_at(P, positions), what)
    solve_and_certify(P, R, what)


# ------------------------------------------------------------------------------------------------ 2. the shift of column 0

SHIFT_TYPES = [(DB, 1.5, 2.0), (UP, 0.0, -1.25), (FX, 2.0, 2.0), (FR, 0.0, 0.0), (LO, 0.0, 0.0), (DB, -0.75, 4.0)]


def test_column_0_is_shifted_for_the_resting_values_of_appended_columns(gpu):
    P, M = dense(gpu, 8, 20, 4)
    n, k = P.n, len(SHIFT_TYPES)
    cols, obj = draw_cols(np.random.default_rng(8), k, P.m)
    assert P.add_dense_cols(cols, obj, [t for t, _, _ in SHIFT_TYPES], [l for _, l, _ in SHIFT_TYPES], [u for _, _, u in SHIFT_TYPES]) == 0
    Mx = M.copy()
    for t, (ty, l, u) in enumerate(SHIFT_TYPES):
        Mx.add_col(cols[t, 1:], ty, l, u, cost=obj[t])
    # a subset of the new columns (every type, one DB stays) together with two old non-basic columns, in no order
    old = cols_at(P, [q for q in structural_positions(P) if q <= n][1:3])
    gone = [n + 4, n + 1, old[1], n + 3, n + 2, old[0], n + 5]
    R, shifted = check_delete(P, Mx, gone, "appended columns")
    assert shifted
    solve_and_certify(P, R, "appended columns, solved")
    # the same through a solve in between: whatever rests non-basic on a non-zero value afterwards
    P, M = dense(gpu, 8, 20, 4)
    assert P.add_dense_cols(cols, obj, [t for t, _, _ in SHIFT_TYPES], [l for _, l, _ in SHIFT_TYPES], [u for _, _, u in SHIFT_TYPES]) == 0
    P.simplex()
    if P.status == OPT:
        new_nb = [j for j in range(n + 1, n + k + 1) if P.col_stat()[j - 1] != capi.BS]
        assert new_nb
        R, _ = check_delete(P, Mx, new_nb, "appended columns after a solve")
        solve_and_certify(P, R, "appended columns after a solve, solved")


@pytest.mark.parametrize("seed", [3, 4])
def test_column_0_shift_on_a_general_root(gpu, seed):
    inst = gs.general_lp(9, 70, seed)
    P, M = gs.load(gpu, inst), gs.model(inst)
    P.simplex()
    _, nb, flag = P.basis()
    lo, hi = M.lo_hi()
    rests = {}
    for q in structural_positions(P):
        k, f = int(nb[q]), int(flag[q])
        rests[q] = {NL: lo[k - 1], NS: lo[k - 1], NU: hi[k - 1], NF: 0.0}[f]
    nonzero = [q for q, x in rests.items() if x != 0.0]
    zero = [q for q, x in rests.items() if x == 0.0]
    assert len(nonzero) >= 6 and zero
    positions = nonzero[::2][:8] + zero[:2]
    R, shifted = check_delete(P, M, cols_at(P, positions), "general root %d" % seed)
    assert shifted
    solve_and_certify(P, R, "general root %d, solved" % seed)


# ------------------------------------------------------------------------------------------------ 3. the solves that follow


def test_deleting_columns_at_zero_costs_no_pivot(gpu):
    P, M = dense(gpu, 20, 40, 8)
    before, z = P.it_cnt, P.obj
    s = structural_positions(P)
    R, shifted = check_delete(P, M, cols_at(P, s[::2]), "at zero")
    assert not shifted
    assert P.simplex() == 0 and P.status == OPT and P.it_cnt == before
    assert same_bits([P.obj], [z])
    cf.certify(R, P, what="at zero, solved")


def test_deleting_a_basic_column_gives_the_tableau_up(gpu):
    A, b, c = synth.dense_lp(10, 30, 13)
    P, M = dense(gpu, 10, 30, 13)
    first = P.it_cnt
    stat = P.col_stat()
    basic = next(j + 1 for j in range(30) if stat[j] == capi.BS)
    nonbasic = next(j + 1 for j in range(30) if stat[j] != capi.BS)
    assert P.del_cols([nonbasic, basic]) == 0 and P.n == 28 and P.status == UNDEF
    with pytest.raises(RuntimeError):
        P.tableau()
    assert P.simplex() == 0
    keep = [j for j in range(30) if j + 1 not in (basic, nonbasic)]
    F = gpu.create()
    F.load_dense(A[:, keep], b, c[keep])
    assert F.simplex() == 0
    assert (P.status, P.obj, P.it_cnt - first) == (F.status, F.obj, F.it_cnt)  # cold: the slack basis of the reduced model
    assert np.array_equal(P.tableau(), F.tableau())
    cf.certify(reduced(M, [basic, nonbasic]), P, what="basic column")


def test_pending_bound_edit_and_clones_survive_the_deletion(gpu):
    P, M = dense(gpu, 16, 40, 11)
    T0 = P.tableau()
    n = P.n
    stat, x = P.col_stat(), P.col_prim()
    j = next(j + 1 for j in range(n) if stat[j] == capi.BS and x[j] > 1.0)
    s = structural_positions(P)
    gone = cols_at(P, s[:12])  # 40 -> 28 columns: a relayout
    assert j not in gone and ld_of(n - len(gone)) == 32 and ld_of(n) == 64
    # a clone, a pending branching bound on a basic column, the deletion, the solve
    Q = P.copy()
    ub = float(np.floor(x[j - 1]))
    Q.api.set_col_bnds(Q.h, j, DB, 0.0, ub)
    assert Q.del_cols(gone) == 0 and Q.api.get_tableau_ld(Q.h) == 32
    assert Q.simplex() == 0
    Mq = M.copy()
    Mq.set_col_bnds(j, DB, 0.0, ub)
    Rq = reduced(Mq, gone)
    jq = j - sum(1 for g in gone if g < j)
    assert Rq.cols[jq - 1] == (DB, 0.0, ub)
    ref = cf.certify(Rq, Q, what="pending edit + deletion")
    assert float(ref.x[16 + jq - 1]) <= ub + 1e-9
    # the source of the clone is untouched by the deletion from the clone
    assert P.n == n and P.status == OPT and same_bits(P.tableau(), T0)
    before = P.it_cnt
    assert P.simplex() == 0 and P.it_cnt == before
    # a clone that is only recorded when the deletion moves its source: it receives the bits from before the deletion
    for cnt in (12, 1):  # with a relayout, and in place
        S_ = P.copy()
        R_ = S_.copy()
        assert S_.del_cols(gone[:cnt]) == 0 and S_.n == n - cnt
        assert R_.n == n and same_bits(R_.tableau(), T0)
        assert R_.simplex() == 0 and R_.status == OPT and R_.it_cnt == before
        assert S_.simplex() == 0
        cf.certify(reduced(M, gone[:cnt]), S_, what="source after the deletion")


# ------------------------------------------------------------------------------------------------ 4. column generation with purge


def test_column_generation_with_purge(gpu):
    A, b, c = synth.dense_lp(24, 96, 7)
    P = gpu.create()
    P.load_dense(A[:, :24], b, c[:24])
    assert P.simplex() == 0 and P.status == OPT
    order = list(range(24))
    rest = list(range(24, 96))
    while rest:
        rc, dj = P.price_cols(A[:, rest].T, c[rest])
        assert rc == 0
        pick = [i for i in np.argsort(-dj, kind="stable")[:8] if dj[i] > cf.TOL_DJ]
        if not pick:
            break
        take = [rest[i] for i in pick]
        assert P.add_dense_cols(A[:, take].T, c[take], [LO] * len(take), [0.0] * len(take), [0.0] * len(take)) == 0
        assert P.simplex() == 0 and P.status == OPT
        order += take
        rest = [j for j in rest if j not in take]
    assert rest and P.n == len(order) > 24
    before, z = P.it_cnt, P.obj
    gone = cols_at(P, structural_positions(P))
    assert gone and P.del_cols(gone) == 0 and P.n == len(order) - len(gone)
    assert P.simplex() == 0 and P.status == OPT and P.it_cnt == before  # no pivot
    assert same_bits([P.obj], [z])
    F = gpu.create()
    F.load_dense(A, b, c)
    assert F.simplex() == 0 and F.status == OPT
    assert abs(P.obj - F.obj) <= 1e-9 * abs(F.obj)
    left = [order[j] for j in range(len(order)) if j + 1 not in gone]
    cf.certify(cf.Model.dense(A[:, left], b, c[left]), P, what="column generation with purge")
    # and the loop goes on from the purged master: nothing outside prices out, the purged columns included
    outside = [j for j in range(96) if j not in left]
    rc, dj = P.price_cols(A[:, outside].T, c[outside])
    assert rc == 0 and not (dj > cf.TOL_DJ).any()


# ------------------------------------------------------------------------------------------------ 5. refusals


def test_refusals_leave_the_live_handle_alone(gpu):
    P, _ = dense(gpu, 10, 30, 13)
    T0 = P.tableau()
    basis0 = P.basis()
    n = P.n

    def call(ncs, nums, null=False):
        num = np.array([0] + list(nums), dtype=np.int32)
        return gpu.del_cols(P.h, ncs, None if null else num.ctypes.data_as(IP))

    for r in (dict(ncs=1, nums=[1], null=True), dict(ncs=0, nums=[1]), dict(ncs=1, nums=[0]), dict(ncs=1, nums=[n + 1]), dict(ncs=2, nums=[5, 5]),
              dict(ncs=n, nums=list(range(1, n + 1)))):
        assert call(**r) == -1, r
        assert P.n == n and P.status == OPT and same_bits(P.tableau(), T0), r
        assert all(np.array_equal(a, b) for a, b in zip(P.basis(), basis0)), r
    assert call(1, cols_at(P, structural_positions(P)[:1])) == 0 and P.n == n - 1
