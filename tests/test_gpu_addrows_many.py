"""GPU: row append across handles (DESIGN.md "Row append across handles (add_cut_rows_many)").  One mvx_add_cut_rows_many call
over a set of clones against mvx_add_cut_rows per handle on a second set and against the per-row path (add_rows, set_mat_row,
set_row_bnds) on the oracle's handles, before the next solve (model, status, basis, tableau, column values) and after it (status,
objective, pivots, tableau, solution).  Every comparison is bitwise.  The out-of-memory path (-2) is not provoked here."""
import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import BS, DB, FX, NU, OPT, UNDEF

from . import lpgen
from .test_gpu_cutloop import TILE, append_per_row, assert_same_unsolved, cut_like_rows
from .test_gpu_parity import assert_same_state

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def live_state(P):
    return (P.m, P.status, bits(P.tableau()).tolist(), [a.tolist() for a in P.basis()])


def solved_pair(gpu, orc, A, b, c):
    G, O = gpu.create(), orc.create()
    for P in (G, O):
        P.load_dense(A, b, c)
        assert P.simplex() == 0 and P.status == OPT
    return G, O


def many_vs_single(Gs, Os, rows, m0, what):
    """Gs[t] / Os[t]: the same handle on the device and on the oracle, rows[t] = (vals, rhs) what it is given (k_t = 0: nothing).
    Copies of them: one many-call, add_cut_rows per handle, the per-row path on the oracle.  m0: the rows of the common root.
    Returns the many-call's handles, solved."""
    many, single, orac = [G.copy() for G in Gs], [G.copy() for G in Gs], [O.copy() for O in Os]
    kept = [live_state(H) if len(r[1]) == 0 else None for H, r in zip(many, rows)]
    assert bnb.add_cut_rows_many(many, [r[0] for r in rows], [r[1] for r in rows]) == 0, what
    for t, (H, S, O, G, (vals, rhs)) in enumerate(zip(many, single, orac, Gs, rows)):
        w = "%s handle %d k=%d" % (what, t, len(rhs))
        if len(rhs) == 0:  # not touched at all: the status stays, and every bit
            assert H.status == G.status and live_state(H) == kept[t], w
            continue
        assert bnb.add_cut_rows(S, vals, rhs) == 0, w
        append_per_row(O, vals, rhs)
        assert H.m == G.m + len(rhs), w
        assert_same_unsolved(H, S, m0, w)
        assert_same_unsolved(H, O, m0, w + " (oracle)")
    for t, (H, S, O) in enumerate(zip(many, single, orac)):
        w = "%s handle %d solved" % (what, t)
        for P in (H, S, O):
            assert P.simplex() == 0, w
        assert_same_state(H, S, w)
        assert_same_state(H, O, w + " (oracle)")
    return many


@pytest.mark.parametrize("n1", [255, 256, 257])
@pytest.mark.parametrize("m", [63, 64, 65])
def test_many_equals_add_cut_rows_at_the_chunk_and_tile_edges(gpu, orc, m, n1):
    """m = 63 and 64 bring the trailing chunk of zero weights into the first and second single append; n + 1 = 255 .. 257 lies
    around the 256-column tile; k_t around the cut tile."""
    A, b, c = synth.dense_lp(m, n1 - 1, 11 + m + n1)
    G, O = solved_pair(gpu, orc, A, b, c)
    rng = np.random.default_rng(m * 1000 + n1)
    x = G.col_prim()
    ks = (1, 2, TILE, TILE + 1)
    many = many_vs_single([G] * len(ks), [O] * len(ks), [cut_like_rows(rng, x, k) for k in ks], m, "%dx%d" % (m, n1 - 1))
    assert all(H.it_cnt > G.it_cnt for H in many)  # the rows cut the vertex off: the dual simplex had work to do


def test_tile_boundaries_inside_and_between_handles(gpu, orc):
    """k_t = (1, 0, 8, 9, 2): tiles 0 | 1 | 2 3 | 4 of the launch; the handle without rows keeps MVX_OPT and its bits."""
    A, b, c = synth.dense_lp(40, 70, 21)
    G, O = solved_pair(gpu, orc, A, b, c)
    rng = np.random.default_rng(5)
    x = G.col_prim()
    ks = (1, 0, TILE, TILE + 1, 2)
    rows = [cut_like_rows(rng, x, k) if k else (np.zeros((0, G.n + 1)), np.zeros(0)) for k in ks]
    many = many_vs_single([G] * 5, [O] * 5, rows, G.m, "tiles")
    assert [H.m for H in many] == [G.m + k for k in ks]
    assert many[1].status == OPT and many[1].it_cnt == G.it_cnt


def carrying(G, O, rng, k, solve):
    """Copies of the solved pair that carry k cut rows, solved again or not (then the bounds of the last rows are pending)."""
    g, o = G.copy(), O.copy()
    vals, rhs = cut_like_rows(rng, G.col_prim(), k)
    assert bnb.add_cut_rows(g, vals, rhs) == 0
    append_per_row(o, vals, rhs)
    if solve:
        for P in (g, o):
            assert P.simplex() == 0 and P.status == OPT
    return g, o


def test_handles_of_different_row_counts_and_the_edit_overflow(gpu, orc):
    """Clones of one root of which two already carry 3 and 70 cut rows, the latter unsolved since its append: it holds MAX_EDITS = 8
    pending bound edits, and k_t = 9 overflows them twice -- older rows' bounds are launched, the new rows' are written by the
    kernel."""
    A, b, c = synth.dense_lp(70, 140, 5)
    G, O = solved_pair(gpu, orc, A, b, c)
    rng = np.random.default_rng(99)
    g3, o3 = carrying(G, O, rng, 3, True)
    g70, o70 = carrying(G, O, rng, 70, False)
    assert g70.status == UNDEF and (G.m, g3.m, g70.m) == (70, 73, 140)
    Gs, Os = [G, g3, g70, g70, g3], [O, o3, o70, o70, o3]
    ks = (2, TILE + 1, TILE + 1, 1, 3)
    rows = [cut_like_rows(rng, P.col_prim() if P.status == OPT else G.col_prim(), k) for P, k in zip(Gs, ks)]
    many_vs_single(Gs, Os, rows, 70, "row counts")


def test_a_handle_that_moves_to_a_larger_slab(gpu, orc):
    """A slab has 64 rows of slack and moves when fewer than 32 would stay spare: a handle that carries 30 appended rows and
    receives 5 moves inside the call, its neighbours stay.  Twice, the second time on recycled slabs."""
    A, b, c = synth.dense_lp(33, 90, 8)
    for again in range(2):
        G, O = solved_pair(gpu, orc, A, b, c)
        rng = np.random.default_rng(33 + again)
        g30, o30 = carrying(G, O, rng, 30, True)
        g30u, o30u = carrying(G, O, rng, 30, False)
        Gs, Os = [G, g30, G, g30u], [O, o30, O, o30u]
        rows = [cut_like_rows(rng, P.col_prim() if P.status == OPT else G.col_prim(), k) for P, k in zip(Gs, (3, 5, TILE + 1, 5))]
        many_vs_single(Gs, Os, rows, 33, "slab move pass %d" % again)
        del G, O, g30, o30, g30u, o30u, Gs, Os


def test_gmi_cuts_dealt_over_branched_clones(gpu, orc):
    """A dense_ilp root: columns non-basic at their upper bound give the new rows a value at the non-basic point (the fma chain of
    base[0]).  Four clones take one branching each on different basic columns (a pending bound edit, not solved) and are dealt the
    root's own repaired GMI cuts."""
    A, b, c, U = synth.dense_ilp(65, 130, 7, 3)
    G, O = lpgen.load_ilp(gpu, A, b, c, U), lpgen.load_ilp(orc, A, b, c, U)
    for P in (G, O):
        assert P.simplex() == 0 and P.status == OPT
    assert any(s == NU for s in G.col_stat())
    found = [(j, bnb.generate_cut_gmi(G, j)) for j in range(1, G.n + 1)]
    found = [(j, g) for j, g in found if g is not None]
    assert len(found) >= TILE + 1
    vals, rhs = np.array([g[0] for _, g in found]), np.array([g[1] for _, g in found])
    x = G.col_prim()
    Gs, Os = [], []
    for t in range(4):
        j = found[t][0]  # a basic integer column with a fractional value
        lo, hi = (0.0, float(np.floor(x[j - 1]))) if t % 2 == 0 else (float(np.ceil(x[j - 1])), float(U))
        pair = G.copy(), O.copy()
        for api, P in zip((gpu, orc), pair):
            api.set_col_bnds(P.h, j, DB if lo < hi else FX, lo, hi)
        Gs.append(pair[0])
        Os.append(pair[1])
    rows = [(vals[t::4], rhs[t::4]) for t in range(4)]
    assert sum(len(r[1]) for r in rows) == len(found)
    many_vs_single(Gs, Os, rows, G.m, "ilp")


def test_clones_around_the_call(gpu, orc):
    """A clone recorded immediately before the call keeps the old row count and the old bits (the recorded clones are flushed in
    front of the edit); a clone taken after equals the edited handle."""
    A, b, c = synth.dense_lp(24, 48, 13)
    G, O = solved_pair(gpu, orc, A, b, c)
    rng = np.random.default_rng(2)
    hs = [G.copy(), G.copy()]
    old = live_state(G)
    rows = [cut_like_rows(rng, G.col_prim(), k) for k in (3, TILE + 1)]
    before = [H.copy() for H in hs]  # recorded, not launched
    assert bnb.add_cut_rows_many(hs, [r[0] for r in rows], [r[1] for r in rows]) == 0
    after = [H.copy() for H in hs]
    for B in before:
        assert live_state(B) == old
    for H, Af, (vals, rhs) in zip(hs, after, rows):
        o = O.copy()
        append_per_row(o, vals, rhs)
        assert_same_unsolved(Af, H, 24, "clone after")
        assert_same_unsolved(Af, o, 24, "clone after (oracle)")
        for P in (H, Af, o):
            assert P.simplex() == 0
        assert_same_state(Af, H, "clone after, solved")
        assert_same_state(Af, o, "clone after, solved (oracle)")
    for B in before:
        assert B.simplex() == 0
        assert_same_state(B, G, "clone before, solved")


def test_130_handles_with_one_row_each(gpu, orc):
    """The handle search of a workgroup runs over 130 descriptors; every handle has its own row."""
    A, b, c = synth.dense_lp(12, 20, 4)
    G, O = solved_pair(gpu, orc, A, b, c)
    rng = np.random.default_rng(130)
    x = G.col_prim()
    many_vs_single([G] * 130, [O] * 130, [cut_like_rows(rng, x, 1) for _ in range(130)], 12, "130 handles")


def test_refusals_on_live_handles_change_nothing(gpu):
    A, b, c = synth.dense_lp(20, 40, 2)
    G = gpu.create()
    G.load_dense(A, b, c)
    assert G.simplex() == 0 and G.status == OPT
    rng = np.random.default_rng(1)
    x = G.col_prim()
    hs = [G.copy() for _ in range(3)]
    twin = G.copy()
    first = cut_like_rows(rng, x, 2)  # hs[0] carries two pending bound edits through the refusals, as its twin does not
    assert bnb.add_cut_rows(hs[0], *first) == 0 and bnb.add_cut_rows(twin, *first) == 0
    gone = G.copy()
    stat = gone.row_stat()
    nonbasic = [i + 1 for i in range(gone.m) if stat[i] != BS]
    assert nonbasic and gone.del_rows([nonbasic[0]]) == 0  # a non-basic row leaves: the tableau is given up
    with pytest.raises(RuntimeError):
        gone.tableau()
    before = [live_state(H) for H in hs]

    def untouched():
        return [live_state(H) for H in hs] == before and gone.m == G.m - 1 and gone.status == UNDEF

    n1 = G.n + 1
    rows = [cut_like_rows(rng, x, k) for k in (1, 2, 1)]
    vals, rhs = [r[0] for r in rows], [r[1] for r in rows]
    nan_v = [v.copy() for v in vals]
    nan_v[2][0, 17] = np.nan
    nan_r = [r.copy() for r in rhs]
    nan_r[2][0] = np.nan
    assert bnb.add_cut_rows_many(hs, nan_v, rhs) == -1 and untouched()  # the last handle's rows are checked before the first is edited
    assert bnb.add_cut_rows_many(hs, vals, nan_r) == -1 and untouched()
    assert bnb.add_cut_rows_many([hs[0], hs[1], hs[0]], vals, rhs) == -1 and untouched()  # a handle listed twice
    L, C = bnb.lib(), bnb.C
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    arr = (C.c_void_p * 3)(*[H.h for H in hs])
    flat_v, flat_r = np.ascontiguousarray(np.concatenate(vals)), np.ascontiguousarray(np.concatenate(rhs))
    for off in ([0, 3, 1, 4], [1, 1, 3, 4]):  # descending; off[0] is not 0
        o = np.array(off, dtype=np.int32)
        assert L.mvx_add_cut_rows_many(arr, 3, o.ctypes.data_as(IP), flat_v.ctypes.data_as(DP), flat_r.ctypes.data_as(DP)) == -1 and untouched(), off
    # a handle whose tableau was given up, to which mvx_add_cut_rows itself returns -1, refuses the whole call ...
    one_v, one_r = cut_like_rows(rng, x, 1)
    assert bnb.add_cut_rows(gone, one_v, one_r) == -1
    assert bnb.add_cut_rows_many([hs[1], gone, hs[2]], [vals[1], one_v, vals[2]], [rhs[1], one_r, rhs[2]]) == -1 and untouched()
    # ... unless it is given nothing
    empty = np.zeros((0, n1)), np.zeros(0)
    assert bnb.add_cut_rows_many([hs[1], gone], [vals[1], empty[0]], [rhs[1], empty[1]]) == 0
    assert hs[1].m == G.m + 2 and gone.m == G.m - 1 and live_state(hs[0]) == before[0] and live_state(hs[2]) == before[2]
    # the pending edits of hs[0] are still there: its next solve is its twin's
    for P in (hs[0], twin):
        assert P.simplex() == 0
    assert_same_state(hs[0], twin, "behind the refusals")
    assert hs[0].it_cnt > G.it_cnt
