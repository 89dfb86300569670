"""Schedules of live tableau edits (DESIGN.md "Live edits"): a committed list of edit sequences, the bookkeeping that walks one
without an engine, and the checks that hold a handle to it after every step.  No tests in here: tests/test_edit_schedules_inputs.py
proves on the oracle and the reference of tests/certify.py that the schedules have the properties the GPU file relies on,
tests/test_gpu_edit_schedules.py walks them on the engine.

A step edits three things together: the handle P (when there is one), a certify.Model M and the expected basis (head, nb,
flag).  Warm edits never change the basis, so the expected basis follows from the optimal basis of the base by renumbering alone
and the whole walk is a function of constants: the targets of a step are picked from the expected state (the rows whose
auxiliaries are basic, the non-basic structurals that rest off zero, ...) by index, its numbers are drawn from a fixed seed and
the reference vertex, and a target that is not there is an assertion, never a skip.

Step specs (tuples; indices pick from ascending lists of the expected state, negative ones from the end):

    ("R+", k, seed)                 k slack rows, one mvx_add_cut_rows call
    ("R+1", seed)                   add_rows(1) + set_mat_row + set_row_bnds
    ("R+m", k, ks, seed)            mvx_add_cut_rows_many over the handle (k rows) and a sibling clone with one row more (ks rows)
    ("R-", sel)                     del_rows of basic rows; sel: indices into basic_rows, or ("last", count)
    ("R-m", sel, sel_s, seed)       mvx_del_rows_many over the handle and a sibling clone with two rows more
    ("C+", k, seed)                 add_dense_cols, types cycling through DB / LO / UP / FX, all resting off zero
    ("C-", off, zero)               del_cols of non-basic structurals: indices into those resting off zero / at zero
    ("Bn", "col" | "row", i, type)  a bound of a non-basic variable that moves its resting value
    ("Bb", [("col" | "row", i, "cut" | "loose"), ...])  bounds of basic variables: pending edits
    ("O", ib, inb)                  set_obj_coef of a basic and of a non-basic column
    ("K", "source" | "clone")       copy; the walk goes on with the one named, the other waits for the end
    ("Cx", i) / ("Rx", i)           give-up: del_cols of a basic column / del_rows of a row whose auxiliary is non-basic
"""
import bisect
import collections

import numpy as np

from mvolps_amd import bnb, synth
from mvolps_amd.capi import BV, DB, FR, FX, IV, LO, NF, NL, NS, NU, OPT, UNDEF, UP

from . import certify as cf

DBL_MAX = np.finfo(np.float64).max
ROW_SLACK, ROW_SPARE, MAX_EDITS = 64, 32, 8  # mvx_internal.hpp
PAIR_KINDS = ("R+", "R-", "C+", "C-", "Bn", "Bb")
PLACED_KINDS = ("R+1", "R+m", "R-m", "O", "K")
SENSITIVITY = 1e-8  # RTOL * growth * (1 + max|T_ref|) stays below this: an entry off by 1e-7 fails (tests/certify.py)
MOVE = 1e-6  # a step that claims to move column 0 moves a basic value and the objective by more than this

# name -> (m, n, seed) of synth.dense_lp.  A: the stride goes 32 <-> 64 at n = 31 / 32.  B: n + 1 = 65, one full 64-column tile and a
# ragged one for k_cutrows, k_delrows and k_delcols, and the stride goes 96 <-> 64 at n = 63 / 64.
# The slack rows of draw_rows have entries of 1..7 in every column, so their row sums enter the growth of the reference with the
# column count: over 64 columns two of them already put RTOL * growth * (1 + max|T|) at 1e-8 and more (40 row seeds on 200 bases
# of 3..16 rows), over 30 columns thirty-three of them do.  So base B meets k_cutrows at its full width with one row (pairs-4),
# takes its other appended rows behind NARROW, and both bases take the long append of the capacity growth on a handful of columns.
# The seeds of the appends are the first of seed, seed + 100, ... that keep every step below SENSITIVITY.
BASES = {"A": (12, 30, 21), "B": (8, 64, 2)}

STD_FLAG = {FR: NF, LO: NL, UP: NU, DB: NL, FX: NS}
COL_TYPES = [(DB, -1.0, 1.0), (LO, 0.5, 0.0), (UP, 0.0, -1.25), (FX, 2.0, 2.0)]

# nine distinct basic variables: with the bounds that appended rows leave pending, more than MAX_EDITS
NINE = {"A": [("col", i, "loose") for i in range(4)] + [("row", i, "loose") for i in range(4)] + [("row", -1, "cut")],
        "B": [("col", i, "loose") for i in range(6)] + [("row", i, "loose") for i in range(2)] + [("row", -1, "cut")]}
NARROW = [("C+", 4, 46), ("C-", [0, 1, 2, 3], ("last", 34))]  # base B down to 30 columns: the stride goes 96 -> 32
GROW = ROW_SLACK - ROW_SPARE + 1  # rows in one append that the spare rows of a fresh slab cannot take

THREE = [("row", -2, "loose"), ("row", -1, "cut"), ("col", 0, "cut")]  # the last two appended rows and a column

SCHEDULES = {
    # every ordered pair of {R+, R-, C+, C-, Bn, Bb} as two adjacent steps, spread over four walks
    "pairs-1": ("A", [("R+", 2, 7), ("R+", 1, 8), ("R-", [-1]), ("R-", [0, -1]), ("C+", 4, 4), ("C+", 3, 5), ("C-", [0, 5], [0]),
                      ("C-", [0], []), ("Bn", "col", 0, LO), ("Bn", "row", 0, DB), ("Bb", [("col", 0, "cut")]),
                      ("Bb", [("row", -1, "cut")])]),
    "pairs-2": ("B", NARROW + [("R+", 2, 9), ("C+", 4, 6), ("R+", 1, 10), ("C-", [1, 2], [3]), ("R+", 1, 11), ("Bn", "col", 2, FX),
                               ("R+", 2, 612), ("Bb", [("row", -2, "cut"), ("col", 3, "loose")]), ("R+", 1, 213)]),
    "pairs-3": ("A", [("R+", 2, 314), ("C+", 4, 15), ("R-", [0]), ("C-", [0, 1], []), ("R-", [-1]), ("Bn", "col", 1, DB), ("R-", [1]),
                      ("Bb", [("row", -1, "loose"), ("col", 1, "cut")]), ("R-", [2]), ("R+", 2, 16)]),
    # base B at its full width: one appended row and its deletion over 65 columns, the stride down to 64 and up again
    "pairs-4": ("B", [("R+", 1, 147), ("R-", [-1]), ("C+", 4, 17), ("Bn", "row", 1, UP), ("C-", [0, 3], ("last", 6)), ("C+", 5, 18),
                      ("Bb", [("col", 2, "cut")]), ("C-", [1], []), ("Bb", [("col", 4, "loose")]), ("Bn", "col", 0, UP), ("C+", 2, 19),
                      ("Bb", [("col", 0, "cut")]), ("C+", 1, 20)]),
    # R+1, R+m, R-m, O and K directly behind a column edit and directly in front of a compaction
    "placed-1": ("A", [("R+", 2, 122), ("C+", 4, 23), ("R+1", 24), ("R-", [0, -1]), ("C-", [0], []), ("R+m", 1, 2, 25), ("R-", [-2]),
                       ("C+", 2, 26), ("K", "source"), ("C-", [0, 2], [0])]),
    "placed-2": ("B", NARROW + [("R+", 3, 127), ("C+", 4, 28), ("R-m", [0, -1], [-2], 29), ("C-", [0], [0]), ("C+", 4, 30), ("O", 0, 0),
                                ("R-", [-1]), ("C-", [1, 2], []), ("K", "clone"), ("R-", [0, 1])]),
    # a pending edit dropped with its row and another renumbered; the ninth pending edit; the row capacity grown under pending edits.
    # The long append comes behind a deletion of all but two of the non-basic columns (see BASES)
    "pending-A": ("A", [("C+", 4, 44), ("C-", [0, 1, 2, 3], ("last", 24)), ("R+", 3, 31), ("Bb", THREE), ("R-", [-3, -2]),
                        ("Bb", NINE["A"]), ("R+", GROW, 332), ("R-", ("last", GROW)), ("C+", 4, 33), ("Bn", "col", 0, LO)]),
    "pending-B": ("B", [("C+", 4, 45), ("C-", [0, 1, 2, 3], ("last", 56)), ("R+", 3, 34), ("Bb", THREE), ("R-", [-3, -2]),
                        ("Bb", NINE["B"]), ("R+", GROW, 35), ("C+", 4, 36), ("R-", ("last", GROW - 2)), ("C-", [0, 1, 2, 3], [])]),
    # the tableau given up under a pending edit, model-only edits behind it
    "give-up-col": ("A", [("R+", 2, 37), ("Bb", [("row", -1, "cut"), ("col", 0, "loose")]), ("C+", 4, 38), ("Cx", 1), ("R+1", 39),
                          ("C+", 4, 40), ("C-", [0, 4], [0]), ("Bn", "col", 2, DB)]),
    "give-up-row": ("B", NARROW + [("R+", 2, 141), ("Bb", [("col", 1, "cut")]), ("Bn", "col", 0, LO), ("Rx", 0), ("R+1", 42),
                                   ("C+", 4, 43), ("C-", [1], [2]), ("Bn", "col", 5, FX)]),
}
MODES = ("quiet", "reads")


def ld_of(n):
    return (n + 1 + 31) // 32 * 32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def base_lp(name):
    m, n, seed = BASES[name]
    return synth.dense_lp(m, n, seed)


def solved_base(api, name):
    A, b, c = base_lp(name)
    P = api.create()
    P.load_dense(A, b, c)
    assert P.simplex() == 0 and P.status == OPT
    return P, cf.Model.dense(A, b, c)


# ------------------------------------------------------------------------------------------------ the expected state


class State:
    """A certify model, the expected basis, and whether the handle still has a tableau / has been edited since its solve."""

    def __init__(self, M, basis, valid=True, edited=False):
        self.M = M
        self.head, self.nb, self.flag = (np.array(a, dtype=np.int32) for a in basis)
        self.valid, self.edited = valid, edited

    def copy(self):
        return State(self.M.copy(), self.basis(), self.valid, self.edited)

    def basis(self):
        return self.head, self.nb, self.flag

    def ref(self):
        return cf.Ref(self.M, self.basis())

    # ascending lists the specs index into
    def basic_rows(self):
        m = self.M.m
        return sorted(int(k) for k in self.head[1:] if k <= m)

    def nonbasic_rows(self):
        m = self.M.m
        return sorted(int(k) for k in self.nb[1:] if k <= m)

    def basic_cols(self):
        m = self.M.m
        return sorted(int(k) - m for k in self.head[1:] if k > m)

    def nonbasic_cols(self):
        m = self.M.m
        return sorted(int(k) - m for k in self.nb[1:] if k > m)

    def rest(self, k):
        """The resting value of the non-basic variable k."""
        q = int(np.nonzero(self.nb == k)[0][0])
        lo, hi = self.M.lo_hi()
        return {NL: lo[k - 1], NS: lo[k - 1], NU: hi[k - 1], NF: 0.0}[int(self.flag[q])]

    def tableau_row(self, k):
        return int(np.nonzero(self.head == k)[0][0])

    def slack_basis(self):
        m, n = self.M.m, self.M.n
        self.head = np.arange(m + 1, dtype=np.int32)
        self.nb = np.concatenate([[0], np.arange(m + 1, m + n + 1)]).astype(np.int32)
        self.flag = np.array([0] + [STD_FLAG[t] for t, _, _ in self.M.cols], dtype=np.int32)


def pick(lst, sel, what):
    if isinstance(sel, tuple) and sel[0] == "last":
        assert len(lst) >= sel[1], "%s: %d wanted, %d there" % (what, sel[1], len(lst))
        return lst[len(lst) - sel[1]:]
    out = []
    for i in sel:
        assert -len(lst) <= i < len(lst), "%s: index %d of %d" % (what, i, len(lst))
        out.append(lst[i])
    assert len(set(out)) == len(out), what
    return sorted(out)


# ------------------------------------------------------------------------------------------------ planning: spec -> concrete edit


def draw_rows(st, k, seed):
    """k MVX_LO rows the reference vertex satisfies with a slack of 5 (cut_rows of test_gpu_live_edits.py, the vertex from the
    reference so that nothing is read from the handle)."""
    n = st.M.n
    rng = np.random.default_rng(seed)
    x = st.ref().x[st.M.m:].astype(np.float64)
    vals = np.zeros((k, n + 1))
    vals[:, 1:] = -np.abs(np.round(rng.normal(size=(k, n)) * 2)) - 1.0
    rhs = vals[:, 1:] @ x - 5.0
    return vals, rhs


def plan_rows(st, kind, k, seed):
    vals, rhs = draw_rows(st, k, seed)
    return dict(kind=kind, vals=vals, rhs=rhs, front=st.M.m, moves=False)


def plan_del_rows(st, sel, what):
    rows = pick(st.basic_rows(), sel, what)  # rows whose auxiliaries are basic
    first = min(st.tableau_row(i) for i in rows)
    return dict(kind="R-", rows=rows, front=first - 1, moves=False)


def plan(st, spec):
    """The concrete edit of a spec on the state st (which is not changed); asserts the step's preconditions."""
    kind, what = spec[0], str(spec)
    m, n = st.M.m, st.M.n
    if kind == "R+":
        return plan_rows(st, "R+", spec[1], spec[2])
    if kind == "R+1":
        return plan_rows(st, "R+1", 1, spec[1])
    if kind == "R+m":
        _, k, ks, seed = spec
        op = plan_rows(st, "R+m", k, seed)
        sib = st.copy()
        op["sib_prep"] = plan_rows(sib, "R+", 1, seed + 1000)
        apply_model(sib, op["sib_prep"])
        op["sib_main"] = plan_rows(sib, "R+", ks, seed + 2000)
        assert sib.M.m != m and ks != k
        return op
    if kind == "R-":
        return plan_del_rows(st, spec[1], what)
    if kind == "R-m":
        _, sel, sel_s, seed = spec
        op = plan_del_rows(st, sel, what)
        op["kind"] = "R-m"
        sib = st.copy()
        op["sib_prep"] = plan_rows(sib, "R+", 2, seed)
        apply_model(sib, op["sib_prep"])
        op["sib_main"] = plan_del_rows(sib, sel_s, what)
        assert op["sib_main"]["rows"] != op["rows"]
        return op
    if kind == "C+":
        _, k, seed = spec
        rng = np.random.default_rng(seed)
        cols = np.round(rng.random((k, m)) * 4.0) / 4.0 + 0.25
        for t in range(k):  # a column without a lower bound enters the rows with the other sign, so that the LP stays bounded
            if COL_TYPES[t % len(COL_TYPES)][0] == UP:
                cols[t] = -cols[t]
        obj = np.round(rng.random(k) * 8.0) / 8.0
        types = [COL_TYPES[t % len(COL_TYPES)] for t in range(k)]
        rests = [{NL: l, NS: l, NU: u, NF: 0.0}[STD_FLAG[ty]] for ty, l, u in types]
        assert any(x != 0.0 for x in rests)
        moved = m + n + 1 + next(t for t, x in enumerate(rests) if x != 0.0)
        return dict(kind="C+", cols=cols, obj=obj, types=types, front=0, moves=True, moved=moved)
    if kind == "C-":
        _, off, zero = spec
        nbc = st.nonbasic_cols()
        off_zero = [j for j in nbc if st.rest(m + j) != 0.0]
        at_zero = [j for j in nbc if st.rest(m + j) == 0.0]
        cols = sorted(list(pick(off_zero, off, what + " off zero")) + list(pick(at_zero, zero, what + " at zero")))
        assert off, what  # at least one resting off zero
        assert len(cols) < n
        return dict(kind="C-", cols=cols, front=0, moves=True)
    if kind == "Bn":
        _, side, i, ty = spec
        if side == "col":
            j = pick(st.nonbasic_cols(), [i], what)[0]
            k = m + j
        else:
            j = pick(st.nonbasic_rows(), [i], what)[0]
            k = j
        q = int(np.nonzero(st.nb == k)[0][0])
        x0, f0 = float(st.rest(k)), int(st.flag[q])
        if ty == LO:
            bnds, f1, x1 = (LO, x0 + 0.5, 0.0), NL, x0 + 0.5
        elif ty == UP:
            bnds, f1, x1 = (UP, 0.0, x0 - 0.5), NU, x0 - 0.5
        elif ty == DB and f0 == NU:
            bnds, f1, x1 = (DB, x0 - 3.0, x0 - 0.25), NU, x0 - 0.25
        elif ty == DB:
            bnds, f1, x1 = (DB, x0 + 0.25, x0 + 3.0), NL, x0 + 0.25
        elif ty == FX:
            bnds, f1, x1 = (FX, x0 + 0.75, x0 + 0.75), NS, x0 + 0.75
        else:
            bnds, f1, x1 = (FR, 0.0, 0.0), NF, 0.0
        assert x1 != x0, what  # chosen so that the resting value changes
        return dict(kind="Bn", side=side, j=j, bnds=bnds, q=q, flag=f1, front=0, moves=True, moved=k)
    if kind == "Bb":
        ref = st.ref()
        edits = []
        for side, i, style in spec[1]:
            if side == "col":
                j = pick(st.basic_cols(), [i], what)[0]
                v = float(ref.x[m + j - 1])
                ty, lb, ub = st.M.cols[j - 1]
                assert ty in (LO, DB), what
                new = (DB, lb, lb + 0.75 * (v - lb)) if (style == "cut" and v > lb + 0.1) else (DB, lb, max(v, lb) + 1.0)
            else:
                j = pick(st.basic_rows(), [i], what)[0]
                a = float(ref.x[j - 1])
                ty, lb, ub = st.M.rows[j - 1]
                assert ty in (LO, UP), what
                d = 0.25 if style == "cut" else -1.0
                new = (LO, a + d, 0.0) if ty == LO else (UP, 0.0, a - d)
            edits.append((side, j, new))
        assert len({(s, j) for s, j, _ in edits}) == len(edits), what
        return dict(kind="Bb", edits=edits, front=m, moves=False)
    if kind == "O":
        _, ib, inb = spec
        jb, jn = pick(st.basic_cols(), [ib], what)[0], pick(st.nonbasic_cols(), [inb], what)[0]
        return dict(kind="O", coefs=[(jb, float(st.M.c[jb - 1]) * 1.25 + 0.125), (jn, float(st.M.c[jn - 1]) - 0.25)], front=m, moves=False)
    if kind == "K":
        return dict(kind="K", go_on=spec[1], front=m, moves=False)
    if kind == "Cx":
        assert st.valid
        return dict(kind="Cx", cols=[pick(st.basic_cols(), [spec[1]], what)[0]], front=0, moves=False)
    if kind == "Rx":
        assert st.valid
        return dict(kind="Rx", rows=[pick(st.nonbasic_rows(), [spec[1]], what)[0]], front=0, moves=False)
    raise AssertionError("unknown step %r" % (spec,))


# ------------------------------------------------------------------------------------------------ the bookkeeping


def reduced_cols(M, cols):
    idx = sorted(j - 1 for j in cols)
    M.A = np.delete(M.A, idx, axis=1)
    M.c = np.delete(M.c, idx)
    M.cols = [b for j, b in enumerate(M.cols) if j not in idx]
    M.kinds = [k for j, k in enumerate(M.kinds) if j not in idx]


def reduced_rows(M, rows):
    idx = sorted(i - 1 for i in rows)
    M.A = np.delete(M.A, idx, axis=0)
    M.rows = [b for i, b in enumerate(M.rows) if i not in idx]


def apply_model(st, op):
    """The edit on the model and the expected basis (mvx.h: the renumbering of mvx_del_rows and mvx_del_cols)."""
    kind = op["kind"]
    M = st.M
    m, n = M.m, M.n
    if kind == "K":
        return
    st.edited = True
    if kind in ("R+", "R+1", "R+m"):
        k = len(op["rhs"])
        for t in range(k):
            M.add_row(op["vals"][t, 1:], LO, float(op["rhs"][t]), 0.0)
        st.head = np.concatenate([np.where(st.head > m, st.head + k, st.head), np.arange(m + 1, m + k + 1)]).astype(np.int32)
        st.nb = np.where(st.nb > m, st.nb + k, st.nb).astype(np.int32)
    elif kind in ("R-", "R-m", "Rx"):
        rows = op["rows"]
        nrs = len(rows)
        reduced_rows(M, rows)
        if kind == "Rx":
            st.valid = False
        if not st.valid:
            return st.slack_basis()

        def ren(k):
            return k - nrs if k > m else k - bisect.bisect_left(rows, k)

        st.head = np.array([0] + [ren(int(k)) for k in st.head[1:] if int(k) not in rows], dtype=np.int32)
        st.nb = np.array([0] + [ren(int(k)) for k in st.nb[1:]], dtype=np.int32)
    elif kind == "C+":
        k = len(op["obj"])
        for t, (ty, l, u) in enumerate(op["types"]):
            M.add_col(op["cols"][t], ty, l, u, cost=float(op["obj"][t]))
        st.nb = np.concatenate([st.nb, np.arange(m + n + 1, m + n + k + 1)]).astype(np.int32)
        st.flag = np.concatenate([st.flag, [STD_FLAG[ty] for ty, _, _ in op["types"]]]).astype(np.int32)
    elif kind in ("C-", "Cx"):
        cols = op["cols"]
        reduced_cols(M, cols)
        if kind == "Cx":
            st.valid = False
        if not st.valid:
            return st.slack_basis()

        def ren(k):
            return k if k <= m else k - bisect.bisect_left(cols, k - m)

        keep = [q for q in range(1, n + 1) if int(st.nb[q]) - m not in cols]
        st.head = np.array([0] + [ren(int(k)) for k in st.head[1:]], dtype=np.int32)
        st.nb = np.array([0] + [ren(int(st.nb[q])) for q in keep], dtype=np.int32)
        st.flag = np.array([0] + [int(st.flag[q]) for q in keep], dtype=np.int32)
    elif kind == "Bn":
        (M.set_col_bnds if op["side"] == "col" else M.set_row_bnds)(op["j"], *op["bnds"])
        st.flag[op["q"]] = op["flag"]
    elif kind == "Bb":
        for side, j, new in op["edits"]:
            (M.set_col_bnds if side == "col" else M.set_row_bnds)(j, *new)
    elif kind == "O":
        for j, v in op["coefs"]:
            M.c[j - 1] = v
    else:
        raise AssertionError(kind)
    if not st.valid and kind in ("R+", "R+1", "C+", "Bn"):
        st.slack_basis()


# ------------------------------------------------------------------------------------------------ the handle


def all_indices(n):
    return np.arange(n + 1, dtype=np.int32)


def apply_handle(P, op):
    """The edit on the handle alone (siblings and clones are the walker's)."""
    kind, api = op["kind"], P.api
    if kind in ("R+", "R+m"):
        assert bnb.add_cut_rows(P, op["vals"], op["rhs"]) == 0
    elif kind == "R+1":
        r = api.add_rows(P.h, 1)
        P.set_mat_row(r, all_indices(P.n), op["vals"][0])
        api.set_row_bnds(P.h, r, LO, float(op["rhs"][0]), 0.0)
    elif kind in ("R-", "R-m", "Rx"):
        assert P.del_rows(op["rows"]) == 0
    elif kind == "C+":
        ty = op["types"]
        assert P.add_dense_cols(op["cols"], op["obj"], [t for t, _, _ in ty], [l for _, l, _ in ty], [u for _, _, u in ty]) == 0
    elif kind in ("C-", "Cx"):
        assert P.del_cols(op["cols"]) == 0
    elif kind == "Bn":
        (api.set_col_bnds if op["side"] == "col" else api.set_row_bnds)(P.h, op["j"], *op["bnds"])
    elif kind == "Bb":
        for side, j, new in op["edits"]:
            (api.set_col_bnds if side == "col" else api.set_row_bnds)(P.h, j, *new)
    elif kind == "O":
        for j, v in op["coefs"]:
            api.set_obj_coef(P.h, j, v)
    else:
        raise AssertionError(kind)


def check_model(P, M, what):
    """The handle's model equals M, accessor by accessor and bit for bit."""
    api, h = P.api, P.h
    m, n = M.m, M.n
    assert (P.m, P.n) == (m, n), what

    def ext(v):
        return -DBL_MAX if v == -np.inf else DBL_MAX if v == np.inf else v

    for i in range(1, m + 1):
        ind, val = P.get_mat_row(i)
        row = np.zeros(n)
        row[ind - 1] = val
        assert same_bits(row, M.A[i - 1]), (what, "row", i)
        t, lb, ub = M.rows[i - 1]
        lo, hi = cf._bounds(t, lb, ub)
        assert api.get_row_type(h, i) == t, (what, "row type", i)
        assert same_bits([api.get_row_lb(h, i), api.get_row_ub(h, i)], [ext(lo), ext(hi)]), (what, "row bounds", i)
    for j in range(1, n + 1):
        t, lb, ub = M.cols[j - 1]
        lo, hi = cf._bounds(t, lb, ub)
        assert api.get_col_type(h, j) == t, (what, "column type", j)
        assert same_bits([api.get_col_lb(h, j), api.get_col_ub(h, j)], [ext(lo), ext(hi)]), (what, "column bounds", j)
        assert same_bits([api.get_obj_coef(h, j)], [M.c[j - 1]]), (what, "objective", j)
        kind = M.kinds[j - 1]
        assert api.get_col_kind(h, j) == (BV if (kind == IV and (t, lo, hi) == (DB, 0.0, 1.0)) else kind), (what, "kind", j)
    assert same_bits([api.get_obj_coef(h, 0)], [M.c0]), (what, "constant")
    assert api.get_obj_dir(h) == M.dir, what


def prim(P, k):
    return P.api.get_row_prim(P.h, k) if k <= P.m else P.api.get_col_prim(P.h, k - P.m)


def read_values(P, st, ref, op, what):
    """The reads of the `reads` mode, before the tableau is fetched: a variable basic in front of the edit, one at or behind it,
    the non-basic variable the step moved, the objective -- each against the reference -- then every value."""
    m = st.M.m
    front = op["front"]
    ks = []
    if front >= 1:
        ks.append(("front", int(st.head[front])))
    if front < m:
        ks.append(("behind", int(st.head[front + 1])))
    if op.get("moved"):
        ks.append(("moved", op["moved"]))
    for name, k in ks:
        got, want = prim(P, k), ref.x[k - 1]
        assert abs(float(np.longdouble(got) - want)) <= ref.tol(want), \
            "%s: %s variable %d reads %.17g, reference %.17g" % (what, name, k, got, float(want))
    z = P.obj
    assert abs(float(np.longdouble(z) - ref.z)) <= ref.tol(ref.z), "%s: objective reads %.17g, reference %.17g" % (what, z, float(ref.z))
    S = cf.Snapshot(P)
    cf.certify_values(ref, S, what)
    return S


def check_handle(P, st, op, mode, what):
    """What every step must leave (the issue's list), against Ref(M, expected basis)."""
    if not st.valid:
        check_model(P, st.M, what)
        assert P.status == UNDEF, what
        try:
            P.tableau()
        except RuntimeError:
            return
        raise AssertionError("%s: the handle still reports a tableau" % what)
    ref = st.ref()
    S = read_values(P, st, ref, op, what) if mode == "reads" else None
    assert (P.m, P.n) == (st.M.m, st.M.n), what
    assert P.api.get_tableau_ld(P.h) == ld_of(st.M.n), what
    assert P.status == (UNDEF if st.edited else OPT), what
    for got, want, name in zip(P.basis(), st.basis(), ("head", "nb", "flag")):
        assert np.array_equal(got, want), "%s: %s is %s, expected %s" % (what, name, got.tolist(), want.tolist())
    check_model(P, st.M, what)
    assert cf.certify_tableau(ref, S.tab if S is not None else P.tableau(), what) <= 1.0


class Walker:
    """Walks a schedule: on the bookkeeping alone (P None), or on a handle that is checked after every step."""

    def __init__(self, st, P=None, mode="quiet", name="", counts=None):
        self.st, self.P, self.mode, self.name = st, P, mode, name
        self.kept = []  # (what, handle or None, state): clones and siblings, as they were when last touched
        self.counts = counts if counts is not None else collections.Counter()
        self.nstep = 0

    def step(self, spec):
        """One step; returns (op, the reference before it or None, the state afterwards)."""
        st, P = self.st, self.P
        self.nstep += 1
        what = "%s/%s step %d %s" % (self.name, self.mode, self.nstep, spec[0])
        op = plan(st, spec)
        before = st.ref() if (op["moves"] and st.valid) else None
        kind = op["kind"]
        if kind == "K":
            other = st.copy()
            Q = P.copy() if P is not None else None
            if op["go_on"] == "source":
                self.kept.append((what + " clone", Q, other))
            else:
                self.kept.append((what + " source", P, other))
                self.P = P = Q
        elif kind in ("R+m", "R-m"):
            sib = st.copy()
            S = P.copy() if P is not None else None
            if S is not None:
                apply_handle(S, op["sib_prep"])
            apply_model(sib, op["sib_prep"])
            if P is not None:
                if kind == "R+m":
                    assert bnb.add_cut_rows_many([P, S], [op["vals"], op["sib_main"]["vals"]], [op["rhs"], op["sib_main"]["rhs"]]) == 0
                else:
                    assert bnb.del_rows_many([P, S], [op["rows"], op["sib_main"]["rows"]]) == 0
            apply_model(sib, op["sib_main"])
            apply_model(st, op)
            if S is not None:
                check_handle(S, sib, op["sib_main"], self.mode, what + " sibling")
            self.kept.append((what + " sibling", S, sib))
        else:
            if P is not None:
                apply_handle(P, op)
            apply_model(st, op)
            if P is not None and kind in ("Cx", "Rx"):
                self.gave_up(what)
        if P is not None:
            check_handle(P, st, op, self.mode, what)
            self.counts[(spec[0], self.mode)] += 1
        return op, before, st

    def gave_up(self, what):
        """The handle reports no tableau, and mvx_add_cut_rows refuses and changes nothing."""
        P, st = self.P, self.st
        n = P.n
        vals = np.zeros((1, n + 1))
        vals[0, 1:] = -1.0
        assert bnb.add_cut_rows(P, vals, np.array([-5.0])) == -1, what
        check_model(P, st.M, what + ", refused append")

    def finish(self):
        """The solve (every pending bound is applied or rejected against M), one forced tableau refresh (the tableau rebuilt from the
        handle's own model), and the handles that were left behind on the way."""
        P, st, api = self.P, self.st, self.P.api
        what = "%s/%s" % (self.name, self.mode)
        assert P.simplex() == 0, what
        cf.certify(st.M, P, status=OPT, what=what + " solved")
        api.set_refresh(8, 0.0)
        try:
            before = api.get_refresh_cnt(P.h)
            api.set_obj_coef(P.h, 0, st.M.c0)  # the status is unknown again: the next solve looks at the residual
            assert P.simplex() == 0, what
            assert api.get_refresh_cnt(P.h) > before, what
        finally:
            api.set_refresh(1024, 1e-9)
        check_model(P, st.M, what + " refreshed")
        cf.certify(st.M, P, status=OPT, what=what + " refreshed")
        self.counts[("end", self.mode)] += 1
        for kwhat, Q, sq in self.kept:
            for got, want in zip(Q.basis(), sq.basis()):
                assert np.array_equal(got, want), kwhat
            check_model(Q, sq.M, kwhat)
            assert cf.certify_tableau(sq.ref(), Q.tableau(), kwhat) <= 1.0
            assert Q.simplex() == 0, kwhat
            cf.certify(sq.M, Q, status=OPT, what=kwhat + " solved")
            self.counts[("kept", self.mode)] += 1


# ------------------------------------------------------------------------------------------------ the GMI case of the GPU file

GMI_CASE = (6, 10, 3, 2)  # one of test_gpu_certify.py's enumerated ILPs (synth.dense_ilp)


def gmi_rewrites(A, i):
    """The two rewrites of original row i (1-based) of the GMI test: different coefficients, the second is what the model keeps.
    Both keep the row's right-hand side meaningful (integer coefficients in 1..20, as synth.dense_ilp draws them)."""
    rng = np.random.default_rng(100 + i)
    n = A.shape[1]
    first = 1.0 + np.floor(rng.random(n) * 20.0)
    second = A[i - 1].copy()
    idx = rng.choice(n, size=max(2, n // 3), replace=False)
    second[idx] = 1.0 + np.floor(rng.random(len(idx)) * 20.0)
    second[idx[0]] = A[i - 1, idx[0]] + 3.0
    assert not np.array_equal(first, second) and not np.array_equal(second, A[i - 1])
    return first, second


def gmi_model(case=GMI_CASE):
    A, b, c, U = synth.dense_ilp(*case)
    return A, b, c, U, cf.Model.ilp(A, b, c, U)


def gmi_rewritten(M, i):
    """The model after the second rewrite of row i."""
    R = M.copy()
    R.A[i - 1] = gmi_rewrites(M.A, i)[1]
    return R


def cut_columns(ref):
    """The basic integer columns the repaired formula cuts (eligible of test_gpu_certify.py)."""
    m = ref.model.m
    return [int(k) - m for k in ref.head if k > m and cf.gmi_ref(ref, int(k) - m) is not None]


def row_feeds_a_cut(ref, i, cols=None):
    """Row i's auxiliary is non-basic and has a non-zero entry in the tableau row of a cut column (of `cols` when given): the
    back-substitution of that cut goes through the coefficients of model row i."""
    m = ref.model.m
    q = np.nonzero(ref.nb == i)[0]
    if not len(q):
        return False
    for j in cut_columns(ref) if cols is None else cols:
        r = int(np.nonzero(ref.head == m + j)[0][0])
        if abs(float(ref.T[r, q[0]])) > 1e-9:
            return True
    return False


GMI_ROWS = (1, 2, 4, 5)  # the original rows whose second rewrite has the property above (test_edit_schedules_inputs.py)
