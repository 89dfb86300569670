"""Node images (mvx_pack / mvx_pack_from / mvx_unpack, DESIGN.md "Distributed") in every state a handle can take: the bases, the
sender states and the one check that every state goes through.  No tests in here: tests/test_images_inputs.py proves on the oracle
and the reference of tests/certify.py that each (state, base) pair has the property its GPU test relies on,
tests/test_gpu_images.py sends the engine's handles through their images.

A state is built by a function of (api, base name): the same function builds it on the oracle and on the engine.  Where the engine
has a call the oracle lacks (mvx_add_cut_rows, mvx_del_rows, mvx_add_dense_cols, ...), `engine_only` says so; mvx_add_cut_rows has
an oracle spelling (k single appends, which the call is defined to equal), so that the CPU file can certify those senders too.

The check (`roundtrip`) talks to the library through a `Kit`: the function table, a buffer with guard bytes around the image, and
the calls that exist on one side only.  Every comparison in it is bitwise (`same_bits`), or is certify.py with its own tolerances."""
import ctypes as C

import numpy as np

from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import BS, DB, EITLIM, FR, FX, IV, LO, NOFEAS, OPT, UP

from . import certify as cf
from . import lpgen
from .thresholds import oracle_cut, same_bits

LD_ALIGN, ROW_SLACK, ROW_SPARE, MAX_EDITS = 32, 64, 32, 8  # mvx_internal.hpp
GUARD, IMAGE_ALIGN, PATTERN = 4096, 256, 0xA5
GROW = ROW_SLACK - ROW_SPARE + 1  # rows in one append that the spare rows of a fresh slab cannot take
GLPK_TOL = (1e-7, 1e-7, 1e-9)
DEFAULT_TOL = (1e-9, 1e-9, 1e-9)
REFRESH_DEFAULT = (1024, 1e-9)

# ------------------------------------------------------------------------------------------------ bases
# name -> ("ilp", (m, n, seed, U)) of synth.dense_ilp, or ("gen", seed) of lpgen.random_general_lp with every column integer.
# ilp-12x31: n + 1 is one ld unit exactly; ilp-8x64: n + 1 = 65, one column into a third unit.  The general seeds: 249 is the
# first with ranged rows, free, fixed and boxed columns and MVX_MIN together that gives every state listed for it below; 20604 is
# the first that leaves a free column non-basic at its optimum (beside one at its upper bound) and still gives two cuts, a child
# of two dual pivots and an infeasible child (a free non-basic column at an optimum needs a reduced cost of zero: it is rare).
BASES = {
    "ilp-12x31": ("ilp", (12, 31, 8, 3)),
    "ilp-24x48": ("ilp", (24, 48, 6, 2)),
    "ilp-8x64": ("ilp", (8, 64, 9, 3)),
    "gen-a": ("gen", 249),
    "gen-b": ("gen", 20604),
}
ILP_BASES = [b for b in BASES if BASES[b][0] == "ilp"]
GEN_BASES = [b for b in BASES if BASES[b][0] == "gen"]


def general_instance(seed):
    return lpgen.random_general_lp(np.random.default_rng(seed), 9, 10)


def load_base(api, name):
    """The base as a fresh, unsolved handle."""
    kind, arg = BASES[name]
    if kind == "ilp":
        return synth.load_ilp(api, *synth.dense_ilp(*arg))
    A, row_b, col_b, c, direction = general_instance(arg)
    P = api.create()
    P.load_general(A, row_b, col_b, c, kinds=[IV] * len(c), direction=direction)
    return P


def solved(api, name):
    """(root, P): the base and a copy of it solved to OPT."""
    root = load_base(api, name)
    P = root.copy()
    assert P.simplex() == 0 and P.status == OPT, name
    return root, P


def engine_only(api):
    return api.prefix == "mvx_"


# ------------------------------------------------------------------------------------------------ small edits


def col_bounds(P, j):
    api, h = P.api, P.h
    return api.get_col_type(h, j), api.get_col_lb(h, j), api.get_col_ub(h, j)


def as_bounds(lo, hi):
    """(type, lb, ub) of the interval [lo, hi] (+-inf where absent)."""
    if lo == -np.inf and hi == np.inf:
        return FR, 0.0, 0.0
    if hi == np.inf:
        return LO, float(lo), 0.0
    if lo == -np.inf:
        return UP, 0.0, float(hi)
    return (FX, float(lo), float(lo)) if lo == hi else (DB, float(lo), float(hi))


def interval(P, j):
    return cf._bounds(*col_bounds(P, j))


def basic_cols(P):
    stat = P.col_stat()
    return [j + 1 for j in range(len(stat)) if stat[j] == BS]


def cut_bound(P, j, x):
    """The bounds of a branch on basic column j with the value x that cuts the vertex off: down where the column's lower bound
    leaves room, else up."""
    lo, hi = interval(P, j)
    down = np.ceil(x) - 1.0
    if lo == -np.inf or down >= lo:
        return as_bounds(lo, down)
    return as_bounds(np.floor(x) + 1.0, hi)


def loose_bound(P, j, x):
    """Another upper bound for basic column j that its value x stays under: the edit is pending and costs no pivot."""
    lo, hi = interval(P, j)
    return as_bounds(lo, np.ceil(x) + 1.25 if hi == np.inf or np.ceil(x) + 1.25 != hi else np.ceil(x) + 2.25)


def set_col(P, j, bnds):
    P.api.set_col_bnds(P.h, j, *bnds)


def gmi(P, cols):
    """The repaired GMI cuts of the basic columns `cols`: (vals (k, n + 1), rhs, ok).  The engine's batched entry, the oracle's
    one-column restatement (test_gpu_gmi.py holds the two to the same bits wherever the oracle gives a cut)."""
    n, k = P.n, len(cols)
    vals, rhs, ok = np.zeros((k, n + 1)), np.zeros(k), np.zeros(k, dtype=np.int32)
    if not k:
        return vals, rhs, ok
    if engine_only(P.api):
        lib = P.api.lib
        arr = np.asarray(cols, dtype=np.int32)
        lib.mvx_gmi_cuts.restype = C.c_int
        lib.mvx_gmi_cuts.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        assert lib.mvx_gmi_cuts(P.h, 1, arr.ctypes.data, k, vals.ctypes.data, rhs.ctypes.data, ok.ctypes.data) == 0
        # the engine reports the free-non-basic rejection only; a fractional part within 1e-6 of an integer and an empty cut
        # are rejected on the host side of the driver (orc_generateCutGMI does both itself)
        for t, j in enumerate(cols):
            f0 = P.api.get_col_prim(P.h, j) - np.floor(P.api.get_col_prim(P.h, j))
            if f0 < 1e-6 or f0 > 1.0 - 1e-6 or not np.any(vals[t, 1:] != 0.0):
                ok[t] = 0
        return vals, rhs, ok
    for t, j in enumerate(cols):
        rc, v, lb = oracle_cut(P.api, P, j, 1)
        if rc == 0:
            vals[t], rhs[t], ok[t] = v, lb, 1
            vals[t, 0] = 0.0
    return vals, rhs, ok


def append_row(P, vals, lb):
    """cut.cpp:23-43: one >= row over every column."""
    r = P.api.add_rows(P.h, 1)
    P.set_mat_row(r, np.arange(P.n + 1, dtype=np.int32), vals)
    P.api.set_row_bnds(P.h, r, LO, float(lb), 0.0)


def add_cut_rows(P, vals, rhs):
    """mvx_add_cut_rows, or on the oracle the k single appends it is defined to equal."""
    if engine_only(P.api):
        assert bnb.add_cut_rows(P, vals, rhs) == 0
    else:
        for v, r in zip(vals, rhs):
            append_row(P, v, r)


def oracle_cuts(root_name, count, orc):
    """The first `count` repaired cuts the ORACLE gives at the optimum of the base: the rows of states 7 and 8 are constants of
    the base, the same on both sides, whichever side's formula is under test elsewhere."""
    _, O = solved(orc, root_name)
    vals, rhs, ok = gmi(O, basic_cols(O))
    pick = [t for t in range(len(ok)) if ok[t]][:count]
    assert len(pick) == count, (root_name, "cuts", len(pick))
    return vals[pick], rhs[pick]


def benign_rows(P, k, seed):
    """k loose MVX_LO rows over three columns each: -x_a - x_b - x_c >= -(what the columns' boxes allow) - 1 - t.  Never binding,
    entries of -1 in three places: nothing like the full-width slack rows that make the reference ill-conditioned."""
    n = P.n
    rng = np.random.default_rng(seed)
    vals = np.zeros((k, n + 1))
    rhs = np.zeros(k)
    for t in range(k):
        cols = rng.choice(n, size=3, replace=False) + 1
        vals[t, cols] = -1.0
        top = sum(interval(P, int(j))[1] for j in cols)
        assert np.isfinite(top)
        rhs[t] = -top - 1.0 - t
    return vals, rhs


# ------------------------------------------------------------------------------------------------ sender states


class Sender:
    """What a state hands to the check: the handles to pack, the base they are packed against (own_base: each handle is its own
    base, mvx_pack), the tolerances of the solve that left the state, and what to put back afterwards."""

    def __init__(self, root, handles, own_base=False, tol=DEFAULT_TOL, cleanup=None, tableau=True, extra=None):
        self.root, self.handles, self.steps, self.own_base, self.tol = root, handles, [], own_base, tol
        self.cleanup, self.tableau, self.extra = cleanup, tableau, extra or {}


# per base: the child of state 5 as column bounds (column, bounds); the pivot limits of state 6 as
# (primal limit, index into the basic columns for the dual leg's branch, dual limit).  Found on the oracle, asserted there.
NOFEAS_CHILD = {"ilp-12x31": [(j, (FX, 3.0, 3.0)) for j in (1, 2, 3)], "ilp-24x48": [(j, (FX, 2.0, 2.0)) for j in range(1, 9)],
                "ilp-8x64": [(j, (FX, 3.0, 3.0)) for j in range(1, 7)], "gen-a": [(1, (FX, 4.0, 4.0))], "gen-b": [(1, (FX, 6.0, 6.0))]}
IT_LIMITS = {"ilp-12x31": (10, 0, 1), "ilp-24x48": (12, 0, 1), "ilp-8x64": (14, 2, 3), "gen-a": (4, 0, 1), "gen-b": (2, 0, 1)}


def st_unsolved(api, base):
    root = load_base(api, base)
    P = root.copy()
    lo, hi = interval(P, 1)
    set_col(P, 1, as_bounds(lo + 1.0, hi))
    lo, hi = interval(P, P.n)
    set_col(P, P.n, as_bounds(lo, hi - 1.0))
    return Sender(root, [P], tableau=False)


def st_opt(api, base):
    root, P = solved(api, base)
    return Sender(root, [P])


def st_one_pending(api, base):
    root, P = solved(api, base)
    j = basic_cols(P)[0]
    set_col(P, j, cut_bound(P, j, P.api.get_col_prim(P.h, j)))
    return Sender(root, [P])


def st_nine_pending(api, base):
    root, P = solved(api, base)
    cols = basic_cols(P)
    assert len(cols) > MAX_EDITS, (base, len(cols))
    x = P.col_prim()
    edits = [(cols[0], cut_bound(P, cols[0], x[cols[0] - 1]))] + [(j, loose_bound(P, j, x[j - 1])) for j in cols[1:MAX_EDITS + 1]]
    for j, b in edits:
        set_col(P, j, b)
    return Sender(root, [P])


def st_nofeas(api, base):
    root, P = solved(api, base)
    for j, bnds in NOFEAS_CHILD[base]:
        set_col(P, j, bnds)
    assert P.simplex() == 0 and P.status == NOFEAS, (base, P.status)
    return Sender(root, [P])


def st_limit_primal(api, base):
    root = load_base(api, base)
    P = root.copy()
    assert P.simplex(it_lim=IT_LIMITS[base][0]) == EITLIM
    return Sender(root, [P])


def st_limit_dual(api, base):
    root, P = solved(api, base)
    _, i, lim = IT_LIMITS[base]
    j = basic_cols(P)[i]
    set_col(P, j, cut_bound(P, j, P.api.get_col_prim(P.h, j)))
    assert P.simplex(it_lim=lim) == EITLIM
    return Sender(root, [P])


def st_gmi_row(api, base, cuts):
    root, P = solved(api, base)
    append_row(P, cuts[0][0], cuts[1][0])
    return Sender(root, [P])


def st_gmi_rows_solved(api, base, cuts):
    root, P = solved(api, base)
    for v, r in zip(*cuts):
        append_row(P, v, r)
    assert P.simplex() == 0
    return Sender(root, [P])


def st_grown(api, base):
    root, P = solved(api, base)
    add_cut_rows(P, *benign_rows(P, GROW, 71))
    assert P.m > root.m + ROW_SLACK - ROW_SPARE
    return Sender(root, [P])


def st_many(api, base):
    root, P = solved(api, base)
    K1, K2 = P.copy(), P.copy()
    (v1, r1), (v2, r2) = benign_rows(P, 2, 72), benign_rows(P, 3, 73)
    if engine_only(api):
        assert bnb.add_cut_rows_many([K1, K2], [v1, v2], [r1, r2]) == 0
    else:
        add_cut_rows(K1, v1, r1)
        add_cut_rows(K2, v2, r2)
    return Sender(root, [K1, K2])


def st_deleted(api, base):
    """State 9, then the first, a middle and the last appended row leave (their auxiliaries are basic: the rows never bind)."""
    s = st_grown(api, base)
    P, m0 = s.handles[0], s.root.m
    assert P.del_rows([m0 + 1, m0 + GROW // 2, P.m]) == 0
    return Sender(s.root, [P])


def st_batch(api, base):
    root = load_base(api, base)
    P = root.copy()
    arr = (C.c_void_p * 1)(P.h)
    rcs = (C.c_int * 1)()
    assert api.simplex_batch(arr, 1, None, rcs) == 0 and rcs[0] == 0
    return Sender(root, [P])


def st_tolerances(api, base):
    root = load_base(api, base)
    P = root.copy()
    api.set_default_tolerances(*GLPK_TOL)
    try:
        assert P.simplex() == 0 and P.status == OPT
    finally:
        api.set_default_tolerances(*DEFAULT_TOL)
    return Sender(root, [P], tol=GLPK_TOL)


def st_refresh(api, base):
    """The primal solve of the base stopped after two thirds of its pivots, under a refresh countdown of one pivot more than that:
    the rest of the solve alone does not use it up (extra["stopped_at"]: the CPU file proves the rest is shorter), so only a handle
    that carries the count of the first leg looks at its residual when the solve is finished -- and, the tolerance being 0,
    rebuilds its tableau."""
    root, P = solved(api, base)
    stop = 2 * P.it_cnt // 3
    assert stop >= 2
    api.set_refresh(stop + 1, 0.0)
    try:
        P = root.copy()
        assert P.simplex(it_lim=stop) == EITLIM and P.it_cnt == stop
    except BaseException:
        api.set_refresh(*REFRESH_DEFAULT)
        raise
    return Sender(root, [P], cleanup=lambda: api.set_refresh(*REFRESH_DEFAULT), extra=dict(refreshes=1, stopped_at=stop))


def st_cols_added(api, base):
    """One dense column more takes 12x31 from a stride of 32 to 64; the handle is its own base."""
    root, P = solved(api, base)
    m = P.m
    col = (np.arange(m) % 4 + 1).astype(np.float64)
    assert P.add_dense_cols(col.reshape(1, m), [3.0], [DB], [0.0], [2.0], kinds=[IV]) == 0
    return Sender(root, [P], own_base=True)


def st_cols_deleted(api, base):
    """Two non-basic columns fewer take 8x64 from a stride of 96 to 64; the handle is its own base."""
    root, P = solved(api, base)
    stat = P.col_stat()
    gone = [j + 1 for j in range(P.n) if stat[j] != BS][-2:]
    assert P.del_cols(gone) == 0
    return Sender(root, [P], own_base=True)


# state -> (builder, the bases it runs on, the oracle's cuts it needs, engine only, the continuation)
STATES = {
    "1-unsolved": (st_unsolved, ILP_BASES, 0, False, ["solve", "repack", "branch"]),
    "2-opt": (st_opt, ILP_BASES + GEN_BASES, 0, False, ["many", "gmi", "gmi_rows", "del"]),
    "3-one-pending": (st_one_pending, ILP_BASES + GEN_BASES, 0, False, ["solve", "ranges"]),
    "4-nine-pending": (st_nine_pending, ["ilp-12x31", "ilp-24x48"], 0, False, ["solve", "many"]),
    "5-nofeas": (st_nofeas, ILP_BASES + GEN_BASES, 0, False, ["repack", "solve"]),
    "6-limit-primal": (st_limit_primal, ILP_BASES + GEN_BASES, 0, False, ["solve", "gmi"]),
    "6-limit-dual": (st_limit_dual, ILP_BASES + GEN_BASES, 0, False, ["solve", "branch"]),
    "7-gmi-row": (st_gmi_row, ILP_BASES, 1, False, ["solve", "ranges"]),
    "8-gmi-rows-solved": (st_gmi_rows_solved, ILP_BASES + GEN_BASES, 2, False, ["branch", "many", "repack"]),
    "9-grown": (st_grown, ILP_BASES, 0, False, ["solve", "gmi", "gmi_rows", "del"]),
    "10-rows-many": (st_many, ILP_BASES, 0, False, ["solve", "branch"]),
    "11-rows-deleted": (st_deleted, ILP_BASES, 0, True, ["solve", "ranges", "repack"]),
    "12-batch": (st_batch, ILP_BASES, 0, False, ["many", "branch"]),
    "13-tolerances": (st_tolerances, ILP_BASES, 0, False, ["short_cut", "branch"]),
    "14-refresh": (st_refresh, ILP_BASES, 0, False, ["solve"]),
    "15-cols-added": (st_cols_added, ["ilp-12x31"], 0, True, ["solve", "gmi", "gmi_rows", "del"]),
    "15-cols-deleted": (st_cols_deleted, ["ilp-8x64"], 0, True, ["solve", "many", "repack"]),
}
CASES = [(s, b) for s in STATES for b in STATES[s][1]]
# The states whose engine image is also held to the oracle's, bit for bit: those the oracle can build (it has no mvx_del_rows, so
# state 11 is not among them) and for which the suite already claims bitwise parity between the two (test_gpu_parity.py,
# test_gpu_thresholds.py, test_gpu_tolerances.py: warm children, pivot limits, appended cut rows, infeasible children;
# test_gpu_general.py: general models).  More than MAX_EDITS pending edits at once (state 4) are compared nowhere: left out.
ORACLE_PARITY = ["1-unsolved", "2-opt", "3-one-pending", "5-nofeas", "6-limit-primal", "6-limit-dual", "7-gmi-row", "8-gmi-rows-solved"]


def case_id(case):
    return "%s/%s" % case


def build(api, state, base, orc):
    """The sender of a case on `api`; `orc` gives the cut rows of states 7 and 8 (constants of the base)."""
    fn, _, ncuts, _, steps = STATES[state]
    sender = fn(api, base, oracle_cuts(base, ncuts, orc)) if ncuts else fn(api, base)
    sender.steps = list(steps)
    return sender


# ------------------------------------------------------------------------------------------------ what is compared


def model_of(P):
    """A certify.Model from the handle's own getters."""
    api, h, m, n = P.api, P.h, P.m, P.n
    A = np.zeros((m, n))
    for i in range(1, m + 1):
        ind, val = P.get_mat_row(i)
        A[i - 1, ind - 1] = val
    rows = [(api.get_row_type(h, i), api.get_row_lb(h, i), api.get_row_ub(h, i)) for i in range(1, m + 1)]
    cols = [col_bounds(P, j) for j in range(1, n + 1)]
    c = [api.get_obj_coef(h, j) for j in range(1, n + 1)]
    kinds = [IV if api.get_col_kind(h, j) != capi.CV else capi.CV for j in range(1, n + 1)]
    return cf.Model(A, rows, cols, c, api.get_obj_coef(h, 0), api.get_obj_dir(h), kinds)


def snapshot(P):
    """Everything the issue lists, as (name, kind, value): kind "f" compares as bits, "i" as integers."""
    api, h, m, n = P.api, P.h, P.m, P.n
    out = [("m", "i", m), ("n", "i", n), ("dir", "i", api.get_obj_dir(h)), ("status", "i", P.status), ("it_cnt", "i", P.it_cnt),
           ("obj_val", "f", P.obj)]
    out.append(("row types", "i", [api.get_row_type(h, i) for i in range(1, m + 1)]))
    out.append(("row bounds", "f", [[api.get_row_lb(h, i), api.get_row_ub(h, i)] for i in range(1, m + 1)]))
    out.append(("column types", "i", [api.get_col_type(h, j) for j in range(1, n + 1)]))
    out.append(("column bounds", "f", [[api.get_col_lb(h, j), api.get_col_ub(h, j)] for j in range(1, n + 1)]))
    out.append(("objective", "f", [api.get_obj_coef(h, j) for j in range(n + 1)]))
    out.append(("kinds", "i", [api.get_col_kind(h, j) for j in range(1, n + 1)]))
    A = np.zeros((m, n))
    for i in range(1, m + 1):
        ind, val = P.get_mat_row(i)
        assert len(set(ind.tolist())) == len(ind)
        A[i - 1, ind - 1] = val
    out.append(("matrix rows", "f", A))
    for name in ("col_prim", "row_prim", "col_dual", "row_dual"):
        out.append((name, "f", getattr(P, name)()))
    out.append(("col_stat", "i", P.col_stat()))
    out.append(("row_stat", "i", P.row_stat()))
    try:
        head, nb, flag = P.basis()
    except RuntimeError:
        out.append(("has a tableau", "i", 0))
        return out
    out.append(("has a tableau", "i", 1))
    out += [("head", "i", head), ("nb", "i", nb), ("flag", "i", flag), ("tableau", "f", P.tableau())]
    rows = np.zeros((m, m + n + 1))
    for i in range(1, m + 1):
        ind, val = P.eval_tab_row(int(head[i]))
        rows[i - 1, ind] = val
    out.append(("eval_tab_row", "f", rows))
    return out


PARITY = ("m", "n", "status", "it_cnt", "obj_val", "has a tableau", "head", "nb", "flag", "tableau", "col_prim", "row_prim", "col_stat",
          "row_stat")  # what test_gpu_parity.assert_same_state compares between the engine and the oracle


def same_snapshots(a, b, what, only=None):
    a = [e for e in a if only is None or e[0] in only]
    b = [e for e in b if only is None or e[0] in only]
    assert [e[0] for e in a] == [e[0] for e in b], what
    for (name, kind, x), (_, _, y) in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        assert same_bits(x, y) if kind == "f" else np.array_equal(x, y), (what, name)


def certify_handle(Q, tol, what):
    """The independent reference on the handle's own model: tableau, values, and the certificate of OPT / NOFEAS."""
    return cf.certify(model_of(Q), Q, what=what, tol_bnd=tol[0], tol_dj=tol[1], tol_piv=tol[2])


# ------------------------------------------------------------------------------------------------ the library behind the check


class Kit:
    """The oracle's side: images in host memory.  tests/test_gpu_images.py derives the engine's, with images on the device."""

    name = "oracle"
    pad_bytes = None  # the bytes of an image no pack writes (alignment); None: not pinned on this side

    def __init__(self, api):
        self.api = api

    def buffer(self, size, fill=PATTERN):
        """(storage, address of the image): `size` bytes with GUARD bytes of `fill` on either side, the image 256-aligned."""
        store = np.full(size + 2 * GUARD + IMAGE_ALIGN, fill, dtype=np.uint8)
        off = GUARD + (-(store.ctypes.data + GUARD)) % IMAGE_ALIGN
        return (store, off, size), store.ctypes.data + off

    def read(self, buf):
        """(bytes in front, image, bytes behind) as host arrays."""
        store, off, size = buf
        return store[:off].copy(), store[off:off + size].copy(), store[off + size:].copy()

    def write(self, buf, image):
        store, off, size = buf
        store[off:off + size] = image

    def fresh(self):
        return self.api.create()

    def used(self):
        """A handle that has held a solved model of another size (the engine's has also built its DevMatrix and rounding model)."""
        Q = synth.load_ilp(self.api, *synth.dense_ilp(6, 10, 3, 2))
        assert Q.simplex() == 0
        return Q

    def step_many(self, handles):
        return None

    def step_ranges(self, P):
        return None

    def short_cut(self, P):
        return None

    def can_delete(self):
        return False


def guards_intact(kit, buf, fill=PATTERN):
    front, image, back = kit.read(buf)
    assert len(front) >= GUARD and len(back) >= GUARD
    assert np.all(front == fill) and np.all(back == fill), "bytes outside the image were written"
    return image


def where(a, b):
    """For a failure's message: how many bytes of two images differ and the first offsets."""
    if len(a) != len(b):
        return len(a), len(b)
    d = np.nonzero(a != b)[0]
    return len(d), d[:8].tolist()


def pack(kit, P, base, what):
    """The image of P against `base` (None: mvx_pack, P its own base), with the checks of the write: size, guard bytes, the same
    bytes a second time, and which bytes of the image were written at all."""
    api = kit.api
    size = api.pack_size(P.h) if base is None else api.pack_size_from(P.h, base.h)
    assert size >= 0, what
    images = []
    for fill in (PATTERN, PATTERN ^ 0xFF, PATTERN):
        buf, addr = kit.buffer(size, fill)
        assert addr % IMAGE_ALIGN == 0
        rc = api.pack(P.h, addr) if base is None else api.pack_from(P.h, base.h, addr)
        assert rc == 0, what
        images.append(guards_intact(kit, buf, fill))
    assert np.array_equal(images[0], images[2]), (what, "two packs of one handle differ", where(images[0], images[2]))
    unwritten = images[0] != images[1]  # a written byte is the same over either background
    if kit.pad_bytes is not None:
        assert not unwritten[0] and not unwritten[-1] and int(unwritten.sum()) <= kit.pad_bytes, (what, int(unwritten.sum()))
    return images[0]


def unpack(kit, Q, base, image, what):
    buf, addr = kit.buffer(len(image))
    kit.write(buf, image)
    assert kit.api.unpack(Q.h, base.h, addr) == 0, what
    assert np.array_equal(guards_intact(kit, buf), image), (what, "unpack wrote into the image")
    return Q


def first_fractional(P):
    x = P.col_prim()
    for j in range(1, P.n + 1):
        if P.api.get_col_kind(P.h, j) != capi.CV and abs(x[j - 1] - round(x[j - 1])) > 1e-6:
            return j, x[j - 1]
    return None


def apply_step(kit, step, group, lead, memo):
    """One continuation step on every handle of `group`, decided on `lead` (a member of it) before anyone is touched.  Returns the
    per-handle results to compare (beyond the snapshots), or None where this side has no such call."""
    api = kit.api
    if step == "solve":
        return [(H.simplex(),) for H in group]
    if step == "branch":
        if lead.status == OPT and first_fractional(lead):
            j, x = first_fractional(lead)
            bnds = cut_bound(lead, j, x)
        else:
            j = 2
            lo, hi = interval(lead, j)
            bnds = as_bounds(lo, lo + 1.0)
        out = []
        for H in group:
            set_col(H, j, bnds)
            out.append((H.simplex(),))
        return out
    if step == "gmi":
        cols = [j for j in basic_cols(lead) if api.get_col_kind(lead.h, j) != capi.CV]
        memo["cuts"] = [gmi(H, cols) for H in group]
        return [tuple(c) for c in memo["cuts"]]
    if step == "gmi_rows":
        vals, rhs, ok = memo["cuts"][group.index(lead)]
        keep = [t for t in range(len(ok)) if ok[t]][:3]
        memo["m_before"] = lead.m
        out = []
        for H in group:
            if keep:
                add_cut_rows(H, vals[keep], rhs[keep])
            out.append((H.simplex(),))
        return out
    if step == "del":
        if not kit.can_delete():
            return None
        rows = list(range(memo["m_before"] + 1, lead.m + 1))
        return [(H.del_rows(rows) if rows else 0, H.simplex()) for H in group]
    if step == "ranges":
        return kit.step_ranges(group)
    if step == "many":
        return kit.step_many(group)
    if step == "short_cut":
        return kit.short_cut(group)
    raise AssertionError(step)


MUTATING = ("solve", "branch", "gmi_rows", "del")


def same_results(res, what):
    for r in res[1:]:
        assert len(r) == len(res[0]), what
        for x, y in zip(res[0], r):
            x, y = np.asarray(x), np.asarray(y)
            assert x.shape == y.shape and (same_bits(x, y) if x.dtype.kind == "f" else np.array_equal(x, y)), what


def roundtrip(kit, P, base, sender, what, trace=None):
    """The check of one sender handle.  `base`: what P is packed against and Q unpacked against (P itself when the sender is its
    own base).  `trace`, when given, collects (label, snapshot of Q) for the comparison between the engine and the oracle."""
    api = kit.api
    own = sender.own_base
    twin = P.copy()  # P': never packed
    refresh0 = {id(H): api.get_refresh_cnt(H.h) for H in (P, twin)}
    image = pack(kit, P, None if own else base, what)
    same_snapshots(snapshot(P), snapshot(twin), what + ": packing changed the sender")
    # the receiver, twice
    Q1 = unpack(kit, kit.fresh(), base, image, what + " into a fresh handle")
    Q2 = unpack(kit, kit.used(), base, image, what + " into a used handle")
    sp = snapshot(P)
    for Q, name in ((Q1, "fresh"), (Q2, "used")):
        same_snapshots(snapshot(Q), sp, "%s: the %s receiver against the sender" % (what, name))
        again = pack(kit, Q, Q if own else base, what + " again")
        assert np.array_equal(again, image), (what, name, "the image of the image differs", where(again, image))
        refresh0[id(Q)] = api.get_refresh_cnt(Q.h)
    if sender.tableau:
        for Q in (Q1, Q2):
            certify_handle(Q, sender.tol, what + " received")
    else:
        assert not [e for e in sp if e[0] == "has a tableau"][0][2], what
    if trace is not None:
        trace.append(("received", snapshot(Q1)))
    # the continuation
    group = [P, twin, Q1, Q2]
    memo = {}
    for k, step in enumerate(sender.steps):
        w = "%s, step %d (%s)" % (what, k + 1, step)
        if step == "repack":
            qbase = Q1 if own else base
            Q1 = unpack(kit, kit.fresh(), qbase, pack(kit, Q1, None if own else base, w), w)
            refresh0[id(Q1)] = api.get_refresh_cnt(Q1.h) - (api.get_refresh_cnt(P.h) - refresh0[id(P)])
            group[2] = Q1
            res = []
        else:
            res = apply_step(kit, step, group, P, memo)
            if res is None:
                if step in MUTATING:
                    break
                continue
            same_results(res, w)
        sp = snapshot(P)
        for H in group[1:]:
            same_snapshots(snapshot(H), sp, w)
        moved = [api.get_refresh_cnt(H.h) - refresh0[id(H)] for H in group]
        assert len(set(moved)) == 1, (w, "refreshes", moved)
        if trace is not None:
            trace.append((step, snapshot(Q1)))
    if "refreshes" in sender.extra:
        assert api.get_refresh_cnt(P.h) - refresh0[id(P)] >= sender.extra["refreshes"], (what, "the countdown never ran out")
    if sp and [e for e in sp if e[0] == "has a tableau"][0][2] and P.status in (OPT, NOFEAS):
        certify_handle(Q1, DEFAULT_TOL, what + " at the end")
    return Q1


def run_case(kit, state, base, orc, trace=None):
    """Build the case on the kit's library and send every sender handle through the check."""
    sender = build(kit.api, state, base, orc)
    try:
        for k, P in enumerate(sender.handles):
            roundtrip(kit, P, P if sender.own_base else sender.root, sender, "%s/%s[%d] on %s" % (state, base, k, kit.name),
                      trace if k == 0 else None)
    finally:
        if sender.cleanup:
            sender.cleanup()
    return sender
