"""Instances at the engine's built-in size limits and path thresholds, shared by test_thresholds_inputs.py (CPU: the
oracle alone proves each instance has the property its GPU test relies on) and test_gpu_thresholds.py (GPU: the engine
against the oracle, bitwise, on those instances).  The constants restate mvx_internal.hpp / kernels.hip /
node_kernels.hip / engine.cpp; they decide which side of a threshold an instance is meant to lie on, never what the
engine does."""
import ctypes as C

import numpy as np

from mvolps_amd import capi, synth

MIB = 1 << 20
LD_ALIGN, ROW_SLACK, ROWCOMB_CHUNK, DCH_MAX = 32, 64, 64, 8  # mvx_internal.hpp (a fresh slab has m + ROW_SLACK rows)
GMI_CH, GMI_CT = 1024, 4  # node_kernels.hip: non-basic positions per pass of k_gmi_work, cuts per lane of k_gmi_backsub
DSEL_MAX = 1024  # k_dsel: one row and one column per lane
PERSIST_MAX_CPW, PERSIST_LDS_MAX, PERSIST_AREA_MIN, PERSIST_AREA_MAX = 16, 150 * 1024, 32768, 700000
COPY_KERNEL_MAX, COPY_ONE_PASS, COPY_WHOLE_SPARE = 64 * MIB, 32 * MIB, 1 * MIB  # engine_copy / launch_copy_many


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


# ------------------------------------------------------------------------------------------------ A: GMI cuts
# (m, n, seed, U) of synth.dense_ilp.  1023 / 1025 / 1100: one pass less one, one position into the second pass, a
# short second pass; 2100: three passes; 65 rows: a second 64-row group of one row in the back-substitution; 63 rows and
# 257 columns: a short group and a second 256-column block of one column.
GMI_CASES = [(24, 1023, 6, 2), (24, 1025, 6, 2), (24, 1100, 6, 2), (70, 2100, 5, 2), (65, 300, 3, 2), (63, 257, 3, 3)]
GMI_ROUNDS = 3
GMI_TAIL_CASE = GMI_CASES[2]  # cut counts 1, 3, 4, 5 against the full call
GMI_CERT_CASES = [GMI_CASES[2], GMI_CASES[3]]


def gmi_id(case):
    return "%dx%d" % (case[0], case[1])


def load_gmi_case(api, case):
    A, b, c, U = synth.dense_ilp(*case)
    return synth.load_ilp(api, A, b, c, U)


def basic_columns(Q):
    stat = Q.col_stat()
    return [j + 1 for j in range(len(stat)) if stat[j] == capi.BS]


def oracle_cut(orc, Q, j, repaired):
    """(rc, vals[0..n], rhs) of orc_generateCutGMI (repaired) or orc_generateCut3 (the formula as written) for column j"""
    n = Q.n
    inds = np.zeros(n + 1, dtype=np.int32)
    vals = np.zeros(n + 1)
    lb = C.c_double(0.0)
    ip, vp = inds.ctypes.data_as(C.POINTER(C.c_int)), vals.ctypes.data_as(C.POINTER(C.c_double))
    if repaired:
        eff = C.c_double(0.0)
        rc = orc.generateCutGMI(Q.h, j, ip, vp, C.byref(lb), C.byref(eff))
    else:
        rc = orc.generateCut3(Q.h, j, ip, vp, C.byref(lb))
    return rc, vals, lb.value


def oracle_round(orc, Q):
    """The basic columns of the oracle's handle and, per mode, the oracle's cut of each: {mode: [(rc, vals, rhs)]}"""
    basic = basic_columns(Q)
    return basic, {mode: [oracle_cut(orc, Q, j, mode) for j in basic] for mode in (0, 1)}


def append_cut(api, H, vals, lb):
    """cut.cpp:23-43: one >= row over every column, then the dual re-solve"""
    r = api.add_rows(H.h, 1)
    H.set_mat_row(r, np.arange(H.n + 1, dtype=np.int32), vals)
    api.set_row_bnds(H.h, r, capi.LO, float(lb), 0.0)
    return H.simplex()


def basic_rows(Q, cols):
    """Tableau rows (positions 1..n) of the basic structural columns `cols`, and the non-basic flags by position"""
    head, nb, flag = Q.basis()
    m = Q.m
    T = Q.tableau()
    where = {int(k): i for i, k in enumerate(head) if i >= 1}
    return np.stack([T[where[m + j], 1:] for j in cols]), flag[1:]


# `temp` across passes: generateCut3 assigns it for GLP_IV and GLP_CV positions only, so a position that reads as GLP_BV
# (an integer column boxed to [0, 1]) re-uses the value of the position before it -- across a pass where it is the first
# of the next.  dense_ilp with every third column boxed to [0, 1]; column 1025 is one of them.
MIXED_CASE = (24, 1100, 6, 2)


def load_mixed(api):
    A, b, c, U = synth.dense_ilp(*MIXED_CASE)
    n = A.shape[1]
    col_b = [(capi.DB, 0.0, 1.0 if j % 3 == 2 else U) for j in range(1, n + 1)]
    P = api.create()
    P.load_general(A, [(capi.UP, 0.0, float(v)) for v in b], col_b, c, kinds=[capi.IV] * n, direction=capi.MAX)
    return P


# the free-non-basic flag across passes: three independent blocks of rows and columns (a block-diagonal model keeps a
# block-diagonal tableau), free continuous columns in two of them.  Block 0 has one at a position of the first pass and
# one in the second, block 1 only one in the second pass, block 2 none; the free columns carry no objective and small
# entries, so that the first pivots leave them alone, and the solve is stopped by its pivot limit.
FREE_N, FREE_ROWS, FREE_LIMIT, FREE_SEED = 1200, 8, 36, 4
FREE_COLS = {0: (700, 1100), 1: (1150,), 2: ()}  # block -> its free columns (1-based)


def free_model():
    """(A, row_b, col_b, c, kinds, block of each column) of the general model above"""
    rng = np.random.default_rng(FREE_SEED)
    n, rows = FREE_N, FREE_ROWS
    block = np.arange(n) % 3
    free = {j: b for b, js in FREE_COLS.items() for j in js}
    for j, b in free.items():
        block[j - 1] = b
    A = np.zeros((3 * rows, n))
    for b in range(3):
        cols = np.nonzero(block == b)[0]
        A[b * rows:(b + 1) * rows, cols] = rng.integers(1, 21, size=(rows, len(cols))).astype(float)
    c = rng.integers(1, 21, size=n).astype(float)
    col_b = [(capi.DB, 0.0, 2.0)] * n
    kinds = [capi.IV] * n
    for j in free:
        A[:, j - 1] = np.where(A[:, j - 1] != 0.0, 0.125, 0.0)
        c[j - 1] = 0.0
        col_b[j - 1] = (capi.FR, 0.0, 0.0)
        kinds[j - 1] = capi.CV
    row_b = [(capi.UP, 0.0, float(np.floor(0.4 * A[i].sum()))) for i in range(3 * rows)]
    return A, row_b, col_b, c, kinds, block


def load_free(api):
    A, row_b, col_b, c, kinds, _ = free_model()
    P = api.create()
    P.load_general(A, row_b, col_b, c, kinds=kinds, direction=capi.MAX)
    return P


def free_positions(Q, cols):
    """Per basic column of `cols`: the positions (1-based, ascending) that hold a non-zero under a free non-basic status
    -- exactly where no valid cut exists (k_gmi_work's code 3, the oracle's ORC_NF branch)"""
    rows, flag = basic_rows(Q, cols)
    return [list(1 + np.nonzero((r != 0.0) & (flag == capi.NF))[0]) for r in rows]


# ------------------------------------------------------------------------------------------------ B: k_dsel
# (m, n, seed, U): lane 1023 owns row 1024 with and without a column of its own, both limits at once, one row short of
# the limit with every column lane busy, and one row past it
DSEL_CASES = [(1024, 600, 7, 3), (1024, 1024, 7, 3), (1023, 1024, 7, 3), (1025, 700, 7, 3)]
DSEL_GROW = (1020, 600, 7, 3)  # eight appended cut rows take m from 1021 to 1028
DSEL_GROW_ROUNDS = 8
DSEL_CHAIN = 8


def grow_plan(orc, Q):
    """One growth round, decided on the oracle's handle: the bug-compatible cut of its last basic column (the row that
    test_gpu_gmi appends) and the down branch of its first fractional column.  On these instances generateCut3's cut is
    never violated by the vertex it is taken from (its coefficients and right-hand side are all negative), so the row
    alone costs no pivot; the bound is what makes the re-solve a dual one.  x = 0 satisfies every row, so rounding down
    keeps the LP feasible."""
    x = Q.col_prim()
    rc, vals, lb = oracle_cut(orc, Q, basic_columns(Q)[-1], 0)
    assert rc == 0
    j = fractional_columns(x)[0]
    return vals, lb, j, float(np.floor(x[j - 1]))


def grow_apply(api, H, plan):
    vals, lb, j, ub = plan
    r = api.add_rows(H.h, 1)
    H.set_mat_row(r, np.arange(H.n + 1, dtype=np.int32), vals)
    api.set_row_bnds(H.h, r, capi.LO, float(lb), 0.0)
    api.set_col_bnds(H.h, j, capi.DB, 0.0, ub)
    return H.simplex()


def dsel_id(case):
    return "%dx%d" % (case[0], case[1])


def fractional_columns(x):
    return [j + 1 for j in range(len(x)) if abs(x[j] - round(x[j])) > 1e-9]


def child_bounds(x, j, up, U):
    return (float(np.ceil(x[j - 1])), U) if up else (0.0, float(np.floor(x[j - 1])))


def dsel_children(orc, case):
    """The oracle's root and both children of its first two fractional columns: (root, x, {(j, up): child})"""
    A, b, c, U = synth.dense_ilp(*case)
    o = synth.load_ilp(orc, A, b, c, U)
    assert o.simplex() == 0
    x = o.col_prim()
    kids = {}
    for j in fractional_columns(x)[:2]:
        for up in (0, 1):
            k = o.copy()
            orc.set_col_bnds(k.h, j, capi.DB, *child_bounds(x, j, up, U))
            k.simplex()
            kids[(j, up)] = k
    return o, x, kids


# ------------------------------------------------------------------------------------------------ C: k_persist
def persist_lds_bytes(m, cpw):  # kernels.hip
    return (m + 1) * (cpw + 4) * 8 + (m + 1) * 4 + 64


def persist_plan(m, n, cus):
    """engine.cpp persist_plan at the default setting: (cpw, workgroups, LDS bytes), or None where k_persist declines"""
    area = (m + 1) * (n + 1)
    if area < PERSIST_AREA_MIN or area > PERSIST_AREA_MAX:
        return None
    cpw = (n + cus - 1) // cus
    if cpw > PERSIST_MAX_CPW:
        return None
    nw = (n + cpw - 1) // cpw
    lds = persist_lds_bytes(m, cpw)
    if nw > 256 or lds > PERSIST_LDS_MAX:
        return None
    return cpw, nw, lds


def update_tile_rows(m_grid, n, slots=1):
    """kernels.hip launch_update: rows per tile of k_update for a grid of m_grid rows (m, or m + 1 in phase 1, whose cost
    row is tableau row m + 1) -- 16 while the launch keeps 2048 workgroups, else 8, else 4"""
    tiles = ((n + 2) // 2 + 255) // 256
    for tr in (16, 8):
        if (m_grid + tr) // tr * tiles * slots >= 2048:
            return tr
    return 4


PERSIST_LIMITS = {"widest-strips": 700, "strips-too-wide": 700}  # pivot limits: these two stall for 10^5 pivots and more


def persist_shapes(cus):
    """name -> (m, n, seed, taken): the shapes of section C for a device with `cus` compute units (256 on an MI355X:
    500x601, 690x1000, 3488x199 / 3489x199, 127x255 / 127x254, 699x999 / 699x1000, 173x4000, 100x4097)"""
    n3 = 3 * (cus * 25 // 32) + 1  # cpw = 3, the last workgroup holds one column
    n4 = min(cus * 125 // 32, 4 * 256)  # cpw = 4 (at most 256 workgroups)
    n1 = min(199, cus)
    tall = (PERSIST_LDS_MAX - 64) // ((1 + 4) * 8 + 4) - 1  # tallest m whose strip, at one column per workgroup, fits the LDS
    lo_n = min(255, cus)
    lo_m = -(-PERSIST_AREA_MIN // (lo_n + 1)) - 1  # smallest m with (m + 1)(n + 1) >= 32768
    hi_n = n4 - 1
    # as many columns per workgroup as 256 workgroups leave room for (16 at 256 units), 250 workgroups
    wide_cpw = max(k for k in range(1, PERSIST_MAX_CPW + 1) if k * 250 > (k - 1) * cus)
    wide_n = wide_cpw * 250
    hi_m = PERSIST_AREA_MAX // (hi_n + 1) - 1  # tallest m with (m + 1)(n + 1) <= 700000
    return {
        "cpw3-short-last-strip": (500, n3, 41030, True),
        "cpw4-under-the-area-cap": (PERSIST_AREA_MAX // (n4 + 1) - 9, n4, 41031, True),
        "lds-ceiling": (tall, n1, 41032, True),
        "lds-ceiling+1": (tall + 1, n1, 41032, False),
        "area-min": (lo_m, lo_n, 41033, True),
        "area-min-1": (lo_m, lo_n - 1, 41033, False),
        "area-max": (hi_m, hi_n, 41034, True),
        "area-max+1": (hi_m, hi_n + 1, 41034, False),
        "widest-strips": (PERSIST_AREA_MAX // (wide_n + 1) - 1, wide_n, 41035, True),
        "strips-too-wide": (100, PERSIST_MAX_CPW * cus + 1, 41036, False),
    }


# ------------------------------------------------------------------------------------------------ D: clones
def align_up(x, a):
    return (x + a - 1) // a * a


def slab_geometry(m, n):
    """engine.cpp slab_layout of a freshly loaded m x n handle: total bytes, the live rows' bytes, the spare bytes
    between them and the small arrays (engine_copy sends two ranges when those exceed 1 MiB)"""
    ld = align_up(n + 1, LD_ALIGN)
    cap = m + ROW_SLACK
    o_bvar = align_up((cap + 1) * ld * 8, 256)
    tail = align_up((cap + 1) * 4, 256) + 2 * align_up((cap + 1) * 8, 256) + 2 * align_up(ld * 4, 256) + 2 * align_up(ld * 8, 256)
    live = (m + 1) * ld * 8
    return dict(total=o_bvar + tail, live=live, spare=o_bvar - live, tail=tail)


def copy_regime(m, n):
    """(path, ranges, looped): 'kernel' (k_copy_many) or 'memcpy'; one range over the slab or two; whether the largest
    range exceeds what the capped grid moves in one pass"""
    g = slab_geometry(m, n)
    whole = g["spare"] <= COPY_WHOLE_SPARE
    largest = g["total"] if whole else max(g["live"], g["tail"])
    return ("kernel" if g["total"] <= COPY_KERNEL_MAX else "memcpy", 1 if whole else 2, largest > COPY_ONE_PASS)


# (m, n, seed, first limit, second limit, expected regime)
CLONE_CASES = [
    (2200, 2100, 31, 24, 17, ("kernel", 2, True)),
    (2000, 4100, 32, 24, 17, ("memcpy", 2, True)),
    (9000, 500, 33, 24, 17, ("kernel", 1, True)),
]


def clone_id(case):
    return "%dx%d" % (case[0], case[1])


def load_clone_case(api, case):
    """Boxed columns (two in three) over synth.dense_lp: flips and columns at their upper bound among the first pivots"""
    m, n, seed = case[:3]
    A, b, c = synth.dense_lp(m, n, seed)
    col_b = [(capi.DB, 0.0, 0.5 + (j % 3)) if j % 3 else (capi.LO, 0.0, 0.0) for j in range(n)]
    P = api.create()
    P.load_general(A, [(capi.UP, 0.0, float(v)) for v in b], col_b, c, direction=capi.MAX)
    return P


def column_bounds(P):
    n = P.n
    return (np.array([P.api.get_col_type(P.h, j) for j in range(1, n + 1)]), np.array([P.api.get_col_lb(P.h, j) for j in range(1, n + 1)]),
            np.array([P.api.get_col_ub(P.h, j) for j in range(1, n + 1)]))


# ------------------------------------------------------------------------------------------------ E: objective row
ROWCOMB_CASES = [(63, 257, 1), (64, 257, 2), (65, 257, 11), (128, 257, 119), (129, 257, 1096)]  # seeds: see test_thresholds_inputs


def change_objective(P):
    P.api.set_obj_coef(P.h, 3, 2.5)
    P.api.set_obj_coef(P.h, 200, -0.75)
    P.api.set_obj_coef(P.h, 0, -1.0)
