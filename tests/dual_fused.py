"""The fused dual path (k_dboot / k_da / k_fb<DUAL>) at its block edges, shared by test_dual_fused_inputs.py (CPU: the
oracle alone proves each instance contains the event its GPU test relies on, at a pivot the engine's schedule hands to
the fused pair) and test_gpu_dual_fused.py (GPU: the engine under mvx_set_dual_fused(2) against the oracle, bitwise, at
every stop, with the fused-pivot counter moving by exactly what the schedule says).

The instances are general_at_size.cold_dual_lp draws.  Seed search rarely lands an event on an edge, so the event is
moved there: the oracle's pivot log names a late pivot's row (column), and that model row (column) is swapped with row m
(column n).  The slack basis holds auxiliary i in tableau row i and structural column j at position j, so the swap moves
the event to tableau row m (position n); `moves` of a case lists the swaps, found on the oracle once and asserted by the
CPU companion.  Nothing here was chosen by looking at the engine.

The constants restate mvx_internal.hpp / kernels.hip / engine.cpp; generic_indices restates the schedule of job_begin /
job_enqueue / job_collect."""
import numpy as np

from mvolps_amd import capi, synth
from mvolps_amd.capi import EITLIM, MAX, NF, NL, NU

from . import general_at_size as ga
from . import thresholds as th

DA_THREADS = 1024  # k_dboot / k_da: columns per workgroup, and the stride of every workgroup's walk over the rows
FB_COLS = 512  # k_fb: columns per tile (256 lanes, a double2 each)
FB_TR, FB_NT = (4, 8, 16, 32), (0, 1, 2)  # launch_db: the twelve k_fb<TR, 1, NT, 1>
BATCH_FIRST, BATCH_MAX = 8, 256  # engine.cpp: pivots queued per host round trip, doubling
DEGEN_TOL = 1e-9  # a dual ratio no longer than this counts towards the stall count


# ------------------------------------------------------------------------------------------------ the schedule
def generic_indices(total, warm, calls, degenerate=None, stall_limit=None):
    """The 0-based pivot indices, among the `total` pivots a solve takes under the call schedule `calls` (pivot limits,
    None = to the end), that the engine's generic step (k_select + k_update) takes when the fused dual pair is always on
    and dual chains are off; every other pivot is k_da + k_fb<DUAL>'s.  The solve is a dual simplex throughout.

    engine.cpp: a call queues batches of 8, 16, ... 256 pivots.  A call on a handle without the dual hint (`warm` false,
    and every call after the first) opens with a batch whose only pivot is the generic step that finds the phase -- sized
    by the limit where there is one above 8 -- and every other batch is one generic pivot, then fused pivots up to the
    batch size or what the limit leaves.  The stall count (consecutive degenerate pivots, restarted by every call) at or
    above `stall_limit` stops the fused run where it stands; the next batch is then generic throughout (Bland's rule
    until a pivot moves), and the one after it is fused again if the count has fallen below the limit by then.
    `degenerate[k]` says whether pivot k is degenerate; without a stall limit the count never matters."""
    generic, done = [], 0
    for ci, lim in enumerate(calls):
        if done >= total:
            break
        left = total - done if lim is None else min(lim, total - done)
        hint = warm and ci == 0
        batch = BATCH_FIRST if hint or lim is None or lim <= BATCH_FIRST else min(lim, BATCH_MAX)
        opening, fused_ok, made, stall = not hint, hint, 0, 0

        def step(k):
            return stall + 1 if (degenerate is not None and degenerate[k]) else 0

        def stalled():
            return stall_limit is not None and stall >= stall_limit

        while made < left:
            depth = min(batch, left - made)
            if opening:
                depth = 1
            for t in range(depth):
                k = done + made
                if opening or not fused_ok or t == 0:
                    generic.append(k)
                elif stalled():
                    break  # k_dboot / k_da give the rest of the batch back
                stall = step(k)
                made += 1
            opening, fused_ok = False, not stalled()
            batch = min(2 * batch, BATCH_MAX)
        done += left
    return generic


def fused_indices(total, warm, calls, **kw):
    g = set(generic_indices(total, warm, calls, **kw))
    return [k for k in range(total) if k not in g]


# ------------------------------------------------------------------------------------------------ instances
def swapped(inst, moves):
    """The instance with model rows / columns exchanged: moves = [("row" | "col", a, b)], 1-based"""
    out = dict(inst)
    A, row_b, col_b, c, x0 = inst["A"].copy(), list(inst["row_b"]), list(inst["col_b"]), inst["c"].copy(), inst["x0"]
    x0 = None if x0 is None else x0.copy()
    for kind, a, b in moves:
        a, b = a - 1, b - 1
        if kind == "row":
            A[[a, b]] = A[[b, a]]
            row_b[a], row_b[b] = row_b[b], row_b[a]
        else:
            A[:, [a, b]] = A[:, [b, a]]
            col_b[a], col_b[b] = col_b[b], col_b[a]
            c[[a, b]] = c[[b, a]]
            if x0 is not None:
                x0[[a, b]] = x0[[b, a]]
    out.update(A=A, row_b=row_b, col_b=col_b, c=c, x0=x0)
    return out


class Case:
    """cold_dual_lp(m, n, seed) with `moves` applied, then (infeasible_seed) the two contradicting rows; solved under the
    call schedule `calls`.  total / status: the oracle's pivot count and end status.  events: what the CPU companion
    asserts of the pivot log at fused indices -- ("q", j) column position j enters, ("p", i) tableau row i leaves."""

    def __init__(self, name, m, n, seed, moves=(), calls=(None,), total=None, status=capi.OPT, events=(), infeasible_seed=None,
                 stall_limit=None, bland=None, repeats=0):
        self.name, self.m, self.n, self.seed, self.moves, self.calls = name, m, n, seed, list(moves), calls
        self.total, self.status, self.events, self.infeasible_seed = total, status, list(events), infeasible_seed
        self.stall_limit, self.bland, self.repeats = stall_limit, bland, repeats

    @property
    def feasible(self):
        return self.infeasible_seed is None

    def instance(self):
        inst = swapped(ga.cold_dual_lp(self.m, self.n, self.seed), self.moves)
        return inst if self.feasible else ga.infeasible(inst, self.infeasible_seed)

    def __repr__(self):
        return self.name


def case_id(case):
    return case.name


class Pivot:
    """One pivot of the oracle's log: tableau row p leaves to `leave` (the flag position q holds afterwards), position q
    enters from `enter`; a is the pivot element, `degenerate` the dual ratio test's verdict (ratio <= DEGEN_TOL), `bland`
    whether Bland's rule chose it."""

    def __init__(self, p, q, a, enter, leave, degenerate, bland):
        self.p, self.q, self.a, self.enter, self.leave, self.degenerate, self.bland = p, q, a, enter, leave, degenerate, bland


def pivot_log(orc, load, sgn, limit=None):
    """As test_gpu_chain_exchange.oracle_pivot_log: the state after j pivots is the full solve cut off at j (the limit only
    truncates), so pivot j is read off two neighbouring truncations.  The dual ratio is recomputed from the tableau in
    front of the pivot as dev_dual_ratio / dual_ratio_col do: r = |d| for a free column, the part of d with the sign that
    the column's bound allows otherwise (d = sgn * T[0][q]), over |a|.  Returns (log, the full solve's handle)."""
    full = load(orc)
    full.rc = full.simplex(it_lim=limit)
    log = []
    prev = load(orc)
    prev.simplex(it_lim=0)
    for j in range(1, full.it_cnt + 1):
        cur = load(orc)
        cur.simplex(it_lim=j)
        (h0, nb0, f0), (h1, nb1, f1) = prev.basis(), cur.basis()
        ps, qs = np.nonzero(h0 != h1)[0], np.nonzero(nb0 != nb1)[0]
        assert len(ps) == 1 and len(qs) == 1, (j, ps, qs)
        p, q = int(ps[0]), int(qs[0])
        T = prev.tableau()
        a, d, f = float(T[p, q]), sgn * float(T[0, q]), int(f0[q])
        r = abs(d) if f == NF else (max(-d, 0.0) if f == NL else max(d, 0.0))
        assert f in (NL, NU, NF) and a != 0.0
        log.append(Pivot(p, q, a, f, int(f1[q]), r / abs(a) <= DEGEN_TOL, cur.bland_cnt > prev.bland_cnt))
        prev = cur
    assert np.array_equal(prev.tableau(), full.tableau()) and prev.bland_cnt == full.bland_cnt
    return log, full


def case_log(orc, case):
    inst = case.instance()
    orc.set_stall_limit(case.stall_limit or 0)
    try:
        return pivot_log(orc, lambda api: ga.load(api, inst), 1.0 if inst["direction"] == MAX else -1.0)
    finally:
        orc.set_stall_limit(0)


def case_generic(case, log=None):
    deg = None if log is None else [x.degenerate for x in log]
    return generic_indices(case.total, False, case.calls, degenerate=deg, stall_limit=case.stall_limit)


def repeats_at(log, fused):
    """Pivots whose leaving row is the row the pivot before them took as well, both of them fused: k_da's p2 == p arm"""
    fs = set(fused)
    return [k for k in range(1, len(log)) if log[k].p == log[k - 1].p and k in fs and k - 1 in fs]


# ------------------------------------------------------------------------------------------------ the cases
# Every figure (moves, total, status, bland, fused) was read from the oracle and is asserted by test_dual_fused_inputs.py.
C513 = [("col", 226, 513), ("col", 462, 512)]
R1025 = [("row", 281, 1025), ("row", 508, 1024)]
# k_dboot / k_da over columns 0..n in workgroups of 1024: at 1023 the one workgroup is exactly full, at 1024 a second one
# (and a third 512-column tile of k_fb) holds column 1024 alone
COLUMNS = [
    Case("cols-40x1022", 40, 1022, 1, [("col", 426, 1022)], total=34, events=[("q", 1022)]),
    Case("cols-40x1023", 40, 1023, 1, [("col", 1012, 1023)], total=34, events=[("q", 1023)]),
    Case("cols-40x1024", 40, 1024, 24, total=31, events=[("q", 1024)]),
    Case("cols-40x1025", 40, 1025, 2, [("col", 796, 1025), ("col", 354, 1024)], total=33, events=[("q", 1025), ("q", 1024)]),
]
# the row walk with stride 1024: row 1024 is thread 1023's only row, row 1025 thread 0's second
ROWS = [
    Case("rows-1023x60", 1023, 60, 1, [("row", 76, 1023)], total=207, events=[("p", 1023)], repeats=3),
    Case("rows-1024x60", 1024, 60, 2, [("row", 25, 1024)], total=202, events=[("p", 1024)], repeats=3),
    Case("rows-1025x60", 1025, 60, 1, R1025, total=178, events=[("p", 1025), ("p", 1024)], repeats=3),
]
# k_fb's 512-column tiles: q == n at an even and an odd n (the half-filled double2), entering columns on both sides of 511 | 512
COLUMN_TILES = [
    Case("tiles-60x510", 60, 510, 6, [("col", 355, 510)], total=78, events=[("q", 510)]),
    Case("tiles-60x511", 60, 511, 6, [("col", 467, 511)], total=61, events=[("q", 511)]),
    Case("tiles-60x512", 60, 512, 6, [("col", 463, 512)], total=65, events=[("q", 512)]),
    Case("tiles-60x513", 60, 513, 6, C513, total=99, events=[("q", 513), ("q", 512)]),
]
# k_fb's row tiles at TR = 32 (set_tuning(32, 1, -1)): one partial block, one full block, a second block of one row
ROW_TILE = 32
ROW_TILES = [
    Case("rowtile-31x513", 31, 513, 1, [("col", 331, 513)], total=21, events=[("p", 31), ("q", 513)]),
    Case("rowtile-32x513", 32, 513, 1, [("col", 34, 513)], total=26, events=[("p", 32), ("q", 513)]),
    Case("rowtile-33x513", 33, 513, 1, [("col", 47, 513)], total=23, events=[("p", 33), ("q", 513)]),
]
# the shape every (tr, nt) of launch_db runs: 61 rows end every tile depth's last block early, column 513 is a tile's second
RAGGED = Case("ragged-61x513", 61, 513, 1, [("col", 79, 513)], total=51, events=[("p", 61), ("q", 513)])
# ends: NOFEAS found by k_da (no entering column) inside a fused stretch; the OPT ends of the cases above are k_da's too
ENDS = [Case("nofeas-40x1024", 40, 1024, 1, total=31, status=capi.NOFEAS, infeasible_seed=9)]
# pivot limits that end a call on the last fused pivot queued, on an opening pivot, on a batch of one generic pivot and behind
# five fused ones; every call restarts the devex weights, so the totals differ from the one-call solves above
LIMIT_CALLS = (12, 1, 2, 7, None)
LIMITS = [
    Case("limits-60x513", 60, 513, 6, C513, calls=LIMIT_CALLS, total=87),
    Case("limits-1025x60", 1025, 60, 1, R1025, calls=LIMIT_CALLS, total=163),
]
# the stall count hands the solve to Bland's rule: for a few pivots at 1025x60, after which the fused pair takes the solve back;
# for most of the solve at 60x513, where no batch ever opens with the count below the limit and the pair is refused
# throughout (limit 1) or stopped after its first pivot (limit 3).  STALL_FUSED is total - len(generic_indices(..)) with the
# log's degenerate pivots, computed and asserted by the CPU companion
STALLS = [
    Case("stall1-1025x60", 1025, 60, 1, R1025, total=178, stall_limit=1, bland=6),
    Case("stall3-1025x60", 1025, 60, 1, R1025, total=192, stall_limit=3, bland=3),
    Case("stall1-60x513", 60, 513, 6, C513, total=894, stall_limit=1, bland=825),
    Case("stall3-60x513", 60, 513, 6, C513, total=555, stall_limit=3, bland=484),
]
STALL_FUSED = {"stall1-1025x60": 158, "stall3-1025x60": 156, "stall1-60x513": 0, "stall3-60x513": 1}
CASES = COLUMNS + ROWS + COLUMN_TILES + [RAGGED] + ENDS + LIMITS + STALLS


def expected_fused(case):
    """Pivots the fused pair takes under mvx_set_dual_fused(2): from the schedule alone, or the table where it needs the log"""
    if case.stall_limit is not None:
        return STALL_FUSED[case.name]
    return case.total - len(case_generic(case))


# ------------------------------------------------------------------------------------------------ warm starts
WARM_ILP = (61, 513, 4, 3)  # synth.dense_ilp(m, n, seed, U)
WARM_COLUMNS = 6  # both branches of the first six fractional columns
WARM_CUTS = 4  # repaired GMI cuts of the root appended in front of the second family: 61 -> 65 rows, past the 64 | 65 tile edge
# pivots of each re-solve on the oracle: children of the root, the cut appends, children of the root with its cuts
WARM_PIVOTS = {"children": [5, 13, 5, 20, 6, 8, 4, 19, 1, 16, 12, 10], "cuts": [3, 7, 4, 6], "cut-children": [5, 6, 2, 18, 10, 10, 1, 30, 15, 2, 14, 11]}


def warm_fused(total):
    return total - len(generic_indices(total, True, (None,)))


def warm_root(api):
    A, b, c, U = synth.dense_ilp(*WARM_ILP)
    P = synth.load_ilp(api, A, b, c, U)
    assert P.simplex() == 0
    return P


def warm_branches(orc_root):
    """[(column, up, (lo, hi))] of the first fractional columns of the oracle's handle"""
    x = orc_root.col_prim()
    return [(j, up, th.child_bounds(x, j, up, float(WARM_ILP[3]))) for j in th.fractional_columns(x)[:WARM_COLUMNS] for up in (0, 1)]


def warm_child(api, root, branch):
    j, up, (lo, hi) = branch
    k = root.copy()
    api.set_col_bnds(k.h, j, capi.DB, lo, hi)
    return k


def warm_cuts(orc, orc_root):
    """(vals, rhs) of the first WARM_CUTS repaired GMI cuts of the oracle's root"""
    _, cuts = th.oracle_round(orc, orc_root)
    return [(vals, rhs) for rc, vals, rhs in cuts[1] if rc == 0][:WARM_CUTS]
