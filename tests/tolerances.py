"""The three simplex tolerances (tol_bnd, tol_dj, tol_piv of mvx_smcp) on every selection path: instances and constants
shared by test_tolerances_inputs.py (CPU: the oracle alone proves that each field of each tolerance set changes what the
solve does on each instance, that the oracle ends in time and that its end states carry the certificate of their status
under the call's own tolerances) and test_gpu_tolerances.py (GPU: the engine against the oracle, bitwise, under the same
`parm`, on each path).

Every coarse value is a power of two, so lb - tol * (1 + |lb|), the comparison with a reduced cost and the comparison
with a pivot candidate are exact on dyadic data.  The definitions restated here are kernels.hip's (and the oracle's):

    a row blocks / a column is a dual ratio candidate     |a| >  tol_piv        (strict)
    a column is eligible                                  |d| >  tol_dj         (strict)
    a basic variable is below its lower bound             beta < lb - tol_bnd * (1 + |lb|)      (strict, relative)
    ... above its upper bound                             beta > ub + tol_bnd * (1 + |ub|)

Nothing here was chosen by looking at the engine: the figures beside each case are the oracle's."""
import ctypes as C

import numpy as np

from mvolps_amd import capi, synth
from mvolps_amd.capi import DB, EITLIM, FEAS, FX, INFEAS, LO, MAX, NOFEAS, OPT, UNBND, UP

from . import general_at_size as ga

# ------------------------------------------------------------------------------------------------ tolerance sets
T9 = 1e-9
DEFAULT = (T9, T9, T9)
BND = (2.0 ** -10, T9, T9)
DJ = (T9, 2.0 ** -5, T9)
PIV = (T9, T9, 2.0 ** -6)
ALL = (2.0 ** -10, 2.0 ** -5, 2.0 ** -6)
GLPK = (1e-7, 1e-7, 1e-9)
SETS = {"DEFAULT": DEFAULT, "BND": BND, "DJ": DJ, "PIV": PIV, "ALL": ALL}
SINGLE = ("BND", "DJ", "PIV")  # one field coarse, the other two at their defaults
SAFETY_CAP = 20000  # pivots: no (case, set) pair of the table comes near it (the 4x rule is the tighter one)


def smcp(api, tol, it_lim=None):
    parm = capi.Smcp()
    api.init_smcp(C.byref(parm))
    parm.tol_bnd, parm.tol_dj, parm.tol_piv = tol
    if it_lim is not None:
        parm.it_lim = it_lim
    return parm


class default_tolerances:
    """with default_tolerances(apis, tol): ... -- what a NULL `parm` means, (1e-9, 1e-9, 1e-9) again on the way out"""

    def __init__(self, apis, tol):
        self.apis, self.tol = apis, tol

    def __enter__(self):
        for a in self.apis:
            a.set_default_tolerances(*self.tol)

    def __exit__(self, *exc):
        for a in self.apis:
            a.set_default_tolerances(*DEFAULT)
        return False


# ------------------------------------------------------------------------------------------------ sensitive_lp
ROW_SCALE, ROW_SCALE_EVERY, ROW_SCALE_AT = 2.0 ** -9, 7, 3
NEAR_ROW, NEAR_LB = 5, 2.0 ** -12


def sensitive_lp(m, n, seed):
    """max c x over synth.dense_lp with (indices from 0) rows i % 7 == 3 scaled, right-hand side included, by 2^-9 -- the
    same polytope, entries below a coarse tol_piv --, row 5 turned into a x >= 2^-12 -- violated at the slack point by less
    than a coarse tol_bnd allows --, and two columns in three boxed: (DB, 0, 0.5 + j % 3) where j % 3 != 0."""
    A, b, c = synth.dense_lp(m, n, seed)
    A, b = A.copy(), b.copy()
    rows = np.arange(m) % ROW_SCALE_EVERY == ROW_SCALE_AT
    A[rows] *= ROW_SCALE
    b[rows] *= ROW_SCALE
    row_b = [(UP, 0.0, float(v)) for v in b]
    row_b[NEAR_ROW] = (LO, NEAR_LB, 0.0)
    col_b = [(DB, 0.0, 0.5 + (j % 3)) if j % 3 else (LO, 0.0, 0.0) for j in range(n)]
    return dict(A=A, row_b=row_b, col_b=col_b, c=c, direction=MAX, x0=None)


load = ga.load  # an instance dict on a handle of `api`
model = ga.model  # ... as a certify.Model


# ------------------------------------------------------------------------------------------------ near children
NEAR_GAP = 2.0 ** -11


def fractional_columns(x):
    return [j + 1 for j in range(len(x)) if abs(x[j] - round(x[j])) > 1e-6]


def near_children(api, P, tol, count=3, solve=True):
    """P: a root of synth.dense_ilp solved on `api`.  For its first `count` fractional columns j two clones: "near", upper
    bound x_j - 2^-11 (violated, but by less than a coarse tol_bnd: no pivot under 2^-10, one dual pivot under 1e-9), and
    "down", upper bound floor(x_j).  Each is solved under `tol` unless solve is False.  [(j, kind, upper bound, clone, rc)]"""
    x = P.col_prim()
    out = []
    for j in fractional_columns(x)[:count]:
        for kind, ub in (("near", float(x[j - 1] - NEAR_GAP)), ("down", float(np.floor(x[j - 1])))):
            k = P.copy()
            api.set_col_bnds(k.h, j, DB, 0.0, ub)
            rc = k.simplex(tol=tol) if solve else None
            out.append((j, kind, ub, k, rc))
    return out


def child_models(M, kids):
    """certify.Model of each child of near_children"""
    out = []
    for j, kind, ub, k, rc in kids:
        Mc = M.copy()
        Mc.set_col_bnds(j, DB, 0.0, ub)
        out.append(Mc)
    return out


# ------------------------------------------------------------------------------------------------ boundary models
# Small constructed LPs inside inert padding of the shape of a path (section "the case table").  The decision under test
# is taken on entries, costs and values that are still the data -- exactly, since every pivot made before it lies in a
# block of its own (`lead` columns LEAD_AT with costs 8, 4, 2, each with a single 1 in its own row of LEAD_AT and
# right-hand side 1: priced first, largest cost first, and a pivot on them changes no entry outside their rows).  With
# lead = 0 the decision is the call's first; with lead = 3 and chains of five it is the fourth step of a chain, chosen by
# the path's own kernel from the slices it carried through three pivots.
POSITIONS = (1, 64, 65, 256, 257, -1)  # -1: the last row / column; a lane tail, a second wave, a second workgroup
POSITIONS_ON_DEVICE = (1, 65, -1)  # the GPU file's loop, thinned by index: its first device run took longer than test_gpu_thresholds.py
LEAD_AT = (10, 11, 12)
LEADS = (0, 3)
OTHER_AT = 20  # the second row of the pivot model, the repairing column of the bound model
EPS = 2.0 ** -52


def place(pos, size):
    """1-based index of a position in a dimension of `size`, or None where the dimension does not reach it"""
    k = size if pos == -1 else pos
    return k if k <= size else None


def _blank(m, n):
    """Padding: zero costs, rows x <= 1, columns >= 0, entries k / 4 over the padding rows and columns"""
    i, j = np.arange(m)[:, None], np.arange(n)[None, :]
    A = ((7 * i + 3 * j) % 5) / 4.0
    return A, [(UP, 0.0, 1.0)] * m, [(LO, 0.0, 0.0)] * n, np.zeros(n)


def _lead(A, row_b, c, lead):
    for t, k in enumerate(LEAD_AT[:lead]):
        A[k - 1, :] = 0.0
        A[:, k - 1] = 0.0
        A[k - 1, k - 1] = 1.0
        row_b[k - 1] = (UP, 0.0, 1.0)
        c[k - 1] = float(2 ** (lead - t))


def _inst(A, row_b, col_b, c):
    return dict(A=A, row_b=list(row_b), col_b=list(col_b), c=c, direction=MAX, x0=None)


def dj_model(m, n, pos, above, lead=0):
    """Every cost <= 2^-5, columns 2, 63, 66 and n - 1 exactly 2^-5, the others k / 256 with k < 8; `above` raises the
    column at `pos` to 2^-5 (1 + 2^-52).  Under DJ: no column is eligible (OPT after `lead` pivots); with `above` exactly
    that one is, and after one more pivot it is basic.  Returns (instance, column)."""
    A, row_b, col_b, c = _blank(m, n)
    A = A + 0.25  # every entry positive: whatever enters is blocked
    c = (np.arange(n) % 8) / 256.0
    q = place(pos, n)
    for k in (2, 63, 66, n - 1, q):
        c[k - 1] = 2.0 ** -5
    if above:
        c[q - 1] = 2.0 ** -5 * (1.0 + EPS)
    _lead(A, row_b, c, lead)
    return _inst(A, row_b, col_b, c), q


def piv_model(m, n, pos, above, lead=0):
    """One eligible column q (cost 1) at column `pos`.  Row r1 (at row `pos`, or the last row where m does not reach it)
    holds 2^-6 in it over a right-hand side 2^-20 -- ratio 2^-14, it would win --, row r2 = 20 holds 1 over 1, no other row
    holds anything in q.  Under PIV r1 is not a candidate (2^-6 > 2^-6 is false) and r2 leaves; with `above`, 2^-6 (1 +
    2^-52), r1 leaves.  Returns (instance, q, r1, r2)."""
    A, row_b, col_b, c = _blank(m, n)
    q = place(pos, n)
    r1 = place(pos, m) or m
    r2 = OTHER_AT
    A[:, q - 1] = 0.0
    A[r1 - 1, :] = 0.0
    A[r2 - 1, :] = 0.0
    A[r1 - 1, q - 1] = 2.0 ** -6 * (1.0 + EPS) if above else 2.0 ** -6
    A[r2 - 1, q - 1] = 1.0
    row_b[r1 - 1] = (UP, 0.0, 2.0 ** -20)
    row_b[r2 - 1] = (UP, 0.0, 1.0)
    c[q - 1] = 1.0
    _lead(A, row_b, c, lead)
    return _inst(A, row_b, col_b, c), q, r1, r2


def bnd_model(m, n, pos, below, lead=0):
    """Row s (at row `pos`, or the last row) is e x_f + x_h >= 1 with x_f fixed at 1 (column `pos`) and x_h >= 0 (column 20,
    cost -1).  With e = 1 - 2^-9 its value at the slack point is lb - tol_bnd (1 + |lb|) exactly under BND: not below it,
    the start is primal feasible, the primal simplex takes the call and makes the `lead` pivots; with the next double
    below (`below`) the row is infeasible and one pivot more brings x_h into it.  Returns (instance, s, h)."""
    A, row_b, col_b, c = _blank(m, n)
    f = place(pos, n)
    s = place(pos, m) or m
    h = OTHER_AT
    A[:, f - 1] = 0.0
    A[:, h - 1] = 0.0
    A[s - 1, :] = 0.0
    e = 1.0 - 2.0 ** -9
    A[s - 1, f - 1] = np.nextafter(e, 0.0) if below else e
    A[s - 1, h - 1] = 1.0
    row_b[s - 1] = (LO, 1.0, 0.0)
    col_b[f - 1] = (FX, 1.0, 1.0)
    c[h - 1] = -1.0
    _lead(A, row_b, c, lead)
    return _inst(A, row_b, col_b, c), s, h


def boundary_outcomes(m, n, pos, lead):
    """Every boundary model at one position: (name, instance, tolerances, pivot limit, expected) where expected is
    (rc, status, pivots, {tableau row: the variable basic in it}) -- derived by hand from the definitions above, never
    taken from an engine.  Where the pivot limit equals the pivots expected, rc and status are None: whether a solve that is
    optimal exactly at its limit reports the optimum or the limit is not a matter of the tolerances (the engine has to say
    what the oracle says)."""
    out = []
    inst, q = dj_model(m, n, pos, False, lead)
    out.append(("dj-equal", inst, DJ, None, (0, OPT, lead, {})))
    inst, q = dj_model(m, n, pos, True, lead)
    out.append(("dj-above", inst, DJ, lead + 1, (None, None, lead + 1, {"basic": m + q})))
    inst, q, r1, r2 = piv_model(m, n, pos, False, lead)
    out.append(("piv-equal", inst, PIV, lead + 1, (None, None, lead + 1, {r2: m + q, r1: r1})))
    inst, q, r1, r2 = piv_model(m, n, pos, True, lead)
    out.append(("piv-above", inst, PIV, lead + 1, (None, None, lead + 1, {r1: m + q, r2: r2})))
    inst, s, h = bnd_model(m, n, pos, False, lead)
    out.append(("bnd-equal", inst, BND, None, (0, OPT, lead, {s: s})))
    inst, s, h = bnd_model(m, n, pos, True, lead)
    out.append(("bnd-below", inst, BND, None, (0, OPT, lead + 1, {s: m + h})))
    return out


def assert_outcome(P, rc, expected, what):
    erc, est, epiv, rows = expected
    assert P.it_cnt == epiv and (erc is None or (rc, P.status) == (erc, est)), (what, rc, P.status, P.it_cnt, expected)
    head = P.basis()[0]
    for r, k in rows.items():
        if r == "basic":
            assert k in head[1:].tolist(), (what, "variable %d is not basic" % k)
        else:
            assert head[r] == k, (what, "row %d holds variable %d, expected %d" % (r, head[r], k))


# ------------------------------------------------------------------------------------------------ the case table
class LpCase:
    """One LP solved in limited calls (`calls`: pivot limits, None = to the end) under each set of `sets`;
    figures[set] = [(rc, status, pivots so far) per call] is the oracle's."""

    fields = SINGLE

    def __init__(self, name, family, m, n, seed, calls, figures, dropped=()):
        self.name, self.family, self.m, self.n, self.seed, self.calls, self.figures, self.dropped = name, family, m, n, seed, calls, figures, dropped

    @property
    def sets(self):
        return list(self.figures)

    def instance(self):
        return sensitive_lp(self.m, self.n, self.seed) if self.family == "sensitive" else ga.general_lp(self.m, self.n, self.seed)

    def __repr__(self):
        return self.name


class ChildCase:
    """A root of synth.dense_ilp(m, n, seed, U) solved under the set (own_root) or under DEFAULT, then near_children of
    it under the set; figures[set] = ((rc, status, pivots) of the root, [(rc, status, pivots) per child]) is the oracle's."""

    def __init__(self, name, m, n, seed, U, count, own_root, fields, figures, dropped=()):
        self.name, self.m, self.n, self.seed, self.U, self.count, self.own_root = name, m, n, seed, U, count, own_root
        self.fields, self.figures, self.dropped = fields, figures, dropped

    @property
    def sets(self):
        return list(self.figures)

    def data(self):
        return synth.dense_ilp(self.m, self.n, self.seed, self.U)

    def __repr__(self):
        return self.name


def run_calls(P, calls, tol):
    stops = []
    for lim in calls:
        rc = P.simplex(it_lim=-1 if lim is None else lim, tol=tol)
        stops.append((rc, P.status, P.it_cnt))
        if rc != EITLIM:
            break
    return stops


def run_children(api, case, tol):
    """(root, its figure, children of near_children, their figures) on `api`"""
    A, b, c, U = case.data()
    root = synth.load_ilp(api, A, b, c, U)
    rc = root.simplex(tol=tol if case.own_root else DEFAULT)
    kids = near_children(api, root, tol, case.count)
    return root, (rc, root.status, root.it_cnt), kids, [(k[4], k[3].status, k[3].it_cnt) for k in kids]


E, F, I = EITLIM, FEAS, INFEAS
FIGURES = {
    "default-96x160": {
        "DEFAULT": [(E, F, 7), (E, F, 27), (0, OPT, 44)],
        "BND": [(E, F, 7), (E, F, 27), (0, OPT, 52)],
        "DJ": [(E, F, 7), (E, F, 27), (0, OPT, 42)],
        "PIV": [(E, F, 7), (E, F, 27), (0, NOFEAS, 45)],
        "ALL": [(E, F, 7), (E, F, 27), (0, OPT, 46)],
    },
    "chain-300x700": {
        "DEFAULT": [(E, F, 7), (0, OPT, 172)],
        "BND": [(E, F, 7), (0, OPT, 239)],
        "DJ": [(E, F, 7), (0, OPT, 161)],
        "PIV": [(E, F, 7), (0, OPT, 391)],
        "ALL": [(E, F, 7), (0, OPT, 250)],
    },
    "persist-200x300": {
        "DEFAULT": [(E, F, 7), (E, F, 57), (0, OPT, 193)],
        "BND": [(E, F, 7), (E, F, 57), (0, OPT, 150)],
        "DJ": [(E, F, 7), (E, F, 57), (0, OPT, 186)],
        "PIV": [(E, F, 7), (E, F, 57), (0, OPT, 282)],
        "ALL": [(E, F, 7), (E, F, 57), (0, NOFEAS, 57)],
    },
    "phase1-62x40": {
        "DEFAULT": [(E, I, 10), (E, F, 120), (0, OPT, 128)],
        "BND": [(E, I, 10), (E, F, 120), (0, OPT, 135)],
        "DJ": [(E, I, 10), (E, F, 120), (0, OPT, 127)],
        "PIV": [(E, I, 10), (E, F, 120), (0, OPT, 127)],
        "ALL": [(E, I, 10), (E, F, 120), (0, OPT, 128)],
    },
    "children-128x256": {
        "DEFAULT": ((0, OPT, 117), [(0, OPT, 118), (0, OPT, 132), (0, OPT, 118), (0, OPT, 123), (0, OPT, 118), (0, OPT, 127), (0, OPT, 118), (0, OPT, 125)]),  # oracle: 0.01s
        "BND": ((0, OPT, 117), [(0, OPT, 117), (0, OPT, 132), (0, OPT, 117), (0, OPT, 123), (0, OPT, 117), (0, OPT, 127), (0, OPT, 117), (0, OPT, 125)]),  # oracle: 0.01s
        "DJ": ((0, OPT, 109), [(0, OPT, 113), (0, OPT, 131), (0, OPT, 112), (0, OPT, 114), (0, OPT, 113), (0, OPT, 117), (0, OPT, 114), (0, OPT, 119)]),  # oracle: 0.01s
        "PIV": ((0, OPT, 129), [(0, OPT, 130), (0, OPT, 144), (0, OPT, 130), (0, OPT, 135), (0, OPT, 130), (0, OPT, 139), (0, OPT, 131), (0, OPT, 135)]),  # oracle: 0.01s
        "ALL": ((0, OPT, 127), [(0, OPT, 127), (0, OPT, 143), (0, OPT, 127), (0, OPT, 135), (0, OPT, 127), (0, OPT, 137), (0, OPT, 127), (0, OPT, 137)]),  # oracle: 0.01s
    },
    "children-1000x2001": {
        "DEFAULT": ((0, OPT, 1436), [(0, OPT, 1437), (0, OPT, 1446), (0, OPT, 1437), (0, OPT, 1475), (0, OPT, 1437), (0, OPT, 1480)]),  # oracle: 0.62s
        "BND": ((0, OPT, 1436), [(0, OPT, 1436), (0, OPT, 1444), (0, OPT, 1436), (0, OPT, 1475), (0, OPT, 1436), (0, OPT, 1475)]),  # oracle: 0.73s
        "DJ": ((0, OPT, 1436), [(0, OPT, 1437), (0, OPT, 1446), (0, OPT, 1437), (0, OPT, 1475), (0, OPT, 1437), (0, OPT, 1480)]),  # oracle: 0.67s
        "PIV": ((0, OPT, 1436), [(0, OPT, 1437), (0, OPT, 1446), (0, OPT, 1437), (0, OPT, 1483), (0, OPT, 1437), (0, OPT, 1493)]),  # oracle: 0.68s
        "ALL": ((0, OPT, 1436), [(0, OPT, 1436), (0, OPT, 1444), (0, OPT, 1436), (0, OPT, 1471), (0, OPT, 1436), (0, OPT, 1482)]),  # oracle: 0.66s
    },
}

# name, family, m, n, seed, calls.  The seeds of the sensitive_lp cases are the first (of 1..39, under the case's schedule)
# at which every set ends on the oracle within four times the DEFAULT pivots and each single-field set leaves the DEFAULT
# pivot count or basis; at 300x700 most seeds run to the pivot cap under PIV or ALL (the rows a coarse tol_piv skips end
# up violated, or the solve stalls) -- the documented meaning of a coarse tolerance, such seeds are not used.  No
# (case, set) pair of the seeds kept had to be dropped.  phase1-62x40 is general_at_size's smallest phase-1 shape.
LP_CASES = [
    LpCase("default-96x160", "sensitive", 96, 160, 3, (7, 20, None), FIGURES["default-96x160"]),
    LpCase("chain-300x700", "sensitive", 300, 700, 37, (7, None), FIGURES["chain-300x700"]),
    LpCase("persist-200x300", "sensitive", 200, 300, 1, (7, 50, None), FIGURES["persist-200x300"]),
    LpCase("phase1-62x40", "general", 62, 40, 4, (10, 110, None), FIGURES["phase1-62x40"]),
]
# name, m, n, seed, U, fractional columns, root under the set itself, fields that must matter.  At 1000x2001 the root is
# solved under DEFAULT for every set: under PIV and ALL the oracle's root runs past four times the DEFAULT pivots (seeds 1,
# 2, 3, 7), and the children of a root that is optimal only to tol_dj = 2^-5 stall in the dual simplex for hundreds of
# pivots.  From a DEFAULT root tol_dj decides nothing in a dual re-solve (k_dboot / k_da do not read it): DJ is run there
# and must equal the oracle, but only tol_bnd and tol_piv are asserted to matter.
CHILD_CASES = [
    ChildCase("children-128x256", 128, 256, 7, 3, 4, True, SINGLE, FIGURES["children-128x256"]),
    ChildCase("children-1000x2001", 1000, 2001, 7, 3, 3, False, ("BND", "PIV"), FIGURES["children-1000x2001"]),
]
CASES = LP_CASES + CHILD_CASES
NO_CERTIFICATE = "skipped rows, no certificate expected"  # NOFEAS under PIV or ALL: never passed to certify_nofeas


def by_name(name):
    return next(c for c in CASES if c.name == name)


def case_id(case):
    return case.name


def tol_kw(tol):
    return dict(tol_bnd=tol[0], tol_dj=tol[1], tol_piv=tol[2])


# ------------------------------------------------------------------------------------------------ B&B leg
BNB_CASE, BNB_NODES = (128, 256, 7, 3), 200  # the 128x256 ILP of the children, a 200-node prefix


# ------------------------------------------------------------------------------------------------ certificates
def certify_opt_at_size(M, P, tol, what=""):
    """OPT at a size where certify.py's longdouble factor takes minutes (1000 x 2001), in fp64 as in test_gpu_certify's
    headline test: the values obey the row equations and every bound to tol_bnd (1 + |bound|), the reduced costs
    c_N - c_B B^-1 N (one solve with B^T, refined once) have the sign of their status to tol_dj and equal the handle's
    duals; the slack on each is 16 RTOL growth, the reference being fp64 itself."""
    from . import certify as cf
    from mvolps_amd.capi import NL, NU

    m, n = M.m, M.n
    head, nb, flag = (np.asarray(v[1:], dtype=np.int64) for v in P.basis())
    assert sorted(np.concatenate([head, nb]).tolist()) == list(range(1, m + n + 1)), what
    Mfull = np.hstack([np.eye(m), -M.A])
    B, N = Mfull[:, head - 1], Mfull[:, nb - 1]
    growth = float(np.abs(np.linalg.inv(B)).sum(axis=1).max() * (1.0 + np.abs(M.A).sum(axis=1).max()))
    slack = 16 * cf.RTOL * growth
    xr, xs = P.row_prim(), P.col_prim()
    assert np.all(np.abs(M.A @ xs - xr) <= slack * (1.0 + np.abs(M.A) @ np.abs(xs))), "%s: row_prim != A col_prim" % what
    lo, hi = M.lo_hi()
    x = np.concatenate([xr, xs])
    with np.errstate(invalid="ignore"):
        low = np.where(np.isfinite(lo), (lo - x) / (1.0 + np.abs(lo)), 0.0).max()
        high = np.where(np.isfinite(hi), (x - hi) / (1.0 + np.abs(hi)), 0.0).max()
    assert max(low, high) <= tol[0] + slack, "%s: OPT but a bound is violated by %.3g" % (what, max(low, high))
    cost = np.concatenate([np.zeros(m), M.c])
    y = np.linalg.solve(B.T, cost[head - 1])
    y = y + np.linalg.solve(B.T, cost[head - 1] - B.T @ y)
    d = cost[nb - 1] - y @ N
    lim = tol[1] + slack * (1.0 + np.abs(d))
    sgn = 1.0 if M.dir == MAX else -1.0
    assert np.all((flag != NL) | (sgn * d <= lim)) and np.all((flag != NU) | (sgn * d >= -lim)), "%s: OPT but a reduced cost improves" % what
    dual = np.zeros(m + n)
    dual[nb - 1] = d
    got = np.array([P.api.get_row_dual(P.h, i) for i in range(1, m + 1)] + [P.api.get_col_dual(P.h, j) for j in range(1, n + 1)])
    assert np.all(np.abs(got - dual) <= slack * (1.0 + np.abs(dual))), "%s: duals differ from the recomputed reduced costs" % what


def certify_end(M, P, tol, what=""):
    """The certificate of an end state under the call's tolerances.  NOFEAS under a coarse tol_piv is not certified (rows
    the ratio test skipped end up violated: the final basis need not hold a Farkas combination)."""
    from . import certify as cf

    if P.status == NOFEAS and tol[2] > T9:
        return NO_CERTIFICATE
    if (M.m + 1) * (M.n + 1) > 1500000:
        assert P.status == OPT, what
        return certify_opt_at_size(M, P, tol, what)
    return cf.certify(M, P, what=what, **tol_kw(tol))
