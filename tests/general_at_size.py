"""General-bound LPs at kernel scale, shared by test_general_at_size_inputs.py (CPU: the oracle alone proves each instance
has the property its GPU test relies on, and the certificates of tests/certify.py hold on the oracle's end states) and
test_gpu_general_at_size.py (GPU: the engine against the oracle, bitwise, at every stop of a call schedule, then the
certificate of the end state and the feasibility witness).

Two families.  `general_lp` is lpgen.random_general_lp's recipe at a fixed shape: every bound type on rows and columns,
integer data, built around a point x0, so the slack basis is neither primal nor dual feasible and the solve starts in
phase 1 with free, fixed and upper-bounded non-basic columns.  `cold_dual_lp` is a minimisation whose slack basis is dual
feasible and primal infeasible: the dual simplex runs from pivot 0 and its ratio test meets NF and NU columns.  Each has
an infeasible variant (two rows that contradict each other).

CASES is the shape table.  A case is solved in limited calls (`calls`: pivot limits, None = to the end); the figures
beside each case (`stops`, `p1`, `secs`) were measured on the oracle alone and are asserted by the CPU companion: the
status and pivot count at every stop and the pivot at which phase 1 ended; `secs`, the oracle's time for the schedule,
is printed beside the measured one, not asserted.  Nothing here was chosen by looking at the engine."""
import numpy as np

from mvolps_amd.capi import DB, FR, FX, LO, MAX, MIN, UP, EITLIM, FEAS, INFEAS, NOFEAS, OPT, UNBND

from . import lpgen

WAVE, P1_LANES, P1_FIX_BLOCK, P1_FIX_UNROLL, PRICE_LANES = 64, 1024, 256, 8, 1024  # kernels.hip: k_p1_head, k_p1_fix, dev_price
CHAIN_WG = 256  # k_chain: rows / columns per workgroup, nw = ceil(max(m, n) / 256)
DUAL_FUSED_MIN, DUAL_FUSED_MAX = 2000000, 12000000  # engine.cpp dual_fused_worth_it: (m + 1)(n + 1) entries
P1_BATCHES = (4, 8, 16, 32, 64)  # engine.cpp: phase-1 iterations queued per host round trip


def general_lp(m, n, seed):
    """lpgen.random_general_lp's body at the shape m x n (its two leading draws, the shape, are not made): feasible by
    construction, x0 is a point of it."""
    rng = np.random.default_rng(seed)
    A = np.round(rng.normal(size=(m, n)) * 3)
    A[rng.random((m, n)) < 0.3] = 0
    x0 = rng.integers(0, 4, size=n).astype(float)
    act = A @ x0
    row_b, col_b = [], []
    for i in range(m):
        t = int(rng.choice([LO, UP, DB, FX, FR], p=[0.25, 0.35, 0.2, 0.1, 0.1]))
        l = act[i] - rng.integers(0, 3)
        u = act[i] + rng.integers(0, 3)
        if t == FX:
            l = u = act[i]
        if t == DB and l == u:
            u = l + 1
        row_b.append((t, float(l), float(u)))
    for j in range(n):
        t = int(rng.choice([LO, UP, DB, FX, FR], p=[0.4, 0.1, 0.35, 0.05, 0.1]))
        l = x0[j] - rng.integers(0, 3)
        u = x0[j] + rng.integers(0, 4)
        if t == FX:
            l = u = x0[j]
        if t == DB and l == u:
            u = l + 1
        col_b.append((t, float(l), float(u)))
    c = np.round(rng.normal(size=n) * 5)
    direction = int(rng.choice([MIN, MAX]))
    return dict(A=A, row_b=row_b, col_b=col_b, c=c, direction=direction, x0=x0)


def cold_dual_lp(m, n, seed):
    """min c x around a point x0: columns LO / DB with c >= 1, UP with c <= -1, one in twelve FR with c = 0; rows LO / DB /
    FX around A x0.  Every non-basic column of the slack basis has a reduced cost of the right sign (dual feasible) and
    the slack point, which is not x0, violates most rows (primal infeasible)."""
    rng = np.random.default_rng(seed)
    A = np.round(rng.normal(size=(m, n)) * 3)
    A[rng.random((m, n)) < 0.3] = 0
    x0 = rng.integers(1, 5, size=n).astype(float)
    act = A @ x0
    row_b, col_b = [], []
    c = np.zeros(n)
    for i in range(m):
        t = int(rng.choice([LO, DB, FX], p=[0.55, 0.35, 0.1]))
        l = act[i] - rng.integers(0, 3)
        u = act[i] + rng.integers(1, 4)
        if t == FX:
            l = u = act[i]
        row_b.append((t, float(l), float(u)))
    for j in range(n):
        t = int(rng.choice([LO, DB, UP, FR], p=[0.45, 0.35, 0.12, 0.08]))
        l = x0[j] - rng.integers(1, 4)
        u = x0[j] + rng.integers(1, 4)
        col_b.append((t, float(l), float(u)))
        mag = float(rng.integers(1, 10))
        c[j] = 0.0 if t == FR else (-mag if t == UP else mag)
    return dict(A=A, row_b=row_b, col_b=col_b, c=c, direction=MIN, x0=x0)


def infeasible(inst, seed):
    """The instance plus two rows that contradict each other, r x >= L and r x <= L - 1 (test_certify.infeasible_general_lp);
    a cold-dual instance keeps its dual feasible slack basis, rows do not touch the reduced costs."""
    rng = np.random.default_rng(seed)
    n = inst["A"].shape[1]
    r = np.round(rng.normal(size=n) * 2)
    r[0] = r[0] or 1.0
    L = float(rng.integers(-3, 4))
    out = dict(inst)
    out["A"] = np.vstack([inst["A"], r, r])
    out["row_b"] = inst["row_b"] + [(LO, L, 0.0), (UP, 0.0, L - 1.0)]
    out["x0"] = None
    return out


def load(api, inst):
    P = api.create()
    P.load_general(inst["A"], inst["row_b"], inst["col_b"], inst["c"], direction=inst["direction"])
    return P


def model(inst):
    from . import certify as cf

    return cf.Model(inst["A"], inst["row_b"], inst["col_b"], inst["c"], direction=inst["direction"])


def witness_holds(inst):
    """x0 against every row and column bound in exact arithmetic: the data are integers held in doubles, so int64 is exact
    (|A x0| stays far below 2^63)."""
    A, x0 = inst["A"], inst["x0"]
    rlo, rhi = lpgen.bounds_arrays(inst["row_b"])
    clo, chi = lpgen.bounds_arrays(inst["col_b"])
    for v in (A, x0, rlo[np.isfinite(rlo)], rhi[np.isfinite(rhi)], clo[np.isfinite(clo)], chi[np.isfinite(chi)]):
        assert np.array_equal(v, np.round(v)) and np.abs(v).max(initial=0) < 2 ** 31
    xi = x0.astype(np.int64)
    act = A.astype(np.int64) @ xi

    def inside(v, lo, hi):
        ok_lo = np.array([not np.isfinite(l) or int(a) >= int(l) for a, l in zip(v, lo)])
        ok_hi = np.array([not np.isfinite(h) or int(a) <= int(h) for a, h in zip(v, hi)])
        return bool(ok_lo.all() and ok_hi.all())

    return inside(xi, clo, chi) and inside(act, rlo, rhi)


# ------------------------------------------------------------------------------------------------ slack-basis facts
def slack_point(inst):
    """Values of the structural columns at the slack basis (NL: lb, NU: ub, NF: 0, NS: lb) and their flags"""
    from mvolps_amd.capi import NF, NL, NS, NU

    x, flag = [], []
    for t, l, u in inst["col_b"]:
        f = {LO: NL, DB: NL, UP: NU, FR: NF, FX: NS}[t]
        flag.append(f)
        x.append(u if f == NU else (0.0 if f == NF else l))
    return np.array(x), np.array(flag)


def slack_signs(inst, tol=1e-9):
    """g of phase 1's first iteration: +1 where the row's auxiliary lies below its lower bound at the slack point, -1 above
    its upper bound, 0 where it is feasible (index 0 = row 1)"""
    x, _ = slack_point(inst)
    act = inst["A"] @ x
    lo, hi = lpgen.bounds_arrays(inst["row_b"])
    g = np.zeros(len(act), dtype=int)
    with np.errstate(invalid="ignore"):
        g[np.isfinite(lo) & (act < lo - tol * (1 + np.abs(np.where(np.isfinite(lo), lo, 0))))] = 1
        g[np.isfinite(hi) & (act > hi + tol * (1 + np.abs(np.where(np.isfinite(hi), hi, 0))))] = -1
    return g


def slack_dual_infeasibilities(inst, tol=1e-9):
    """Columns of the slack basis whose reduced cost (c itself) has the improving sign for their flag"""
    from mvolps_amd.capi import NF, NL, NU

    _, flag = slack_point(inst)
    d = (1.0 if inst["direction"] == MAX else -1.0) * inst["c"]
    up = np.isin(flag, (NL, NF)) & (d > tol)
    dn = np.isin(flag, (NU, NF)) & (d < -tol)
    return int((up | dn).sum())


def p1_chunk(m):
    """k_p1_head: rows per lane R = ceil(m / 1024); lane t owns rows t R + 1 .. (t + 1) R"""
    return -(-m // P1_LANES)


# ------------------------------------------------------------------------------------------------ the shape table
class Case:
    def __init__(self, name, family, m, n, seed, calls, stops, p1=None, secs=None, infeasible_seed=None, moves=""):
        self.name, self.family, self.m, self.n, self.seed = name, family, m, n, seed
        self.calls, self.stops, self.p1, self.secs, self.infeasible_seed, self.moves = calls, stops, p1, secs, infeasible_seed, moves

    @property
    def feasible(self):
        return self.infeasible_seed is None

    def instance(self):
        inst = (general_lp if self.family == "general" else cold_dual_lp)(self.m, self.n, self.seed)
        return inst if self.feasible else infeasible(inst, self.infeasible_seed)

    @property
    def rows(self):  # the loaded model's rows
        return self.m + (0 if self.feasible else 2)

    def __repr__(self):
        return self.name


E, I, F = EITLIM, INFEAS, FEAS
# name, family, m, n, seed, calls, stops [(rc, status, pivots so far) per call], p1 = the pivot count at which phase 1 ended
# (where the schedule has a stop past it), secs = the oracle's seconds for the schedule (three threads of a desktop CPU).  A first short call ends inside phase 1 (or inside the cold dual); where phase 2 follows, the second call is
# the one that crosses into it; None runs to the end.
CASES = [
    # phase 1 at the wave edge of k_p1_head's count and scan; 62 / 63: the cost row m + 1 closes a 4-row tile / opens one
    Case("p1-62x40", "general", 62, 40, 4, (10, 110, None), [(E, I, 10), (E, F, 120), (0, OPT, 128)], p1=102, secs=0.01, moves="cost row closes a 4-row tile of k_update"),
    Case("p1-63x40", "general", 63, 40, 1, (10, 75, None), [(E, I, 10), (E, F, 85), (0, OPT, 106)], p1=68, secs=0.01, moves="one row short of a wave; cost row opens a tile"),
    Case("p1-64x40", "general", 64, 40, 5, (10, 80, None), [(E, I, 10), (E, F, 90), (0, OPT, 118)], p1=74, secs=0.01, moves="one full wave of rows"),
    Case("p1-65x40", "general", 65, 40, 1, (10, 95, None), [(E, I, 10), (E, F, 105), (0, OPT, 122)], p1=82, secs=0.01, moves="row 65 is the second wave's only row"),
    Case("p1-65x40-infeasible", "general", 65, 40, 1, (10, None), [(E, I, 10), (0, NOFEAS, 84)], secs=0.01, infeasible_seed=9, moves="phase 1 ends NOFEAS"),
    # k_p1_fix's 256-column block edge
    Case("p1-300x255", "general", 300, 255, 2, (40, 700, None), [(E, I, 40), (E, F, 740), (0, OPT, 1093)], p1=616, secs=0.1, moves="k_p1_fix: one block, one column short"),
    Case("p1-300x256", "general", 300, 256, 2, (40, 800, None), [(E, I, 40), (E, F, 840), (0, OPT, 1195)], p1=689, secs=0.1, moves="k_p1_fix: column 256 opens the second block"),
    # dev_price's 1024-lane stride in k_p1_select; phase 2 on general flags behind it
    Case("p1-300x1023", "general", 300, 1023, 1, (40, 700, None), [(E, I, 40), (E, F, 740), (0, UNBND, 1082)], p1=598, secs=0.2, moves="k_p1_select: one column short of a stride"),
    Case("p1-300x1024", "general", 300, 1024, 2, (40, 700, None), [(E, I, 40), (E, F, 740), (0, UNBND, 1183)], p1=610, secs=0.2, moves="k_p1_select: one full stride"),
    Case("p1-300x1025", "general", 300, 1025, 3, (40, 700, None), [(E, I, 40), (E, F, 740), (0, UNBND, 1190)], p1=652, secs=0.2, moves="k_p1_select: column 1025 opens the second stride"),
    Case("p2-300x700", "general", 300, 700, 6, (40, 700, None), [(E, I, 40), (E, F, 740), (0, UNBND, 1554)], p1=570, secs=0.2, moves="k_chain with 3 workgroups; k_persist at cpw 3 with the cluster off"),
    Case("p2-700x300", "general", 700, 300, 7, (40, 5000, None), [(E, I, 40), (E, F, 5040), (0, OPT, 5328)], p1=4842, secs=0.5, moves="k_chain with 3 workgroups, rows the longer side"),
    # rows per lane of k_p1_head: R = 1 with every lane busy, R = 2 with lanes 513.. idle, R = 3
    Case("p1-1024x300", "general", 1024, 300, 4, (40, 6800, None), [(E, I, 40), (E, F, 6840), (0, OPT, 7353)], p1=6783, secs=2.2, moves="R = 1, lane 1023 owns row 1024"),
    Case("p1-1025x300", "general", 1025, 300, 1, (40, 6500, None), [(E, I, 40), (E, F, 6540), (0, OPT, 7149)], p1=6293, secs=1.9, moves="R = 2, lane 512 owns row 1025 alone"),
    Case("p2-1100x1030", "general", 1100, 1030, 2, (40, 7000, None), [(E, I, 40), (E, F, 7040), (0, OPT, 9274)], p1=5660, secs=3.3, moves="R = 2; k_chain with 5 workgroups; past k_dsel"),
    # tile depths 8 and 16 of k_update on the m + 1 grid; 40 pivots cross the 4 / 8 / 16 / 32 batch schedule of phase 1
    Case("p1-1025x8192", "general", 1025, 8192, 8, (40,), [(E, I, 40)], secs=0.6, moves="8-row tiles"),
    Case("p1-2048x8192", "general", 2048, 8192, 9, (40,), [(E, I, 40)], secs=0.7, moves="16-row tiles"),
    # cold dual starts
    Case("dual-300x600", "cold", 300, 600, 1, (40, None), [(E, I, 40), (0, OPT, 1236)], secs=0.1, moves="k_dsel"),
    Case("dual-300x600-infeasible", "cold", 300, 600, 1, (40, None), [(E, I, 40), (0, NOFEAS, 943)], secs=0.1, infeasible_seed=9, moves="k_dsel; the dual ends NOFEAS"),
    Case("dual-1024x1024", "cold", 1024, 1024, 2, (40, None), [(E, I, 40), (0, OPT, 6625)], secs=2.6, moves="k_dsel at both of its limits"),
    Case("dual-1025x300", "cold", 1025, 300, 3, (40, None), [(E, I, 40), (0, OPT, 2810)], secs=0.8, moves="one row past k_dsel"),
    Case("dual-1100x2000", "cold", 1100, 2000, 4, (40,), [(E, I, 40)], secs=0.1, moves="2.2 M entries: k_da + k_fb<DUAL>"),
]


# general_lp(2049, 256, 5) in calls of 500: rows per lane R = 3, and the instance of the NOFEAS recheck; its
# call patterns are the tests' own (calls of 500 to the end, calls of 20 from pivot 7500)
STEPWISE = Case("stepwise-2049x256", "general", 2049, 256, 5, None, None, p1=6742, secs=4.0, moves="R = 3; the NOFEAS recheck")


def case_id(case):
    return case.name


def by_name(name):
    return next(c for c in CASES if c.name == name)


def run_calls(P, calls):
    """The case's schedule on a handle: [(rc, status, pivots so far)] per call, ending early when a call ends the solve"""
    stops = []
    for lim in calls:
        rc = P.simplex(it_lim=lim)
        stops.append((rc, P.status, P.it_cnt))
        if rc != EITLIM:
            break
    return stops


def certify_sampled_rows(M, P, count=64, seed=0):
    """A pivot-limited stop at a size where certify.py's full longdouble factor takes minutes: `count` tableau rows
    recomputed as in test_gpu_certify's 4096x8192 test -- one solve with B^T each (fp64, refined once), per-row growth
    ||e_i B^-1||_1 ||M||_inf, entries and column 0 within 16 RTOL growth (1 + |ref|): the reference is fp64 itself, so its
    own error is a few u growth -- and every value against the bounds its status names."""
    from . import certify as cf
    from mvolps_amd.capi import NF, NL, NS, NU

    m, n = M.m, M.n
    head, nb, flag = (np.asarray(v[1:], dtype=np.int64) for v in P.basis())
    assert sorted(np.concatenate([head, nb]).tolist()) == list(range(1, m + n + 1))
    Mfull = np.hstack([np.eye(m), -M.A])
    B, N = Mfull[:, head - 1], Mfull[:, nb - 1]
    rows = np.random.default_rng(seed).choice(m, min(count, m), replace=False)
    E = np.zeros((m, len(rows)))
    E[rows, np.arange(len(rows))] = 1.0
    Y = np.linalg.solve(B.T, E)
    Y = Y + np.linalg.solve(B.T, E - B.T @ Y)
    Tr = -(Y.T @ N)
    growth = np.abs(Y).sum(axis=0) * (1.0 + np.abs(M.A).sum(axis=1).max())
    T = P.tableau()
    lim = 16 * cf.RTOL * growth[:, None] * (1.0 + np.abs(Tr))
    err = np.abs(T[1 + rows, 1:] - Tr)
    assert np.all(err <= lim), "sampled tableau rows: worst error / tolerance %.3g" % float((err / lim).max())
    lo, hi = M.lo_hi()
    xN = np.where(flag == NU, hi[nb - 1], np.where(flag == NF, 0.0, lo[nb - 1]))
    assert np.all(np.isfinite(xN)) and np.all((flag != NS) | (lo[nb - 1] == hi[nb - 1])) and set(flag.tolist()) <= {NL, NU, NF, NS}
    x0 = Tr @ xN
    scale = np.abs(Tr) @ np.abs(xN)
    assert np.all(np.abs(T[1 + rows, 0] - x0) <= 16 * cf.RTOL * growth * (1.0 + scale)), "sampled rows: column 0"
    x = np.concatenate([P.row_prim(), P.col_prim()])
    assert np.array_equal(x[nb - 1], xN) and np.array_equal(x[head - 1], T[1:, 0])
    xs = x[m:]
    assert np.all(np.abs(M.A @ xs - x[:m]) <= 16 * cf.RTOL * (growth.max()) * (1.0 + np.abs(M.A) @ np.abs(xs))), "row_prim != A col_prim"
    return float((err / lim).max())


def certify_end(case, inst, P, rc, exact=None):
    """The certificate of the state a schedule ends on, and the feasibility witness: a full solve gets certify.certify for
    its status (exact arithmetic up to EXACT_M rows, unless `exact` says otherwise: with hundreds of columns the fractions
    take seconds), a pivot-limited one its tableau -- whole where certify.py can afford it, else sampled rows.  A NOFEAS on
    an instance built around a point is a failure whatever else agrees."""
    from . import certify as cf

    M = model(inst)
    if case.feasible:
        assert witness_holds(inst), "%s: x0 is not a point of the instance" % case.name
        assert P.status != NOFEAS, "%s: NOFEAS on an LP that has the point x0" % case.name
    if rc == 0:
        assert P.status in (OPT, UNBND, NOFEAS)
        return cf.certify(M, P, exact=(M.m <= cf.EXACT_M) if exact is None else exact, what=case.name)
    if (M.m + 1) * (M.n + 1) > 1500000:
        return certify_sampled_rows(M, P)
    return cf.certify(M, P, what=case.name)
