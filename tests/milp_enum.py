"""Mixed-integer optima by enumeration: a reference that shares nothing with the project (numpy; scipy's linprog for the
ranges and for the continuous remainder of a mixed model).

The model is  opt c x + c0,  rlo <= A x <= rhi,  clo <= x <= chi  (+-inf where a bound is absent), x_j integer where
isint[j].  enumerate_milp

  1. solves the LP relaxation: infeasible is the answer "infeasible"; unbounded means the model cannot be enumerated;
  2. finds the range of every integer column over the relaxation (two LPs per column, presolve off) and rounds it inward;
     an infinite range means the model cannot be enumerated;
  3. visits every integer assignment of that box.  An all-integer model is decided in exact integer arithmetic on the
     doubled data (the data is integer or half-integer; no tolerance anywhere).  A mixed model solves the LP over its
     continuous columns for every assignment that a row-interval test does not exclude.

The result is a dict: status "optimal" / "infeasible" / "dropped" (with "reason"), "relaxation" ("optimal" / "infeasible" /
"unbounded"), "optimum" (c0 included), "x" (one optimal point; the first in lexicographic order of the integer columns
among equally good ones), "points" (the size of the box that was enumerated).
"""
import itertools

import numpy as np

PURE_LIMIT = 600000   # the limit certify.integer_points uses
MIXED_LIMIT = 20000
UNBOUNDED = "relaxation unbounded"
INF_RANGE = "integer column with infinite LP range"
BOX = "box too large"
_EPS = 1e-9           # inward rounding of an LP range: ceil(lo - _EPS), floor(hi + _EPS)


def _lp(c, A, rlo, rhi, clo, chi):
    """min c x over the polyhedron: ("optimal", value, x) / ("infeasible",) / ("unbounded",).  Dual simplex, presolve off."""
    from scipy.optimize import linprog

    m, n = A.shape
    eq = np.isfinite(rlo) & (rlo == rhi)
    up = np.isfinite(rhi) & ~eq
    lo = np.isfinite(rlo) & ~eq
    A_ub = np.vstack([A[up], -A[lo]]) if (up.any() or lo.any()) else None
    b_ub = np.concatenate([rhi[up], -rlo[lo]]) if A_ub is not None else None
    A_eq = A[eq] if eq.any() else None
    b_eq = rlo[eq] if eq.any() else None
    bounds = [(None if not np.isfinite(l) else float(l), None if not np.isfinite(u) else float(u)) for l, u in zip(clo, chi)]
    r = linprog(c, A_ub=A_ub, b_ub=b_ub, A_eq=A_eq, b_eq=b_eq, bounds=bounds, method="highs-ds", options={"presolve": False})
    if r.status == 0:
        return ("optimal", float(r.fun), np.asarray(r.x, dtype=float))
    if r.status == 2:
        return ("infeasible",)
    if r.status == 3:
        return ("unbounded",)
    raise RuntimeError("linprog status %d: %s" % (r.status, r.message))


def lp_ranges(A, rlo, rhi, clo, chi, isint):
    """[(lo_j, hi_j)] of the integer columns over the relaxation (floats, +-inf where unbounded); None: it is empty."""
    n = A.shape[1]
    out = []
    for j in np.nonzero(isint)[0]:
        e = np.zeros(n)
        e[j] = 1.0
        a = _lp(e, A, rlo, rhi, clo, chi)
        if a[0] == "infeasible":
            return None
        b = _lp(-e, A, rlo, rhi, clo, chi)
        out.append((a[1] if a[0] == "optimal" else -np.inf, -b[1] if b[0] == "optimal" else np.inf))
    return out


def _doubled(v):
    """2 v as Python-int-exact int64 (inf kept out by the caller); the data must be integer or half-integer."""
    d = np.asarray(v, dtype=float) * 2.0
    if not np.array_equal(d, np.rint(d)) or np.abs(d).max(initial=0.0) > 2 ** 40:
        raise ValueError("exact enumeration needs integer or half-integer data")
    return d.astype(np.int64)


def _pure(A, rlo, rhi, clo, chi, c, ranges, maximize):
    """Exact: rows 2 A x against 2 rlo / 2 rhi in int64, objective 2 c x in int64.  Returns (best doubled objective, x) or
    None."""
    n = A.shape[1]
    A2, c2 = _doubled(A), _doubled(c)
    fl, fu = np.isfinite(rlo), np.isfinite(rhi)
    l2, u2 = _doubled(np.where(fl, rlo, 0.0)), _doubled(np.where(fu, rhi, 0.0))
    cl, cu = np.isfinite(clo), np.isfinite(chi)
    cl2, cu2 = _doubled(np.where(cl, clo, 0.0)), _doubled(np.where(cu, chi, 0.0))
    axes = [np.arange(a, b + 1, dtype=np.int64) for a, b in ranges]
    best, bestx = None, None
    # the first column in chunks, the rest as one grid: lexicographic order, bounded memory
    rest = np.stack(np.meshgrid(*axes[1:], indexing="ij"), axis=-1).reshape(-1, n - 1) if n > 1 else np.zeros((1, 0), dtype=np.int64)
    for v in axes[0]:
        X = np.concatenate([np.full((len(rest), 1), v, dtype=np.int64), rest], axis=1)
        act = X @ A2.T                                   # = 2 A x, exact
        ok = np.all((~fl | (act >= l2)) & (~fu | (act <= u2)), axis=1)
        ok &= np.all((~cl | (2 * X >= cl2)) & (~cu | (2 * X <= cu2)), axis=1)
        if not ok.any():
            continue
        Xo = X[ok]
        obj = Xo @ c2
        k = int(np.argmax(obj) if maximize else np.argmin(obj))   # the first of equals
        if best is None or (obj[k] > best if maximize else obj[k] < best):
            best, bestx = int(obj[k]), Xo[k].astype(float)
    return None if best is None else (best, bestx)


def _interval(Ac, lo, hi):
    """Per row the least and greatest activity of the continuous columns over their bounds (+-inf allowed)."""
    pos, neg = np.maximum(Ac, 0.0), np.minimum(Ac, 0.0)
    with np.errstate(invalid="ignore"):
        least = np.where(pos != 0, pos * lo, 0.0).sum(axis=1) + np.where(neg != 0, neg * hi, 0.0).sum(axis=1)
        most = np.where(pos != 0, pos * hi, 0.0).sum(axis=1) + np.where(neg != 0, neg * lo, 0.0).sum(axis=1)
    return least, most


def _mixed(A, rlo, rhi, clo, chi, c, isint, ranges, maximize):
    ii, ci = np.nonzero(isint)[0], np.nonzero(~isint)[0]
    AI, AC = A[:, ii], A[:, ci]
    least, most = _interval(AC, clo[ci], chi[ci])
    sgn = -1.0 if maximize else 1.0
    best, bestx = None, None
    for xi in itertools.product(*[range(a, b + 1) for a, b in ranges]):
        xi = np.array(xi, dtype=float)
        if np.any(xi < clo[ii]) or np.any(xi > chi[ii]):
            continue
        act = AI @ xi
        if np.any(act + most < rlo - 1e-7) or np.any(act + least > rhi + 1e-7):   # no continuous completion can exist
            continue
        r = _lp(sgn * c[ci], AC, rlo - act, rhi - act, clo[ci], chi[ci])
        if r[0] == "unbounded":
            raise RuntimeError("bounded relaxation, unbounded remainder")
        if r[0] != "optimal":
            continue
        val = float(c[ii] @ xi) + sgn * r[1]
        if best is None or (val > best + 1e-9 if maximize else val < best - 1e-9):
            x = np.zeros(A.shape[1])
            x[ii], x[ci] = xi, r[2]
            best, bestx = val, x
    return None if best is None else (best, bestx)


def enumerate_milp(A, rlo, rhi, clo, chi, c, c0, isint, maximize, pure_limit=PURE_LIMIT, mixed_limit=MIXED_LIMIT, ranges=None):
    """See the module's text.  ranges: the integer columns' boxes [(lo, hi)] when the caller knows them (then no LP is
    solved for an all-integer model); None: from the relaxation."""
    A = np.asarray(A, dtype=float)
    rlo, rhi, clo, chi, c = (np.asarray(v, dtype=float) for v in (rlo, rhi, clo, chi, c))
    isint = np.asarray(isint, dtype=bool)
    out = {"status": "dropped", "reason": None, "relaxation": None, "optimum": None, "x": None, "points": 0}
    if ranges is None:
        rel = _lp(-c if maximize else c, A, rlo, rhi, clo, chi)
        out["relaxation"] = rel[0]
        if rel[0] == "infeasible":
            out["status"] = "infeasible"
            return out
        if rel[0] == "unbounded":
            out["reason"] = UNBOUNDED
            return out
        ranges = lp_ranges(A, rlo, rhi, clo, chi, isint)
        assert ranges is not None
        if any(not (np.isfinite(a) and np.isfinite(b)) for a, b in ranges):
            out["reason"] = INF_RANGE
            return out
    ii = np.nonzero(isint)[0]
    box = []
    for (a, b), j in zip(ranges, ii):
        a = max(int(np.ceil(a - _EPS)), int(np.ceil(clo[j])) if np.isfinite(clo[j]) else int(np.ceil(a - _EPS)))
        b = min(int(np.floor(b + _EPS)), int(np.floor(chi[j])) if np.isfinite(chi[j]) else int(np.floor(b + _EPS)))
        box.append((a, b))
    points = 1
    for a, b in box:
        points *= max(0, b - a + 1)
    pure = bool(isint.all())
    if points > (pure_limit if pure else mixed_limit):
        out["reason"] = BOX
        out["points"] = points
        return out
    out["points"] = points
    if points == 0:
        got = None
    elif pure:
        got = _pure(A, rlo, rhi, clo, chi, c, box, maximize)
        if got is not None:
            got = (got[0] / 2.0, got[1])
    elif len(ii) == 0:
        rel = _lp(-c if maximize else c, A, rlo, rhi, clo, chi)
        got = ((-rel[1] if maximize else rel[1]), rel[2])
    else:
        got = _mixed(A, rlo, rhi, clo, chi, c, isint, box, maximize)
    if got is None:
        out["status"] = "infeasible"
        return out
    out["status"] = "optimal"
    out["optimum"] = float(got[0]) + float(c0)
    out["x"] = [float(v) for v in got[1]]
    return out


def highs_milp(A, rlo, rhi, clo, chi, c, c0, isint, maximize, presolve):
    """scipy.optimize.milp's answer, a second opinion: ("optimal", value) / ("infeasible", None) / ("other:<status>", None)."""
    from scipy.optimize import Bounds, LinearConstraint, milp

    c = np.asarray(c, dtype=float)
    r = milp(-c if maximize else c, constraints=LinearConstraint(np.asarray(A, dtype=float), rlo, rhi), bounds=Bounds(clo, chi),
             integrality=np.asarray(isint, dtype=int), options={"presolve": bool(presolve)})
    if r.status == 0:
        return "optimal", (-float(r.fun) if maximize else float(r.fun)) + float(c0)
    if r.status == 2:
        return "infeasible", None
    return "other:%d" % r.status, None
