"""CPU: sensitivity ranges of a solved LP (mvx_bnb_ranges, DESIGN.md "Sensitivity ranges (ranges)") over the ORACLE's table.

The host twin of k_rangecols / k_rangefin / k_rangerows is checked bit for bit against a plain restatement of the definition
(scalar loops over the exported tableau, one operation at a time), against the branching penalties it shares part B with, and by
certificates: the oracle re-solves the LP with a non-basic column fixed inside and beyond its activity range, and with a basic
column's cost moved inside and beyond its allowable change.  Then the shapes of the rule (ties, a column of zeros, one row), the
refusals, the report and the command line."""
import math
import os
import subprocess

import numpy as np
import pytest

import mvolps_amd
from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import BS, DB, FX, IV, LO, MAX, MIN, NF, NL, NS, NU, OPT, UP

from . import lpgen
from .test_bnb_branching import basic_fractional
from .test_bnb_general import DRAWN, instance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9  # the default pivot tolerance
INF = math.inf
ACT_DN, ACT_UP, OBJ_DN, OBJ_UP, COST_DN, COST_UP = range(6)
LIM_DN, LIM_UP, ENT_DN, ENT_UP = range(4)
DBL_MAX = np.finfo(float).max


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    assert t.get_tableau and t.get_basis
    return t


def bounds_by_variable(P):
    """[l_k, u_k] for k = 1..m+n, +-inf for an absent bound (the table reports it as -+DBL_MAX)."""
    api, m, n = P.api, P.m, P.n
    lo, hi = [0.0] * (m + n + 1), [0.0] * (m + n + 1)
    for k in range(1, m + n + 1):
        l = api.get_row_lb(P.h, k) if k <= m else api.get_col_lb(P.h, k - m)
        u = api.get_row_ub(P.h, k) if k <= m else api.get_col_ub(P.h, k - m)
        lo[k] = -INF if l <= -DBL_MAX else float(l)
        hi[k] = INF if u >= DBL_MAX else float(u)
    return lo, hi


def moves_of(flag):
    return {NL: (1,), NU: (-1,), NF: (1, -1)}.get(int(flag), ())


def np_ranges(P, tol=TOL):
    """The definition, restated on Python floats from the exported tableau, basis and bounds."""
    T = P.tableau()
    head, nb, flag = P.basis()
    m, n = P.m, P.n
    lo, hi = bounds_by_variable(P)
    is_max = P.api.get_obj_dir(P.h) == MAX
    val = np.zeros((m + n + 1, 6))
    var = np.zeros((m + n + 1, 4), dtype=np.int32)
    for q in range(1, n + 1):  # A: a non-basic position
        k, d = int(nb[q]), abs(float(T[0, q]))
        best = {"up": (INF, 0), "dn": (INF, 0)}
        for i in range(1, m + 1):
            a, beta = float(T[i, q]), float(T[i, 0])
            if not abs(a) > tol:
                continue
            l, u = lo[int(head[i])], hi[int(head[i])]
            cases = []
            if a > 0 and u != INF:
                cases.append(("up", max(u - beta, 0.0) / a))
            if a < 0 and l != -INF:
                cases.append(("up", max(beta - l, 0.0) / (-a)))
            if a > 0 and l != -INF:
                cases.append(("dn", max(beta - l, 0.0) / a))
            if a < 0 and u != INF:
                cases.append(("dn", max(u - beta, 0.0) / (-a)))
            for side, t in cases:
                if t < best[side][0]:
                    best[side] = (t, i)
        for side, ca, co, cl in (("dn", ACT_DN, OBJ_DN, LIM_DN), ("up", ACT_UP, OBJ_UP, LIM_UP)):
            t, i = best[side]
            val[k, ca] = t
            var[k, cl] = int(head[i]) if i else 0
            val[k, co] = (INF if d > 0 else 0.0) if t == INF else d * t
        f = int(flag[q])
        at_lower = d if f == NL else INF if f == NU else d if f == NF else INF  # the NL column of the table
        at_upper = INF if f == NL else d if f == NU else d if f == NF else INF
        val[k, COST_UP], val[k, COST_DN] = (at_lower, at_upper) if is_max else (at_upper, at_lower)
    for i in range(1, m + 1):  # B: a basic variable
        k = int(head[i])
        best = {"up": (INF, 0), "dn": (INF, 0)}
        for q in range(1, n + 1):
            a = float(T[i, q])
            if not abs(a) > tol:
                continue
            r = abs(float(T[0, q])) / abs(a)
            dirs = moves_of(flag[q])
            for side, ok in (("dn", any(s * a < 0 for s in dirs)), ("up", any(s * a > 0 for s in dirs))):
                if ok and r < best[side][0]:
                    best[side] = (r, q)
        up, dn = (best["up"], best["dn"]) if is_max else (best["dn"], best["up"])
        val[k, COST_UP], var[k, ENT_UP] = up[0], int(nb[up[1]]) if up[1] else 0
        val[k, COST_DN], var[k, ENT_DN] = dn[0], int(nb[dn[1]]) if dn[1] else 0
    return val, var


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)


def check_twin(P, tab):
    rc, val, var = bnb.ranges(P, table=tab)
    assert rc == 0
    rval, rvar = np_ranges(P)
    assert same_bits(val, rval), np.argwhere(val != rval)[:4]
    assert same_bits(var, rvar), np.argwhere(var != rvar)[:4]
    assert not val[0].any() and not var[0].any()
    return val, var


def dense_roots(orc):
    """Solved roots of the synthetic families: (name, handle)."""
    out = []
    for m, n, seed in ((5, 7, 3), (24, 48, 5), (40, 30, 9)):
        P = orc.create()
        P.load_dense(*synth.dense_lp(m, n, seed))
        out.append(("dense_lp %dx%d" % (m, n), P))
    for m, n, seed, U, cap in ((10, 20, 3, 3, 0.4), (24, 48, 5, 3, 0.3), (32, 64, 7, 1, 0.2)):
        out.append(("dense_ilp %dx%d U=%g" % (m, n, U), lpgen.load_ilp(orc, *synth.dense_ilp(m, n, seed, U, cap))))
    for _name, P in out:
        P.simplex()
        assert P.status == OPT
    return out


def general_roots(orc):
    """Every drawn general fixture whose root LP solves."""
    for rec in DRAWN:
        P = lpgen.load_milp(orc, instance(rec))
        P.simplex()
        if P.status == OPT:
            yield rec, P


# ------------------------------------------------------------------------------------------------ 1. twin = restatement


def test_twin_matches_the_restatement_on_dense_roots(orc, tab):
    for _name, P in dense_roots(orc):
        check_twin(P, tab)


def test_twin_matches_the_restatement_on_every_general_fixture(orc, tab):
    flags, dirs, rtypes, done = set(), set(), set(), 0
    for rec, P in general_roots(orc):
        check_twin(P, tab)
        flags |= set(P.basis()[2][1:].tolist())
        dirs.add(P.api.get_obj_dir(P.h))
        rtypes |= {P.api.get_row_type(P.h, i) for i in range(1, P.m + 1)}
        done += 1
    assert done >= 150
    # (a free column is never non-basic at these optima: test_a_column_of_zeros has the NF position)
    assert {NL, NU, NS} <= flags and dirs == {MIN, MAX} and rtypes == {capi.FR, LO, UP, DB, FX}


# ------------------------------------------------------------------------------------------------ 2. part B = penalties


def test_cost_ranges_are_the_branching_penalties(orc, tab):
    seen = 0
    roots = [P for _n, P in dense_roots(orc)] + [P for _r, P in general_roots(orc)]
    for P in roots:
        cols = [j for j in basic_fractional(P, tab) if P.api.get_col_kind(P.h, j) != capi.CV]
        if not cols:
            continue
        rc, (pd, pu, ad, au) = bnb.penalties(P, cols, TOL, table=tab)
        assert rc == 0
        rc, val, var = bnb.ranges(P, table=tab)
        assert rc == 0
        T = P.tableau()
        head, nb, _flag = P.basis()
        is_max = P.api.get_obj_dir(P.h) == MAX
        for t, j in enumerate(cols):
            k = P.m + j
            i = int(np.nonzero(head == k)[0][0])
            v = T[i, 0]
            fd, fu = v - np.floor(v), np.ceil(v) - v
            min_dn, min_up = (val[k, COST_DN], val[k, COST_UP]) if is_max else (val[k, COST_UP], val[k, COST_DN])
            ent_dn, ent_up = (var[k, ENT_DN], var[k, ENT_UP]) if is_max else (var[k, ENT_UP], var[k, ENT_DN])
            assert (fd * min_dn == pd[t]) if ad[t] else (min_dn == INF and pd[t] == INF)
            assert (fu * min_up == pu[t]) if au[t] else (min_up == INF and pu[t] == INF)
            assert ent_dn == (nb[ad[t]] if ad[t] else 0) and ent_up == (nb[au[t]] if au[t] else 0)
            seen += 1
    assert seen >= 100


# ------------------------------------------------------------------------------------------------ 3. / 4. certificates


def limiting_entry(P, k_limit, k_other):
    """|T[i][q]| with one of the two variables basic in row i and the other non-basic in position q."""
    T = P.tableau()
    head, nb, _flag = P.basis()
    for kb, kn in ((k_limit, k_other), (k_other, k_limit)):
        rows, pos = np.nonzero(head == kb)[0], np.nonzero(nb == kn)[0]
        if len(rows) and len(pos):
            return abs(float(T[int(rows[0]), int(pos[0])]))
    raise AssertionError("no such entry")


def resolved(P, edit):
    Q = P.copy()
    edit(Q)
    Q.simplex()
    return Q


def activity_certificates(P, val, var):
    """(checked, beyond checked, beyond left out) over the non-basic structurals of one solved root."""
    head, nb, flag = P.basis()
    m, api = P.m, P.api
    x = P.col_prim()
    obj0, it0 = P.obj, P.it_cnt
    T0 = P.tableau()[0]
    checked = beyond = left = 0
    for q in range(1, P.n + 1):
        k = int(nb[q])
        if k <= m:
            continue
        j, d = k - m, abs(float(T0[q]))
        for s, ca, cl in ((1, ACT_UP, LIM_UP), (-1, ACT_DN, LIM_DN)):
            t = float(val[k, ca])
            if s not in moves_of(flag[q]) or t == INF:
                continue
            v = float(x[j - 1])
            at = v + s * (t / 2)
            Q = resolved(P, lambda Q: api.set_col_bnds(Q.h, j, FX, at, at))
            assert Q.status == OPT and Q.it_cnt == it0, (j, s, t, Q.status, Q.it_cnt - it0)
            move = d * (t / 2)
            assert abs(abs(Q.obj - obj0) - move) <= 1e-9 * max(1.0, abs(obj0), abs(Q.obj)), (j, s, Q.obj, obj0, move)
            checked += 1
            excess = t * 1e-3 + 1e-6
            if t == 0.0 or limiting_entry(P, int(var[k, cl]), k) * excess <= 1e-7:
                left += 1
                continue
            at = v + s * (t + excess)
            Q = resolved(P, lambda Q: api.set_col_bnds(Q.h, j, FX, at, at))
            assert Q.it_cnt > it0 or Q.status != OPT, (j, s, t)
            beyond += 1
    return checked, beyond, left


def cost_certificates(P, val, var):
    """(checked, beyond checked, beyond left out) over the basic structurals of one solved root."""
    head, _nb, _flag = P.basis()
    m, api = P.m, P.api
    it0 = P.it_cnt
    checked = beyond = left = 0
    for i in range(1, m + 1):
        k = int(head[i])
        if k <= m:
            continue
        j = k - m
        c = api.get_obj_coef(P.h, j)
        for s, cc, ce in ((1, COST_UP, ENT_UP), (-1, COST_DN, ENT_DN)):
            delta = float(val[k, cc])
            if delta == INF:
                continue
            Q = resolved(P, lambda Q: api.set_obj_coef(Q.h, j, c + s * (delta / 2)))
            assert Q.status == OPT and Q.it_cnt == it0, (j, s, delta, Q.status, Q.it_cnt - it0)
            checked += 1
            excess = delta * 1e-3 + 1e-6
            if delta == 0.0 or limiting_entry(P, k, int(var[k, ce])) * excess <= 1e-7:
                left += 1
                continue
            Q = resolved(P, lambda Q: api.set_obj_coef(Q.h, j, c + s * (delta + excess)))
            assert Q.it_cnt > it0, (j, s, delta)
            beyond += 1
    return checked, beyond, left


# the models of the two certificate tests: dense_lp roots (columns without an upper bound) and dense_ilp roots with U = 3
# (bounded columns, NL and NU non-basics)
CERT_LP = ((24, 48, 5), (40, 30, 9), (12, 24, 2))
CERT_ILP = ((10, 20, 3, 3, 0.4), (24, 48, 5, 3, 0.3))


def cert_roots(orc):
    out = []
    for m, n, seed in CERT_LP:
        P = orc.create()
        P.load_dense(*synth.dense_lp(m, n, seed))
        out.append(("dense_lp %dx%d seed %d" % (m, n, seed), P))
    for m, n, seed, U, cap in CERT_ILP:
        out.append(("dense_ilp %dx%d seed %d" % (m, n, seed), lpgen.load_ilp(orc, *synth.dense_ilp(m, n, seed, U, cap))))
    for _name, P in out:
        P.simplex()
        assert P.status == OPT
    return out


def test_activity_ranges_certified_by_resolving(orc, tab):
    """Every non-basic structural of the five roots, in every direction it may move with a finite limit: fixed half way the basis
    stays (no pivot, OPT, the objective moved by |d| t / 2); fixed beyond the limit a pivot follows.  With the twin over the
    oracle (inside / beyond / beyond left out): dense_lp 24x48 41 / 41 / 0, 40x30 22 / 22 / 0, 12x24 19 / 19 / 0; dense_ilp
    10x20 14 / 14 / 0, 24x48 38 / 38 / 0."""
    for name, P in cert_roots(orc):
        rc, val, var = bnb.ranges(P, table=tab)
        assert rc == 0
        checked, beyond, left = activity_certificates(P, val, var)
        print("%s: %d inside, %d beyond, %d left out" % (name, checked, beyond, left))
        assert checked >= 5 and left <= 0.1 * checked, (name, checked, beyond, left)


def test_cost_ranges_certified_by_resolving(orc, tab):
    """Every basic structural of the five roots, both finite cost limits: moved by half the limit no pivot follows, moved beyond
    it one does.  With the twin over the oracle (inside / beyond / beyond left out): dense_lp 24x48 14 / 14 / 0, 40x30
    16 / 16 / 0, 12x24 10 / 10 / 0; dense_ilp 10x20 12 / 12 / 0, 24x48 20 / 20 / 0."""
    for name, P in cert_roots(orc):
        rc, val, var = bnb.ranges(P, table=tab)
        assert rc == 0
        checked, beyond, left = cost_certificates(P, val, var)
        print("%s: %d inside, %d beyond, %d left out" % (name, checked, beyond, left))
        assert checked >= 5 and left <= 0.1 * checked, (name, checked, beyond, left)


# ------------------------------------------------------------------------------------------------ 5. shapes of the rule


def tie_model(api, m=6, n=8, seed=4, adjacent=False):
    """dense_lp with every row written twice: the copy of row i is row i + m (adjacent: row i + 1).  Wherever both auxiliaries
    are basic, the two rows tie in every column."""
    A, b, c = synth.dense_lp(m, n, seed)
    P = api.create()
    if adjacent:
        P.load_dense(np.repeat(A, 2, axis=0), np.repeat(b, 2), c)
    else:
        P.load_dense(np.concatenate([A, A]), np.concatenate([b, b]), c)
    return P


def ties_go_to_the_lower_row(P, val, var):
    """Every limiting row of part A is the lowest row that attains the minimum; returns how many minima were attained twice."""
    T = P.tableau()
    head, nb, _flag = P.basis()
    lo, hi = bounds_by_variable(P)
    tied = 0
    for q in range(1, P.n + 1):
        k = int(nb[q])
        for s, ca, cl in ((1, ACT_UP, LIM_UP), (-1, ACT_DN, LIM_DN)):
            if var[k, cl] == 0:
                continue
            hits = []
            for i in range(1, P.m + 1):
                a, beta = float(T[i, q]) * s, float(T[i, 0])
                if not abs(a) > TOL:
                    continue
                room = hi[int(head[i])] - beta if a > 0 else beta - lo[int(head[i])]
                if room != INF and max(room, 0.0) / abs(a) == val[k, ca]:
                    hits.append(i)
            assert hits and int(head[hits[0]]) == var[k, cl], (q, s, hits)
            tied += len(hits) > 1
    return tied


def test_ties_go_to_the_lower_tableau_row(orc, tab):
    P = tie_model(orc)
    P.simplex()
    assert P.status == OPT
    val, var = check_twin(P, tab)
    assert ties_go_to_the_lower_row(P, val, var) >= 4


def zero_column_model(api, direction=MAX):
    """Column 3 is free, has no entry in any row and no cost: a free non-basic position, nothing limits it and the objective does
    not move.  Column 5 has
    no entry either but a cost that keeps it at the bound it likes: nothing limits it, and the objective moves without limit."""
    A, b, c = synth.dense_lp(4, 6, 8)
    A[:, 2] = 0.0
    A[:, 4] = 0.0
    c[2] = 0.0
    c[4] = 2.0
    P = api.create()
    cols = [(LO, 0.0, 0.0)] * 6
    cols[2] = (capi.FR, 0.0, 0.0)
    cols[4] = (DB, 0.0, 1.0)
    sg = 1.0 if direction == MAX else -1.0
    P.load_general(A, [(UP, 0.0, float(v)) for v in b], cols, sg * c, direction=direction)
    return P


@pytest.mark.parametrize("direction", [MAX, MIN], ids=["max", "min"])
def test_a_column_of_zeros(orc, tab, direction):
    P = zero_column_model(orc, direction)
    P.simplex()
    assert P.status == OPT
    val, var = check_twin(P, tab)
    k3, k5 = P.m + 3, P.m + 5
    assert P.api.get_col_stat(P.h, 3) != BS and P.api.get_col_stat(P.h, 5) != BS
    assert P.api.get_col_stat(P.h, 3) == NF
    assert list(val[k3]) == [INF, INF, 0.0, 0.0, 0.0, 0.0] and list(var[k3]) == [0, 0, 0, 0]
    assert list(val[k5, :4]) == [INF, INF, INF, INF] and list(var[k5]) == [0, 0, 0, 0]
    assert sorted(val[k5, 4:]) == [2.0, INF]


def test_one_row(orc, tab):
    A, b, c = synth.dense_lp(1, 9, 6)
    P = orc.create()
    P.load_dense(A, b, c)
    P.simplex()
    assert P.status == OPT and P.m == 1
    val, var = check_twin(P, tab)
    head, nb, _f = P.basis()
    assert val.shape == (11, 6) and np.count_nonzero(var[:, [LIM_DN, LIM_UP]]) >= 1
    assert set(var[:, [LIM_DN, LIM_UP]].ravel().tolist()) <= {0, int(head[1])}


# ------------------------------------------------------------------------------------------------ 6. refusals


def test_refusals(orc, tab):
    A, b, c, U = synth.dense_ilp(8, 16, 3, 1, 0.3)
    P = lpgen.load_ilp(orc, A, b, c, U)
    assert bnb.ranges(P, table=tab)[0] == -3  # never solved
    P.simplex()
    assert P.status == OPT and bnb.ranges(P, table=tab)[0] == 0
    Q = P.copy()
    Q.api.set_col_bnds(Q.h, 1, DB, 0.0, 0.5)  # a bound edited after the solve
    assert bnb.ranges(Q, table=tab)[0] == -3
    bare = bnb.table_from(orc)
    bare.get_tableau = None
    assert bnb.ranges(P, table=bare)[0] == -2
    L = bnb.lib()
    DP, IP = bnb.C.POINTER(bnb.C.c_double), bnb.C.POINTER(bnb.C.c_int)
    val, var = np.zeros((P.m + P.n + 1, 6)), np.zeros((P.m + P.n + 1, 4), dtype=np.int32)
    tptr = bnb.C.cast(bnb.C.pointer(tab), bnb.C.c_void_p)
    assert L.mvx_bnb_ranges(tptr, None, val.ctypes.data_as(DP), var.ctypes.data_as(IP)) == -1
    assert L.mvx_bnb_ranges(tptr, P.h, None, var.ctypes.data_as(IP)) == -1
    assert L.mvx_bnb_ranges(tptr, P.h, val.ctypes.data_as(DP), None) == -1
    assert L.mvx_ranges(None, val.ctypes.data_as(DP), var.ctypes.data_as(IP)) == -1
    assert L.mvx_bnb_print_ranges(tptr, P.h, None, var.ctypes.data_as(IP), None) == -1
    assert bnb.print_ranges(Q, val, var, table=tab) == -3
    assert bnb.print_ranges(P, val, var, path=os.path.join(ROOT, "no", "such", "dir", "r.txt"), table=tab) == -4
    assert bnb.ranges_chunk() >= 64 and bnb.ranges_chunk() % 4 == 0


# ------------------------------------------------------------------------------------------------ 7. report and CLI


def parse_report(path):
    """The report back as (val, var, names, status words, values); its 14 fields are described in DESIGN.md."""
    lines = open(path).read().splitlines()
    rows = len(lines) + 1
    val, var = np.zeros((rows, 6)), np.zeros((rows, 4), dtype=np.int32)
    names, stats, xs = [None], [None], [None]
    for ln, line in enumerate(lines, 1):
        f = line.split()
        assert len(f) == 14 and int(f[0]) == ln, line
        names.append(f[1])
        stats.append(f[2])
        xs.append(float(f[3]))
        val[ln] = [float(f[4]), float(f[6]), float(f[8]), float(f[9]), float(f[10]), float(f[12])]
        var[ln] = [int(f[5]), int(f[7]), int(f[11]), int(f[13])]
    return val, var, names, stats, xs


def test_report_parses_back_to_the_numbers(orc, tab, tmp_path):
    for rec, P in general_roots(orc):
        if P.m + P.n >= 12:
            break
    rc, val, var = bnb.ranges(P, table=tab)
    assert rc == 0
    path = str(tmp_path / "ranges.txt")
    assert bnb.print_ranges(P, val, var, path=path, table=tab) == 0
    pval, pvar, names, stats, xs = parse_report(path)
    assert same_bits(pval, val) and same_bits(pvar, var)  # %.17g reads back to the same double
    m, n = P.m, P.n
    assert names[1:] == ["R%d" % i for i in range(1, m + 1)] + ["C%d" % j for j in range(1, n + 1)]
    word = {BS: "B", NL: "NL", NU: "NU", NF: "NF", NS: "NS"}
    assert stats[1:] == [word[s] for s in P.row_stat()] + [word[s] for s in P.col_stat()]
    assert xs[1:] == list(P.row_prim()) + list(P.col_prim())


def test_cli_flag_parses():
    exe = os.path.join(ROOT, "mvolps_amd", "bin", "mvolps")
    f1 = os.path.join(ROOT, "tests", "golden", "f1.lp")
    assert "--ranges" in subprocess.run([exe, "-h"], capture_output=True, text=True).stdout
    for flags in (("--ranges",), ("--ranges", "--repaired"), ("--repaired", "--ranges")):
        r = subprocess.run([exe, "-f", f1, *flags], capture_output=True, text=True)
        assert r.returncode != 0 and "Unknown parameter value for --ranges" in r.stderr, (flags, r.stderr)


def test_python_front_end():
    assert bnb.RANGE_VAL == ("ACT_DN", "ACT_UP", "OBJ_DN", "OBJ_UP", "COST_DN", "COST_UP")
    assert bnb.RANGE_VAR == ("LIM_DN", "LIM_UP", "ENT_DN", "ENT_UP")
    assert callable(capi.Prob.ranges) and callable(mvolps_amd.api().ranges) and mvolps_amd.api().ranges_chunk() == bnb.ranges_chunk()
