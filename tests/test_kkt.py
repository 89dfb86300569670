"""CPU: the KKT check of a solved LP (mvx_bnb_kkt, mvx_bnb_kkt_values, kkt = 1; DESIGN.md "KKT check (kkt)") over the ORACLE's table.

The host twin of k_kkt_rows / k_kkt_cols / k_kkt_fin is checked bit for bit against a plain restatement of the definition that
works from the values the getters return (so the four vectors the twin derives from the tableau are the getters' bits), against an
independent long-double product inside the standard forward-error bound, on corrupted numbers, on the shapes of the rule (ties,
all zero), the refusals, small trees with the flag on, the binding's names and the command line."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mvolps_amd
from mvolps_amd import bnb, capi, synth, treedigest
from mvolps_amd.capi import BS, DB, FEAS, INFEAS, LO, MAX, MIN, NL, NOFEAS, NU, OPT, UNBND, UNDEF, UP

from . import lpgen
from .test_bnb_general import DRAWN, instance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf
DBL_MAX = np.finfo(float).max
PE, PB, DE, DB_ = 0, 1, 2, 3  # conditions: val[2 c] = ae_max, val[2 c + 1] = re_max


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    assert t.get_tableau and t.get_basis and bnb.table_entry(t, "kkt_many") is None
    return t


def fma(a, b, c):
    """a * b + c rounded once.  Exact rational arithmetic and one correctly rounded conversion; the sums here start from +0.0
    and never reach -0.0, so an exact zero is +0.0 as the hardware's is."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def chain_sum(a, v):
    """sum_k a[k] v[k], k = 1..len - 1: 64 chains, chain l taking k = l+1, l+65, ... ascending with fma from +0.0, combined by
    s[l] += s[l+h], h = 32 .. 1.  Zeros are not skipped."""
    s = [0.0] * 64
    for l in range(64):
        acc = 0.0
        for k in range(l + 1, len(v), 64):
            acc = fma(float(a[k]), float(v[k]), acc)
        s[l] = acc
    h = 32
    while h >= 1:
        for l in range(h):
            s[l] = s[l] + s[l + h]
        h //= 2
    return s[0]


class Maxi:
    def __init__(self):
        self.v, self.i = 0.0, 0

    def see(self, w, k):
        if w > self.v:
            self.v, self.i = w, k


def np_kkt(rows, c, xs, xr, lam, dj, lb, ub, stat, is_min):
    """The definition on Python floats.  Every vector is 1-based (entry 0 unused); rows is (m, n + 1)."""
    m, n = rows.shape[0], rows.shape[1] - 1
    sg = 1.0 if is_min else -1.0
    mx = [Maxi() for _ in range(8)]
    r_pe, r_de = np.zeros(m + 1), np.zeros(n + 1)
    for i in range(1, m + 1):
        r = float(xr[i]) - chain_sum(rows[i - 1], xs)
        r_pe[i] = r
        mx[0].see(abs(r), i)
        mx[1].see(abs(r) / (1.0 + abs(float(xr[i]))), i)
    for j in range(1, n + 1):
        col = np.concatenate([[0.0], rows[:, j]])
        r = (float(c[j]) - chain_sum(col, lam)) - float(dj[j])
        r_de[j] = r
        mx[4].see(abs(r), j)
        mx[5].see(abs(r) / (1.0 + abs(float(c[j]))), j)
    for k in range(1, m + n + 1):
        x = float(xr[k]) if k <= m else float(xs[k - m])
        d = float(lam[k]) if k <= m else float(dj[k - m])
        l, u = float(lb[k]), float(ub[k])
        ae = re = 0.0
        if abs(l) != INF and x < l:
            ae, re = l - x, (l - x) / (1.0 + abs(l))
        elif abs(u) != INF and x > u:
            ae, re = x - u, (x - u) / (1.0 + abs(u))
        mx[2].see(ae, k)
        mx[3].see(re, k)
        e, s = sg * d, int(stat[k])
        v = max(-e, 0.0) if s == NL else max(e, 0.0) if s == NU else abs(e) if s == capi.NF else 0.0 if s == capi.NS else abs(d)
        mx[6].see(v, k)
        mx[7].see(v / (1.0 + abs(d)), k)
    return np.array([q.v for q in mx]), np.array([q.i for q in mx], dtype=np.int32), r_pe, r_de


def lead(v, dtype=np.float64):
    return np.concatenate([np.zeros(1, dtype=dtype), np.asarray(v, dtype=dtype)])


def by_getters(P):
    """What a caller reads of a solved handle: the dense rows, the objective, the four value vectors through the getters, the
    bounds and statuses by variable -- 1-based."""
    api, m, n = P.api, P.m, P.n
    rows = np.zeros((m, n + 1))
    for i in range(1, m + 1):
        ind, val = P.get_mat_row(i)
        rows[i - 1, ind] = val
    c = np.array([0.0] + [api.get_obj_coef(P.h, j) for j in range(1, n + 1)])
    lo, hi = np.zeros(m + n + 1), np.zeros(m + n + 1)
    for k in range(1, m + n + 1):
        l = api.get_row_lb(P.h, k) if k <= m else api.get_col_lb(P.h, k - m)
        u = api.get_row_ub(P.h, k) if k <= m else api.get_col_ub(P.h, k - m)
        lo[k] = -INF if l <= -DBL_MAX else l
        hi[k] = INF if u >= DBL_MAX else u
    stat = lead(np.concatenate([P.row_stat(), P.col_stat()]), np.int32)
    return dict(rows=rows, c=c, xs=lead(P.col_prim()), xr=lead(P.row_prim()), lam=lead(P.row_dual()), dj=lead(P.col_dual()), lb=lo, ub=hi,
                stat=stat, is_min=api.get_obj_dir(P.h) == MIN)


def values_call(g):
    """bnb.kkt_values on the numbers of by_getters (0-based arguments)."""
    return bnb.kkt_values(g["rows"][:, 1:], g["c"][1:], g["xs"][1:], g["xr"][1:], g["lam"][1:], g["dj"][1:], g["lb"][1:], g["ub"][1:],
                          g["stat"][1:], MIN if g["is_min"] else MAX)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_twin(P, tab, what):
    """mvx_bnb_kkt through the table == the restatement on the getters' values == mvx_bnb_kkt_values on them, every bit."""
    g = by_getters(P)
    want = np_kkt(**g)
    rc, val, ind, r_pe, r_de = bnb.kkt(P, table=tab)
    assert rc == 0, (what, rc)
    got2 = values_call(g)
    assert got2[0] == 0
    for got in ((val, ind, r_pe, r_de), got2[1:]):
        assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), (what, got[0], want[0], got[1], want[1])
        assert same_bits(got[2], want[2]) and same_bits(got[3], want[3]), what
    assert r_pe[0] == 0.0 and r_de[0] == 0.0
    # the handle has not moved
    assert bnb.kkt(P, table=tab, residuals=False)[1].tolist() == val.tolist()
    return g, want


def longdouble_bound(g, r_pe, r_de):
    """|r_i - r_i^ld| <= (n + 2) 2^-53 (sum_j |a_ij xS_j| + |xR_i|), and the mirror with m, lambda and c_j on the dual side: the
    standard forward-error bound of n products summed in any order and the differences behind them, so nothing is measured."""
    L = np.longdouble
    rows, m, n = g["rows"].astype(L), g["rows"].shape[0], g["rows"].shape[1] - 1
    u = L(2.0) ** -53
    xs, xr, lam, dj, c = (g[k].astype(L) for k in ("xs", "xr", "lam", "dj", "c"))
    for i in range(1, m + 1):
        prod = rows[i - 1, 1:] * xs[1:]
        ld = xr[i] - prod.sum()
        assert abs(L(r_pe[i]) - ld) <= (n + 2) * u * (np.abs(prod).sum() + abs(xr[i])), ("PE", i)
    for j in range(1, n + 1):
        prod = rows[:, j] * lam[1:]
        ld = (c[j] - prod.sum()) - dj[j]
        assert abs(L(r_de[j]) - ld) <= (m + 2) * u * (np.abs(prod).sum() + abs(c[j])), ("DE", j)


def dense_root(api, case=(16, 32, 9, 3, 0.2)):
    A, b, c, U = synth.dense_ilp(*case)
    return synth.load_ilp(api, A, b, c, U)


def min_model(api):
    rng = np.random.default_rng(11)
    A = rng.integers(0, 4, size=(7, 9)).astype(float)
    P = api.create()
    P.load_general(A, [(LO, float(v), 0.0) for v in rng.integers(3, 9, size=7)], [(DB, 0.0, 5.0)] * 9, rng.integers(1, 9, size=9).astype(float),
                   direction=MIN)
    return P


def test_twin_restatement_and_getters_agree_bit_for_bit(orc, tab):
    seen = set()
    for rec in DRAWN:
        inst = instance(rec)
        for lim in (None, 0, 1, 2, 3):
            P = lpgen.load_milp(orc, inst)
            P.simplex(it_lim=lim)
            seen.add(P.status)
            g, want = check_twin(P, tab, (rec["index"], lim))
            longdouble_bound(g, want[2], want[3])
    assert {OPT, FEAS, INFEAS, NOFEAS} <= seen, seen
    # an unbounded relaxation
    P = orc.create()
    P.load_general(np.array([[1.0, -1.0]]), [(UP, 0.0, 1.0)], [(LO, 0.0, 0.0)] * 2, [1.0, 1.0])
    P.simplex()
    assert P.status == UNBND
    check_twin(P, tab, "unbounded")
    for P, what in ((dense_root(orc), "dense_ilp"), (lpgen.load_degenerate(orc, *lpgen.degenerate_lp(12, 20, 4)), "degenerate"),
                    (min_model(orc), "min")):
        assert P.simplex() == 0 and P.status == OPT, what
        g, want = check_twin(P, tab, what)
        longdouble_bound(g, want[2], want[3])
        # a solved LP satisfies its model: equations to rounding, bounds and dual signs to the solve's tolerances
        assert want[0][2 * PE + 1] < 1e-12 and want[0][2 * DE + 1] < 1e-12 and want[0][2 * PB] < 1e-8 and want[0][2 * DB_] < 1e-8, (what, want[0])
    assert orc.get_obj_dir(P.h) == MIN


def test_sign_identity_on_a_max_and_a_min_model(orc, tab):
    """c - A'lambda - d = 0 in this sign, NL duals <= 0 and NU duals >= 0 under MAX (the mirror under MIN), basic duals 0."""
    for P, is_min in ((dense_root(orc), False), (min_model(orc), True)):
        P.simplex()
        g = by_getters(P)
        sg = 1.0 if is_min else -1.0
        t = g["rows"][:, 1:].T @ g["lam"][1:]
        assert np.abs(g["c"][1:] - t - g["dj"][1:]).max() < 1e-12 and np.abs(g["c"][1:] + t - g["dj"][1:]).max() > 1e-3
        dual = np.concatenate([g["lam"][1:], g["dj"][1:]])
        st = g["stat"][1:]
        assert np.all(dual[st == BS] == 0.0) and np.all(sg * dual[st == NL] >= -1e-9) and np.all(sg * dual[st == NU] <= 1e-9)


def test_corrupted_numbers_are_reported_where_they_are(orc):
    P = dense_root(orc)
    P.simplex()
    g = by_getters(P)
    m, n = P.m, P.n
    rc, val0, ind0, pe0, de0 = values_call(g)
    assert rc == 0 and val0[2 * PB] == 0.0 and val0[2 * DB_] == 0.0

    def others_unchanged(val, ind, cond):
        for c in range(4):
            if c != cond:
                assert same_bits(val[2 * c:2 * c + 2], val0[2 * c:2 * c + 2]) and np.array_equal(ind[2 * c:2 * c + 2], ind0[2 * c:2 * c + 2]), (cond, c)

    # one xR_i: the rows are <= rows, so a lower activity breaks no bound
    i = 5
    h = dict(g, xr=g["xr"].copy())
    h["xr"][i] = g["xr"][i] - 1.0
    rc, val, ind, r_pe, _ = values_call(h)
    want = abs(h["xr"][i] - chain_sum(g["rows"][i - 1], g["xs"]))
    assert rc == 0 and ind[2 * PE] == i and ind[2 * PE + 1] == i and val[2 * PE] == want and val[2 * PE + 1] == want / (1.0 + abs(h["xr"][i]))
    assert r_pe[i] == h["xr"][i] - chain_sum(g["rows"][i - 1], g["xs"])
    others_unchanged(val, ind, PE)
    # one d_j: a column at its lower bound with a strictly negative dual (MAX), pushed further down -- the sign stays right
    st = g["stat"]
    j = next(j for j in range(1, n + 1) if st[m + j] == NL and g["dj"][j] < -1e-6)
    h = dict(g, dj=g["dj"].copy())
    h["dj"][j] = g["dj"][j] - 0.5
    rc, val, ind, _, r_de = values_call(h)
    col = np.concatenate([[0.0], g["rows"][:, j]])
    want = abs((g["c"][j] - chain_sum(col, g["lam"])) - h["dj"][j])
    assert rc == 0 and ind[2 * DE] == j and ind[2 * DE + 1] == j and val[2 * DE] == want and val[2 * DE + 1] == want / (1.0 + abs(g["c"][j]))
    assert abs(want - 0.5) < 1e-9
    others_unchanged(val, ind, DE)
    # one bound: the lower bound of a basic column moves above its value
    k = next(k for k in range(m + 1, m + n + 1) if st[k] == BS)
    h = dict(g, lb=g["lb"].copy())
    h["lb"][k] = g["xs"][k - m] + 0.25
    rc, val, ind, _, _ = values_call(h)
    want = h["lb"][k] - g["xs"][k - m]
    assert rc == 0 and ind[2 * PB] == k and ind[2 * PB + 1] == k and val[2 * PB] == want and val[2 * PB + 1] == want / (1.0 + abs(h["lb"][k]))
    others_unchanged(val, ind, PB)
    # one status: that column called NU -- its dual has the wrong sign for an upper bound
    h = dict(g, stat=g["stat"].copy())
    h["stat"][m + j] = NU
    rc, val, ind, _, _ = values_call(h)
    want = abs(g["dj"][j])
    assert rc == 0 and ind[2 * DB_] == m + j and ind[2 * DB_ + 1] == m + j and val[2 * DB_] == want and val[2 * DB_ + 1] == want / (1.0 + want)
    others_unchanged(val, ind, DB_)


def test_an_iteration_limit_inside_phase_one_shows_in_pb(orc, tab):
    A, c = lpgen.setcover_ilp(6, 10, 1)
    P = lpgen.load_setcover(orc, A, c)
    P.simplex(it_lim=1)
    assert P.status == INFEAS
    g, want = check_twin(P, tab, "phase 1")
    x = np.concatenate([g["xr"][1:], g["xs"][1:]])
    viol = np.maximum(np.maximum(g["lb"][1:] - x, x - g["ub"][1:]), 0.0)
    assert viol.max() > 0.5 and want[0][2 * PB] == viol.max() and want[1][2 * PB] == int(np.argmax(viol)) + 1


def test_ties_go_to_the_lowest_index_and_zero_gives_index_zero():
    rows = np.eye(3)
    zero3 = np.zeros(3)
    fr = dict(lb=np.full(6, -INF), ub=np.full(6, INF), stat=np.array([BS] * 3 + [capi.NF] * 3, dtype=np.int32))
    rc, val, ind, r_pe, r_de = bnb.kkt_values(rows, zero3, zero3, zero3, zero3, zero3, **fr)
    assert rc == 0 and not val.any() and not ind.any() and not r_pe.any() and not r_de.any()
    # rows 2 and 3 are off by the same amount; columns 1 and 3; variables 2 and 5 below their bounds; duals 4 and 6 non-zero on NF
    xr = np.array([0.0, 0.5, -0.5])
    dj = np.array([0.25, 0.0, -0.25])
    lb = np.array([-INF, 1.5, -INF, -INF, 1.0, -INF])
    rc, val, ind, r_pe, r_de = bnb.kkt_values(rows, zero3, zero3, xr, zero3, dj, lb, fr["ub"], fr["stat"], MIN)
    assert rc == 0 and ind.tolist() == [2, 2, 2, 5, 1, 1, 4, 4], ind
    assert val.tolist() == [0.5, 0.5 / 1.5, 1.0, 1.0 / 2.0, 0.25, 0.25, 0.25, 0.25 / 1.25], val
    assert r_pe.tolist() == [0.0, 0.0, 0.5, -0.5] and r_de.tolist() == [0.0, -0.25, 0.0, 0.25]


def test_refusals(orc, tab):
    P = dense_root(orc)
    assert bnb.kkt(P, table=tab)[0] == -3  # never solved
    P.simplex()
    assert bnb.kkt(P, table=tab)[0] == 0
    for edit in (lambda: orc.set_col_bnds(P.h, 1, DB, 0.0, 1.0), lambda: orc.set_row_bnds(P.h, 1, UP, 0.0, 1.0),
                 lambda: orc.set_obj_coef(P.h, 1, 2.0), lambda: orc.add_rows(P.h, 1)):
        P.simplex()
        assert P.status != UNDEF
        edit()
        assert P.status == UNDEF and bnb.kkt(P, table=tab)[0] == -3
    P.simplex()
    L = bnb.lib()
    tptr = bnb.C.cast(bnb.C.pointer(tab), bnb.C.c_void_p)
    val, ind = (bnb.C.c_double * 8)(), (bnb.C.c_int * 8)()
    assert L.mvx_bnb_kkt(tptr, None, val, ind, None, None) == -1 and L.mvx_bnb_kkt(tptr, P.h, None, ind, None, None) == -1
    assert L.mvx_bnb_kkt(tptr, P.h, val, None, None, None) == -1 and L.mvx_bnb_kkt(tptr, P.h, val, ind, None, None) == 0
    bare = bnb.table_from(orc)
    bare.get_tableau = None
    assert bnb.kkt(P, table=bare)[0] == -2
    # mvx_check_kkt and the device entries look at their arguments before they look for a device
    G = mvolps_amd.api().create()
    assert G.check_kkt(0)[0] == -1 and G.check_kkt(5)[0] == -1 and G.check_kkt(1, sol=2)[0] == -1
    assert L.mvx_check_kkt(None, 1, 1, None, None, None, None) == -1 and L.mvx_kkt(None, val, ind, None, None) == -1
    assert L.mvx_kkt_many(None, None, 0, None, None) == -1 and L.mvx_kkt_many(G.h, None, -1, None, None) == -1
    assert L.mvx_kkt_many(G.h, None, 0, None, None) == 0 and L.mvx_kkt_many(G.h, None, 1, val, ind) == -1
    assert bnb.kkt_values(np.eye(2), np.zeros(2), np.zeros(2), np.zeros(2), np.zeros(2), np.zeros(2), np.zeros(4), np.zeros(4),
                          np.full(4, BS, dtype=np.int32), 3)[0] == -1
    # the drivers: outside 0..1, and with the best-bound window; both coordinators
    for kw in (dict(kkt=2), dict(kkt=-1), dict(kkt=1, node_strat=1, best_window=8)):
        r = bnb.branch_and_bound(dense_root(orc, (8, 16, 3, 1, 0.1)), table=tab, quirks=0, **kw)
        assert r["rc"] == -1 and r["n_nodes"] == 0 and r["kkt_nodes"] == 0, kw
    from mvolps_amd import dist_bnb, dist_native

    for mod in (dist_bnb, dist_native):
        with pytest.raises(ValueError):
            (mod.branch_and_bound(None, P, kkt=1) if mod is dist_bnb else mod.branch_and_bound(P, kkt=1))
    pr = bnb.make_params(quirks=0, kkt=1)
    res, st = bnb.BnbResult(), dist_native.DistStats()
    assert dist_native._lib().mvx_branchAndBound_dist(tptr, None, P.h, bnb.C.byref(pr), None, None, bnb.C.byref(res), bnb.C.byref(st)) == capi.EFAIL


def replay_nodes(orc, tab, case, quirks, r):
    """The node LPs of the tree `r` as the serial driver solves them, by oid: the children of a branched node are made from its
    solved LP (mvx_bnb_make_children), solved once as children and once more, on a copy, when they are popped."""
    picks = {e[1]: e[7] for e in r["events"] if e[0] == 4}
    kids = {}
    for oid, par in enumerate(r["parent"], start=1):
        kids.setdefault(par, []).append(oid)
    root = dense_root(orc, case)
    if not quirks:
        bnb.integral_bounds(root, table=tab)
    own, solved = {1: root}, {}
    for oid in sorted(picks) + [o for o in range(1, r["n_nodes"] + 1) if o not in picks]:
        if oid not in own:
            continue
        a = own[oid].copy(capi.OFF)
        a.simplex()
        solved[oid] = a
        if oid in picks:
            s2, s3 = bnb.make_children(a, picks[oid], quirks=quirks, table=tab)
            for kid, h in zip(sorted(kids[oid]), (s2, s3)):
                h.simplex()
                own[kid] = h
    return solved


@pytest.mark.parametrize("case", [(8, 16, 3, 1, 0.1), (24, 48, 5, 1, 0.06)])
@pytest.mark.parametrize("quirks", [0, 1])
def test_small_trees_with_the_flag_on(orc, tab, case, quirks):
    kw = dict(table=tab, quirks=quirks, max_nodes=60 if quirks else 0)
    base = bnb.branch_and_bound(dense_root(orc, case), window=1, **kw)
    assert base["rc"] == 0 and base["kkt_nodes"] == 0 and base["kkt_re"] == [0.0] * 4 and base["kkt_oid"] == [0] * 4
    runs = {}
    for w in (1, 8, 64):
        r = bnb.branch_and_bound(dense_root(orc, case), window=w, kkt=1, **kw)
        assert r["rc"] == 0 and treedigest.digest(r) == treedigest.digest(base), (case, quirks, w)
        for key in base:
            if key not in bnb.KKT_COUNTERS:
                assert r[key] == base[key], (key, w)
        assert r["kkt_nodes"] == r["count"] > 1
        runs[w] = r
    assert all(runs[w]["kkt_re"] == runs[1]["kkt_re"] and runs[w]["kkt_oid"] == runs[1]["kkt_oid"] for w in (8, 64))
    # the worst values are the maxima of per-node twin calls, at the lowest oid that reaches them
    solved = replay_nodes(orc, tab, case, quirks, runs[1])
    popped = sorted(solved)[: runs[1]["count"]] if quirks else sorted(solved)
    assert len(popped) == runs[1]["count"]
    worst, at = [0.0] * 4, [0] * 4
    for oid in popped:
        rc, val, _, _, _ = bnb.kkt(solved[oid], table=tab, residuals=False)
        assert rc == 0
        for c in range(4):
            if val[2 * c + 1] > worst[c]:
                worst[c], at[c] = float(val[2 * c + 1]), oid
    assert runs[1]["kkt_re"] == worst and runs[1]["kkt_oid"] == at, (runs[1]["kkt_re"], worst, runs[1]["kkt_oid"], at)


@pytest.mark.parametrize("opts", [dict(cut_strat=1), dict(quirks=1, cut_strat=1, max_nodes=80), dict(heur=2, rc_fix=1, prop=4),
                                  dict(cut_strat=1, heur=2, rc_fix=1, prop=4, node_purge=2), dict(cut_rounds=3, node_cliques=4)],
                         ids=lambda o: "-".join(sorted(o)))
def test_the_booked_values_do_not_depend_on_the_window_with_the_rules_on(orc, tab, opts):
    """The window driver checks a node as its round's solves left it (a re-solve done ahead included), the serial driver behind
    its own solve: the same state, so kkt_nodes, kkt_re and kkt_oid are those of window 1 with cuts, rc_fix, prop, the purge and
    the clique rows on too -- and the flag still changes nothing else."""
    kw = dict(dict(table=tab, quirks=0, max_nodes=3000), **opts)
    for case in ((24, 48, 5, 1, 0.06), (16, 32, 9, 3, 0.2)):
        runs = [bnb.branch_and_bound(dense_root(orc, case), window=w, kkt=1, **kw) for w in (1, 8, 64)]
        off = bnb.branch_and_bound(dense_root(orc, case), window=64, **kw)
        assert all(r["rc"] == 0 for r in runs + [off]) and runs[0]["kkt_nodes"] == runs[0]["count"] > 1
        for r in runs[1:]:
            assert all(r[k] == runs[0][k] for k in bnb.KKT_COUNTERS), (case, r["kkt_re"], runs[0]["kkt_re"])
        assert all(runs[2][k] == off[k] for k in off if k not in bnb.KKT_COUNTERS)


def test_python_front_end_lists_the_new_names():
    C = bnb.C
    assert bnb._TABLE_MORE == ["kkt_many"] and list(bnb.BnbParams._more_) == ["kkt"] and tuple(bnb.BnbResult._more_) == bnb.KKT_COUNTERS
    assert bnb.KKT_CONDS == ("PE", "PB", "DE", "DB")
    for cls in (bnb.LpApiTable, bnb.BnbParams, bnb.BnbResult):  # the further list sits right behind the tail
        last, (off, ctype) = list(cls._tail_.items())[-1]
        first = list(cls._more_.values())[0][0]
        assert off + C.sizeof(ctype) <= first < off + C.sizeof(ctype) + 8 and first < C.sizeof(cls._full_)
    hdr = open(os.path.join(ROOT, "include", "mvx_bnb.h")).read()
    assert hdr.index("(*add_cut_rows_many)") < hdr.index("(*kkt_many)") < hdr.index("} mvx_lp_api;")
    assert hdr.index("int node_cliques;") < hdr.index("int kkt;") < hdr.index("} mvx_bnb_params;")
    assert hdr.index("node_clique_rows;") < hdr.index("kkt_nodes;") < hdr.index("kkt_re[4];") < hdr.index("kkt_oid[4];") < hdr.index("} mvx_bnb_result;")
    assert "glp_check_kkt mvx_check_kkt" in open(os.path.join(ROOT, "include", "glpk_on_mvx.h")).read()
    t = bnb.LpApiTable.from_address(bnb.lib().mvx_hip_lp_api())
    assert bnb.table_entry(t, "kkt_many") and bnb.table_entry(t, "add_cut_rows_many")
    mine = bnb.LpApiTable()
    assert bnb.table_entry(mine, "kkt_many") is None
    bnb.set_table_entry(mine, "kkt_many", 7)
    assert bnb.table_entry(mine, "kkt_many") == 7 and bnb.table_entry(mine, "add_cut_rows_many") is None
    pr = bnb.BnbParams()
    pr.kkt = 5
    bnb.lib().mvx_bnb_default_params(C.byref(pr))  # writes the whole struct
    assert pr.kkt == 0 and pr.node_cliques == 0 and pr.window == 64
    assert bnb.make_params(kkt=1).kkt == 1 and bnb.make_params().kkt == 0
    res = bnb.BnbResult()
    assert res.kkt_nodes == 0 and res.kkt_re == [0.0] * 4 and res.kkt_oid == [0] * 4
    assert hasattr(capi.Prob, "kkt") and hasattr(capi.Prob, "check_kkt") and callable(bnb.kkt_many) and callable(bnb.kkt_values)


def test_cli_flag_parses():
    """--kkt on tests/golden/f1.lp.  Without a device the front end can not solve, so the flag is followed up to its refusals."""
    exe = os.path.join(ROOT, "mvolps_amd", "bin", "mvolps")
    f1 = os.path.join(ROOT, "tests", "golden", "f1.lp")
    assert "--kkt" in subprocess.run([exe, "-h"], capture_output=True, text=True).stdout
    for flags in (("--kkt",), ("--kkt", "--repaired")):
        r = subprocess.run([exe, "-f", f1, *flags], capture_output=True, text=True)
        assert r.returncode != 0 and "Unknown parameter value for --kkt" in r.stderr, (flags, r.stderr)
    r = subprocess.run([exe, "-f", f1, "--kkt", os.devnull, "-bs", "1", "--best-window", "8"], capture_output=True, text=True)
    assert r.returncode != 0 and "--kkt is not supported with --best-window" in r.stderr, r.stderr
