"""CPU: the Farkas proof of an infeasible LP (mvx_bnb_farkas, mvx_bnb_farkas_values, farkas = 1; DESIGN.md "Infeasibility and
unboundedness proofs (farkas)") over the ORACLE's table.

The host twin of k_farkas_rows .. k_farkas_fin is checked bit for bit against mvx_bnb_farkas_values and against a plain
restatement of the definition (64 chains, exact fma) on every node LP of the serial trees of the drawn general instances and of
three dense_ilp trees; every proof it reports is confirmed in exact rational arithmetic from the weights it returns; no feasible
node has one and every MVX_NOFEAS node has one; then the shapes of the rule, the refusals, trees with the flag on, the binding's
names and the command line."""
import ctypes
import ctypes.util
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mvolps_amd
from mvolps_amd import bnb, capi, synth, treedigest
from mvolps_amd.capi import FEAS, NOFEAS, OPT, UNDEF, UP

from . import lpgen
from .test_bnb_general import DRAWN, instance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf
DBL_MAX = np.finfo(float).max
Z = 1e-9  # the zero rule's size
REL = 1e-9  # a side proves above this
DENSE_CASES = [(10, 20, 3, 1, 0.1), (24, 48, 5, 1, 0.06), (16, 32, 9, 3, 0.2)]


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    assert t.get_tableau and t.get_basis and bnb.table_entry(t, "farkas_many") is None
    return t


def _libm_fma():
    name = ctypes.util.find_library("m")
    if not name:
        return None
    fn = getattr(ctypes.CDLL(name), "fma", None)
    if fn is None:
        return None
    fn.restype = ctypes.c_double
    fn.argtypes = [ctypes.c_double] * 3
    return fn if fn(2.0 ** -30, 2.0 ** -30, 1.0) == 1.0 and fn(1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0) == -(2.0 ** -60) else None


_FMA = getattr(math, "fma", None) or _libm_fma()


def fma(a, b, c):
    """a * b + c rounded once: the C library's fma, else exact rational arithmetic and one correctly rounded conversion.  The sums
    here start from +0.0 and never reach -0.0, so an exact zero is +0.0 as the hardware's is."""
    if _FMA is not None:
        return _FMA(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


class Side:
    def __init__(self):
        self.sum, self.act, self.inf, self.drop = 0.0, 0.0, 0, 0

    def term(self, f, b):
        if abs(b) == INF:
            if abs(f) <= Z:
                self.drop += 1
            else:
                self.inf += 1
            b = 0.0
        self.sum = fma(f, b, self.sum)
        self.act = fma(abs(f), abs(b), self.act)


def interval(first, last, f, l, u):
    """The interval rule over p = first..last: 64 chains, chain c taking p = first + c, first + c + 64, ..., halving tree.
    Returns (Lo, Hi, rel_lo, rel_hi, inf_lo, inf_hi, drop_lo, drop_hi)."""
    lo, hi = [Side() for _ in range(64)], [Side() for _ in range(64)]
    for c in range(64):
        for p in range(first + c, last + 1, 64):
            fp = float(f(p))
            bl, bh = (float(u(p)), float(l(p))) if fp < 0.0 else (float(l(p)), float(u(p)))
            if fp == 0.0:
                bl = bh = 0.0
            lo[c].term(fp, bl)
            hi[c].term(fp, bh)
    h = 32
    while h >= 1:
        for c in range(h):
            for s in (lo, hi):
                s[c].sum = s[c].sum + s[c + h].sum
                s[c].act = s[c].act + s[c + h].act
                s[c].inf += s[c + h].inf
                s[c].drop += s[c + h].drop
        h //= 2
    L, H = lo[0], hi[0]
    rel_lo = L.sum / (1.0 + L.act) if L.inf == 0 else -INF
    rel_hi = -H.sum / (1.0 + H.act) if H.inf == 0 else -INF
    return L.sum, H.sum, rel_lo, rel_hi, L.inf, H.inf, L.drop, H.drop


def chain_sum(a, v, cnt):
    """sum_k a(k) v[k], k = 1..cnt, in the KKT check's order."""
    s = [0.0] * 64
    for c in range(64):
        acc = 0.0
        for k in range(c + 1, cnt + 1, 64):
            acc = fma(float(a(k)), float(v[k]), acc)
        s[c] = acc
    h = 32
    while h >= 1:
        for c in range(h):
            s[c] = s[c] + s[c + h]
        h //= 2
    return s[0]


def py_farkas(T, head, nb, rows, lb, ub):
    """The definition on Python floats.  T (m+1, n+1) as get_tableau packs it, head[0..m], nb[0..n], rows (m, n+1), lb / ub
    [0..m+n]: everything 1-based.  Returns (val[4], ind[4], y[0..m])."""
    m, n = rows.shape[0], rows.shape[1] - 1
    best, bi, bside = REL, 0, 0
    for i in range(1, m + 1):
        var = lambda p: int(head[i]) if p == 0 else int(nb[p])  # noqa: E731
        I = interval(0, n, lambda p: 1.0 if p == 0 else -float(T[i, p]), lambda p: lb[var(p)], lambda p: ub[var(p)])
        if I[2] > best:
            best, bi, bside = I[2], i, 1
        if I[3] > best:
            best, bi, bside = I[3], i, 2
    val, ind, y = np.zeros(4), np.zeros(4, dtype=np.int32), np.zeros(m + 1)
    if bi == 0:
        return val, ind, y
    f = np.zeros(m + n + 1)
    f[int(head[bi])] = 1.0
    for q in range(1, n + 1):
        f[int(nb[q])] = -float(T[bi, q])
    g = f.copy()
    de = 0.0
    for j in range(1, n + 1):
        w = chain_sum(lambda r: rows[r - 1, j], f, m)
        g[m + j] = -w
        z = float(f[m + j])
        de = max(de, abs(-w - z) / (1.0 + abs(z)))
    I = interval(1, m + n, lambda k: g[k], lambda k: lb[k], lambda k: ub[k])
    upper = I[3] > I[2]
    rel = I[3] if upper else I[2]
    inf = I[5] if upper else I[4]
    val[:] = [best, rel, -INF if inf else (-I[1] if upper else I[0]), de]
    ind[:] = [2 if rel > REL else 1, bi, bside, I[7] if upper else I[6]]
    y[:] = f[: m + 1]
    y[0] = 0.0
    return val, ind, y


def view(P):
    """What the proof reads of a handle, through the Python getters: 1-based."""
    api, m, n = P.api, P.m, P.n
    rows = np.zeros((m, n + 1))
    for i in range(1, m + 1):
        ind, val = P.get_mat_row(i)
        rows[i - 1, ind] = val
    lo, hi = np.zeros(m + n + 1), np.zeros(m + n + 1)
    for k in range(1, m + n + 1):
        l = api.get_row_lb(P.h, k) if k <= m else api.get_col_lb(P.h, k - m)
        u = api.get_row_ub(P.h, k) if k <= m else api.get_col_ub(P.h, k - m)
        lo[k] = -INF if l <= -DBL_MAX else l
        hi[k] = INF if u >= DBL_MAX else u
    head, nb, _ = P.basis()
    return dict(T=P.tableau(), head=head, nb=nb, rows=rows, lb=lo, ub=hi)


def values_call(v):
    return bnb.farkas_values(v["T"][1:, 1:], v["head"][1:], v["nb"][1:], v["rows"][:, 1:], v["lb"][1:], v["ub"][1:])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_twin(P, tab, what):
    """mvx_bnb_farkas through the table == mvx_bnb_farkas_values == the restatement, every bit.  Returns (view, val, ind, y)."""
    v = view(P)
    want = py_farkas(**v)
    rc, val, ind, y = bnb.farkas(P, table=tab)
    assert rc == 0, (what, rc)
    got2 = values_call(v)
    assert got2[0] == 0
    for got in ((val, ind, y), got2[1:]):
        assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_bits(got[2], want[2]), (what, got, want)
    if ind[0] == 0:
        assert not val.any() and not ind.any() and not y.any(), what
    else:
        assert val[0] > REL and 1 <= ind[1] <= P.m and ind[2] in (1, 2) and (ind[0] == 2) == (val[1] > REL), what
    return v, val, ind, y


def exact_proof(v, y, allow_drops=True):
    """The proof in exact arithmetic from the weights alone: w = A'y exactly, the zero rule on the exact g = (y, -w), and the box
    interval of sum_k g_k x_k.  Returns (proves, dropped) of the better side."""
    rows, lb, ub = v["rows"], v["lb"], v["ub"]
    m, n = rows.shape[0], rows.shape[1] - 1
    yq = [Fraction(float(t)) for t in y]
    g = yq[: m + 1] + [-sum((Fraction(float(rows[r - 1, j])) * yq[r] for r in range(1, m + 1)), Fraction(0)) for j in range(1, n + 1)]
    out = []
    for upper in (False, True):
        total, dropped, finite = Fraction(0), 0, True
        for k in range(1, m + n + 1):
            if g[k] == 0:
                continue
            b = float(ub[k] if (g[k] < 0) != upper else lb[k])
            if abs(b) == INF:
                if abs(g[k]) <= Fraction(Z) and allow_drops:
                    dropped += 1
                else:
                    finite = False
                continue
            total += g[k] * Fraction(b)
        out.append((finite and (total < 0 if upper else total > 0), dropped))
    return out[1] if out[1][0] and not out[0][0] else out[0]


def replay(orc, tab, load, r, quirks=0):
    """The node LPs of the tree `r` as the serial driver solves them, by oid: the children of a branched node are made from its
    solved LP (mvx_bnb_make_children), solved once as children and once more, on a copy, when they are popped."""
    picks = {e[1]: e[7] for e in r["events"] if e[0] == 4}
    kids = {}
    for oid, par in enumerate(r["parent"], start=1):
        kids.setdefault(par, []).append(oid)
    root = load()
    if not quirks and bnb.integral_bounds(root, table=tab) == 2:
        return {}
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


def dense_root(api, case):
    A, b, c, U = synth.dense_ilp(*case)
    return synth.load_ilp(api, A, b, c, U)


def general_trees(orc, tab):
    for rec in DRAWN:
        inst = instance(rec)
        load = lambda inst=inst: lpgen.load_milp(orc, inst)  # noqa: E731
        r = bnb.branch_and_bound(load(), quirks=0, table=tab, max_nodes=200, window=1)
        assert r["rc"] == 0, rec["index"]
        yield ("general", inst["family"], rec["index"]), replay(orc, tab, load, r)


def dense_trees(orc, tab):
    for case in DENSE_CASES:
        load = lambda case=case: dense_root(orc, case)  # noqa: E731
        r = bnb.branch_and_bound(load(), quirks=0, table=tab, max_nodes=600, window=1)
        assert r["rc"] == 0, case
        yield ("dense_ilp", case), replay(orc, tab, load, r)


@pytest.fixture(scope="module")
def census(orc, tab):
    """Every node LP of the trees, checked once: [(family, what, oid, status, view, val, ind, y)]."""
    out = []
    for trees, family in ((general_trees, "general"), (dense_trees, "dense_ilp")):
        for what, solved in trees(orc, tab):
            for oid, P in sorted(solved.items()):
                if P.status == NOFEAS:
                    v, val, ind, y = check_twin(P, tab, (what, oid))
                else:
                    rc, val, ind, y = bnb.farkas(P, table=tab)
                    assert rc == 0, (what, oid)
                    v = view(P) if ind[0] else None
                out.append((family, what, oid, P.status, v, val, ind, y))
    return out


def test_twin_values_and_restatement_agree_on_every_nofeas_node(census):
    """The comparison itself runs in the census (check_twin); here: it had something to compare, in every family."""
    for family, least in (("general", 100), ("dense_ilp", 100)):
        assert sum(1 for c in census if c[0] == family and c[3] == NOFEAS) >= least, family
    # family c: LP-infeasible at the root by construction
    roots = [c for c in census if c[0] == "general" and c[1][1] == "c" and c[2] == 1]
    assert roots and all(c[3] == NOFEAS for c in roots)


def test_a_feasible_node_has_no_proof(census):
    seen = 0
    for family, what, oid, status, v, val, ind, y in census:
        if status in (OPT, FEAS):
            seen += 1
            assert ind[0] == 0 and not val.any() and not ind.any() and not y.any(), (what, oid, val, ind)
    assert seen >= 200


def test_every_proof_holds_in_exact_arithmetic(census):
    proved = 0
    for family, what, oid, status, v, val, ind, y in census:
        if ind[0] != 2:
            continue
        proved += 1
        ok, dropped = exact_proof(v, y)
        assert ok, (what, oid, val, ind)
        if family == "dense_ilp":  # every bound a coefficient needs is finite: a proof without qualification
            assert ind[3] == 0 and exact_proof(v, y, allow_drops=False) == (True, 0), (what, oid, ind)
    assert proved >= 200


# MVX_NOFEAS node LPs of the fixture that no single tableau row proves: (instance, oid).  Both are family c roots on which the
# primal phase 1 stops with several basic variables outside their bounds at once and every row's form unbounded on both sides
# (two to five non-basic variables without the bound the side needs): the proof there is the sum of the violated rows, the
# sum-of-infeasibilities form this rule does not build.  2 of 985 general nodes; the restatement finds found = 0 on both.
UNPROVED = {"general": [(78, 1), (470, 1)], "dense_ilp": []}


def test_every_nofeas_node_is_proved_on_the_model(census):
    """The condition: no MVX_NOFEAS node of these trees ends with found < 2, but for the nodes named in UNPROVED."""
    for family in ("general", "dense_ilp"):
        nodes = [c for c in census if c[0] == family and c[3] == NOFEAS]
        failed = [(c[1][-1], c[2], int(c[6][0])) for c in nodes if c[6][0] != 2]
        assert failed == [(index, oid, 0) for index, oid in UNPROVED[family]], (family, len(nodes), failed)
        assert 50 * len(failed) <= len(nodes), (family, len(failed), len(nodes))  # never more than 2 % of a family
        assert sum(1 for c in nodes if c[6][0] == 2) == len(nodes) - len(UNPROVED[family])


# ------------------------------------------------------------------------------------------------ the shapes of the rule


def two_row_view(t12=1.0):
    """x1 + x2 = xR1 <= 1 and x1 + x2 = xR2 >= 3 on 0 <= x <= 5: the tableau with both auxiliaries basic is the model itself."""
    rows = np.array([[0.0, 1.0, 1.0], [0.0, 1.0, 1.0]])
    T = np.zeros((3, 3))
    T[1, 1:] = [1.0, t12]
    T[2, 1:] = [1.0, 1.0]
    lb = np.array([0.0, -INF, 3.0, 0.0, 0.0])
    ub = np.array([0.0, 1.0, INF, 5.0, 5.0])
    return dict(T=T, head=np.array([0, 1, 2], dtype=np.int32), nb=np.array([0, 3, 4], dtype=np.int32), rows=rows, lb=lb, ub=ub)


def both(v):
    rc, val, ind, y = values_call(v)
    want = py_farkas(**v)
    assert rc == 0 and same_bits(val, want[0]) and np.array_equal(ind, want[1]) and same_bits(y, want[2]), (val, ind, want)
    return val, ind, y


def test_a_row_that_cannot_reach_its_bound_proves():
    # row 2: xR2 - x1 - x2 >= 3 - 10 < 0 on the lower side, <= inf; nothing proves: the LP is feasible (x = (1.5, 1.5) fails row 1,
    # but each row alone is satisfiable)
    val, ind, y = both(two_row_view())
    assert ind[0] == 0 and not val.any() and not y.any()
    # columns capped at 1: row 2's form has Lo = 3 - 2 = 1 > 0
    v = two_row_view()
    v["ub"][3:] = 1.0
    val, ind, y = both(v)
    assert ind.tolist() == [2, 2, 1, 0] and y.tolist() == [0.0, 0.0, 1.0]
    assert val[0] == 1.0 / (1.0 + 5.0) and val[1] == val[0] and val[2] == 1.0 and val[3] == 0.0
    # columns from 2 upwards: row 1's form has Hi = 1 - 4 = -3 < 0, the upper side
    v = two_row_view()
    v["lb"][3:] = 2.0
    val, ind, y = both(v)
    assert ind.tolist() == [2, 1, 2, 0] and y.tolist() == [0.0, 1.0, 0.0] and val[2] == 3.0 and val[0] == 3.0 / (1.0 + 5.0)


def test_tableau_row_that_the_model_does_not_confirm_gives_found_one_and_de_rises():
    v = two_row_view()
    v["ub"][3:] = 1.0
    base = both(v)
    # the rows handed in are not the tableau's: the model's row 2 is x1 + x2 with a coefficient the tableau does not have
    w = dict(v, rows=v["rows"].copy())
    w["rows"][1, 1:] = [3.0, 3.0]  # the model says xR2 = 3 x1 + 3 x2: inside the box it reaches 3
    val, ind, y = both(w)
    assert ind[0] == 1 and ind[1:3].tolist() == [2, 1] and val[0] == base[0][0] and val[1] <= REL and val[3] == 2.0 / 2.0
    # one corrupted alpha: the tableau row still proves, the model confirms it, and de reports the distance
    for eps, lo_de in ((1e-12, 1e-13), (1e-6, 1e-7), (1e-2, 1e-3)):
        w = dict(v, T=v["T"].copy())
        w["T"][2, 2] = 1.0 + eps
        val, ind, y = both(w)
        assert ind[0] == 2 and ind[1] == 2 and lo_de < val[3] < eps, (eps, val)
    assert base[0][3] == 0.0


def test_ties_go_to_the_lowest_row_and_the_lower_side_and_all_zero_rows_prove_nothing():
    m, n = 3, 2
    zero = dict(T=np.zeros((m + 1, n + 1)), head=np.arange(m + 1, dtype=np.int32), nb=np.array([0, 4, 5], dtype=np.int32),
                rows=np.zeros((m, n + 1)), lb=np.full(m + n + 1, -1.0), ub=np.full(m + n + 1, 1.0))
    val, ind, y = both(zero)  # every form is its own auxiliary inside [-1, 1]
    assert ind[0] == 0 and not val.any()
    v = dict(zero, lb=zero["lb"].copy(), ub=zero["ub"].copy())
    v["lb"][2], v["ub"][2] = 1.0, 3.0  # rows 2 and 3 prove by the same amount on the lower side
    v["lb"][3], v["ub"][3] = 1.0, 3.0
    val, ind, y = both(v)
    assert ind.tolist() == [2, 2, 1, 0] and val[0] == 0.5 and y.tolist() == [0.0, 0.0, 1.0, 0.0]
    v["lb"][1], v["ub"][1] = -3.0, -1.0  # row 1 proves by as much on the upper side: the lowest row wins
    val, ind, y = both(v)
    assert ind.tolist() == [2, 1, 2, 0] and val[0] == 0.5 and val[2] == 1.0


def test_the_zero_rule_on_a_free_column():
    v = two_row_view()
    v["ub"][3], v["ub"][4] = 1.0, INF  # x2 has no upper bound: row 2's lower side needs it
    v["lb"][4] = -INF
    val, ind, y = both(v)
    assert ind[0] == 0  # 1.0 on a free column: the side is infinite
    for t, found in ((1e-8, 0), (1e-17, 2)):
        w = dict(v, T=v["T"].copy(), rows=v["rows"].copy())
        w["T"][2, 2] = t
        w["rows"][1, 2] = t
        val, ind, y = both(w)
        assert ind[0] == found, (t, val, ind)
        if found:  # dropped and counted, on both sides of the evaluation; Lo = 3 - 1
            assert ind.tolist() == [2, 2, 1, 1] and val[2] == 2.0 and val[0] == 2.0 / (1.0 + 4.0)
            assert exact_proof(w, y) == (True, 1) and exact_proof(w, y, allow_drops=False)[0] is False


def test_refusals(orc, tab):
    P = dense_root(orc, (16, 32, 9, 3, 0.2))
    assert bnb.farkas(P, table=tab)[0] == -3  # never solved
    P.simplex()
    assert bnb.farkas(P, table=tab)[0] == 0
    orc.set_col_bnds(P.h, 1, capi.DB, 0.0, 1.0)
    assert P.status == UNDEF and bnb.farkas(P, table=tab)[0] == -3
    P.simplex()
    L = bnb.lib()
    tptr = bnb.C.cast(bnb.C.pointer(tab), bnb.C.c_void_p)
    val, ind = (bnb.C.c_double * 4)(), (bnb.C.c_int * 4)()
    assert L.mvx_bnb_farkas(tptr, None, val, ind, None) == -1 and L.mvx_bnb_farkas(tptr, P.h, None, ind, None) == -1
    assert L.mvx_bnb_farkas(tptr, P.h, val, None, None) == -1 and L.mvx_bnb_farkas(tptr, P.h, val, ind, None) == 0
    for name in ("get_tableau", "get_basis", "get_mat_row"):
        bare = bnb.table_from(orc)
        setattr(bare, name, None)
        assert bnb.farkas(P, table=bare)[0] == -2, name
    # the device entries look at their arguments before they look for a device
    G = mvolps_amd.api().create()
    assert L.mvx_farkas(None, val, ind, None) == -1
    assert L.mvx_farkas_many(None, None, 0, None, None) == -1 and L.mvx_farkas_many(G.h, None, -1, None, None) == -1
    assert L.mvx_farkas_many(G.h, None, 0, None, None) == 0 and L.mvx_farkas_many(G.h, None, 1, val, ind) == -1
    assert L.mvx_bnb_farkas_values(0, 1, val, ind, ind, val, val, val, val, ind, None) == -1
    assert L.mvx_bnb_farkas_values(1, 1, None, ind, ind, val, val, val, val, ind, None) == -1
    # the drivers: outside 0..1, and with the best-bound window; both coordinators
    for kw in (dict(farkas=2), dict(farkas=-1), dict(farkas=1, node_strat=1, best_window=8)):
        r = bnb.branch_and_bound(dense_root(orc, (8, 16, 3, 1, 0.1)), table=tab, quirks=0, **kw)
        assert r["rc"] == -1 and r["n_nodes"] == 0 and r["farkas_nodes"] == 0, kw
    from mvolps_amd import dist_bnb, dist_native

    for mod in (dist_bnb, dist_native):
        with pytest.raises(ValueError):
            (mod.branch_and_bound(None, P, farkas=1) if mod is dist_bnb else mod.branch_and_bound(P, farkas=1))
    pr = bnb.make_params(quirks=0, farkas=1)
    res, st = bnb.BnbResult(), dist_native.DistStats()
    assert dist_native._lib().mvx_branchAndBound_dist(tptr, None, P.h, bnb.C.byref(pr), None, None, bnb.C.byref(res), bnb.C.byref(st)) == capi.EFAIL


@pytest.mark.parametrize("case", [(8, 16, 3, 1, 0.1), (24, 48, 5, 1, 0.06)])
@pytest.mark.parametrize("quirks", [0, 1])
def test_small_trees_with_the_flag_on(orc, tab, case, quirks):
    kw = dict(table=tab, quirks=quirks, max_nodes=60 if quirks else 0)
    base = bnb.branch_and_bound(dense_root(orc, case), window=1, **kw)
    assert base["rc"] == 0 and all(base[k] == 0 for k in bnb.FARKAS_COUNTERS)
    runs = {}
    for w in (1, 8, 64):
        r = bnb.branch_and_bound(dense_root(orc, case), window=w, farkas=1, **kw)
        assert r["rc"] == 0 and treedigest.digest(r) == treedigest.digest(base), (case, quirks, w)
        for key in base:
            if key not in bnb.FARKAS_COUNTERS:
                assert r[key] == base[key], (key, w)
        runs[w] = r
    assert all(runs[w][k] == runs[1][k] for w in (8, 64) for k in bnb.FARKAS_COUNTERS)
    # the counters are those of per-node twin calls on a replay
    solved = replay(orc, tab, lambda: dense_root(orc, case), runs[1], quirks)
    popped = sorted(solved)[: runs[1]["count"]] if quirks else sorted(solved)
    assert len(popped) == runs[1]["count"]
    want = dict.fromkeys(bnb.FARKAS_COUNTERS, 0)
    want["farkas_rel_min"] = want["farkas_de_max"] = 0.0
    for oid in popped:
        if solved[oid].status != NOFEAS:
            continue
        rc, val, ind, _ = bnb.farkas(solved[oid], table=tab, weights=False)
        assert rc == 0
        want["farkas_nodes"] += 1
        want[("farkas_none", "farkas_tableau_only", "farkas_proved")[ind[0]]] += 1
        if ind[0] == 2 and (want["farkas_rel_oid"] == 0 or val[1] < want["farkas_rel_min"]):
            want["farkas_rel_min"], want["farkas_rel_oid"] = float(val[1]), oid
        if ind[0] > 0:
            want["farkas_dropped"] += int(ind[3] > 0)
            if val[3] > want["farkas_de_max"]:
                want["farkas_de_max"], want["farkas_de_oid"] = float(val[3]), oid
    assert {k: runs[1][k] for k in bnb.FARKAS_COUNTERS} == want
    if not quirks:
        assert want["farkas_nodes"] > 0 and want["farkas_proved"] == want["farkas_nodes"]


# ------------------------------------------------------------------------------------------------ the unbounded ray


def py_ray(P):
    """The definition on Python floats, from what the getters give of the handle.  Returns (val[4], ind[6], d[0..m+n])."""
    v = view(P)
    T, head, nb, rows, lb, ub = (v[k] for k in ("T", "head", "nb", "rows", "lb", "ub"))
    _, _, flag = P.basis()
    m, n = P.m, P.n
    sg = 1.0 if P.api.get_obj_dir(P.h) == capi.MIN else -1.0
    c = np.array([0.0] + [P.api.get_obj_coef(P.h, j) for j in range(1, n + 1)])
    val, ind, d = np.zeros(4), np.zeros(6, dtype=np.int32), np.zeros(m + n + 1)
    qp, sp = 0, 0.0
    for q in range(1, n + 1):
        e, f = sg * float(T[0, q]), int(flag[q])
        sigma = 1.0 if e < -1e-9 and f in (capi.NL, capi.NF) else -1.0 if e > 1e-9 and f in (capi.NU, capi.NF) else 0.0
        if sigma == 0.0 or (ub[nb[q]] != INF if sigma > 0 else lb[nb[q]] != -INF):
            continue
        moves = [(sigma * float(T[i, q]), int(head[i])) for i in range(1, m + 1) if abs(float(T[i, q])) > Z]
        if all((ub[k] == INF if mv > 0.0 else lb[k] == -INF) for mv, k in moves):
            qp, sp = q, sigma
            break
    if qp == 0:
        return val, ind, d
    d[int(nb[qp])] = sp
    for i in range(1, m + 1):
        d[int(head[i])] = sp * float(T[i, qp])
    ds = d[m:].copy()
    ae = re = 0.0
    ai = ri = 0
    for i in range(1, m + 1):
        a = abs(float(d[i]) - chain_sum(lambda j: rows[i - 1, j], ds, n))
        r = a / (1.0 + abs(float(d[i])))
        if a > ae:
            ae, ai = a, i
        if r > re:
            re, ri = r, i
    slope = chain_sum(lambda j: c[j], ds, n)
    blocked = sum(1 for k in range(1, m + n + 1) if abs(d[k]) > Z and (ub[k] != INF if d[k] > 0.0 else lb[k] != -INF))
    val[:] = [float(T[0, qp]), ae, re, slope]
    ind[:] = [2 if sg * slope < 0.0 and re <= 1e-9 and blocked == 0 else 1, int(nb[qp]), 1 if sp > 0 else -1, blocked, ai, ri]
    return val, ind, d


def cone(api, direction, n=3, cap=None):
    """max x1 + ... + xn (or the MIN mirror) over x1 - x2 <= 1, xj - x(j+1) <= 1, ..., x >= 0: every column can grow with the next
    one.  cap: an upper bound on the last column, which closes the cone."""
    A = np.zeros((n - 1, n))
    for i in range(n - 1):
        A[i, i], A[i, i + 1] = 1.0, -1.0
    col_b = [(capi.LO, 0.0, 0.0)] * n
    if cap is not None:
        col_b = col_b[:-1] + [(capi.DB, 0.0, cap)]
    P = api.create()
    P.load_general(A, [(UP, 0.0, 1.0)] * (n - 1), col_b, np.ones(n) if direction == capi.MAX else -np.ones(n), direction=direction)
    return P


def check_ray_twin(P, tab, what):
    want = py_ray(P)
    rc, val, ind, d = bnb.ray(P, table=tab)
    assert rc == 0, (what, rc)
    assert same_bits(val, want[0]) and np.array_equal(ind, want[1]) and same_bits(d, want[2]), (what, val, want[0], ind, want[1], d, want[2])
    nrc, nval, nind, nd = bnb.ray(P, table=tab, direction=False)
    assert nrc == 0 and nd is None and same_bits(nval, val) and np.array_equal(nind, ind)
    return val, ind, d


def test_the_ray_of_an_unbounded_cone_and_its_min_mirror(orc, tab):
    for direction in (capi.MAX, capi.MIN):
        for n in (2, 3, 9):
            P = cone(orc, direction, n)
            P.simplex()
            assert P.status == capi.UNBND, (direction, n)
            val, ind, d = check_ray_twin(P, tab, (direction, n))
            assert ind[0] == 2 and ind[3] == 0 and 1 <= ind[1] <= P.m + P.n and ind[2] in (1, -1) and val[1] == 0.0 and val[2] == 0.0
            assert (val[3] > 0.0) == (direction == capi.MAX) and val[3] != 0.0
            # the ray by itself: inside the recession cone of the model
            rows = view(P)["rows"]
            assert np.all(rows[:, 1:] @ d[P.m + 1:] == d[1:P.m + 1]) and np.all(d[P.m + 1:] >= 0.0) and np.all(d[1:P.m + 1] <= 0.0)
    # the published duals of the two directions mirror each other
    a, b = cone(orc, capi.MAX), cone(orc, capi.MIN)
    a.simplex()
    b.simplex()
    ra, rb = bnb.ray(a, table=tab), bnb.ray(b, table=tab)
    assert ra[1][0] == -rb[1][0] and ra[1][3] == -rb[1][3] and np.array_equal(ra[2], rb[2]) and same_bits(ra[3], rb[3])


def test_a_ray_that_one_finite_bound_blocks_is_refused(orc, tab):
    P = cone(orc, capi.MAX, 3, cap=50.0)
    P.simplex()
    assert P.status == OPT
    val, ind, d = check_ray_twin(P, tab, "capped")
    assert not val.any() and not ind.any() and not d.any()
    # stopped inside the cone by an iteration limit: improving columns exist, each is blocked by a row or the capped column
    for lim in (0, 1, 2):
        P = cone(orc, capi.MAX, 3, cap=50.0)
        P.simplex(it_lim=lim)
        val, ind, d = check_ray_twin(P, tab, ("capped", lim))
        assert ind[0] == 0, (lim, ind)
    # the solved, feasible and the infeasible node LPs of a tree have none either
    P = dense_root(orc, (16, 32, 9, 3, 0.2))
    P.simplex()
    assert check_ray_twin(P, tab, "opt")[1][0] == 0
    orc.set_col_bnds(P.h, 1, capi.LO, 1e6, 0.0)
    P.simplex()
    assert P.status == NOFEAS and check_ray_twin(P, tab, "nofeas")[1][0] == 0


def test_ray_refusals(orc, tab):
    P = cone(orc, capi.MAX)
    assert bnb.ray(P, table=tab)[0] == -3  # never solved
    P.simplex()
    L = bnb.lib()
    tptr = bnb.C.cast(bnb.C.pointer(tab), bnb.C.c_void_p)
    val, ind = (bnb.C.c_double * 4)(), (bnb.C.c_int * 6)()
    assert L.mvx_bnb_ray(tptr, None, val, ind, None) == -1 and L.mvx_bnb_ray(tptr, P.h, None, ind, None) == -1
    assert L.mvx_bnb_ray(tptr, P.h, val, None, None) == -1 and L.mvx_bnb_ray(tptr, P.h, val, ind, None) == 0
    for name in ("get_tableau", "get_basis", "get_mat_row", "get_obj_coef"):
        bare = bnb.table_from(orc)
        setattr(bare, name, None)
        assert bnb.ray(P, table=bare)[0] == -2, name
    # the device entries look at their arguments and at the handle before they look for a device
    G = mvolps_amd.api().create()
    assert L.mvx_ray(None, val, ind, None) == -1 and L.mvx_ray(G.h, None, ind, None) == -1 and L.mvx_ray(G.h, val, ind, None) == -3
    assert L.mvx_get_unbnd_ray(None) == 0 and G.get_unbnd_ray() == 0
    assert "glp_get_unbnd_ray mvx_get_unbnd_ray" in open(os.path.join(ROOT, "include", "glpk_on_mvx.h")).read()
    assert hasattr(capi.Prob, "ray") and hasattr(capi.Prob, "get_unbnd_ray") and callable(bnb.ray)


def test_python_front_end_lists_the_new_names():
    C = bnb.C
    assert bnb._TABLE_EXTRA == ["farkas_many"] and list(bnb.BnbParams._extra_) == ["farkas"]
    assert tuple(bnb.BnbResult._extra_) == bnb.FARKAS_COUNTERS
    # the lists the earlier members sit in have not moved
    assert bnb._TABLE_MORE == ["kkt_many"] and list(bnb.BnbParams._more_) == ["kkt"] and tuple(bnb.BnbResult._more_) == bnb.KKT_COUNTERS
    for cls in (bnb.LpApiTable, bnb.BnbParams, bnb.BnbResult):  # the new list sits right behind the one before
        last, (off, ctype) = list(cls._more_.items())[-1]
        first = list(cls._extra_.values())[0][0]
        assert off + C.sizeof(ctype) <= first < off + C.sizeof(ctype) + 8 and first < C.sizeof(cls._full_)
    hdr = open(os.path.join(ROOT, "include", "mvx_bnb.h")).read()
    assert hdr.index("(*kkt_many)") < hdr.index("(*farkas_many)") < hdr.index("} mvx_lp_api;")
    assert hdr.index("int kkt;") < hdr.index("int farkas;") < hdr.index("} mvx_bnb_params;")
    at = [hdr.index(" %s;" % name) for name in ("kkt_oid[4]",) + bnb.FARKAS_COUNTERS] + [hdr.index("} mvx_bnb_result;")]
    assert at == sorted(at)
    t = bnb.LpApiTable.from_address(bnb.lib().mvx_hip_lp_api())
    assert bnb.table_entry(t, "farkas_many") and bnb.table_entry(t, "kkt_many")
    mine = bnb.LpApiTable()
    assert bnb.table_entry(mine, "farkas_many") is None
    bnb.set_table_entry(mine, "farkas_many", 7)
    assert bnb.table_entry(mine, "farkas_many") == 7 and bnb.table_entry(mine, "kkt_many") is None
    pr = bnb.BnbParams()
    pr.farkas = 5
    bnb.lib().mvx_bnb_default_params(C.byref(pr))  # writes the whole struct
    assert pr.farkas == 0 and pr.kkt == 0 and pr.window == 64
    assert bnb.make_params(farkas=1).farkas == 1 and bnb.make_params().farkas == 0
    res = bnb.BnbResult()
    assert all(getattr(res, k) == 0 for k in bnb.FARKAS_COUNTERS)
    assert hasattr(capi.Prob, "farkas") and callable(bnb.farkas) and callable(bnb.farkas_many) and callable(bnb.farkas_values)


def test_cli_flag_parses():
    """--farkas on tests/golden/f1.lp.  Without a device the front end can not solve, so the flag is followed up to its refusals."""
    exe = os.path.join(ROOT, "mvolps_amd", "bin", "mvolps")
    f1 = os.path.join(ROOT, "tests", "golden", "f1.lp")
    assert "--farkas" in subprocess.run([exe, "-h"], capture_output=True, text=True).stdout
    for flags in (("--farkas",), ("--farkas", "--repaired")):
        r = subprocess.run([exe, "-f", f1, *flags], capture_output=True, text=True)
        assert r.returncode != 0 and "Unknown parameter value for --farkas" in r.stderr, (flags, r.stderr)
    r = subprocess.run([exe, "-f", f1, "--farkas", os.devnull, "-bs", "1", "--best-window", "8"], capture_output=True, text=True)
    assert r.returncode != 0 and "--farkas is not supported with --best-window" in r.stderr, r.stderr
