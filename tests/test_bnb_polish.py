"""CPU: incumbent polishing (mvx_bnb_params.polish, DESIGN.md "Incumbent polishing (polish)"), driver over the ORACLE's table.

mvx_bnb_polish (the host twin of k_lsact / k_lsmove / k_lsapply) is checked bit for bit against a plain-Python restatement of
the definition (scalar loops, one operation at a time), structurally (feasible, never worse, locally optimal by a brute-force
scan, refusals, continuous columns), on hand-made tie models, and in whole trees: every general fixture closes on its
enumerated pin with it under every single-GPU driver, the windows give the serial tree, polish = 0 is the run without the
keyword, and the refusals return their codes."""
import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import DB, IV, MAX, OPT, UP

from . import lpgen
from .test_bnb_general import DRAWN, INSTANCES, check_pin, instance, run
from .test_bnb_heuristic import Model
from .test_bnb_host import same_result

# dense_ilp(m, n, seed, U, cap): the six small models of DESIGN.md's table; a numpy prototype over the HiGHS vertex reached the
# same values; what the twin reaches from the oracle's vertex is recorded in REACHED
DENSE = [(10, 20, 3, 3, 0.4), (24, 48, 5, 3, 0.3), (32, 64, 7, 3, 0.4), (64, 128, 7, 3, 0.4), (128, 256, 7, 3, 0.4), (32, 64, 7, 1, 0.2)]
# (heur 2 root point, after the search, moves) over the oracle's root vertex
REACHED = {
    (10, 20, 3, 3, 0.4): (87.0, 98.0, 2),
    (24, 48, 5, 3, 0.3): (236.0, 242.0, 3),
    (32, 64, 7, 3, 0.4): (370.0, 387.0, 3),
    (64, 128, 7, 3, 0.4): (881.0, 897.0, 7),
    (128, 256, 7, 3, 0.4): (1689.0, 1731.0, 9),
    (32, 64, 7, 1, 0.2): (182.0, 188.0, 1),
}


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    assert not t.polish_many  # the host twin is what runs over the oracle
    return t


def tol(b):
    return 1e-9 * max(1.0, abs(b))


class Plain:
    """The definition, one operation at a time on Python floats.  Columns are 0-based here: unit move u = 2 j + (d < 0)."""

    def __init__(self, M):
        self.M = M
        self.m, self.n = M.A.shape
        self.A = [[float(M.A[i, j]) for j in range(self.n)] for i in range(self.m)]
        self.rows_of = [[i for i in range(self.m) if self.A[i][j] != 0.0] for j in range(self.n)]
        self.lo_t = [float(M.rlo[i]) - tol(float(M.rlo[i])) for i in range(self.m)]
        self.hi_t = [float(M.rhi[i]) + tol(float(M.rhi[i])) for i in range(self.m)]
        self.c = [float(t) for t in M.c]

    def activity(self, x):
        out = []
        for i in range(self.m):
            s = 0.0
            for j in range(self.n):
                if self.A[i][j] != 0.0 and x[j] != 0.0:
                    s = s + self.A[i][j] * x[j]
            out.append(s)
        return out

    def feasible(self, x, r):
        M = self.M
        for j in range(self.n):
            if not (M.clo[j] <= x[j] <= M.chi[j]):
                return False
        for i in range(self.m):
            if not (self.lo_t[i] <= r[i] <= self.hi_t[i]):
                return False
        return True

    def objective(self, x):
        s = 0.0
        for j in range(self.n):
            s = s + self.c[j] * x[j]
        return s + self.M.c0

    def inside(self, i, t):
        return self.lo_t[i] <= t <= self.hi_t[i]

    def moves(self, x):
        """(u, j, d, gain) of every admissible unit move, ascending u."""
        M = self.M
        out = []
        for j in range(self.n):
            if not M.isint[j]:
                continue
            for d in (1.0, -1.0):
                if float(np.ceil(M.clo[j])) <= x[j] + d <= float(np.floor(M.chi[j])):
                    out.append((2 * j + (1 if d < 0 else 0), j, d, M.sg * (d * self.c[j])))
        return out

    def best(self, x, r):
        """The choice of one iteration: (gain, u move, v move or None), or None."""
        mv = self.moves(x)
        best, pick = 0.0, None
        for u in mv:
            _, j, d, g = u
            if g > best and all(self.inside(i, r[i] + d * self.A[i][j]) for i in self.rows_of[j]):
                best, pick = g, (u, None)
        for a, u in enumerate(mv):
            _, ju, du, gu = u
            for v in mv[a + 1:]:
                _, jv, dv, gv = v
                if jv == ju:
                    continue
                g = gu + gv
                if not g > best:
                    continue
                good = True
                for i in sorted(set(self.rows_of[ju]) | set(self.rows_of[jv])):
                    if not self.inside(i, (r[i] + du * self.A[i][ju]) + dv * self.A[i][jv]):
                        good = False
                        break
                if good:
                    best, pick = g, (u, v)
        return pick

    def polish(self, x_in, max_moves):
        """(x, obj, moves, ok) as mvx_bnb_polish returns them for the point x_in[0..n-1]."""
        M = self.M
        x = [float(t) for t in x_in]
        for j in range(self.n):
            if M.isint[j]:
                ri = float(np.rint(x[j]))
                if not abs(x[j] - ri) <= 1e-9:
                    return list(x_in), 0.0, 0, 0
                x[j] = ri
        r = self.activity(x)
        if not self.feasible(x, r):
            return list(x_in), 0.0, 0, 0
        x0, obj0 = list(x), self.objective(x)
        taken = 0
        while taken < max_moves:
            pick = self.best(x, r)
            if pick is None:
                break
            for mvv in pick:
                if mvv is None:
                    continue
                _, j, d, _ = mvv
                for i in range(self.m):
                    if self.A[i][j] != 0.0:
                        r[i] = r[i] + d * self.A[i][j]
                x[j] = x[j] + d
            taken += 1
        if self.feasible(x, self.activity(x)):
            return x, self.objective(x), taken, 1
        return x0, obj0, 0, 1


def twin(root, x, max_moves, tab):
    """mvx_bnb_polish on the point x[0..n-1]: (x, obj, moves, ok)."""
    rc, xs, obj, moves, ok = bnb.polish_many(root, np.concatenate(([0.0], x)), max_moves, table=tab)
    assert rc == 0
    return xs[0, 1:], float(obj[0]), int(moves[0]), int(ok[0])


def same_bits(got, want):
    gx, gobj, gmoves, gok = got
    wx, wobj, wmoves, wok = want
    assert gok == wok and gmoves == wmoves, (gok, wok, gmoves, wmoves)
    assert np.array_equal(np.asarray(gx), np.asarray(wx)), (gx, wx)
    assert gobj == wobj, (gobj, wobj)


def dense_model(case):
    m, n, seed, U, cap = case
    A, b, c, U = synth.dense_ilp(m, n, seed, U, cap)
    row_b = [(UP, 0.0, float(bi)) for bi in b]
    col_b = [(DB, 0.0, U)] * n
    return Model(A, row_b, col_b, c, 0.0, [IV] * n, MAX), (A, b, c, U)


def heur2_root(orc, tab, root, mode=2):
    """The root's heur 2 (or heur 1) point x[0..n-1], or None when the root LP is not optimal or the heuristic finds nothing."""
    node = root.copy()
    node.simplex()
    if node.status != OPT:
        return None
    rc, _obj, found, x = bnb.round_node(node, root, mode, table=tab)
    assert rc == 0
    return x[1:].copy() if found else None


_DENSE_CACHE = {}


def dense_root(orc, tab, case):
    """(model, root handle, heur 2 point) of a dense case, computed once."""
    if case not in _DENSE_CACHE:
        M, (A, b, c, U) = dense_model(case)
        root = lpgen.load_ilp(orc, A, b, c, U)
        _DENSE_CACHE[case] = (M, root, heur2_root(orc, tab, root))
    return _DENSE_CACHE[case]


def general_model(inst):
    return Model(inst["A"], inst["row_b"], inst["col_b"], inst["c"], inst["c0"], inst["kinds"], inst["direction"])


# ------------------------------------------------------------------------------------------------ 1. the twin's bits


def test_twin_matches_definition_on_general_fixtures(orc, tab):
    """Mixed signs, ranged rows, minimisation, continuous columns: the rounded (heur 1) and the filled (heur 2) root point of
    every fixture that has one.  Both are nearly always locally optimal on these small models, so each is also walked away
    from the optimum first (the restatement with the sense turned round, which ends on a feasible point) and polished from there."""
    seen = moved = 0
    for rec in INSTANCES:
        if rec["status"] != "optimal":
            continue
        inst = instance(rec)
        root = lpgen.load_milp(orc, inst)
        if bnb.fractional_bounds(root, table=tab) != 0:
            continue  # the drivers round such bounds first; the model as loaded is not the tree's
        P = Plain(general_model(inst))
        away = general_model(inst)
        away.sg = -away.sg
        for mode in (1, 2):
            x = heur2_root(orc, tab, root, mode)
            if x is None:
                continue
            far = np.array(Plain(away).polish(x, 1000)[0])
            for start in (x, far):
                for cap in (1, 2, 1000):
                    want = P.polish(start, cap)
                    same_bits(twin(root, start, cap, tab), want)
                seen += 1
                moved += want[2] > 0
    assert seen >= 240 and moved >= 40, (seen, moved)  # coverage: enough starts that really move


@pytest.mark.parametrize("case", DENSE, ids=str)
def test_twin_matches_definition_on_dense_ilps(orc, tab, case):
    M, root, x = dense_root(orc, tab, case)
    assert x is not None
    same_bits(twin(root, x, 1000, tab), Plain(M).polish(x, 1000))


# ------------------------------------------------------------------------------------------------ 2. structure


def brute_force_best_gain(M, x):
    """The greatest gain of a feasible candidate at the feasible integer point x, by vectors: every single, every pair."""
    A = M.A
    m, n = A.shape
    r = np.array(Plain(M).activity([float(t) for t in x]))
    lo_t = np.array([M.rlo[i] - tol(M.rlo[i]) for i in range(m)])
    hi_t = np.array([M.rhi[i] + tol(M.rhi[i]) for i in range(m)])
    cols = [j for j in range(n) if M.isint[j]]
    units = [(j, d) for j in cols for d in (1.0, -1.0) if float(np.ceil(M.clo[j])) <= x[j] + d <= float(np.floor(M.chi[j]))]
    best = 0.0
    for a, (ju, du) in enumerate(units):
        s = r + du * A[:, ju]
        gu = M.sg * (du * M.c[ju])
        if gu > best and np.all((s >= lo_t) & (s <= hi_t) | (A[:, ju] == 0)):
            best = gu
        for jv, dv in units[a + 1:]:
            if jv == ju:
                continue
            g = gu + M.sg * (dv * M.c[jv])
            if g > best:
                t = s + dv * A[:, jv]
                if np.all((t >= lo_t) & (t <= hi_t) | ((A[:, ju] == 0) & (A[:, jv] == 0))):
                    best = g
    return best


def entry_point(M, x):
    return [float(np.rint(t)) if M.isint[j] else float(t) for j, t in enumerate(x)]


def check_structure(tab, M, root, x, check):
    e = Plain(M)
    entry = entry_point(M, x)
    entry_obj = e.objective(entry)
    px, pobj, pmoves, pok = twin(root, x, 1000, tab)
    assert pok == 1
    assert check(px) and e.feasible(list(px), e.activity(list(px)))  # mvx_bnb_round's check, and its restatement
    assert M.sg * pobj >= M.sg * entry_obj
    assert (pmoves > 0) == (M.sg * pobj > M.sg * entry_obj)
    cont = ~M.isint
    assert np.array_equal(px[cont], np.asarray(x)[cont])
    assert pmoves < 1000 and brute_force_best_gain(M, px) == 0.0
    # max_moves = 1 is the first move of the longer run
    x1, _obj1, moves1, ok1 = twin(root, x, 1, tab)
    assert ok1 == 1 and moves1 == min(1, pmoves)
    want = list(entry)
    if pmoves:
        for mvv in e.best(entry, e.activity(entry)):
            if mvv is not None:
                want[mvv[1]] += mvv[2]
    assert np.array_equal(x1, np.array(want))
    return pmoves


def round_check(orc, tab, root):
    """mvx_bnb_round's Feasible rule on a point, through a handle whose LP is the point: mode 1 on a fixed copy."""

    def check(px):
        node = root.copy()
        for j, v in enumerate(px):
            orc.set_col_bnds(node.h, j + 1, 5, float(v), float(v))  # FX
        node.simplex()
        if node.status != OPT:
            return False
        rc, _obj, found, xr = bnb.round_node(node, root, 1, table=tab)
        return rc == 0 and found == 1 and np.array_equal(xr[1:], px)

    return check


@pytest.mark.parametrize("case", DENSE[:4], ids=str)
def test_structure_dense(orc, tab, case):
    M, root, x = dense_root(orc, tab, case)
    moves = check_structure(tab, M, root, x, round_check(orc, tab, root))
    assert moves >= 1


def test_structure_general(orc, tab):
    done = 0
    for rec in DRAWN[::3]:
        if rec["status"] != "optimal":
            continue
        inst = instance(rec)
        root = lpgen.load_milp(orc, inst)
        if bnb.fractional_bounds(root, table=tab) != 0:
            continue
        x = heur2_root(orc, tab, root)
        if x is None:
            continue
        check_structure(tab, general_model(inst), root, x, round_check(orc, tab, root))
        done += 1
    assert done >= 20


def test_refused_points_come_back_untouched(orc, tab):
    M, root, x = dense_root(orc, tab, DENSE[0])
    frac = x.copy()
    frac[3] += 0.25
    over = x.copy()
    over[:] = 3.0  # every row violated
    near = x.copy()
    near[2] += 5e-10  # within 1e-9 of an integer: taken as the integer
    for bad in (frac, over):
        px, pobj, pmoves, pok = twin(root, bad, 1000, tab)
        assert pok == 0 and pmoves == 0 and pobj == 0.0 and np.array_equal(px, bad)
    same_bits(twin(root, near, 1000, tab), twin(root, x, 1000, tab))
    # a mixed model: a continuous column outside its bounds
    for rec in DRAWN:
        inst = instance(rec)
        Mg = general_model(inst)
        if rec["status"] != "optimal" or Mg.isint.all():
            continue
        rootg = lpgen.load_milp(orc, inst)
        xg = None if bnb.fractional_bounds(rootg, table=tab) != 0 else heur2_root(orc, tab, rootg)
        bounded = [j for j in np.flatnonzero(~Mg.isint) if np.isfinite(Mg.chi[j])]
        if xg is None or not bounded:
            continue
        badg = xg.copy()
        badg[bounded[0]] = Mg.chi[bounded[0]] + 1.0
        px, pobj, pmoves, pok = twin(rootg, badg, 1000, tab)
        assert pok == 0 and pmoves == 0 and pobj == 0.0 and np.array_equal(px, badg)
        return
    raise AssertionError("no mixed fixture with a bounded continuous column")


# ------------------------------------------------------------------------------------------------ 3. the dense models


@pytest.mark.parametrize("case", DENSE, ids=str)
def test_dense_ilps_rise_strictly(orc, tab, case):
    M, root, x = dense_root(orc, tab, case)
    entry = Plain(M).objective([float(t) for t in x])
    _px, pobj, pmoves, pok = twin(root, x, 1000, tab)
    print("dense_ilp%r: heur 2 root point %.10g, after the search %.10g, %d moves" % (case, entry, pobj, pmoves))
    assert pok == 1 and pmoves >= 1 and pobj > entry
    assert (entry, pobj, pmoves) == REACHED[case]  # the values reached, recorded


# ------------------------------------------------------------------------------------------------ 4. the tie rule


def tie_model(orc, A, b, c):
    A = np.asarray(A, dtype=float)
    n = A.shape[1]
    row_b = [(UP, 0.0, float(t)) for t in b]
    col_b = [(DB, 0.0, 1.0)] * n
    M = Model(A, row_b, col_b, c, 0.0, [IV] * n, MAX)
    P = orc.create()
    P.load_general(A, row_b, col_b, np.asarray(c, dtype=float), kinds=[IV] * n, direction=MAX)
    return M, P


# 2 rows x 6 binary columns, maximisation, from x = 0; `first` is the point the tie rule must reach with its first move
TIES = {
    # Equal costs give a single gain 1 and a pair gain 2, 0 or -2: the two can only tie when one column costs what two others
    # do.  Column 2 costs 2 and fills row 1 alone; every pair of the other columns also gains 2 and fits, the pair
    # (+col 0, +col 1) with the lowest index(u) of all candidates: the single wins.
    "single_before_pair": dict(A=[[1, 1, 2, 1, 1, 1], [0, 0, 0, 0, 0, 0]], b=[2, 0], c=[1, 1, 2, 1, 1, 1], first=[0, 0, 1, 0, 0, 0]),
    # equal costs; row 1 holds one unit, so only singles fit and all gain 1; row 2 forbids column 0: the next index wins
    "lower_index_u": dict(A=[[1, 1, 1, 1, 1, 1], [1, 0, 0, 0, 0, 0]], b=[1, 0], c=[1] * 6, first=[0, 1, 0, 0, 0, 0]),
    # equal costs; row 1 holds two units, every pair gains 2; row 2 keeps columns 0 and 1 apart: u = +col 0, the lowest v that
    # fits is +col 2
    "lower_index_v": dict(A=[[1, 1, 1, 1, 1, 1], [1, 1, 0, 0, 0, 0]], b=[2, 1], c=[1] * 6, first=[1, 0, 1, 0, 0, 0]),
}


@pytest.mark.parametrize("name", sorted(TIES))
def test_tie_rule(orc, tab, name):
    t = TIES[name]
    M, P = tie_model(orc, t["A"], t["b"], t["c"])
    x = np.zeros(6)
    px, _obj, moves, ok = twin(P, x, 1, tab)
    assert ok == 1 and moves == 1
    assert np.array_equal(px, np.array(t["first"], dtype=float)), (name, px)
    same_bits(twin(P, x, 1000, tab), Plain(M).polish(x, 1000))


# ------------------------------------------------------------------------------------------------ 5. trees

DRIVERS = {
    "serial": dict(window=1),
    "window64": dict(window=64),
    "best": dict(node_strat=1, window=1),
    "best_window8": dict(node_strat=1, best_window=8),
}


def same_polish(a, b):
    for k in bnb.POLISH_COUNTERS + ("heur_calls", "heur_found", "heur_improved", "incumbent_heur"):
        assert a[k] == b[k], k


@pytest.mark.parametrize("driver", sorted(DRIVERS))
def test_general_fixtures_close_on_their_pins(orc, tab, driver):
    bad, polished, improved = [], 0, 0
    for rec in INSTANCES:
        inst = instance(rec)
        try:
            r = run(orc, rec, inst, table=tab, heur=2, polish=1000, **DRIVERS[driver])
            check_pin(rec, inst, r)
        except AssertionError as e:
            bad.append("instance %d: %s" % (rec["index"], str(e).splitlines()[0][:200]))
            continue
        polished += r["polish_calls"]
        improved += r["polish_improved"]
    assert not bad, "\n".join(bad)
    assert polished > 100 and improved > 10, (polished, improved)


def windows_equal_serial(load, tab, **kw):
    ref = bnb.branch_and_bound(load(), window=1, quirks=0, table=tab, heur=2, polish=1000, **kw)
    assert ref["rc"] == 0
    for w in (2, 8, 64):
        got = bnb.branch_and_bound(load(), window=w, quirks=0, table=tab, heur=2, polish=1000, **kw)
        assert got["rc"] == 0
        same_result(got, ref)
        same_polish(got, ref)
    bref = bnb.branch_and_bound(load(), node_strat=1, best_window=0, quirks=0, table=tab, heur=2, polish=1000, **kw)
    assert bref["rc"] == 0
    for w in (2, 8, 64):
        got = bnb.branch_and_bound(load(), node_strat=1, best_window=w, quirks=0, table=tab, heur=2, polish=1000, **kw)
        assert got["rc"] == 0
        same_result(got, bref)
        same_polish(got, bref)
    return ref, bref


def test_windows_equal_serial_on_general_fixtures(orc, tab):
    calls = 0
    for rec in DRAWN[::10]:
        inst = instance(rec)
        ref, _ = windows_equal_serial(lambda: lpgen.load_milp(orc, inst), tab, max_nodes=50 * rec["points"] + 1000)
        calls += ref["polish_calls"]
    assert calls > 0


def test_windows_equal_serial_on_dense_ilp(orc, tab):
    A, b, c, U = synth.dense_ilp(24, 48, 5, 3, 0.3)
    ref, bref = windows_equal_serial(lambda: lpgen.load_ilp(orc, A, b, c, U), tab, max_nodes=600)
    assert ref["polish_calls"] > 0 and ref["polish_moves"] > 0 and ref["polish_improved"] > 0
    assert bref["polish_calls"] > 0


def test_polish_zero_is_the_run_without_it(orc, tab):
    A, b, c, U = synth.dense_ilp(10, 20, 3, 3, 0.4)
    for kw in (dict(window=1), dict(window=64), dict(node_strat=1, best_window=8)):
        ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), quirks=0, table=tab, heur=2, max_nodes=400, **kw)
        got = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), quirks=0, table=tab, heur=2, max_nodes=400, polish=0, **kw)
        assert ref == got
        assert all(got[k] == 0 for k in bnb.POLISH_COUNTERS)
        on = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), quirks=0, table=tab, heur=2, max_nodes=400, polish=1000, **kw)
        assert on["rc"] == 0 and on["polish_calls"] > 0 and on["polish_improved"] > 0
        assert on["best_lower"] >= ref["best_lower"]


def test_refusals(orc, tab):
    from mvolps_amd import dist_bnb, dist_native

    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    for kw in (dict(polish=-1, quirks=0), dict(polish=100001, quirks=0), dict(polish=1, quirks=1), dict(polish=1000)):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, **kw)
        assert r["rc"] == -1 and r["n_nodes"] == 0 and r["count"] == 0, kw
    r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, polish=100000, quirks=0, node_strat=1, best_window=8)
    assert r["rc"] == 0 and r["polish_calls"] > 0  # allowed with best_window
    P = lpgen.load_ilp(orc, A, b, c, U)
    with pytest.raises(ValueError):
        dist_native.branch_and_bound(P, table=tab, polish=10, quirks=0)
    with pytest.raises(ValueError):
        dist_bnb.branch_and_bound(None, P, polish=10, quirks=0)
    # neither polish_many nor the twin's accessors: the tree ends with -2, not with unpolished incumbents
    bare = bnb.table_from(orc)
    bare.get_mat_row = None
    for kw in (dict(window=1), dict(window=64), dict(node_strat=1, best_window=8)):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bare, polish=10, quirks=0, **kw)
        assert r["rc"] == -2 and r["polish_calls"] == 0, kw
    # mvx_bnb_polish's own codes
    x = np.zeros((1, 17))
    assert bnb.polish_many(P, x, 0, table=tab)[0] == -1
    assert bnb.polish_many(P, x, 100001, table=tab)[0] == -1
    assert bnb.polish_many(P, x, 1, table=bare)[0] == -2
    rc, _x, _obj, _moves, ok = bnb.polish_many(P, x, 1, table=tab)
    assert rc == 0 and ok[0] == 1


def test_cli_flag_parses():
    """--polish on tests/golden/f1.lp.  Without a device the front end can not solve, so the value is followed up to the driver's
    refusal: without --repaired the driver refuses it and the message names the flag; values out of range are refused by the
    parser itself."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "mvolps_amd", "bin", "mvolps")
    f1 = os.path.join(root, "tests", "golden", "f1.lp")
    assert "--polish" in subprocess.run([exe, "-h"], capture_output=True, text=True).stdout
    for flags in (("--polish",), ("--polish", "50")):
        r = subprocess.run([exe, "-f", f1, *flags], capture_output=True, text=True)
        assert r.returncode != 0 and "/ --polish are not supported" in r.stderr and "Unknown parameter" not in r.stderr, (flags, r.stderr)
    for bad in ("0", "100001"):
        r = subprocess.run([exe, "-f", f1, "--repaired", "--polish", bad], capture_output=True, text=True)
        assert r.returncode != 0 and "Unknown parameter value for --polish" in r.stderr, (bad, r.stderr)
