"""CPU: the primal rounding heuristic (mvx_bnb_params.heur, DESIGN.md "Primal rounding heuristic"), driver over the ORACLE's
table.

mvx_bnb_round (the host twin of k_round) is checked bit for bit against a numpy restatement of the definition built from the
test's own model arrays; the incumbents it books are checked for feasibility and against the HiGHS optima; the serial, FIFO
window and best-bound window drivers must give one tree with it; and the refusals are pinned."""
import numpy as np
import pytest

from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import CV, DB, FR, FX, IV, LO, MAX, MIN, OPT, UP

from . import lpgen
from .test_bnb_branching import HIGHS
from .test_bnb_host import same_result


class Model:
    """The root's model as the test built it: dense rows, row / column bounds (+-inf where absent), c, c0, kinds, sense."""

    def __init__(self, A, row_b, col_b, c, c0, kinds, direction):
        self.A = np.asarray(A, dtype=float)
        self.rlo, self.rhi = lpgen.bounds_arrays(row_b)
        self.clo, self.chi = lpgen.bounds_arrays(col_b)
        self.c = np.asarray(c, dtype=float)
        self.c0 = float(c0)
        self.isint = np.array([k != CV for k in kinds])
        self.sg = -1.0 if direction == MIN else 1.0

    def load(self, api, row_b, col_b, kinds, direction):
        P = api.create()
        P.load_general(self.A, row_b, col_b, self.c, c0=self.c0, kinds=kinds, direction=direction)
        return P


def build(A, row_b, col_b, c, kinds, direction, c0=0.0):
    return Model(A, row_b, col_b, c, c0, kinds, direction), (row_b, col_b, kinds, direction)


def tol(b):
    return 1e-9 * max(1.0, abs(b))


def np_round(M, v, mode):
    """The definition of DESIGN.md "Primal rounding heuristic", one operation at a time on Python floats (IEEE double,
    every product and sum rounded, divisions correctly rounded)."""
    m, n = M.A.shape
    dlock = np.zeros(n, bool)
    ulock = np.zeros(n, bool)
    for i in range(m):
        for j in range(n):
            a = M.A[i, j]
            lo, hi = np.isfinite(M.rlo[i]), np.isfinite(M.rhi[i])
            dlock[j] |= (a > 0 and lo) or (a < 0 and hi)
            ulock[j] |= (a > 0 and hi) or (a < 0 and lo)
    x = [float(t) for t in v]
    for j in range(n):
        if not M.isint[j]:
            continue
        t = float(v[j])
        r = float(np.rint(t))
        if abs(t - r) <= 1e-9:
            xr = r
        elif not dlock[j]:
            xr = float(np.floor(t))
        elif not ulock[j]:
            xr = float(np.ceil(t))
        else:
            xr = float(np.floor(t + 0.5))
        xr = max(xr, float(np.ceil(M.clo[j])))
        xr = min(xr, float(np.floor(M.chi[j])))
        x[j] = xr

    def activity():
        out = []
        for i in range(m):
            s = 0.0
            for j in range(n):
                if M.A[i, j] != 0.0 and x[j] != 0.0:
                    s = s + float(M.A[i, j]) * x[j]
            out.append(s)
        return out

    r = activity()

    def feasible():
        if any(not (M.clo[j] <= x[j] <= M.chi[j]) for j in range(n)):
            return False
        return all(M.rlo[i] - tol(M.rlo[i]) <= r[i] <= M.rhi[i] + tol(M.rhi[i]) for i in range(m))

    ok = feasible()
    if ok and mode == 2:
        order = sorted((j for j in range(n) if M.isint[j]), key=lambda j: (-(float(v[j]) - float(np.floor(v[j]))), j))
        for j in order:
            sc = M.sg * M.c[j]
            if sc == 0.0:
                continue
            d = 1.0 if sc > 0 else -1.0
            t = (float(np.floor(M.chi[j])) - x[j]) if d > 0 else (x[j] - float(np.ceil(M.clo[j])))
            for i in range(m):
                da = d * float(M.A[i, j])
                if da > 0 and np.isfinite(M.rhi[i]):
                    t = min(t, float(np.floor(((M.rhi[i] + tol(M.rhi[i])) - r[i]) / da)))
                elif da < 0 and np.isfinite(M.rlo[i]):
                    t = min(t, float(np.floor(((r[i] - M.rlo[i]) + tol(M.rlo[i])) / -da)))
            if not t > 0 or np.isinf(t):
                continue
            step = d * t
            for i in range(m):
                if M.A[i, j] != 0.0:
                    r[i] = r[i] + step * float(M.A[i, j])
            x[j] = x[j] + step
        ok = feasible()
    s = 0.0
    for j in range(n):
        s = s + float(M.c[j]) * x[j]
    return s + M.c0, int(ok), np.array(x)


def check_twin(M, root, node, tab):
    v = node.col_prim()
    out = []
    for mode in (1, 2):
        rc, obj, found, x = bnb.round_node(node, root, mode, table=tab)
        assert rc == 0
        eo, ef, ex = np_round(M, v, mode)
        assert obj == eo or (np.isnan(obj) and np.isnan(eo)), (mode, obj, eo)
        assert found == ef, mode
        assert np.array_equal(x[1:], ex), (mode, x[1:], ex)
        out.append(found)
    return out


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    assert not t.round_many  # the host twin is what runs over the oracle
    return t


def test_twin_matches_definition_mixed_rows(orc, tab):
    """<=, >=, = and ranged rows, free rows, every column bound type, negative coefficients, continuous columns,
    minimisation and maximisation, a constant term."""
    rng = np.random.default_rng(11)
    seen_rows, seen_dir, checked, found, negative = set(), set(), 0, 0, 0
    for _ in range(120):
        A, row_b, col_b, c, d = lpgen.random_general_lp(rng, 10, 12)
        kinds = [IV if rng.random() < 0.7 else CV for _ in c]
        M, spec = build(A, row_b, col_b, c, kinds, d, c0=float(rng.integers(-3, 4)))
        root = M.load(orc, *spec)
        node = root.copy()
        node.simplex()
        if node.status != OPT:
            continue
        seen_rows |= {t for t, _, _ in row_b}
        seen_dir.add(d)
        negative += int((np.asarray(A) < 0).any())
        found += sum(check_twin(M, root, node, tab))
        checked += 1
    assert checked > 40 and found > 10
    assert {LO, UP, DB, FX, FR} <= seen_rows and seen_dir == {MIN, MAX}
    assert negative > 20  # compared cases with negative coefficients


def test_twin_matches_definition_on_children(orc, tab):
    """Nodes with tightened column bounds: the model is the root's, not the node's."""
    A, b, c, U = synth.dense_ilp(12, 24, 5, 3)
    n = len(c)
    M, spec = build(A, [(UP, 0.0, float(x)) for x in b], [(DB, 0.0, float(U))] * n, c, [IV] * n, MAX)
    root = M.load(orc, *spec)
    queue, done = [root.copy()], 0
    while queue and done < 12:
        P = queue.pop(0)
        P.simplex()
        if P.status != OPT:
            continue
        check_twin(M, root, P, tab)
        done += 1
        st, viol = bnb.print_info(P, quirks=0, table=tab)
        if viol:
            queue += list(bnb.make_children(P, viol[0], quirks=0, table=tab))
    assert done >= 8


def test_near_integral_values_and_infinite_bounds(orc, tab):
    """max x1 + x2: 3 x1 <= 6.000000000000001 gives x1 = 2.0000000000000004 (within 1e-9 of 2: rounds to 2); x2 = 9.5 has
    no upper bound, only the >= row x1 - x2 >= -7.5 holds it (an up-lock, no down-lock: rounded down).  Both rows then
    leave the fill no whole step, and the columns' infinite upper bounds never limit it."""
    A = np.array([[3.0, 0.0], [1.0, -1.0]])
    row_b = [(UP, 0.0, 6.000000000000001), (LO, -7.5, 0.0)]
    col_b = [(LO, 0.0, 0.0), (LO, 0.0, 0.0)]
    M, spec = build(A, row_b, col_b, [1.0, 1.0], [IV, IV], MAX)
    root = M.load(orc, *spec)
    node = root.copy()
    node.simplex()
    assert node.status == OPT
    v = node.col_prim()
    assert v[0] != 2.0 and abs(v[0] - 2.0) < 1e-9
    assert check_twin(M, root, node, tab) == [1, 1]
    rc, obj, found, x = bnb.round_node(node, root, 2, table=tab)
    assert x[1] == 2.0 and x[2] == 9.0 and obj == 11.0


def incumbent_ok(orc, case, r):
    """The incumbent is integral, feasible in the original model and no better than the HiGHS optimum.  A heuristic point
    meets the heuristic's own tests exactly; an integral node LP's vertex holds within the LP tolerances."""
    P = lpgen.load_case(orc, case)
    m, n = P.m, P.n
    x = np.array(r["x"])
    exact = r["incumbent_heur"] == 1
    if exact:
        assert np.array_equal(x, np.round(x))
    else:
        assert np.abs(x - np.round(x)).max() <= 1e-9
    A = np.zeros((m, n))
    for i in range(1, m + 1):
        ind, val = P.get_mat_row(i)
        A[i - 1, ind - 1] = val
    act = A @ x
    for i in range(1, m + 1):
        lo, hi = orc.get_row_lb(P.h, i), orc.get_row_ub(P.h, i)
        e = 1e-9 if exact else 1e-7
        assert lo - e * max(1, abs(lo)) <= act[i - 1] <= hi + e * max(1, abs(hi))
    for j in range(1, n + 1):
        e = 0.0 if exact else 1e-9
        assert orc.get_col_lb(P.h, j) - e <= x[j - 1] <= orc.get_col_ub(P.h, j) + e
    c = np.array([orc.get_obj_coef(P.h, j) for j in range(1, n + 1)])
    obj = float(c @ x) + orc.get_obj_coef(P.h, 0)
    assert abs(obj - r["best_lower"]) <= 1e-9 * (1 + abs(obj))
    sg = -1.0 if orc.get_obj_dir(P.h) == MIN else 1.0
    assert sg * r["best_lower"] <= sg * HIGHS[case] + 1e-6 * (1 + abs(HIGHS[case]))


@pytest.mark.parametrize("heur", [1, 2])
@pytest.mark.parametrize("case", list(HIGHS), ids=str)
def test_incumbents_are_feasible_and_trees_close_on_the_optimum(orc, tab, case, heur):
    r = bnb.branch_and_bound(lpgen.load_case(orc, case), quirks=0, table=tab, heur=heur)
    assert r["rc"] == 0 and r["hit_limit"] == 0 and r["has_incumbent"]
    assert r["heur_calls"] > 0 and r["heur_found"] <= r["heur_calls"] and r["heur_improved"] <= r["heur_found"]
    incumbent_ok(orc, case, r)
    assert abs(r["best_lower"] - HIGHS[case]) <= 1e-6 * (1 + abs(HIGHS[case]))
    # partial trees: whatever incumbent they hold is feasible too
    for mx in (5, 40):
        p = bnb.branch_and_bound(lpgen.load_case(orc, case), quirks=0, table=tab, heur=heur, max_nodes=mx)
        if p["has_incumbent"]:
            incumbent_ok(orc, case, p)


def test_heuristic_finds_incumbents():
    """Measured over the oracle's table (FIFO, repaired mode): the heuristic's points are found and some become the
    incumbent; heur 0 reports nothing."""
    from oracle import oracle

    orc = oracle.api()
    tab = bnb.table_from(orc)
    total = {1: 0, 2: 0}
    for case in HIGHS:
        r0 = bnb.branch_and_bound(lpgen.load_case(orc, case), quirks=0, table=tab)
        assert (r0["heur_calls"], r0["heur_found"], r0["heur_improved"], r0["incumbent_heur"]) == (0, 0, 0, 0)
        for h in (1, 2):
            total[h] += bnb.branch_and_bound(lpgen.load_case(orc, case), quirks=0, table=tab, heur=h)["heur_improved"]
    assert total[1] > 0 and total[2] > 0


def same_heur(a, b):
    assert (a["heur_calls"], a["heur_found"], a["heur_improved"], a["incumbent_heur"]) == (
        b["heur_calls"], b["heur_found"], b["heur_improved"], b["incumbent_heur"])


@pytest.mark.parametrize("cut_strat", [0, 1])
@pytest.mark.parametrize("var_strat", [0, 2, 3])
@pytest.mark.parametrize("heur", [1, 2])
def test_windows_equal_serial(orc, tab, heur, var_strat, cut_strat):
    A, b, c, U = synth.dense_ilp(10, 20, 4, 3)
    kw = dict(var_strat=var_strat, quirks=0, cut_strat=cut_strat, max_nodes=400, table=tab, heur=heur)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), window=1, **kw)
    assert ref["rc"] == 0 and ref["count"] > 50 and ref["heur_calls"] > 0 and ref["heur_improved"] > 0
    for w in (2, 8, 64):
        got = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), window=w, **kw)
        assert got["rc"] == 0
        same_result(got, ref)
        same_heur(got, ref)
    if var_strat >= 3:
        return  # var_strat 3 / 4 are not in the best-bound window
    bref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), node_strat=1, best_window=0, **kw)
    assert bref["rc"] == 0 and bref["heur_calls"] > 0
    for w in (2, 8, 64):
        got = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), node_strat=1, best_window=w, **kw)
        assert got["rc"] == 0 and got["rounds"] > 0
        same_result(got, bref)
        same_heur(got, bref)


@pytest.mark.parametrize("case", [(10, 20, 4, 3), (16, 32, 5, 2), ("setcover", 40, 60, 3), ("setcover", 30, 50, 4)], ids=str)
def test_monotone_node_count(orc, tab, case):
    """FIFO order: node LPs and branching choices depend on the path only, and an incumbent found earlier prunes at least
    what a later one would -- a closed tree with the heuristic has no more nodes and the same optimum."""
    r0 = bnb.branch_and_bound(lpgen.load_case(orc, case), quirks=0, table=tab)
    assert r0["rc"] == 0 and r0["hit_limit"] == 0
    for h in (1, 2):
        r = bnb.branch_and_bound(lpgen.load_case(orc, case), quirks=0, table=tab, heur=h)
        assert r["rc"] == 0 and r["hit_limit"] == 0
        assert r["count"] <= r0["count"], (h, r["count"], r0["count"])
        assert abs(r["best_lower"] - r0["best_lower"]) <= 1e-6 * (1 + abs(r0["best_lower"]))


def test_refusals(orc, tab):
    from mvolps_amd import dist_bnb, dist_native

    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    for kw in (dict(heur=3, quirks=0), dict(heur=-1, quirks=0), dict(heur=1, quirks=1), dict(heur=2), dict(heur=2, node_strat=1, best_window=8)):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, **kw)
        assert r["rc"] == -1 and r["n_nodes"] == 0 and r["count"] == 0, kw
    P = lpgen.load_ilp(orc, A, b, c, U)
    with pytest.raises(ValueError):
        dist_native.branch_and_bound(P, table=tab, heur=1, quirks=0)
    with pytest.raises(ValueError):
        dist_bnb.branch_and_bound(None, P, heur=2, quirks=0)
    # neither round_many nor the host twin's accessors: an error, not a run without the heuristic
    bare = bnb.table_from(orc)
    bare.get_mat_row = None
    for kw in (dict(window=1), dict(window=64), dict(node_strat=1, best_window=8)):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bare, heur=1, quirks=0, **kw)
        assert r["rc"] == -2 and r["count"] == 0, kw
    # mvx_bnb_round's own codes
    root = lpgen.load_ilp(orc, A, b, c, U)
    node = root.copy()
    node.simplex()
    assert bnb.round_node(node, root, 0, table=tab)[0] == -1
    assert bnb.round_node(node, root, 3, table=tab)[0] == -1
    assert bnb.round_node(root, root, 1, table=tab)[0] == -3  # never solved
    assert bnb.round_node(node, root, 1, table=bare)[0] == -2
    assert bnb.round_node(node, root, 2, table=tab)[0] == 0
