"""CPU: clique cuts in the root cut rounds (mvx_bnb_params.cut_families, DESIGN.md "Clique cuts (cut_families)"), driver over the
ORACLE's table, whose table has no conflict_graph entry, so the host twin mvx_bnb_conflict_graph runs.

The twin and the separation are checked with == against plain-Python restatements of the definition; on enumerated all-integer
models no feasible point violates an edge of the graph or a row the loop appends; every fixture instance closes on its pin with
both families; on the binary dense_ilp cases the root bound falls to the optimum or near it and the trees shrink to the pinned
counts; windows give the serial tree; cut_families 0 / 1 is the parent's loop; the refusals return their codes."""
import itertools
import math

import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import CV, DB, FX, IV, LO, MAX, MIN, OPT, UP

from . import certify as cf
from . import lpgen
from .test_bnb_cutloop import rows_behind
from .test_bnb_general import INSTANCES, check_pin, failures, instance, run
from .test_bnb_host import same_result
from .test_bnb_prop import TIGHT, set_bounds, sparse_rows, tol

COUNTERS = bnb.CUTLOOP_COUNTERS + bnb.CLIQUE_COUNTERS + ("cutloop_bound0", "cutloop_bound")
# the binary dense_ilp cases (U = 1, tight capacity) and their node counts (n_nodes) under cut_rounds = 5 with cut_families 2 / 3;
# without the loop they have 195, 401 and 545 nodes
BINARY = {TIGHT: (1, 1), (24, 48, 5, 1, 0.06): (21, 7), (32, 64, 7, 1, 0.045): (11, 11)}


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    assert not t.conflict_graph and not t.gmi_cuts and not t.cut_scores  # the host side of the definition runs over the oracle
    return t


# ------------------------------------------------------------------------------------------------ the graph twin


def restate_graph(rows, rlo, rhi, isint, l, u, seen=None):
    """Section 1 of the definition, one operation at a time on Python floats.  rows: per row the (j, a_ij) in ascending j
    (0-based j); l / u the handle's column bounds (+-inf when absent).  Returns the boolean (n + 1) x (n + 1) matrix."""
    n = len(l)
    note = seen.add if seen is not None else (lambda s: None)
    inB = [bool(isint[j]) and l[j] == 0.0 and u[j] == 1.0 for j in range(n)]
    adj = np.zeros((n + 1, n + 1), dtype=bool)
    for i, row in enumerate(rows):
        lmin = lmax = 0.0
        kmin = kmax = 0
        for j, a in row:
            bmin, bmax = (l[j], u[j]) if a > 0 else (u[j], l[j])
            if math.isinf(bmin):
                kmin += 1
            else:
                lmin = lmin + a * bmin
            if math.isinf(bmax):
                kmax += 1
            else:
                lmax = lmax + a * bmax
        for (j, aj), (k, ak) in itertools.combinations(row, 2):  # j < k
            if not (inB[j] and inB[k]):
                continue
            if aj > 0 and ak > 0 and math.isfinite(rhi[i]):
                if kmin != 0:
                    note("silenced by an infinite term")
                elif (lmin + aj) + ak > rhi[i] + tol(rhi[i]):
                    note("upper side")
                    adj[j + 1, k + 1] = adj[k + 1, j + 1] = True
            if aj < 0 and ak < 0 and math.isfinite(rlo[i]):
                if kmax != 0:
                    note("silenced by an infinite term")
                elif (lmax + aj) + ak < rlo[i] - tol(rlo[i]):
                    note("lower side")
                    adj[j + 1, k + 1] = adj[k + 1, j + 1] = True
    return adj


def mixed_models(rng, count):
    """lpgen.random_general_lp(rng, 10, 12) with about 60 % of the columns made integer with bounds [0, 1], the rest as drawn
    (70 % of them integer), each followed by clones with one or two binaries fixed to 1 or 0.  Yields (A, row_b, col_b, kinds,
    c, direction, [(column 0-based, value), ...] per variant)."""
    for _ in range(count):
        A, row_b, col_b, c, d = lpgen.random_general_lp(rng, 10, 12)
        n = len(c)
        kinds = []
        for j in range(n):
            if rng.random() < 0.6:
                col_b[j] = (DB, 0.0, 1.0)
                kinds.append(IV)
            else:
                kinds.append(IV if rng.random() < 0.7 else CV)
        binaries = [j for j in range(n) if col_b[j] == (DB, 0.0, 1.0) and kinds[j] == IV]
        variants = [[]]
        for k in (1, 2):
            if len(binaries) >= k:
                variants.append([(int(j), float(rng.integers(0, 2))) for j in rng.choice(binaries, size=k, replace=False)])
        yield A, row_b, col_b, kinds, c, d, variants


def load_variants(api, A, row_b, col_b, kinds, c, d, variants):
    """The root and its clones with the variants' columns fixed: [(handle, l, u)]."""
    root = api.create()
    root.load_general(A, row_b, col_b, c, kinds=kinds, direction=d)
    clo, chi = (list(map(float, v)) for v in lpgen.bounds_arrays(col_b))
    out = []
    for fixes in variants:
        P, l, u = (root.copy() if fixes else root), list(clo), list(chi)
        for j, v in fixes:
            l[j] = u[j] = v
            set_bounds(api, P, j + 1, v, v)
        out.append((P, l, u))
    return out


def test_graph_twin_matches_the_restatement(orc, tab):
    rng = np.random.default_rng(20261019)
    seen, models, handles, edges_total, empty = set(), 0, 0, 0, 0
    for A, row_b, col_b, kinds, c, d, variants in mixed_models(rng, 1800):
        rows = sparse_rows(A)
        rlo, rhi = (list(map(float, v)) for v in lpgen.bounds_arrays(row_b))
        isint = [k != CV for k in kinds]
        models += 1
        for P, l, u in load_variants(orc, A, row_b, col_b, kinds, c, d, variants):
            want = restate_graph(rows, rlo, rhi, isint, l, u, seen)
            rc, got, edges = bnb.conflict_graph(P, table=tab)
            assert rc == 0 and np.array_equal(got, want), (models, np.argwhere(got != want)[:4])
            assert edges == int(want.sum()) // 2 and not got[0].any() and not got[:, 0].any() and not got.diagonal().any()
            assert np.array_equal(got, got.T)
            edges_total += edges
            empty += edges == 0
            handles += 1
    assert models == 1800 and handles > 4000, (models, handles)
    assert seen >= {"upper side", "lower side", "silenced by an infinite term"}, seen
    assert empty > 0 and edges_total > 1000, (empty, edges_total)


def test_graph_twin_reads_the_handle_not_a_solve(orc, tab):
    """The handle need not be solved and is not changed; solving it changes nothing; columns outside B have empty rows."""
    A, b, c, U = synth.dense_ilp(*TIGHT)
    P = lpgen.load_ilp(orc, A, b, c, U)
    rc, adj, edges = bnb.conflict_graph(P, table=tab)
    assert rc == 0 and edges == 190 and P.status != OPT and P.m == 10
    P.simplex()
    assert bnb.conflict_graph(P, table=tab)[2] == 190
    set_bounds(orc, P, 3, 0.0, 2.0)  # no longer binary: its row empties, the others keep their edges among themselves
    rc, adj2, edges2 = bnb.conflict_graph(P, table=tab)
    assert rc == 0 and not adj2[3].any() and not adj2[:, 3].any() and edges2 == edges - int(adj[3].sum())
    bare = bnb.table_from(orc)
    bare.get_mat_row = None
    assert bnb.conflict_graph(P, table=bare)[0] == -2


# ------------------------------------------------------------------------------------------------ the separation


def restate_cliques(adj, x, max_cuts, seen=None):
    """The separation of the definition on Python floats: the kept cliques, each as its ascending columns."""
    note = seen.add if seen is not None else (lambda s: None)
    n = adj.shape[0] - 1
    order = sorted((j for j in range(1, n + 1) if adj[j].any()), key=lambda j: (-x[j], j))
    if any(x[a] == x[b] for a, b in zip(order, order[1:])):
        note("tie in x")
    kept = []
    for seed in order:
        if len(kept) >= max_cuts:
            note("max_cuts stop")
            break
        if not x[seed] > 1e-6:
            continue
        Q, mask = [seed], adj[seed].copy()
        for col in order:
            if mask[col]:
                Q.append(col)
                mask &= adj[col]
        Q.sort()
        s = 0.0
        for j in Q:
            s = s + float(x[j])
        if not s - 1.0 > 1e-6:
            continue
        if Q in kept:
            note("duplicate from two seeds")
            continue
        if any(x[j] == 0.0 for j in Q):
            note("zero-valued column lifted in")
        kept.append(Q)
    return kept


def random_graph(rng, n):
    """A few planted cliques plus noise: symmetric, no self loops, row 0 empty."""
    adj = np.zeros((n + 1, n + 1), dtype=bool)
    for _ in range(int(rng.integers(1, 5))):
        q = rng.choice(np.arange(1, n + 1), size=int(rng.integers(2, max(3, n // 2 + 1))), replace=False)
        adj[np.ix_(q, q)] = True
    noise = rng.random((n + 1, n + 1)) < 0.1
    adj |= noise | noise.T
    adj[0] = adj[:, 0] = False
    np.fill_diagonal(adj, False)
    return adj


def test_clique_cuts_match_the_restatement():
    rng = np.random.default_rng(7)
    seen, rows = set(), 0
    for trial in range(300):
        n = int(rng.integers(2, 90)) if trial % 10 else int(rng.integers(120, 140))  # one, two and three words a row
        adj = random_graph(rng, n)
        x = np.round(rng.random(n + 1) * 4) / 4 * (rng.random(n + 1) < 0.7)  # ties and zeros
        if trial % 3 == 0:
            x = x * rng.random(n + 1)
        x[0] = 0.0
        for max_cuts in (1 << 20, 2, 0):
            want = restate_cliques(adj, x, max_cuts, seen)
            rc, vals, rhs = bnb.clique_cuts(adj, x, max_cuts)
            assert rc == 0 and len(vals) == len(want) <= max_cuts, (trial, max_cuts, len(vals), len(want))
            for t, Q in enumerate(want):
                row = np.zeros(n + 1)
                row[Q] = -1.0
                assert np.array_equal(vals[t], row) and rhs[t] == -1.0, (trial, t)
                assert all(adj[a, b] for a, b in itertools.combinations(Q, 2))  # a clique
                assert not any(adj[j, Q].all() for j in range(1, n + 1) if j not in Q and adj[j].any())  # maximal
                assert vals[t] @ x < rhs[t] - 1e-6  # violated
            rows += len(want)
    assert rows > 300, rows
    assert seen >= {"tie in x", "max_cuts stop", "duplicate from two seeds", "zero-valued column lifted in"}, seen


def test_clique_cuts_hand_cases():
    adj = np.zeros((6, 6), dtype=bool)
    tri = [1, 2, 3]
    adj[np.ix_(tri, tri)] = True
    adj[4, 5] = adj[5, 4] = True
    np.fill_diagonal(adj, False)
    # the triangle is violated and found once although all three are seeds; the pair {4, 5} sums to 1: not violated
    rc, vals, rhs = bnb.clique_cuts(adj, [0, 0.5, 0.5, 0.5, 0.5, 0.5], 8)
    assert rc == 0 and vals.tolist() == [[0, -1, -1, -1, 0, 0]] and rhs.tolist() == [-1.0]
    # column 3 at zero is lifted into the violated pair's clique; a seed needs x > 1e-6
    rc, vals, rhs = bnb.clique_cuts(adj, [0, 0.75, 0.75, 0.0, 0.0, 0.0], 8)
    assert rc == 0 and vals.tolist() == [[0, -1, -1, -1, 0, 0]]
    assert bnb.clique_cuts(adj, [0, 0.5, 0.5, 0.0, 1.0, 0.0], 8)[1].shape[0] == 0  # s - 1 must exceed 1e-6
    assert bnb.clique_cuts(adj, [0, 0.5, 0.5, 0.5, 0.5, 0.5], 0)[1].shape[0] == 0
    assert bnb.clique_cuts(adj, [0, 0.5, 0.5, 0.5, 0.5, 0.5], -1)[0] == -1


# ------------------------------------------------------------------------------------------------ validity by enumeration


def integer_model(rng):
    """An all-integer model with at most 12 columns, binaries plus up to three columns in boxes of width <= 3, rows bounded
    around the activity of a point of the box (so the model is feasible), coefficients of both signs."""
    n = int(rng.integers(4, 13))
    m = int(rng.integers(2, 9))
    wide = set(int(j) for j in rng.choice(n, size=int(rng.integers(0, 4)), replace=False))
    col_b = []
    for j in range(n):
        if j in wide:
            lo = float(rng.integers(-2, 3))
            w = float(rng.integers(1, 4))
            col_b.append((DB, lo, lo + w))
        else:
            col_b.append((DB, 0.0, 1.0))
    A = np.round(rng.normal(size=(m, n)) * 3)
    A[rng.random((m, n)) < 0.3] = 0
    if rng.random() < 0.5:
        A = np.abs(A)  # packing-like rows give the denser graphs
    x0 = np.array([float(rng.integers(int(l), int(u) + 1)) for _t, l, u in col_b])
    act = A @ x0
    row_b = []
    for i in range(m):
        t = int(rng.choice([UP, LO, DB, FX], p=[0.5, 0.25, 0.2, 0.05]))
        l, u = act[i] - rng.integers(0, 3), act[i] + rng.integers(0, 3)
        if t == FX:
            l = u = act[i]
        if t == DB and l == u:
            u = l + 1
        row_b.append((t, float(l), float(u)))
    c = np.round(rng.normal(size=n) * 5)
    return dict(A=A, row_b=row_b, col_b=col_b, c=c, c0=0.0, kinds=[IV] * n, direction=int(rng.choice([MIN, MAX])))


def feasible_points(inst):
    """Every integer point of the box that satisfies the rows (exact: the data are small integers)."""
    A, rlo, rhi, clo, chi, _c, _c0, _isint, _mx = lpgen.milp_arrays(inst)
    grids = np.meshgrid(*[np.arange(l, u + 1) for l, u in zip(clo, chi)], indexing="ij")
    pts = np.stack([g.ravel() for g in grids], axis=1)
    act = pts @ A.T
    return pts[np.all(act >= rlo, axis=1) & np.all(act <= rhi, axis=1)]


def test_edges_and_loop_rows_keep_every_feasible_point(orc, tab):
    rng = np.random.default_rng(4242)
    with_edge = with_clique_row = rows_checked = 0
    bad = []
    for index in range(300):
        inst = integer_model(rng)
        pts = feasible_points(inst)
        assert len(pts) >= 1
        rc, adj, edges = bnb.conflict_graph(lpgen.load_milp(orc, inst), table=tab)
        assert rc == 0
        with_edge += edges > 0
        for j, k in np.argwhere(np.triu(adj)):
            if np.any(pts[:, j - 1] + pts[:, k - 1] > 1):
                bad.append("model %d: a feasible point has x_%d = x_%d = 1" % (index, j, k))
        appended = 0
        for fam in (2, 3):
            P = lpgen.load_milp(orc, inst)
            m0 = P.m
            rc, out = bnb.cut_loop(P, rounds=5, table=tab, families=fam)
            assert rc == 0 and out["cutloop_conflicts"] == edges, (index, fam, rc)
            rows = rows_behind(orc, P, m0)
            assert len(rows) == out["cutloop_rows"] >= out["cutloop_clique_rows"]
            assert fam == 3 or out["cutloop_rows"] == out["cutloop_clique_rows"]
            cliques = 0
            for coef, rhs in rows:
                rows_checked += 1
                is_clique = rhs == -1.0 and set(coef.tolist()) <= {0.0, -1.0}
                cliques += is_clique
                off = (pts @ coef < rhs) if is_clique else np.isin(np.arange(len(pts)), cf.cut_cuts_off(coef, rhs, pts))
                if off.any():
                    bad.append("model %d, families %d: a row excludes the feasible point %s" % (index, fam, pts[off][0].tolist()))
            assert cliques >= out["cutloop_clique_rows"]
            appended += out["cutloop_clique_rows"]
        with_clique_row += appended > 0
    assert not bad, "\n".join(bad[:20])
    assert with_edge >= 100 and with_clique_row >= 50 and rows_checked > 200, (with_edge, with_clique_row, rows_checked)


# ------------------------------------------------------------------------------------------------ whole trees


@pytest.mark.parametrize("window", [1, 64])
def test_fixture_trees_close_on_the_enumerated_optimum(orc, tab, window):
    def one(rec):
        inst = instance(rec)
        check_pin(rec, inst, run(orc, rec, inst, table=tab, cut_rounds=5, cut_families=3, window=window))

    bad = failures(INSTANCES, one)
    assert not bad, "\n".join(bad)


def dense(orc, tab, case, **kw):
    A, b, c, U = synth.dense_ilp(*case)
    return bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), quirks=0, table=tab, **kw)


@pytest.mark.parametrize("case", list(BINARY), ids=lambda c: "%dx%d_cap%g" % (c[0], c[1], c[4]))
def test_binary_dense_trees_shrink(orc, tab, case):
    off = dense(orc, tab, case)
    assert off["rc"] == 0 and off["has_incumbent"] and off["cutloop_conflicts"] == 0
    nodes = []
    for fam in (2, 3):
        on = dense(orc, tab, case, cut_rounds=5, cut_families=fam)
        assert on["rc"] == 0 and on["hit_limit"] == 0 and on["has_incumbent"]
        assert abs(on["best_lower"] - off["best_lower"]) <= 1e-6 * (1 + abs(off["best_lower"]))
        assert on["cutloop_bound"] >= off["best_lower"] - 1e-6  # a maximisation: the root LP stays a bound
        assert on["cutloop_bound"] < on["cutloop_bound0"]
        assert on["n_nodes"] < off["n_nodes"] and on["cutloop_clique_rows"] >= 1 and on["cutloop_conflicts"] > 0
        nodes.append(on["n_nodes"])
    assert tuple(nodes) == BINARY[case], (nodes, off["n_nodes"])


def test_windows_give_the_serial_tree(orc, tab):
    def same(a, b):
        same_result(a, b)
        for k in COUNTERS:
            assert a[k] == b[k], k

    for case in BINARY:
        for fam in (2, 3):
            ref = dense(orc, tab, case, cut_rounds=5, cut_families=fam, window=1)
            for w in (8, 64):
                same(dense(orc, tab, case, cut_rounds=5, cut_families=fam, window=w), ref)
            ref = dense(orc, tab, case, cut_rounds=5, cut_families=fam, node_strat=1, window=1)
            same(dense(orc, tab, case, cut_rounds=5, cut_families=fam, node_strat=1, best_window=8), ref)

    def one(rec):
        inst = instance(rec)
        ref = run(orc, rec, inst, table=tab, window=1, cut_rounds=5, cut_families=3)
        for w in (8, 64):
            same(run(orc, rec, inst, table=tab, window=w, cut_rounds=5, cut_families=3), ref)
        ref = run(orc, rec, inst, table=tab, node_strat=1, window=1, cut_rounds=5, cut_families=3)
        same(run(orc, rec, inst, table=tab, node_strat=1, best_window=8, cut_rounds=5, cut_families=3), ref)

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)


def test_families_0_and_1_are_the_parents_loop(orc, tab):
    def same(got, ref):
        same_result(got, ref)
        for k in COUNTERS:
            assert got[k] == ref[k], k
        assert all(got[k] == 0 for k in bnb.CLIQUE_COUNTERS)

    def one(rec):
        inst = instance(rec)
        for kw in (dict(window=1), dict(window=64, heur=2, rc_fix=1, prop=8)):
            ref = run(orc, rec, inst, table=tab, cut_rounds=5, **kw)
            for fam in (0, 1):
                same(run(orc, rec, inst, table=tab, cut_rounds=5, cut_families=fam, **kw), ref)
            # with the loop off the field is not read
            assert run(orc, rec, inst, table=tab, cut_rounds=0, cut_families=9, **kw) == run(orc, rec, inst, table=tab, **kw)

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)
    for case in list(BINARY) + [(8, 16, 3, 2)]:
        ref = dense(orc, tab, case, cut_rounds=5)
        for fam in (0, 1):
            same(dense(orc, tab, case, cut_rounds=5, cut_families=fam), ref)
        assert dense(orc, tab, case, cut_rounds=0, cut_families=9) == dense(orc, tab, case)
        # the loop's own entries: mvx_bnb_cut_loop is mvx_bnb_cut_loop_families with families = 1
        A, b, c, U = synth.dense_ilp(*case)
        old = bnb.cut_loop(lpgen.load_ilp(orc, A, b, c, U), rounds=5, table=tab)
        for fam in (0, 1):
            rc, new = bnb.cut_loop(lpgen.load_ilp(orc, A, b, c, U), rounds=5, table=tab, families=fam)
            assert rc == old[0] == 0 and all(new[k] == 0 for k in bnb.CLIQUE_COUNTERS)
            assert {k: v for k, v in new.items() if k not in bnb.CLIQUE_COUNTERS} == old[1]


def test_refusals(orc, tab):
    A, b, c, U = synth.dense_ilp(*TIGHT)
    for fam in (-1, 4):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0, cut_rounds=1, cut_families=fam)
        assert r["rc"] == -1 and r["n_nodes"] == 0 and r["count"] == 0, fam
        assert bnb.cut_loop(lpgen.load_ilp(orc, A, b, c, U), rounds=1, table=tab, families=fam)[0] == -1
    for fam in (0, 1, 2, 3):
        assert bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0, cut_rounds=1, cut_families=fam)["rc"] == 0
    # a graph that cannot be computed: an error with the unsolved root as the tree, not a run without the family
    bare = bnb.table_from(orc)
    bare.get_mat_row = None
    for fam in (2, 3):
        assert bnb.cut_loop(lpgen.load_ilp(orc, A, b, c, U), table=bare, families=fam)[0] == -2
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bare, quirks=0, cut_rounds=5, cut_families=fam)
        assert r["rc"] == -2 and r["n_nodes"] == 1 and r["count"] == 0 and not r["has_incumbent"], fam


def test_the_callers_handle_is_left_as_it_was(orc, tab):
    A, b, c, U = synth.dense_ilp(24, 48, 5, 1, 0.06)
    P = lpgen.load_ilp(orc, A, b, c, U)
    m0 = P.m
    before = [P.get_mat_row(i) for i in range(1, m0 + 1)]
    r = bnb.branch_and_bound(P, quirks=0, table=tab, cut_rounds=5, cut_families=3)
    assert r["rc"] == 0 and r["cutloop_clique_rows"] >= 1
    assert P.m == m0 and orc.get_num_rows(P.h) == m0 and P.status != OPT
    for i, (ind, val) in enumerate(before, start=1):
        got = P.get_mat_row(i)
        assert np.array_equal(got[0], ind) and np.array_equal(got[1], val)
    assert all(orc.get_col_lb(P.h, j) == 0.0 and orc.get_col_ub(P.h, j) == 1.0 for j in range(1, P.n + 1))


def test_cli_flag_parses():
    """--cut-families on tests/golden/f1.lp.  Without a device the front end can not solve, so the value is followed up to the
    driver's refusal (cut rounds need --repaired); values out of range are refused by the parser itself."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "mvolps_amd", "bin", "mvolps")
    f1 = os.path.join(root, "tests", "golden", "f1.lp")
    assert "--cut-families" in subprocess.run([exe, "-h"], capture_output=True, text=True).stdout
    r = subprocess.run([exe, "-f", f1, "--cut-rounds", "--cut-families", "3"], capture_output=True, text=True)
    assert r.returncode != 0 and "/ --cut-rounds are not supported" in r.stderr and "Unknown parameter" not in r.stderr, r.stderr
    for bad in ("0", "4", "x"):
        r = subprocess.run([exe, "-f", f1, "--repaired", "--cut-rounds", "--cut-families", bad], capture_output=True, text=True)
        assert r.returncode != 0 and "Unknown parameter value for --cut-families" in r.stderr, (bad, r.stderr)
