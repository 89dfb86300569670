"""GPU: the Farkas proof on the device (k_farkas_rows / k_farkas_pick / k_farkas_vars / k_farkas_cols / k_farkas_fin through
mvx_farkas and mvx_farkas_many) against the host twin through the engine's own table (mvx_bnb_farkas), every bit of val, ind and
y, on the shapes where the kernels can go wrong: rows and columns either side of the 64 chains of a wave and beyond two of them,
one row, one column, both directions, free, fixed and upper-bounded columns, a verdict the dual simplex reaches from a warm start
and one the primal phase 1 reaches from a cold one; windows of handles with feasible ones mixed in and cut rows; the call's
purity; a tree; the command line."""
import os
import subprocess

import numpy as np
import pytest

from mvolps_amd import bnb, synth, treedigest
from mvolps_amd.capi import DB, FR, FX, LO, MAX, MIN, NOFEAS, OPT, UNBND, UNDEF, UP

from . import lpgen
from .test_farkas import REL, cone, exact_proof, py_farkas, py_ray, same_bits, view
from .test_gpu_purge import state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 63, 64, 65, 130]  # the chain and wave boundaries of the row pass, the column pass and the final interval


def device_vs_twin(P):
    rc, val, ind, y = bnb.farkas(P)
    trc, tval, tind, ty = bnb.farkas(P, table=None)
    assert rc == trc == 0, (rc, trc)
    assert same_bits(val, tval) and np.array_equal(ind, tind), (val, tval, ind, tind)
    assert same_bits(y, ty), np.argwhere(y != ty)[:4]
    assert y[0] == 0.0
    prc, pval, pind, py = P.farkas()  # the handle's own method is the same call
    assert prc == 0 and same_bits(pval, val) and np.array_equal(pind, ind) and same_bits(py, y)
    nrc, nval, nind, ny = bnb.farkas(P, weights=False)  # without the weights
    assert nrc == 0 and ny is None and same_bits(nval, val) and np.array_equal(nind, ind)
    return val, ind, y


def kind_of(j):
    """Column j's bound type: LO and DB columns carry the rows' capacity, FX, UP and FR columns sit among them."""
    return (LO, FX, UP, FR, DB)[j % 5]


def mixed_model(api, m, n, direction, seed, cold=False):
    """max c x (or min -c x) over A x <= b, A ~ U[0, 1), with LO [0, inf), FX {0.5}, UP (-inf, 2], FR and DB [0, 4] columns.  Row 1
    has coefficients on the LO and DB columns only, so its activity is bounded below by 0 and it caps every column the objective
    rewards: the UP and FR columns cost nothing, which keeps the LP bounded.  cold: the LP is infeasible as it is
    loaded -- with m >= 2 the last row repeats row 1 as >= b_1 + 2; with one row that row asks for an activity of at least 1 from
    columns capped at 0.5 / n."""
    A, b, c = synth.dense_lp(m, n, seed)
    A, c = A.copy(), c.copy()
    kinds = [kind_of(j) for j in range(n)]
    for j, t in enumerate(kinds):
        if t in (FX, UP, FR):
            A[0, j] = 0.0
        if t in (UP, FR):
            c[j] = 0.0
    cap = 0.5 / n
    col_b = [{LO: (LO, 0.0, 0.0), FX: (FX, 0.5, 0.5), UP: (UP, 0.0, 2.0), FR: (FR, 0.0, 0.0), DB: (DB, 0.0, 4.0)}[t] for t in kinds]
    row_b = [(UP, 0.0, float(bi)) for bi in b]
    if cold and m >= 2:
        A[m - 1] = A[0]
        row_b[m - 1] = (LO, float(b[0]) + 2.0, 0.0)
    elif cold:
        col_b = [(DB, 0.0, cap) if t in (LO, DB) else cb for t, cb in zip(kinds, col_b)]
        row_b[0] = (LO, 1.0, 0.0)
    P = api.create()
    P.load_general(A, row_b, col_b, c if direction == MAX else -c, direction=direction)
    return P, A, b


def warm_nofeas(api, m, n, direction, seed):
    """The solved model, then a clone whose first column is pushed past row 1's capacity: the dual simplex ends MVX_NOFEAS."""
    P, A, b = mixed_model(api, m, n, direction, seed)
    P.simplex()
    assert P.status == OPT, (m, n, P.status)
    ch = P.copy()
    ch.api.set_col_bnds(ch.h, 1, LO, (float(b[0]) + 1.0) / float(A[0, 0]), 0.0)
    ch.simplex()
    return P, ch


def cold_nofeas(api, m, n, direction, seed):
    P, _, _ = mixed_model(api, m, n, direction, seed, cold=True)
    P.simplex()
    return P


@pytest.mark.parametrize("m", SIZES)
def test_device_matches_twin(gpu, m):
    for n in SIZES:
        for direction in (MAX, MIN):
            seed = 20261021 + 7 * n + 31 * m + direction
            root, warm = warm_nofeas(gpu, m, n, direction, seed)
            cold = cold_nofeas(gpu, m, n, direction, seed)
            for P, how in ((warm, "warm"), (cold, "cold")):
                assert P.status == NOFEAS, (how, m, n, direction, P.status)
                val, ind, y = device_vs_twin(P)
                assert ind[0] == 2 and val[0] > REL and val[1] > REL, (how, m, n, direction, val, ind)
            val, ind, y = device_vs_twin(root)  # a solved, feasible LP has no proof
            assert not val.any() and not ind.any() and not y.any(), (m, n, direction)
            if warm.it_cnt > root.it_cnt:
                assert warm.it_cnt > 0  # the verdict came out of pivots on the warm tableau
    # the non-basic variables of such an end state include fixed, upper-bounded and free columns
    root, warm = warm_nofeas(gpu, 65, 130, MAX, 5)
    _, nb, flag = warm.basis()
    kinds = {kind_of(int(k) - warm.m - 1) for k in nb[1:] if k > warm.m}
    assert {FX, UP} <= kinds, kinds
    cold = cold_nofeas(gpu, 65, 130, MIN, 5)
    _, nb, flag = cold.basis()
    assert {FX, UP, FR} <= {kind_of(int(k) - cold.m - 1) for k in nb[1:] if k > cold.m}


def test_restatement_and_exact_proof_on_the_engine(gpu):
    """The independent restatement and the rational check once on the engine's own handles (the CPU file runs them over the oracle's)."""
    for P in (warm_nofeas(gpu, 65, 63, MIN, 9)[1], cold_nofeas(gpu, 64, 130, MAX, 9)):
        val, ind, y = device_vs_twin(P)
        v = view(P)
        want = py_farkas(**v)
        assert same_bits(val, want[0]) and np.array_equal(ind, want[1]) and same_bits(y, want[2])
        assert ind[0] == 2 and exact_proof(v, y)[0]


def window_nodes(gpu, root, A, b, count):
    """`count` solved clones of the solved root: the even ones with a column's upper bound pulled under its value (they stay
    feasible), the odd ones with a column pushed past a row's capacity (MVX_NOFEAS)."""
    x = root.col_prim()
    order = np.argsort(-x)
    nodes = []
    for t in range(count):
        ch = root.copy()
        if t % 2 == 0:
            j = int(order[(t // 2) % len(order)])
            ub = float(max(0.0, np.floor(x[j]) - (t // 2) // len(order)))
            ch.api.set_col_bnds(ch.h, j + 1, DB if ub > 0.0 else FX, 0.0, ub)
        else:
            i, j = (t // 2) % root.m, (t // 2) % root.n
            ch.api.set_col_bnds(ch.h, j + 1, DB, min(3.0, np.floor(float(b[i]) / float(A[i, j])) + 1.0), 3.0)
        nodes.append(ch)
    hs = (bnb.C.c_void_p * count)(*[p.h for p in nodes])
    gpu.simplex_batch(hs, count, None, None)
    assert all(p.status != UNDEF for p in nodes)
    return nodes


def many_vs_twin(root, nodes):
    rc, val, ind = bnb.farkas_many(root, nodes)
    trc, tval, tind = bnb.farkas_many(root, nodes, table=None)
    assert rc == trc == 0, (rc, trc)
    assert same_bits(val, tval) and np.array_equal(ind, tind), np.argwhere(val != tval)[:4]
    for p, i in zip(nodes, ind):
        assert (i[0] == 2) == (p.status == NOFEAS), (p.status, i)
    return val, ind


def ilp_root(gpu, m=24, n=48):
    A, b, c, U = synth.dense_ilp(m, n, 5, 3, 0.3)
    for i in range(m):  # a column at its upper bound 3 alone can exceed a row: b_i < 3 a_i,i
        A[i, i % n] = np.floor(b[i] / 3.0) + 1.0
    root = lpgen.load_ilp(gpu, A, b, c, U)
    root.simplex()
    assert root.status == OPT
    return root, A, b, c, U


@pytest.mark.parametrize("count", [1, 2, 70])
def test_farkas_many_counts(gpu, count):
    root, A, b, _, _ = ilp_root(gpu)
    nodes = window_nodes(gpu, root, A, b, count)
    val, ind = many_vs_twin(root, nodes)
    assert count < 2 or any(p.status == NOFEAS for p in nodes)
    assert count < 2 or any(p.status == OPT for p in nodes)
    one = bnb.farkas(nodes[-1], weights=False)  # a handle against itself: the same numbers
    assert one[0] == 0 and same_bits(one[1], val[-1]) and np.array_equal(one[2], ind[-1])
    assert bnb.farkas_many(root, [])[0] == 0


def test_farkas_many_with_cut_rows_and_a_stranger(gpu):
    root, A, b, c, U = ilp_root(gpu, 24, 65)
    nodes = window_nodes(gpu, root, A, b, 4)
    m0, n = root.m, root.n
    # handle 0 (feasible so far): one cut row that contradicts row 1 -- the proof needs the cut row's weight;
    # handle 2 (feasible): three cut rows that only cut its vertex off; handles 1 and 3 keep the root's rows
    vals = np.zeros((1, n + 1))
    vals[0, 1:] = A[0]
    assert bnb.add_cut_rows(nodes[0], vals, np.array([float(b[0]) + 1.0])) == 0
    x = nodes[2].col_prim()
    vals = np.zeros((3, n + 1))
    rhs = np.zeros(3)
    for r in range(3):
        vals[r, 1:] = -A[3 * r + 2]
        rhs[r] = -float(A[3 * r + 2] @ x) + 0.25
    assert bnb.add_cut_rows(nodes[2], vals, rhs) == 0
    for t in (0, 2):
        nodes[t].simplex()
    assert nodes[0].m == m0 + 1 and nodes[2].m == m0 + 3 and nodes[0].status == NOFEAS and nodes[2].status != UNDEF
    val, ind = many_vs_twin(root, nodes)
    assert ind[0][0] == 2
    rc, _, _, y = bnb.farkas(nodes[0])
    assert rc == 0 and y[m0 + 1] != 0.0 and exact_proof(view(nodes[0]), y)[0]  # the cut row carries weight
    for t in range(4):  # each handle against itself, with its cut rows as its own model rows
        one = bnb.farkas(nodes[t], weights=False)
        assert one[0] == 0 and same_bits(one[1], val[t]) and np.array_equal(one[2], ind[t]), t
    other = lpgen.load_ilp(gpu, A, b, c, U)  # the same numbers, other row objects
    other.simplex()
    before = val.copy()
    rc, val2, ind2 = bnb.farkas_many(root, nodes[:2] + [other])
    assert rc == -3 and not val2.any() and not ind2.any()
    unsolved = root.copy()
    unsolved.api.set_col_bnds(unsolved.h, 1, DB, 0.0, 1.0)
    assert bnb.farkas_many(root, [unsolved])[0] == -3 and bnb.farkas(unsolved)[0] == -3 and bnb.farkas(unsolved, table=None)[0] == -3
    narrow = ilp_root(gpu)[0]
    assert bnb.farkas_many(root, [narrow])[0] == -1  # another column count
    assert same_bits(many_vs_twin(root, nodes)[0], before)


def test_the_calls_are_pure(gpu):
    root, A, b, _, _ = ilp_root(gpu)
    nodes = window_nodes(gpu, root, A, b, 4)
    held = [root] + nodes
    before = [(state(p), p.status, p.obj, p.it_cnt, list(p.col_prim()), list(p.row_dual())) for p in held]
    many_vs_twin(root, nodes)
    for p in held:
        device_vs_twin(p)
    for p, (st, status, obj, it, x, lam) in zip(held, before):
        now = state(p)
        assert same_bits(now[0], st[0]) and all(np.array_equal(a, b) for a, b in zip(now[1:], st[1:]))
        assert (p.status, p.obj, p.it_cnt, list(p.col_prim()), list(p.row_dual())) == (status, obj, it, x, lam)


def test_trees_on_the_engine_and_over_the_oracle(gpu, orc):
    """Repaired mode, window 64: the engine's driver (farkas_many on the device) and the same driver over the oracle's table (the
    twin) book the same counters, bit for bit, and the flag changes nothing else about the tree."""
    case = (24, 48, 5, 1, 0.06)
    tab = bnb.table_from(orc)
    on = bnb.branch_and_bound(lpgen.load_ilp(gpu, *synth.dense_ilp(*case)), quirks=0, window=64, farkas=1)
    off = bnb.branch_and_bound(lpgen.load_ilp(gpu, *synth.dense_ilp(*case)), quirks=0, window=64)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, *synth.dense_ilp(*case)), table=tab, quirks=0, window=64, farkas=1)
    assert on["rc"] == off["rc"] == ref["rc"] == 0
    assert treedigest.digest(on) == treedigest.digest(off) == treedigest.digest(ref)
    for key in off:
        if key not in bnb.FARKAS_COUNTERS:
            assert on[key] == off[key], key
    assert all(off[k] == 0 for k in bnb.FARKAS_COUNTERS)
    for k in bnb.FARKAS_COUNTERS:
        assert same_bits([on[k]], [ref[k]]), (k, on[k], ref[k])
    assert on["farkas_nodes"] > 0 and on["farkas_proved"] == on["farkas_nodes"] and on["farkas_dropped"] == 0
    assert on["farkas_rel_min"] > REL and on["farkas_rel_oid"] > 0
    serial = bnb.branch_and_bound(lpgen.load_ilp(gpu, *synth.dense_ilp(*case)), quirks=0, window=1, farkas=1)
    assert all(same_bits([serial[k]], [on[k]]) for k in bnb.FARKAS_COUNTERS)


def ray_device_vs_twin(P):
    rc, val, ind, d = bnb.ray(P)
    trc, tval, tind, td = bnb.ray(P, table=None)
    assert rc == trc == 0, (rc, trc)
    assert same_bits(val, tval) and np.array_equal(ind, tind) and same_bits(d, td), (val, tval, ind, tind)
    prc, pval, pind, pd = P.ray()  # the handle's own method is the same call
    assert prc == 0 and same_bits(pval, val) and np.array_equal(pind, ind) and same_bits(pd, d) and d[0] == 0.0
    nrc, nval, nind, nd = bnb.ray(P, direction=False)
    assert nrc == 0 and nd is None and same_bits(nval, val) and np.array_equal(nind, ind)
    return val, ind, d


@pytest.mark.parametrize("n", [1, 2, 64, 65])
def test_the_ray_of_the_cone(gpu, n):
    for direction in (MAX, MIN):
        if n == 1:  # one column, one empty row: the column itself is the ray
            P = gpu.create()
            P.load_general(np.zeros((1, 1)), [(UP, 0.0, 1.0)], [(LO, 0.0, 0.0)], np.ones(1) if direction == MAX else -np.ones(1), direction=direction)
        else:
            P = cone(gpu, direction, n)
        P.simplex()
        assert P.status == UNBND, (n, direction)
        before = (state(P), P.status, P.it_cnt)
        val, ind, d = ray_device_vs_twin(P)
        want = py_ray(P)
        assert same_bits(val, want[0]) and np.array_equal(ind, want[1]) and same_bits(d, want[2])
        assert ind[0] == 2 and ind[3] == 0 and P.get_unbnd_ray() == ind[1] and 1 <= ind[1] <= P.m + P.n
        now = state(P)  # pure
        assert same_bits(now[0], before[0][0]) and all(np.array_equal(a, b) for a, b in zip(now[1:], before[0][1:]))
        assert (P.status, P.it_cnt) == before[1:]


def test_no_ray_on_solved_and_infeasible_handles(gpu):
    P = cone(gpu, MAX, 65, cap=50.0)
    P.simplex()
    assert P.status == OPT and P.get_unbnd_ray() == 0
    val, ind, d = ray_device_vs_twin(P)
    assert not val.any() and not ind.any() and not d.any()
    for lim in (1, 5):  # stopped on the way: every improving column is blocked
        Q = cone(gpu, MAX, 65, cap=50.0)
        Q.simplex(it_lim=lim)
        assert ray_device_vs_twin(Q)[1][0] == 0 and Q.get_unbnd_ray() == 0
    root, warm = warm_nofeas(gpu, 65, 64, MAX, 3)
    assert warm.status == NOFEAS and warm.get_unbnd_ray() == 0 and root.get_unbnd_ray() == 0
    ray_device_vs_twin(warm)
    ray_device_vs_twin(root)
    fresh = cone(gpu, MAX, 3)
    assert fresh.get_unbnd_ray() == 0 and bnb.ray(fresh)[0] == -3 and bnb.ray(fresh, table=None)[0] == -3  # never solved


UNBOUNDED = """\\ an open cone
Maximize
 obj: x1 + x2
Subject To
 c1: x1 - x2 <= 1
End
"""


def test_cli_farkas_reports_the_root_ray(gpu, tmp_path):
    exe = os.path.join(ROOT, "mvolps_amd", "bin", "mvolps")
    lp = str(tmp_path / "cone.lp")
    open(lp, "w").write(UNBOUNDED)
    report = str(tmp_path / "cone.farkas")
    plain = subprocess.run([exe, "-f", lp, "--repaired"], capture_output=True, text=True)
    r = subprocess.run([exe, "-f", lp, "--repaired", "--farkas", report], capture_output=True, text=True)
    assert r.returncode == plain.returncode and r.stdout == plain.stdout, r.stderr
    L = bnb.lib()
    L.mvx_read_lp.restype = bnb.C.c_int
    L.mvx_read_lp.argtypes = [bnb.C.c_void_p, bnb.C.c_void_p, bnb.C.c_char_p]
    P = gpu.create()
    assert L.mvx_read_lp(P.h, None, lp.encode()) == 0
    P.simplex()
    assert P.status == UNBND
    rc, val, ind, _ = bnb.ray(P, table=None, direction=False)
    assert rc == 0 and ind[0] == 2
    lines = open(report).read().splitlines()
    assert lines[0].split()[0] == "RAY.ROOT" and lines[1].split() == ["FARKAS.NODES", "0"]
    f = lines[0].split()
    assert [int(t) for t in f[1:7]] == ind.tolist() and [float(t) for t in f[7:11]] == val.tolist(), lines[0]


TWO_ROWS = """\\ two rows that contradict each other
Maximize
 obj: x1 + 2 x2
Subject To
 c1: x1 + x2 <= 1
 c2: x1 + x2 >= 3
Bounds
 x1 <= 5
 x2 <= 5
End
"""


def test_cli_farkas_on_an_infeasible_lp(gpu, tmp_path):
    exe = os.path.join(ROOT, "mvolps_amd", "bin", "mvolps")
    lp = str(tmp_path / "two_rows.lp")
    open(lp, "w").write(TWO_ROWS)
    report = str(tmp_path / "two_rows.farkas")
    plain = subprocess.run([exe, "-f", lp, "--repaired"], capture_output=True, text=True)
    r = subprocess.run([exe, "-f", lp, "--repaired", "--farkas", report], capture_output=True, text=True)
    assert r.returncode == plain.returncode, r.stderr
    assert r.stdout == plain.stdout  # the flag changes nothing else about the run
    L = bnb.lib()
    L.mvx_read_lp.restype = bnb.C.c_int
    L.mvx_read_lp.argtypes = [bnb.C.c_void_p, bnb.C.c_void_p, bnb.C.c_char_p]
    P = gpu.create()
    assert L.mvx_read_lp(P.h, None, lp.encode()) == 0
    bnb.integral_bounds(P)
    P.simplex()
    assert P.status == NOFEAS
    rc, val, ind, _ = bnb.farkas(P, table=None, weights=False)
    assert rc == 0 and ind[0] == 2
    lines = open(report).read().splitlines()
    assert [ln.split()[0] for ln in lines] == ["FARKAS.ROOT", "FARKAS.NODES", "FARKAS.PROVED", "FARKAS.TABLEAU_ONLY", "FARKAS.NONE",
                                              "FARKAS.DROPPED", "FARKAS.REL_MIN", "FARKAS.DE_MAX"]
    f = lines[0].split()
    assert [int(t) for t in f[1:5]] == ind.tolist() and [float(t) for t in f[5:9]] == val.tolist(), lines[0]
    P2 = gpu.create()
    assert L.mvx_read_lp(P2.h, None, lp.encode()) == 0
    tree = bnb.branch_and_bound(P2, quirks=0, farkas=1)
    assert [int(ln.split()[1]) for ln in lines[1:6]] == [tree[k] for k in bnb.FARKAS_COUNTERS[:5]] == [1, 1, 0, 0, 0]
    assert (float(lines[6].split()[1]), int(lines[6].split()[2])) == (tree["farkas_rel_min"], tree["farkas_rel_oid"]) == (float(val[1]), 1)
    assert (float(lines[7].split()[1]), int(lines[7].split()[2])) == (tree["farkas_de_max"], tree["farkas_de_oid"])


def test_cli_farkas_without_a_writable_file_runs_the_tree_unchecked(gpu, tmp_path):
    """No half report: when FILE cannot be written the front end says so and the run is the one without the flag."""
    exe = os.path.join(ROOT, "mvolps_amd", "bin", "mvolps")
    f1 = os.path.join(ROOT, "tests", "golden", "f1.lp")
    report = str(tmp_path / "no such directory" / "f1.farkas")
    plain = subprocess.run([exe, "-f", f1, "--repaired", "-v"], capture_output=True, text=True)
    r = subprocess.run([exe, "-f", f1, "--repaired", "-v", "--farkas", report], capture_output=True, text=True)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    assert r.stdout == plain.stdout and "Farkas proofs:" not in r.stdout
    assert "--farkas: no report" in r.stderr and "the tree runs unchecked" in r.stderr and not os.path.exists(report)
