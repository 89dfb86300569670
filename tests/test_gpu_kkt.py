"""GPU: the KKT check on the device (k_kkt_vals / k_kkt_rows / k_kkt_cols / k_kkt_fin through mvx_kkt, mvx_kkt_many and
mvx_check_kkt) against the host twin through the engine's own table (mvx_bnb_kkt), every bit of val, ind, r_pe and r_de, on the
shapes where the kernels can go wrong: rows and columns either side of the 64 chains of a wave and beyond two of them, one row,
one column, both directions, free, fixed and upper-bounded columns, every end status; windows of handles with cut rows and an
objective of their own; a long run without refresh; the call's purity; trees; the command line."""
import os
import subprocess

import numpy as np
import pytest

from mvolps_amd import bnb, synth, treedigest
from mvolps_amd.capi import DB, FEAS, FR, FX, INFEAS, LO, MAX, MIN, NOFEAS, OPT, UNBND, UNDEF, UP

from . import lpgen
from .test_gpu_purge import state
from .test_kkt import by_getters, longdouble_bound, np_kkt, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 63, 64, 65, 130]  # the chain and wave boundaries of both passes


def device_vs_twin(P):
    rc, val, ind, r_pe, r_de = bnb.kkt(P)
    trc, tval, tind, tpe, tde = bnb.kkt(P, table=None)
    assert rc == trc == 0, (rc, trc)
    assert same_bits(val, tval) and np.array_equal(ind, tind), (val, tval, ind, tind)
    assert same_bits(r_pe, tpe), np.argwhere(r_pe != tpe)[:4]
    assert same_bits(r_de, tde), np.argwhere(r_de != tde)[:4]
    assert r_pe[0] == 0.0 and r_de[0] == 0.0
    prc, pval, pind, ppe, pde = P.kkt()  # the handle's own method is the same call
    assert prc == 0 and same_bits(pval, val) and np.array_equal(pind, ind) and same_bits(ppe, r_pe) and same_bits(pde, r_de)
    nrc, nval, nind, npe, nde = bnb.kkt(P, residuals=False)  # without the residual vectors
    assert nrc == 0 and npe is None and nde is None and same_bits(nval, val) and np.array_equal(nind, ind)
    return val, ind, r_pe, r_de


def general_model(api, m, n, direction, seed):
    """Mixed signs, every row type, DB / LO / UP / FR / FX columns around a point that is feasible by construction."""
    rng = np.random.default_rng(seed)
    A = np.round(rng.normal(size=(m, n)) * 3)
    A[rng.random((m, n)) >= 0.4] = 0
    x0 = rng.integers(0, 4, size=n).astype(float)
    col_b = []
    for j in range(n):
        t = int(rng.choice([DB, LO, UP, FR, FX], p=[0.55, 0.1, 0.15, 0.1, 0.1]))
        col_b.append((t, x0[j], x0[j]) if t == FX else (t, -1.0, 4.5))
    act = A @ x0
    row_b = []
    for i in range(m):
        t = int(rng.choice([LO, UP, DB, FR, FX], p=[0.3, 0.3, 0.25, 0.05, 0.1]))
        row_b.append((t, float(act[i]), float(act[i])) if t == FX else (t, float(act[i] - rng.integers(0, 20)), float(act[i] + rng.integers(0, 20))))
    P = api.create()
    P.load_general(A, row_b, col_b, np.round(rng.normal(size=n) * 5), c0=1.5, direction=direction)
    return P


@pytest.mark.parametrize("m", SIZES)
def test_device_matches_twin(gpu, m):
    seen = set()
    for n in SIZES:
        P = lpgen.load_ilp(gpu, *synth.dense_ilp(m, n, 11 + n + m, 3, 0.4))
        P.simplex()
        assert P.status == OPT
        device_vs_twin(P)
        for direction in (MIN, MAX):
            for lim in (None, 2):
                P = general_model(gpu, m, n, direction, 20261021 + 7 * n + 31 * m + direction)
                P.simplex(it_lim=lim)
                seen.add(P.status)
                device_vs_twin(P)
    assert OPT in seen or UNBND in seen


def test_every_end_status(gpu):
    """OPT, FEAS and INFEAS with an iteration limit on a general model, NOFEAS on a contradictory row, UNBND on an open cone."""
    seen = {}
    for seed in range(8):
        for lim in (None, 0, 1, 3, 8, 20):
            P = general_model(gpu, 65, 66, MAX if seed % 2 else MIN, 500 + seed)
            P.simplex(it_lim=lim)
            if P.status not in seen:
                seen[P.status] = device_vs_twin(P)
    P = lpgen.load_ilp(gpu, *synth.dense_ilp(24, 48, 5, 3, 0.3))  # the slack basis is feasible: two pivots into phase 2
    P.simplex(it_lim=2)
    seen.setdefault(P.status, device_vs_twin(P))
    P = general_model(gpu, 65, 66, MAX, 77)
    for j in range(1, P.n + 1):
        P.api.set_col_bnds(P.h, j, DB, -1.0, 4.5)
    P.api.set_row_bnds(P.h, 3, FX, 1e6, 1e6)
    P.simplex()
    seen.setdefault(P.status, device_vs_twin(P))
    rng = np.random.default_rng(5)
    P = gpu.create()
    P.load_general(-rng.integers(0, 3, size=(64, 65)).astype(float), [(UP, 0.0, 4.0)] * 64, [(LO, 0.0, 0.0)] * 65, np.ones(65))
    P.simplex()
    seen.setdefault(P.status, device_vs_twin(P))
    assert {OPT, FEAS, INFEAS, NOFEAS, UNBND} <= set(seen), sorted(seen)
    assert seen[INFEAS][0][2] > 0.0 and seen[NOFEAS][0][2] > 0.0  # PB says so
    assert seen[OPT][0][2] < 1e-8 and seen[OPT][0][6] < 1e-8


def test_restatement_and_longdouble_on_the_engine(gpu):
    """The independent restatement once on the engine's own handle (the CPU file runs it over the oracle's)."""
    P = general_model(gpu, 65, 63, MIN, 9)
    P.simplex()
    val, ind, r_pe, r_de = device_vs_twin(P)
    g = by_getters(P)
    want = np_kkt(**g)
    assert same_bits(val, want[0]) and np.array_equal(ind, want[1]) and same_bits(r_pe, want[2]) and same_bits(r_de, want[3])
    longdouble_bound(g, r_pe, r_de)


def window_nodes(gpu, root, count):
    """`count` solved clones of the solved root, each with one column's upper bound pulled under its value."""
    x = root.col_prim()
    order = np.argsort(-x)
    nodes = []
    for t in range(count):
        ch = root.copy()
        j = int(order[t % len(order)])
        ub = float(max(0.0, np.floor(x[j]) - t // len(order)))
        ch.api.set_col_bnds(ch.h, j + 1, DB if ub > 0.0 else FX, 0.0, ub)
        nodes.append(ch)
    hs = (bnb.C.c_void_p * count)(*[p.h for p in nodes])
    gpu.simplex_batch(hs, count, None, None)
    assert all(p.status != UNDEF for p in nodes)
    return nodes


def many_vs_twin(root, nodes):
    rc, val, ind = bnb.kkt_many(root, nodes)
    trc, tval, tind = bnb.kkt_many(root, nodes, table=None)
    assert rc == trc == 0, (rc, trc)
    assert same_bits(val, tval) and np.array_equal(ind, tind), np.argwhere(val != tval)[:4]
    return val, ind


@pytest.mark.parametrize("count", [1, 2, 70])
def test_kkt_many_counts(gpu, count):
    root = lpgen.load_ilp(gpu, *synth.dense_ilp(24, 48, 5, 3, 0.3))
    root.simplex()
    nodes = window_nodes(gpu, root, count)
    val, _ind = many_vs_twin(root, nodes)
    one = bnb.kkt(nodes[-1], residuals=False)  # a handle against itself: the same numbers
    assert one[0] == 0 and same_bits(one[1], val[-1])
    assert bnb.kkt_many(root, [])[0] == 0


def test_kkt_many_with_cut_rows_an_own_objective_and_a_stranger(gpu):
    A, b, c, U = synth.dense_ilp(24, 65, 5, 3, 0.3)
    root = lpgen.load_ilp(gpu, A, b, c, U)
    root.simplex()
    nodes = window_nodes(gpu, root, 4)
    m0, n = root.m, root.n
    for t, k in ((1, 1), (2, 3)):  # copies of model rows as >= rows that cut the node's vertex off
        x = nodes[t].col_prim()
        vals = np.zeros((k, n + 1))
        rhs = np.zeros(k)
        for r in range(k):
            vals[r, 1:] = -A[3 * r + t]
            rhs[r] = -float(A[3 * r + t] @ x) + 0.25
        assert bnb.add_cut_rows(nodes[t], vals, rhs) == 0
        nodes[t].simplex()
        assert nodes[t].m == m0 + k and nodes[t].status != UNDEF
    own = np.concatenate([[0.0], np.round(np.random.default_rng(3).normal(size=n) * 4)])
    assert bnb.set_obj_many([nodes[3]], [own]) == 0
    nodes[3].simplex()
    assert nodes[3].status != UNDEF
    val, ind = many_vs_twin(root, nodes)
    assert not same_bits(val[0], val[3])
    for t in range(4):  # each handle against itself, with its cut rows as its own model rows
        one = bnb.kkt(nodes[t], residuals=False)
        assert one[0] == 0 and same_bits(one[1], val[t]) and np.array_equal(one[2], ind[t]), t
    other = lpgen.load_ilp(gpu, A, b, c, U)  # the same numbers, other row objects
    other.simplex()
    before = val.copy()
    rc, val2, _ = bnb.kkt_many(root, nodes[:2] + [other])
    assert rc == -3 and not val2.any()
    unsolved = root.copy()
    unsolved.api.set_col_bnds(unsolved.h, 1, DB, 0.0, 1.0)
    assert bnb.kkt_many(root, [unsolved])[0] == -3 and bnb.kkt(unsolved)[0] == -3 and bnb.kkt(unsolved, table=None)[0] == -3
    narrow = lpgen.load_ilp(gpu, *synth.dense_ilp(24, 48, 5, 3, 0.3))
    narrow.simplex()
    assert bnb.kkt_many(root, [narrow])[0] == -1  # another column count
    assert same_bits(many_vs_twin(root, nodes)[0], before)


def test_a_long_run_without_refresh(gpu):
    """Warm-started clones of clones with the residual check switched off: the rounding of every pivot stays in the tableau,
    the residuals are not all zero, and they are still the twin's bits and inside the forward-error bound."""
    gpu.set_refresh(1 << 30, 1.0)
    try:
        P = gpu.create()
        P.load_dense(*synth.dense_lp(64, 128, seed=3))
        P.simplex()
        assert P.status == OPT
        rng = np.random.default_rng(1)
        it0 = P.it_cnt
        for step in range(150):
            ch = P.copy()
            x = ch.col_prim()
            j = int(rng.integers(ch.n))
            if step % 2:
                ch.api.set_col_bnds(ch.h, j + 1, DB, 0.0, float(x[j]) * 0.5 + 0.25)
            else:
                ch.api.set_col_bnds(ch.h, j + 1, LO, 0.0, 0.0)
            ch.simplex()
            if ch.status == OPT:
                P = ch
        assert P.it_cnt > it0 + 20 and gpu.get_refresh_cnt(P.h) == 0
        val, _ind, r_pe, r_de = device_vs_twin(P)
        assert np.count_nonzero(r_pe) + np.count_nonzero(r_de) > 0 and val[0] > 0.0
        longdouble_bound(by_getters(P), r_pe, r_de)
    finally:
        gpu.set_refresh(1024, 1e-9)


def test_the_calls_are_pure(gpu):
    root = lpgen.load_ilp(gpu, *synth.dense_ilp(24, 48, 5, 3, 0.3))
    root.simplex()
    nodes = window_nodes(gpu, root, 3)
    held = [root] + nodes
    before = [(state(p), p.status, p.obj, p.it_cnt, list(p.col_prim()), list(p.row_dual())) for p in held]
    many_vs_twin(root, nodes)
    device_vs_twin(root)
    for cond in (1, 2, 3, 4):
        assert root.check_kkt(cond)[0] == 0
    for p, (st, status, obj, it, x, lam) in zip(held, before):
        now = state(p)
        assert same_bits(now[0], st[0]) and all(np.array_equal(a, b) for a, b in zip(now[1:], st[1:]))
        assert (p.status, p.obj, p.it_cnt, list(p.col_prim()), list(p.row_dual())) == (status, obj, it, x, lam)


def test_check_kkt_agrees_with_kkt(gpu):
    P = general_model(gpu, 63, 65, MAX, 21)
    P.simplex(it_lim=4)
    val, ind, _, _ = device_vs_twin(P)
    for cond in (1, 2, 3, 4):
        rc, ae, ai, re, ri = P.check_kkt(cond)
        assert rc == 0 and (ae, re) == (val[2 * cond - 2], val[2 * cond - 1]) and (ai, ri) == (ind[2 * cond - 2], ind[2 * cond - 1])
    assert P.check_kkt(0)[0] == -1 and P.check_kkt(5)[0] == -1 and P.check_kkt(1, sol=2)[0] == -1
    fresh = general_model(gpu, 5, 6, MAX, 2)
    assert fresh.check_kkt(1)[0] == -3 and bnb.kkt(fresh)[0] == -3  # never solved


def test_trees_on_the_engine_and_over_the_oracle(gpu, orc):
    """Repaired mode, window 64: the engine's driver (kkt_many on the device) and the same driver over the oracle's table (the
    twin) book the same worst values, bit for bit, and the flag changes nothing else about the tree."""
    case = (24, 48, 5, 1, 0.06)
    tab = bnb.table_from(orc)
    on = bnb.branch_and_bound(lpgen.load_ilp(gpu, *synth.dense_ilp(*case)), quirks=0, window=64, kkt=1)
    off = bnb.branch_and_bound(lpgen.load_ilp(gpu, *synth.dense_ilp(*case)), quirks=0, window=64)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, *synth.dense_ilp(*case)), table=tab, quirks=0, window=64, kkt=1)
    assert on["rc"] == off["rc"] == ref["rc"] == 0
    assert treedigest.digest(on) == treedigest.digest(off) == treedigest.digest(ref)
    for key in off:
        if key not in bnb.KKT_COUNTERS:
            assert on[key] == off[key], key
    assert off["kkt_nodes"] == 0 and on["kkt_nodes"] == on["count"] == ref["kkt_nodes"]
    assert same_bits(on["kkt_re"], ref["kkt_re"]) and on["kkt_oid"] == ref["kkt_oid"], (on["kkt_re"], ref["kkt_re"])
    assert on["kkt_re"][1] > 1.0 and on["kkt_re"][0] < 1e-10  # the infeasible nodes show in PB, the equations hold
    serial = bnb.branch_and_bound(lpgen.load_ilp(gpu, *synth.dense_ilp(*case)), quirks=0, window=1, kkt=1)
    assert same_bits(serial["kkt_re"], on["kkt_re"]) and serial["kkt_oid"] == on["kkt_oid"] and serial["kkt_nodes"] == on["kkt_nodes"]


def test_cli_kkt_on_f1(gpu, tmp_path):
    exe = os.path.join(ROOT, "mvolps_amd", "bin", "mvolps")
    f1 = os.path.join(ROOT, "tests", "golden", "f1.lp")
    report = str(tmp_path / "f1.kkt")
    plain = subprocess.run([exe, "-f", f1, "--repaired"], capture_output=True, text=True)
    r = subprocess.run([exe, "-f", f1, "--repaired", "--kkt", report], capture_output=True, text=True)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    assert r.stdout == plain.stdout  # the flag changes nothing else about the run
    L = bnb.lib()
    L.mvx_read_lp.restype = bnb.C.c_int
    L.mvx_read_lp.argtypes = [bnb.C.c_void_p, bnb.C.c_void_p, bnb.C.c_char_p]
    P = gpu.create()
    assert L.mvx_read_lp(P.h, None, f1.encode()) == 0
    bnb.integral_bounds(P)
    P.simplex()
    rc, val, ind, _, _ = bnb.kkt(P, table=None, residuals=False)
    assert rc == 0
    lines = open(report).read().splitlines()
    assert [ln.split()[0] for ln in lines] == ["KKT.PE", "KKT.PB", "KKT.DE", "KKT.DB", "KKT.NODES", "KKT.TREE.PE", "KKT.TREE.PB", "KKT.TREE.DE",
                                              "KKT.TREE.DB"]
    for c in range(4):
        f = lines[c].split()
        assert (float(f[1]), int(f[2]), float(f[3]), int(f[4])) == (val[2 * c], ind[2 * c], val[2 * c + 1], ind[2 * c + 1]), lines[c]
    P2 = gpu.create()
    assert L.mvx_read_lp(P2.h, None, f1.encode()) == 0
    tree = bnb.branch_and_bound(P2, quirks=0, kkt=1)
    assert int(lines[4].split()[1]) == tree["kkt_nodes"] > 0
    for c in range(4):
        f = lines[5 + c].split()
        assert (float(f[1]), int(f[2])) == (tree["kkt_re"][c], tree["kkt_oid"][c]), lines[5 + c]


def test_cli_kkt_without_a_writable_file_runs_the_tree_unchecked(gpu, tmp_path):
    """No half report: when FILE cannot be written the front end says so and the run is the one without the flag."""
    exe = os.path.join(ROOT, "mvolps_amd", "bin", "mvolps")
    f1 = os.path.join(ROOT, "tests", "golden", "f1.lp")
    report = str(tmp_path / "no such directory" / "f1.kkt")
    plain = subprocess.run([exe, "-f", f1, "--repaired", "-v"], capture_output=True, text=True)
    r = subprocess.run([exe, "-f", f1, "--repaired", "-v", "--kkt", report], capture_output=True, text=True)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    assert r.stdout == plain.stdout and "KKT check:" not in r.stdout
    assert "--kkt: no report" in r.stderr and "the tree runs unchecked" in r.stderr and not os.path.exists(report)

