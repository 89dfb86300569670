"""GPU: incumbent polishing on the device (k_lsact / k_lsmove / k_lsapply through mvx_polish_many) against the host twin through
the engine's own table (mvx_bnb_polish), bit for bit: x, obj, moves and ok, on shapes where the kernels can go wrong (word
boundaries of the partner columns, a best pair in the last word, one row, the enqueue's group boundaries, several points in one
call with a refused and a locally optimal one among them, the tie models); the call's purity; and whole trees on the HIP engine
against the same trees with the table entry removed."""
import os

import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import CV, DB, FR, IV, LO, MAX, MIN, OPT, UP

from . import lpgen
from .test_bnb_general import DRAWN, instance
from .test_bnb_host import same_result
from .test_bnb_polish import TIES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_vs_twin(P, xs, max_moves):
    """One mvx_polish_many call for all points against mvx_bnb_polish point by point."""
    xs = np.atleast_2d(np.asarray(xs, dtype=float))
    pts = np.concatenate((np.zeros((xs.shape[0], 1)), xs), axis=1)
    rc, x, obj, moves, ok = bnb.polish_many(P, pts, max_moves)
    trc, tx, tobj, tmoves, tok = bnb.polish_many(P, pts, max_moves, table=None)
    assert rc == trc == 0
    assert np.array_equal(ok, tok), (ok, tok)
    assert np.array_equal(moves, tmoves), (moves, tmoves)
    assert np.array_equal(x[:, 1:], tx[:, 1:]), np.argwhere(x != tx)[:4]
    assert np.array_equal(obj, tobj), (obj, tobj)
    return x[:, 1:], obj, moves, ok


def packing(gpu, m, n, seed, U, ramp):
    """dense_ilp's model at any size; with ramp the costs are 1..n, so the best pair is the last two columns: the partner lies
    in the last word, and for n = 64 the two sit either side of a word boundary."""
    A, b, c, U = synth.dense_ilp(m, n, seed, U, 0.4)
    if ramp:
        c = np.arange(1.0, n + 1.0)
    return lpgen.load_ilp(gpu, A, b, c, U), A, b, c, U


@pytest.mark.parametrize("U", [1, 3])
@pytest.mark.parametrize("m", [1, 3, 70])
@pytest.mark.parametrize("n", [5, 63, 64, 65, 129])
def test_packing_shapes(gpu, n, m, U):
    """From x = 0 every move is there to make; 1, 2 and 1000 moves end inside the first group of the enqueue and, where the
    search is long enough, behind several groups."""
    for ramp in (False, True):
        P, A, b, c, _U = packing(gpu, m, n, 11 + n + m, U, ramp)
        zero = np.zeros(n)
        for cap in (1, 2, 1000):
            x, _obj, moves, ok = device_vs_twin(P, zero, cap)
            assert ok[0] == 1 and 1 <= moves[0] <= cap
            if cap == 1 and ramp and n >= 63:  # a row holds 0.4 of its coefficients' sum: any two columns fit
                assert list(np.flatnonzero(x[0])) == [n - 2, n - 1]


def general_sized(gpu, rng, m, n, direction):
    """Mixed signs, every row type, integer and continuous columns, around a point x0 that is feasible by construction."""
    A = np.round(rng.normal(size=(m, n)) * 3)
    A[rng.random((m, n)) >= 0.3] = 0
    kinds = [IV if rng.random() < 0.85 else CV for _ in range(n)]
    x0 = np.array([float(rng.integers(0, 4)) if k == IV else float(rng.random() * 3) for k in kinds])
    col_b = []
    for j in range(n):
        t = DB if rng.random() < 0.8 else int(rng.choice([LO, UP, FR]))
        col_b.append((t, -1.0, 4.5))
    act = A @ x0
    row_b = []
    for i in range(m):
        t = int(rng.choice([LO, UP, DB, FR], p=[0.3, 0.3, 0.3, 0.1]))
        row_b.append((t, float(np.floor(act[i]) - rng.integers(0, 20)), float(np.ceil(act[i]) + rng.integers(0, 20))))
    c = np.round(rng.normal(size=n) * 5)
    P = gpu.create()
    P.load_general(A, row_b, col_b, c, c0=1.5, kinds=kinds, direction=direction)
    return P, x0


@pytest.mark.parametrize("direction", [MAX, MIN], ids=["max", "min"])
@pytest.mark.parametrize("shape", [(3, 5), (7, 63), (12, 64), (70, 65), (33, 129)], ids=lambda s: "%dx%d" % s)
def test_mixed_sign_ranged_models(gpu, shape, direction):
    rng = np.random.default_rng(20261019 + 7 * shape[1] + direction)
    P, x0 = general_sized(gpu, rng, shape[0], shape[1], direction)
    for cap in (1, 2, 1000):
        _x, _obj, moves, ok = device_vs_twin(P, x0, cap)
        assert ok[0] == 1 and 1 <= moves[0] <= cap


def test_general_fixture_and_points_in_one_call(gpu):
    """count = 1 and count = 5 in one call on a mixed-sign ranged general fixture: its heur 2 point, the polished point
    (locally optimal: no move), a refused point, and the polished point walked off by single moves."""
    done = 0
    for rec in DRAWN:
        if rec["status"] != "optimal":
            continue
        inst = instance(rec)
        root = lpgen.load_milp(gpu, inst)
        isint = np.array([k != CV for k in inst["kinds"]])
        if bnb.fractional_bounds(root) != 0 or not isint.any():
            continue
        node = root.copy()
        node.simplex()
        if node.status != OPT:
            continue
        rc, _o, found, xr = bnb.round_many(root, [node], 1)
        if rc != 0 or not found[0]:
            continue
        x = xr[0, 1:]
        px, _obj, _moves, ok = device_vs_twin(root, x, 1000)
        assert ok[0] == 1
        refused = x.copy()
        refused[int(np.flatnonzero(isint)[0])] += 0.5
        pts = np.array([x, px[0], refused, x, px[0]])
        gx, _gobj, gmoves, gok = device_vs_twin(root, pts, 1000)
        assert list(gok) == [1, 1, 0, 1, 1] and gmoves[1] == 0 and gmoves[4] == 0
        assert np.array_equal(gx[2], refused) and np.array_equal(gx[0], px[0]) and np.array_equal(gx[3], px[0])
        done += 1
        if done >= 12:
            break
    assert done >= 12


def test_points_in_one_call_on_a_packing_model(gpu):
    P, A, b, c, U = packing(gpu, 70, 129, 5, 3, False)
    n = 129
    zero = np.zeros(n)
    px, _obj, moves, _ok = device_vs_twin(P, zero, 1000)
    assert moves[0] > 8  # more than one group of the enqueue
    frac = zero.copy()
    frac[128] = 0.5
    over = np.full(n, 3.0)  # every row violated
    half = device_vs_twin(P, zero, 5)[0][0]
    pts = np.array([zero, px[0], frac, half, over])
    for cap in (1, 2, 1000):
        gx, _gobj, gmoves, gok = device_vs_twin(P, pts, cap)
        assert list(gok) == [1, 1, 0, 1, 0] and gmoves[1] == 0
        assert np.array_equal(gx[2], frac) and np.array_equal(gx[4], over)
    assert np.array_equal(gx[0], px[0]) and np.array_equal(gx[3], px[0])  # the same local optimum from half way


@pytest.mark.parametrize("name", sorted(TIES))
def test_tie_models(gpu, name):
    t = TIES[name]
    A = np.asarray(t["A"], dtype=float)
    P = gpu.create()
    P.load_general(A, [(UP, 0.0, float(v)) for v in t["b"]], [(DB, 0.0, 1.0)] * 6, np.asarray(t["c"], dtype=float), kinds=[IV] * 6,
                   direction=MAX)
    x1, _obj, moves, ok = device_vs_twin(P, np.zeros(6), 1)
    assert ok[0] == 1 and moves[0] == 1 and np.array_equal(x1[0], np.array(t["first"], dtype=float))
    device_vs_twin(P, np.zeros(6), 1000)


def test_the_call_is_pure(gpu):
    A, b, c, U = synth.dense_ilp(24, 48, 5, 3, 0.3)
    P = lpgen.load_ilp(gpu, A, b, c, U)
    P.simplex()
    assert P.status == OPT
    tab0, basis0, obj0, it0 = P.tableau(), P.basis(), P.obj, P.it_cnt
    rc, _o, found, xr = bnb.round_many(P, [P], 2)
    assert rc == 0 and found[0]
    _x, _obj, moves, ok = device_vs_twin(P, xr[0, 1:], 1000)
    assert ok[0] == 1 and moves[0] >= 1
    assert P.status == OPT and P.obj == obj0 and P.it_cnt == it0
    assert np.array_equal(P.tableau(), tab0)
    assert all(np.array_equal(a, b_) for a, b_ in zip(P.basis(), basis0))


def test_argument_errors(gpu):
    L = bnb.lib()
    A, b, c, U = synth.dense_ilp(8, 16, 3, 1, 0.3)
    P = lpgen.load_ilp(gpu, A, b, c, U)
    x = np.zeros((1, 17))
    DP, IP = bnb.C.POINTER(bnb.C.c_double), bnb.C.POINTER(bnb.C.c_int)
    obj, moves, ok = np.zeros(1), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    args = (x.ctypes.data_as(DP), 10, obj.ctypes.data_as(DP), moves.ctypes.data_as(IP), ok.ctypes.data_as(IP))
    assert L.mvx_polish_many(None, 1, *args) == -1
    assert L.mvx_polish_many(P.h, -1, *args) == -1
    assert L.mvx_polish_many(P.h, 1, None, *args[1:]) == -1
    assert L.mvx_polish_many(P.h, 1, args[0], 0, *args[2:]) == -1
    assert L.mvx_polish_many(P.h, 1, args[0], 100001, *args[2:]) == -1
    assert L.mvx_polish_many(P.h, 0, *args) == 0
    assert L.mvx_polish_many(P.h, 1, *args) == 0 and ok[0] == 1


def trees_with_and_without_the_entry(gpu, load, **kw):
    host = bnb.table_from(gpu)
    assert host.polish_many
    host.polish_many = None
    got = bnb.branch_and_bound(load(), quirks=0, heur=2, polish=1000, window=64, **kw)
    ref = bnb.branch_and_bound(load(), quirks=0, heur=2, polish=1000, window=64, table=host, **kw)
    assert got["rc"] == ref["rc"] == 0
    same_result(got, ref)
    for k in bnb.POLISH_COUNTERS + ("heur_calls", "heur_found", "heur_improved", "incumbent_heur"):
        assert got[k] == ref[k], k
    return got


def test_tree_on_dense_ilp_matches_the_twin(gpu):
    A, b, c, U = synth.dense_ilp(32, 64, 7, 3, 0.4)
    got = trees_with_and_without_the_entry(gpu, lambda: lpgen.load_ilp(gpu, A, b, c, U), max_nodes=2000)
    assert got["polish_calls"] >= 1 and got["polish_moves"] >= 1 and got["polish_improved"] >= 1


def test_tree_on_a_general_fixture_matches_the_twin(gpu):
    # the first drawn fixture whose tree polishes a point that moves (CPU: tests/test_bnb_polish.py closes all of them)
    for rec in DRAWN:
        if rec["status"] != "optimal":
            continue
        inst = instance(rec)
        got = trees_with_and_without_the_entry(gpu, lambda: lpgen.load_milp(gpu, inst), max_nodes=50 * rec["points"] + 1000)
        assert abs(got["best_lower"] - rec["optimum"]) <= 1e-6 * (1 + abs(rec["optimum"]))
        if got["polish_moves"] >= 1:
            return
    raise AssertionError("no general fixture whose tree takes a polishing move")


def test_cli_polish_on_f1(gpu):
    import subprocess

    exe = os.path.join(ROOT, "mvolps_amd", "bin", "mvolps")
    f1 = os.path.join(ROOT, "tests", "golden", "f1.lp")
    plain = subprocess.run([exe, "-f", f1, "--repaired", "-v"], capture_output=True, text=True)
    r = subprocess.run([exe, "-f", f1, "--repaired", "-v", "--heur", "2", "--polish"], capture_output=True, text=True)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    assert "Incumbent polishing:" in r.stdout and "Incumbent polishing:" not in plain.stdout
    for out in (plain.stdout, r.stdout):  # the pinned optimum of F1
        line = [ln for ln in out.splitlines() if "Solution is:" in ln]
        assert len(line) == 1 and float(line[0].rsplit(" = ", 1)[1]) == 35.0, out
