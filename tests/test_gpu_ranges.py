"""GPU: sensitivity ranges on the device (k_rangecols / k_rangefin / k_rangerows through mvx_ranges) against the host twin through
the engine's own table (mvx_bnb_ranges), bit for bit, on the shapes where the kernels can go wrong: column strips of 64 either
side of a boundary, one row, row counts either side of the row chunk and beyond two chunks, ties across a chunk boundary and
across the waves' row interleave, a column of zeros; then the call's purity, its error codes, the certificates by re-solving on
the engine, and the command line."""
import os
import subprocess

import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import DB, FX, MAX, MIN, OPT, UP

from . import lpgen
from .test_gpu_polish import general_sized
from .test_ranges import (activity_certificates, cost_certificates, np_ranges, parse_report, same_bits, tie_model, ties_go_to_the_lower_row,
                          zero_column_model)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = bnb.ranges_chunk()


def device_vs_twin(P):
    rc, val, var = bnb.ranges(P)
    trc, tval, tvar = bnb.ranges(P, table=None)
    assert rc == trc == 0
    assert same_bits(val, tval), np.argwhere(val != tval)[:4]
    assert same_bits(var, tvar), np.argwhere(var != tvar)[:4]
    assert not val[0].any() and not var[0].any()
    prc, pval, pvar = P.ranges()  # the handle's own method is the same call
    assert prc == 0 and same_bits(pval, val) and same_bits(pvar, var)
    return val, var


def solved_general(gpu, m, n, direction):
    """general_sized's model; a draw whose LP is unbounded gets the box of its other columns on its LO / UP / FR columns."""
    rng = np.random.default_rng(20261020 + 7 * n + 31 * m + direction)
    P, _x0 = general_sized(gpu, rng, m, n, direction)
    P.simplex()
    if P.status != OPT:
        for j in range(1, n + 1):
            P.api.set_col_bnds(P.h, j, DB, -1.0, 4.5)
        P.simplex()
    assert P.status == OPT
    return P


@pytest.mark.parametrize("m", [1, 3, 70, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
@pytest.mark.parametrize("n", [5, 63, 64, 65, 129])
def test_device_matches_twin(gpu, n, m):
    for U in (1, 3):
        P = lpgen.load_ilp(gpu, *synth.dense_ilp(m, n, 11 + n + m, U, 0.4))
        P.simplex()
        assert P.status == OPT
        device_vs_twin(P)
    for direction in (MIN, MAX):
        device_vs_twin(solved_general(gpu, m, n, direction))


def test_restatement_on_the_engine(gpu):
    """The independent restatement once on the engine's own tableau (the CPU file runs it over the oracle's)."""
    P = solved_general(gpu, 70, 65, MIN)
    val, var = device_vs_twin(P)
    rval, rvar = np_ranges(P)
    assert same_bits(val, rval) and same_bits(var, rvar)


@pytest.mark.parametrize("shape", ["rows 6 apart", "rows a chunk apart", "adjacent rows"])
def test_ties(gpu, shape):
    if shape == "rows 6 apart":
        P = tie_model(gpu)
    elif shape == "rows a chunk apart":  # a row in one chunk, its copy at the same place in the next: k_rangefin decides
        P = tie_model(gpu, m=CHUNK, n=8, seed=6)
    else:  # a row and its copy in two waves of one workgroup: the LDS combine decides
        P = tie_model(gpu, m=40, n=8, seed=6, adjacent=True)
    P.simplex()
    assert P.status == OPT
    val, var = device_vs_twin(P)
    assert ties_go_to_the_lower_row(P, val, var) >= 4


@pytest.mark.parametrize("direction", [MAX, MIN], ids=["max", "min"])
def test_a_column_of_zeros(gpu, direction):
    P = zero_column_model(gpu, direction)
    P.simplex()
    assert P.status == OPT
    val, var = device_vs_twin(P)
    inf = np.inf
    assert list(val[P.m + 3]) == [inf, inf, 0.0, 0.0, 0.0, 0.0] and list(var[P.m + 3]) == [0, 0, 0, 0]
    assert list(val[P.m + 5, :4]) == [inf, inf, inf, inf] and list(var[P.m + 5]) == [0, 0, 0, 0]


def test_the_call_is_pure(gpu):
    P = lpgen.load_ilp(gpu, *synth.dense_ilp(24, 48, 5, 3, 0.3))
    P.simplex()
    assert P.status == OPT
    untouched = P.copy()
    tab0, basis0, obj0, it0 = P.tableau(), P.basis(), P.obj, P.it_cnt
    device_vs_twin(P)
    assert P.status == OPT and P.obj == obj0 and P.it_cnt == it0
    assert np.array_equal(P.tableau(), tab0)
    assert all(np.array_equal(a, b) for a, b in zip(P.basis(), basis0))
    x = P.col_prim()
    j = int(np.flatnonzero(np.abs(x - np.round(x)) > 1e-6)[0]) + 1  # a fractional column: its down branch takes a pivot
    kids = []
    for src in (P, untouched):
        ch = src.copy()
        ch.api.set_col_bnds(ch.h, j, UP, 0.0, float(np.floor(x[j - 1])))
        ch.simplex()
        kids.append(ch)
    assert kids[0].status == kids[1].status and kids[0].it_cnt == kids[1].it_cnt > it0
    assert same_bits(kids[0].tableau(), kids[1].tableau())
    assert all(np.array_equal(a, b) for a, b in zip(kids[0].basis(), kids[1].basis()))


def test_error_codes_and_a_tiny_model(gpu):
    L = bnb.lib()
    DP, IP = bnb.C.POINTER(bnb.C.c_double), bnb.C.POINTER(bnb.C.c_int)
    P = lpgen.load_ilp(gpu, *synth.dense_ilp(8, 16, 3, 1, 0.3))
    assert bnb.ranges(P)[0] == -3 and bnb.ranges(P, table=None)[0] == -3  # never solved
    P.simplex()
    assert P.status == OPT
    val, var = np.zeros((P.m + P.n + 1, 6)), np.zeros((P.m + P.n + 1, 4), dtype=np.int32)
    assert L.mvx_ranges(None, val.ctypes.data_as(DP), var.ctypes.data_as(IP)) == -1
    assert L.mvx_ranges(P.h, None, var.ctypes.data_as(IP)) == -1
    assert L.mvx_ranges(P.h, val.ctypes.data_as(DP), None) == -1
    assert not val.any() and not var.any()
    Q = P.copy()
    Q.api.set_col_bnds(Q.h, 1, DB, 0.0, 0.5)  # a bound edited after the solve
    assert bnb.ranges(Q)[0] == -3 and bnb.ranges(Q, table=None)[0] == -3
    device_vs_twin(P)
    one = gpu.create()
    one.load_dense(*synth.dense_lp(1, 1, 4))
    one.simplex()
    assert one.status == OPT
    val, _var = device_vs_twin(one)
    assert val.shape == (3, 6)


def test_certificates_by_resolving_on_the_engine(gpu):
    P = lpgen.load_ilp(gpu, *synth.dense_ilp(24, 48, 5, 3, 0.3))
    P.simplex()
    assert P.status == OPT
    val, var = device_vs_twin(P)
    checked, beyond, left = activity_certificates(P, val, var)
    assert checked >= 20 and beyond >= 1 and left <= 0.1 * checked, (checked, beyond, left)
    checked, beyond, left = cost_certificates(P, val, var)
    assert checked >= 10 and beyond >= 1 and left <= 0.1 * checked, (checked, beyond, left)


def test_cli_ranges_on_f1(gpu, tmp_path):
    exe = os.path.join(ROOT, "mvolps_amd", "bin", "mvolps")
    f1 = os.path.join(ROOT, "tests", "golden", "f1.lp")
    report = str(tmp_path / "f1.ranges")
    plain = subprocess.run([exe, "-f", f1, "--repaired", "-v"], capture_output=True, text=True)
    r = subprocess.run([exe, "-f", f1, "--repaired", "-v", "--ranges", report], capture_output=True, text=True)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    assert r.stdout == plain.stdout  # the flag changes nothing else about the run
    line = [ln for ln in r.stdout.splitlines() if "Solution is:" in ln]
    assert len(line) == 1 and float(line[0].rsplit(" = ", 1)[1]) == 35.0, r.stdout  # the pinned optimum of F1
    # the same root here: read, bounds rounded as the repaired driver does, solved; the twin's numbers through the same printer
    L = bnb.lib()
    L.mvx_read_lp.restype = bnb.C.c_int
    L.mvx_read_lp.argtypes = [bnb.C.c_void_p, bnb.C.c_void_p, bnb.C.c_char_p]
    P = gpu.create()
    assert L.mvx_read_lp(P.h, None, f1.encode()) == 0
    bnb.integral_bounds(P)
    P.simplex()
    assert P.status == OPT
    rc, val, var = bnb.ranges(P, table=None)
    assert rc == 0
    twin = str(tmp_path / "f1.twin")
    assert bnb.print_ranges(P, val, var, path=twin) == 0
    assert open(report).read() == open(twin).read() and len(open(report).read().splitlines()) == P.m + P.n
    pval, pvar, _names, _stats, xs = parse_report(report)
    assert same_bits(pval, val) and same_bits(pvar, var)
    assert xs[1:] == list(P.row_prim()) + list(P.col_prim())
