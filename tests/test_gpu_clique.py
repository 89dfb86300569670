"""GPU: the conflict graph on the device (k_conflict_rows / k_conflict through mvx_conflict_graph) against the host twin through
the engine's own table (mvx_bnb_conflict_graph), every word and the edge count, and clique-cut trees on the HIP engine against
the same driver over the oracle's table."""
import math

import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import CV, DB, FR, FX, IV, LO, UP

from . import lpgen
from .test_bnb_clique import COUNTERS, load_variants, mixed_models
from .test_bnb_host import same_result

pytestmark = pytest.mark.gpu

RND_NMAX = 4096  # mvx_internal.hpp: the columns k_prop holds; k_conflict keeps nothing per column and has no such limit


def device_vs_twin(P):
    """One mvx_conflict_graph call against mvx_bnb_conflict_graph on the same handle: all words and the edge count."""
    rc, words, edges = bnb.conflict_words(P)
    trc, twords, tedges = bnb.conflict_words(P, table=None)
    assert rc == trc == 0 and edges == tedges, (rc, trc, edges, tedges)
    assert np.array_equal(words, twords), np.argwhere(words != twords)[:4]
    assert not words[0].any() and not (words[:, 0] & np.uint64(1)).any()
    return edges


def test_mixed_kinds_general_models(gpu):
    rng = np.random.default_rng(20261019)
    edges = with_edge = handles = 0
    for A, row_b, col_b, kinds, c, d, variants in mixed_models(rng, 80):
        for P, _l, _u in load_variants(gpu, A, row_b, col_b, kinds, c, d, variants):
            e = device_vs_twin(P)
            edges += e
            with_edge += e > 0
            handles += 1
    assert handles > 200 and with_edge >= 10 and edges >= 30, (handles, with_edge, edges)


def sized_model(gpu, rng, m, n, dens):
    """test_gpu_prop.sized_model's recipe with most integer columns boxed to [0, 1] and rows a few units from their least / largest
    activity, so that pairs of binaries collide: integer data, every bound type on the rows."""
    A = np.round(rng.normal(size=(m, n)) * 3)
    A[rng.random((m, n)) >= dens] = 0
    kinds, col_b = [], []
    for j in range(n):
        kinds.append(IV if rng.random() < 0.9 else CV)
        if kinds[-1] == IV and rng.random() < 0.9:
            col_b.append((DB, 0.0, 1.0))
        else:
            t = DB if rng.random() < 0.8 else int(rng.choice([LO, UP, FR]))
            lo = float(rng.integers(-2, 2))
            col_b.append((t, lo, lo + float(rng.integers(1, 4))))
    clo, chi = lpgen.bounds_arrays(col_b)
    pos, neg = np.maximum(A, 0), np.minimum(A, 0)
    with np.errstate(invalid="ignore"):
        lmin = np.where(pos != 0, pos * clo, 0).sum(axis=1) + np.where(neg != 0, neg * chi, 0).sum(axis=1)
        lmax = np.where(pos != 0, pos * chi, 0).sum(axis=1) + np.where(neg != 0, neg * clo, 0).sum(axis=1)
    row_b = []
    for i in range(m):
        t = int(rng.choice([LO, UP, DB, FR], p=[0.3, 0.4, 0.2, 0.1]))
        lo = float(lmax[i] - rng.integers(2, 7)) if math.isfinite(lmax[i]) else 0.0
        hi = float(lmin[i] + rng.integers(2, 7)) if math.isfinite(lmin[i]) else 0.0
        if t == DB and lo >= hi:
            t = UP
        row_b.append((t, lo, hi))
    P = gpu.create()
    P.load_general(A, row_b, col_b, np.ones(n), kinds=kinds)
    return P


# the word and wave boundaries at 7 rows; one row, rows around one pass of k_conflict_rows' workgroup and several of them at 48
# columns; the widest model of the other node kernels and one column beyond it
SHAPES = [(7, 63, 0.5), (7, 64, 0.5), (7, 65, 0.5), (7, 130, 0.5), (1, 48, 0.6), (255, 48, 0.2), (257, 48, 0.2), (1100, 48, 0.2),
          (6, RND_NMAX, 0.002), (6, RND_NMAX + 1, 0.002)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % (s[0], s[1]))
def test_sizes_where_the_kernel_takes_another_path(gpu, shape):
    m, n, dens = shape
    P = sized_model(gpu, np.random.default_rng(1000 * m + n), m, n, dens)
    assert device_vs_twin(P) > 0
    # a clone with a few binaries fixed: they leave B, their terms move into the activities
    Q = P.copy()
    fixed = 0
    for j in range(1, n + 1):
        if gpu.get_col_kind(Q.h, j) != CV and gpu.get_col_lb(Q.h, j) == 0.0 and gpu.get_col_ub(Q.h, j) == 1.0 and fixed < 3:
            gpu.set_col_bnds(Q.h, j, FX, float(fixed % 2), float(fixed % 2))
            fixed += 1
    assert fixed == 3
    device_vs_twin(Q)
    device_vs_twin(P)  # the first handle's model is still its own


def test_no_binary_column(gpu):
    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    P = lpgen.load_ilp(gpu, A, b, c, U)
    rc, words, edges = bnb.conflict_words(P)
    assert rc == 0 and edges == 0 and not words.any()
    assert device_vs_twin(P) == 0


def test_dense_binary_sample(gpu):
    """The test_gpu_prop sample (128 x 256, cap 0.01): almost every pair is a conflict."""
    A, b, c, U = synth.dense_ilp(128, 256, 7, 1, 0.01)
    P = lpgen.load_ilp(gpu, A, b, c, U)
    edges = device_vs_twin(P)
    assert edges > 0.99 * 256 * 255 / 2
    P.simplex()
    assert device_vs_twin(P) == edges  # solved or not


def test_argument_errors(gpu):
    L = bnb.lib()
    A, b, c, U = synth.dense_ilp(8, 16, 3, 1, 0.1)
    P = lpgen.load_ilp(gpu, A, b, c, U)
    words = np.zeros((17, 1), dtype=np.uint64)
    edges = bnb.C.c_longlong(0)
    UP_ = bnb.C.POINTER(bnb.C.c_ulonglong)
    assert L.mvx_conflict_graph(None, words.ctypes.data_as(UP_), bnb.C.byref(edges)) == -1
    assert L.mvx_conflict_graph(P.h, None, bnb.C.byref(edges)) == -1
    assert L.mvx_conflict_graph(P.h, words.ctypes.data_as(UP_), None) == -1
    assert L.mvx_bnb_conflict_graph(None, None, words.ctypes.data_as(UP_), bnb.C.byref(edges)) == -1
    # k_conflict has no size limit: there is no -5 (SHAPES holds the model one column beyond the other node kernels' 4096)
    assert L.mvx_conflict_graph(P.h, words.ctypes.data_as(UP_), bnb.C.byref(edges)) == 0


@pytest.mark.parametrize("fam", [2, 3])
@pytest.mark.parametrize("case", [(24, 48, 5, 1, 0.06), (32, 64, 7, 1, 0.03)], ids=lambda c: "%dx%d_cap%g" % (c[0], c[1], c[4]))
def test_trees_match_the_oracle_table(gpu, orc, case, fam):
    tab = bnb.table_from(orc)
    A, b, c, U = synth.dense_ilp(*case)
    kw = dict(quirks=0, cut_rounds=5, cut_families=fam, window=64)
    got = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), **kw)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, **kw)
    assert got["rc"] == ref["rc"] == 0
    same_result(got, ref)
    for k in COUNTERS:  # the loop's counters and, bit for bit, the root LP before and after the loop
        assert got[k] == ref[k], k
    assert got["cutloop_clique_rows"] >= 1 and got["cutloop_conflicts"] > 0


def test_cli_cut_families_on_a_binary_model(gpu, tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "mvolps_amd", "bin", "mvolps")
    A, b, c, U = synth.dense_ilp(24, 48, 5, 1, 0.06)
    path = str(tmp_path / "binary.lp")
    n = len(c)
    with open(path, "w") as f:  # max c x, A x <= b, x binary, in the CPLEX LP dialect of tests/golden/f1.lp
        f.write("Maximize\n obj: " + " + ".join("%.17g x%d" % (c[j], j + 1) for j in range(n)) + "\nSubject To\n")
        for i in range(len(b)):
            f.write(" r%d: " % (i + 1) + " + ".join("%.17g x%d" % (A[i, j], j + 1) for j in range(n)) + " <= %.17g\n" % b[i])
        f.write("Binary\n " + " ".join("x%d" % (j + 1) for j in range(n)) + "\nEnd\n")
    assert U == 1.0
    plain = subprocess.run([exe, "-f", path, "--repaired", "-v", "--cut-rounds"], capture_output=True, text=True)
    r = subprocess.run([exe, "-f", path, "--repaired", "-v", "--cut-rounds", "--cut-families", "3"], capture_output=True, text=True)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    assert "Clique cuts: 1087 conflicts," in r.stdout and "Clique cuts:" not in plain.stdout
