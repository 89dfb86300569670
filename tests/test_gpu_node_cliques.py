"""GPU: clique cuts in the tree (DESIGN.md "Clique cuts in the tree (node_cliques)").  k_cliquesep through mvx_clique_cuts_many
against the host twin mvx_bnb_clique_masks through the engine's own table: every count, word and sum.  The LP points are
controlled: a node handle is a copy of the root with its rows set free and every column fixed at a chosen value, solved (no
pivot), so its column values are what the test wrote.  Then the call's purity, the cached graph behind a bound edit of the
root, whole trees against the same driver over the oracle's table and over the engine's table without the two new entries,
argument errors and the command line."""
import os
import subprocess

import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import DB, FR, FX, IV, OPT, UP

from . import lpgen
from .test_bnb_host import same_result
from .test_gpu_clique import RND_NMAX, sized_model
from .test_gpu_purge import bits, state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clique_model(gpu, n, cliques):
    """n binary columns and one row sum_{j in C} x_j <= 1 per clique C (1-based columns): the graph is the union of the cliques."""
    A = np.zeros((max(1, len(cliques)), n))
    for i, C in enumerate(cliques):
        A[i, np.asarray(C) - 1] = 1.0
    P = gpu.create()
    P.load_general(A, [(UP, 0.0, 1.0)] * A.shape[0], [(DB, 0.0, 1.0)] * n, np.ones(n), kinds=[IV] * n)
    return P


def node(gpu, root, x):
    """A solved handle with root's columns whose values are x[1..n]."""
    P = root.copy()
    for i in range(1, P.m + 1):
        gpu.set_row_bnds(P.h, i, FR, 0.0, 0.0)
    for j in range(1, P.n + 1):
        gpu.set_col_bnds(P.h, j, FX, float(x[j]), float(x[j]))
    assert P.simplex() == 0 and P.status == OPT
    return P


def points(rng, n, count):
    out = []
    for t in range(count):
        x = np.round(rng.random(n + 1) * 4) / 4 * (rng.random(n + 1) < 0.7)  # ties and zeros
        if t % 3 == 0:
            x = x * rng.random(n + 1)
        x[0] = 0.0
        out.append(x)
    return out


def device_vs_twin(root, nodes, max_cuts):
    """One mvx_clique_cuts_many call against mvx_bnb_clique_masks handle by handle: (cnt, q, sum) of the device."""
    rc, cnt, q, s = bnb.clique_cuts_many(root, nodes, max_cuts)
    trc, tcnt, tq, ts = bnb.clique_cuts_many(root, nodes, max_cuts, table=None)
    assert rc == trc == 0, (rc, trc)
    assert np.array_equal(cnt, tcnt), (cnt, tcnt)
    assert np.array_equal(q, tq), np.argwhere(q != tq)[:4]
    assert np.array_equal(bits(s), bits(ts)), np.argwhere(s != ts)[:4]
    for t in range(len(nodes)):
        assert not q[t, cnt[t]:].any() and not s[t, cnt[t]:].any()  # the slots behind the kept ones are zero
    assert not (q[:, :, 0] & np.uint64(1)).any()
    return cnt, q, s


# ------------------------------------------------------------------------------------------------ device against twin


@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_word_and_lane_boundaries(gpu, n):
    rng = np.random.default_rng(7000 + n)
    root = sized_model(gpu, rng, 7, n, 0.5)
    nodes = [node(gpu, root, x) for x in points(rng, n, 6)]
    kept = 0
    for max_cuts in (8, 1):
        kept += int(device_vs_twin(root, nodes, max_cuts)[0].sum())
    assert kept >= 4, kept
    # all values equal: the order is by column
    same = node(gpu, root, np.concatenate([[0.0], np.full(n, 0.375)]))
    assert device_vs_twin(root, [same], 8)[0][0] >= 1


def test_widest_model_and_one_column_beyond(gpu):
    rng = np.random.default_rng(6 * 1000 + RND_NMAX)
    root = sized_model(gpu, rng, 6, RND_NMAX, 0.002)
    xs = points(rng, RND_NMAX, 2)
    _rc, words, edges = bnb.conflict_words(root)
    assert edges >= 1  # a sparse graph: the few columns with a neighbour sit at 0.75, so every edge is violated
    xs[1][np.flatnonzero(words.any(axis=1))] = 0.75
    cnt, _q, _s = device_vs_twin(root, [node(gpu, root, x) for x in xs], 16)
    assert cnt[1] >= 1
    wide = sized_model(gpu, rng, 6, RND_NMAX + 1, 0.002)
    rc, _c, _q2, _s2 = bnb.clique_cuts_many(wide, [wide], 4)
    assert rc == -5


def test_complete_graph_every_seed_gives_the_same_set(gpu):
    """40 positive columns in one clique row: 40 seeds, ten batches of a workgroup, one set kept."""
    root = clique_model(gpu, 48, [list(range(1, 41))])
    x = np.zeros(49)
    x[1:41] = 0.05 + np.arange(40) * 1e-3
    cnt, q, s = device_vs_twin(root, [node(gpu, root, x)], 64)
    assert cnt[0] == 1 and q[0, 0, 0] == np.uint64(((1 << 41) - 1) & ~1)
    assert device_vs_twin(root, [node(gpu, root, x)], 1)[0][0] == 1


def test_zero_and_1e6_values_are_no_seeds_but_join(gpu):
    root = clique_model(gpu, 6, [[1, 2, 3, 4], [5, 6]])
    x = np.array([0.0, 0.6, 0.6, 0.0, 1e-6, 0.0, 0.0])
    cnt, q, s = device_vs_twin(root, [node(gpu, root, x)], 8)
    assert cnt[0] == 1 and q[0, 0, 0] == 0b11110 and s[0, 0] == 0.6 + 0.6 + 0.0 + 1e-6
    # nothing above 1e-6: no seed at all, although the columns would form a clique
    x = np.array([0.0, 1e-6, 1e-6, 0.0, 1e-6, 1e-6, 0.0])
    assert device_vs_twin(root, [node(gpu, root, x)], 8)[0][0] == 0


def test_violation_a_few_ulps_either_side_of_1e6(gpu):
    root = clique_model(gpu, 2, [[1, 2]])
    base = 0.5 + 1e-6
    cands = [base]
    for _ in range(6):
        cands.append(np.nextafter(cands[-1], 1.0))
    lo = base
    for _ in range(6):
        lo = np.nextafter(lo, 0.0)
        cands.append(lo)
    nodes = [node(gpu, root, np.array([0.0, 0.5, v])) for v in cands]
    cnt, _q, s = device_vs_twin(root, nodes, 4)
    want = [1 if (0.5 + float(v)) - 1.0 > 1e-6 else 0 for v in cands]
    assert cnt.tolist() == want and 0 < sum(want) < len(want), (cnt.tolist(), want)
    for t, v in enumerate(cands):
        if want[t]:
            assert s[t, 0] == 0.5 + float(v)


@pytest.mark.parametrize("max_cuts", [1, 64])
def test_more_violated_cliques_than_max_cuts(gpu, max_cuts):
    n = 140
    root = clique_model(gpu, n, [[2 * i + 1, 2 * i + 2] for i in range(70)])
    x = np.concatenate([[0.0], 0.6 + np.arange(n) * 1e-4])
    cnt, q, _s = device_vs_twin(root, [node(gpu, root, x)], max_cuts)
    assert cnt[0] == max_cuts
    assert len({q[0, c].tobytes() for c in range(max_cuts)}) == max_cuts  # distinct sets


def test_seventy_handles_with_other_row_counts_and_no_seeds(gpu):
    rng = np.random.default_rng(70)
    n = 65
    root = sized_model(gpu, rng, 7, n, 0.5)
    nodes = []
    for t, x in enumerate(points(rng, n, 70)):
        if t % 7 == 3:
            x = np.zeros(n + 1)  # no seed at all
        P = node(gpu, root, x)
        if t % 5 == 1:  # cut rows of its own: another row count, the same column values
            k = 1 + t % 3
            vals = np.zeros((k, n + 1))
            vals[:, 1 + t % n] = -1.0
            assert bnb.add_cut_rows(P, vals, np.full(k, -10.0)) == 0
            assert P.simplex() == 0 and P.status == OPT and P.m == root.m + k
        nodes.append(P)
    cnt, _q, _s = device_vs_twin(root, nodes, 4)
    assert (cnt > 0).sum() >= 10 and (cnt == 0).sum() >= 10, cnt.tolist()
    # a call with one handle of the batch gives that handle's slice
    one = device_vs_twin(root, [nodes[6]], 4)
    many = bnb.clique_cuts_many(root, nodes, 4)
    assert np.array_equal(one[1][0], many[2][6]) and one[0][0] == many[1][6]


def test_empty_graph(gpu):
    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    root = lpgen.load_ilp(gpu, A, b, c, U)
    assert bnb.conflict_words(root)[2] == 0
    P = root.copy()
    assert P.simplex() == 0 and P.status == OPT
    cnt, q, s = device_vs_twin(root, [P, P.copy()], 8)
    assert not cnt.any() and not q.any() and not s.any()


# ------------------------------------------------------------------------------------------------ purity, the cached graph


def test_the_call_changes_no_handle(gpu):
    A, b, c, U = synth.dense_ilp(24, 48, 5, 1, 0.06)
    root = lpgen.load_ilp(gpu, A, b, c, U)
    nodes = bnb.node_sample(root, 8, quirks=0)
    assert len(nodes) == 8
    before = [(P.status, P.it_cnt, P.m) + tuple(x.copy() for x in state(P)) for P in nodes]
    cnt, _q, _s = device_vs_twin(root, nodes, 4)
    assert cnt.sum() >= 1
    for P, old in zip(nodes, before):
        new = (P.status, P.it_cnt, P.m) + state(P)
        assert new[:3] == old[:3]
        assert np.array_equal(bits(new[3]), bits(old[3])) and all(np.array_equal(a, b) for a, b in zip(new[4:], old[4:]))
    assert root.status != OPT and root.m == 24  # the root was never solved, and is not now


def test_cached_graph_follows_a_bound_edit_of_the_root(gpu):
    rng = np.random.default_rng(65)
    n = 65
    root = sized_model(gpu, rng, 7, n, 0.5)
    nodes = [node(gpu, root, x) for x in points(rng, n, 6)]
    first = device_vs_twin(root, nodes, 8)
    _rc, words, _e = bnb.conflict_words(root)
    busiest = int(np.argmax(bnb.words_to_bool(words, n).sum(axis=1)))
    gpu.set_col_bnds(root.h, busiest, FX, 0.0, 0.0)  # it leaves the graph, with all its edges
    _rc, words2, _e2 = bnb.conflict_words(root)
    assert not words2[busiest].any() and words[busiest].any()
    second = device_vs_twin(root, nodes, 8)  # against the twin on the edited root
    assert not np.array_equal(first[1], second[1])
    assert not (bnb.words_to_bool(second[1].reshape(-1, second[1].shape[2]), n)[:, busiest]).any()
    # and a second call on the unchanged root gives the same answer (the graph it kept)
    third = device_vs_twin(root, nodes, 8)
    assert np.array_equal(second[1], third[1]) and np.array_equal(second[0], third[0])


def test_argument_errors(gpu):
    L = bnb.lib()
    C = bnb.C
    root = clique_model(gpu, 6, [[1, 2, 3]])
    x = np.array([0.0, 0.6, 0.6, 0.0, 0.0, 0.0, 0.0])
    P = node(gpu, root, x)
    other = node(gpu, clique_model(gpu, 7, [[1, 2, 3]]), np.append(x, 0.0))
    IP, UP_, DP = C.POINTER(C.c_int), C.POINTER(C.c_ulonglong), C.POINTER(C.c_double)
    cnt, q, s = np.full(2, 7, dtype=np.int32), np.zeros((2, 64, 1), dtype=np.uint64), np.zeros((2, 64))
    cp, qp, sp = cnt.ctypes.data_as(IP), q.ctypes.data_as(UP_), s.ctypes.data_as(DP)
    hs = (C.c_void_p * 2)(P.h, P.h)
    call = L.mvx_clique_cuts_many
    assert call(None, hs, 2, 4, cp, qp, sp) == -1 and call(root.h, None, 2, 4, cp, qp, sp) == -1
    assert call(root.h, hs, 2, 4, None, qp, sp) == -1 and call(root.h, hs, 2, 4, cp, None, sp) == -1
    assert call(root.h, hs, 2, 4, cp, qp, None) == -1 and call(root.h, hs, -1, 4, cp, qp, sp) == -1
    for k in (0, -1, 65):
        assert call(root.h, hs, 2, k, cp, qp, sp) == -1
    assert call(root.h, (C.c_void_p * 2)(P.h, None), 2, 4, cp, qp, sp) == -1
    assert call(root.h, (C.c_void_p * 2)(P.h, other.h), 2, 4, cp, qp, sp) == -1  # another column count
    assert call(root.h, (C.c_void_p * 2)(P.h, root.h), 2, 4, cp, qp, sp) == -3  # the root is not solved
    assert cnt.tolist() == [7, 7] and not q.any() and not s.any()  # nothing was written
    assert call(root.h, hs, 0, 4, cp, qp, sp) == 0 and call(root.h, None, 0, 4, None, None, None) == 0 and cnt.tolist() == [7, 7]
    assert call(root.h, hs, 2, 64, cp, qp, sp) == 0 and cnt.tolist() == [1, 1] and q[0, 0, 0] == 0b1110 and s[1, 0] == 1.2


# ------------------------------------------------------------------------------------------------ trees

CASES = [(24, 48, 5, 1, 0.06), (32, 64, 7, 1, 0.05)]
MODES = {"plain": dict(), "node_purge": dict(node_purge=2), "cut_strat": dict(cut_strat=1)}
COUNTERS = bnb.NODE_CLIQUE_COUNTERS + bnb.NODE_PURGE_COUNTERS
_TREES = {}


def engine_tree(gpu, case, mode):
    if (case, mode) not in _TREES:
        A, b, c, U = synth.dense_ilp(*case)
        _TREES[case, mode] = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), quirks=0, node_cliques=4, window=64, **MODES[mode])
    return _TREES[case, mode]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_cap%g" % (c[0], c[1], c[4]))
def test_trees_match_the_oracle_table(gpu, orc, case, mode):
    """The engine's driver against the same driver over the oracle's table, bit for bit.  With node_purge the oracle's table has
    no del_rows, so its driver purges a row by making it a free row: the same LP, not the same bits as the engine's deletion
    (DESIGN.md "Cut purging in the tree (node_purge)").  Measured on 32x64 cap 0.05 with node_purge = 2: the two trees agree in
    every node, label, pivot count and counter, and their event streams first differ in the last bit of a sum of infeasibilities
    (event 541: 2.640270880849954 where the engine deletes, 2.6402708808499544 where the oracle frees).  So in that mode the bit-for-bit
    comparison gives the engine's driver the oracle's purge path (its table without del_rows and del_rows_many), and the tree of
    the engine's own path is compared with the oracle's in everything but the bits of the LP values."""
    A, b, c, U = synth.dense_ilp(*case)
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bnb.table_from(orc), quirks=0, node_cliques=4, window=64, **MODES[mode])
    own = engine_tree(gpu, case, mode)
    got = own
    if "node_purge" in MODES[mode]:
        table = bnb.table_from(gpu)
        table.del_rows = table.del_rows_many = None
        got = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), table=table, quirks=0, node_cliques=4, window=64, **MODES[mode])
        for k in ("n_nodes", "parent", "prune", "count", "has_incumbent", "incumbent_oid", "hit_limit", "total_pivots") + COUNTERS:
            assert own[k] == ref[k], k
        assert np.allclose(own["node_bound"], ref["node_bound"], rtol=1e-9, atol=1e-9) and np.allclose(own["x"], ref["x"], atol=1e-9)
    assert got["rc"] == ref["rc"] == own["rc"] == 0
    same_result(got, ref)
    for k in COUNTERS:
        assert got[k] == ref[k], k
    assert got["node_clique_rows"] >= 1 and got["node_clique_conflicts"] > 0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_cap%g" % (c[0], c[1], c[4]))
def test_fallbacks_give_the_same_tree(gpu, case, mode):
    """The engine's table without clique_cuts_many and add_cut_rows_many: the twin separates, add_cut_rows appends."""
    table = bnb.table_from(gpu)
    assert bnb.table_entry(table, "clique_cuts_many") and bnb.table_entry(table, "add_cut_rows_many") and table.add_cut_rows
    bnb.set_table_entry(table, "clique_cuts_many", None)
    bnb.set_table_entry(table, "add_cut_rows_many", None)
    A, b, c, U = synth.dense_ilp(*case)
    got = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), table=table, quirks=0, node_cliques=4, window=64, **MODES[mode])
    ref = engine_tree(gpu, case, mode)
    assert got["rc"] == 0
    same_result(got, ref)
    for k in COUNTERS:
        assert got[k] == ref[k], k
    if mode == "plain":  # and row by row, and the serial driver
        table.add_cut_rows = None
        for w in (64, 1):
            got = bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), table=table, quirks=0, node_cliques=4, window=w)
            same_result(got, ref)
        same_result(bnb.branch_and_bound(lpgen.load_ilp(gpu, A, b, c, U), quirks=0, node_cliques=4, window=1), ref)


def test_cli_node_cliques_on_a_binary_model(gpu, tmp_path):
    exe = os.path.join(ROOT, "mvolps_amd", "bin", "mvolps")
    A, b, c, U = synth.dense_ilp(24, 48, 5, 1, 0.06)
    path = str(tmp_path / "binary.lp")
    n = len(c)
    with open(path, "w") as f:  # max c x, A x <= b, x binary, in the CPLEX LP dialect of tests/golden/f1.lp
        f.write("Maximize\n obj: " + " + ".join("%.17g x%d" % (c[j], j + 1) for j in range(n)) + "\nSubject To\n")
        for i in range(len(b)):
            f.write(" r%d: " % (i + 1) + " + ".join("%.17g x%d" % (A[i, j], j + 1) for j in range(n)) + " <= %.17g\n" % b[i])
        f.write("Binary\n " + " ".join("x%d" % (j + 1) for j in range(n)) + "\nEnd\n")
    assert U == 1.0
    plain = subprocess.run([exe, "-f", path, "--repaired", "-v"], capture_output=True, text=True)
    r = subprocess.run([exe, "-f", path, "--repaired", "-v", "--node-cliques"], capture_output=True, text=True)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    assert "Node cliques:" not in plain.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Node cliques:")]
    assert len(line) == 1 and line[0].startswith("Node cliques: 1087 conflicts, "), r.stdout
    assert int(line[0].split()[-2]) >= 1  # R of "E conflicts, C nodes separated, R rows"
