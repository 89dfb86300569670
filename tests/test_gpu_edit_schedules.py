"""GPU: live tableau edits in every order, values read in between (DESIGN.md "Live edits"), and the device copies of the model
behind model edits.

1. The schedules of tests/edit_schedules.py, each in two observation modes.  tests/test_edit_schedules_inputs.py proves on the
   oracle and the reference that every step finds its targets, that the certificate would notice an entry off by 1e-7 at every
   state, and that the steps which claim to move column 0 move it far beyond the tolerance; the proof carries over because the
   engine's optimal basis of each base is the oracle's, which is asserted first.  After every step the handle is held to the
   reference of the model that was edited alongside and to the expected basis (edit_schedules.check_handle); `quiet` reads nothing
   else, so every edit meets mirrors that the one before left stale, `reads` reads single values and the objective before the
   tableau is fetched, so every edit meets an exported solution and the reads meet whatever `fresh_rows` the edit left.
2. GMI cuts (`dmat`) around model edits, a row rewritten twice among them: the device matrix must not be taken as current by the
   address of a row that was freed and handed out again.
3. mvx_round_many and mvx_dive_pick_many (`rmod`) behind edits of the root, against their host twins on the edited root."""
import collections
import json
import os

import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import CV, DB, IV, LO, MAX, MIN, OPT, UP

from . import certify as cf
from . import edit_schedules as es
from . import lpgen
from .test_bnb_dive import RULES
from .test_gpu_certify import device_cuts

pytestmark = pytest.mark.gpu

COUNTS = collections.Counter()  # (kind, mode) -> steps certified


# ------------------------------------------------------------------------------------------------ 1. the schedules


@pytest.mark.parametrize("mode", es.MODES)
@pytest.mark.parametrize("name", list(es.SCHEDULES))
def test_schedule(gpu, orc, name, mode):
    base, steps = es.SCHEDULES[name]
    P, M = es.solved_base(gpu, base)
    o, _ = es.solved_base(orc, base)
    for got, want in zip(P.basis(), o.basis()):
        assert np.array_equal(got, want)  # the bit parity of engine and oracle: what carries the CPU proof over
    w = es.Walker(es.State(M, P.basis()), P, mode, name, COUNTS)
    for spec in steps:
        w.step(spec)
    w.finish()


# ------------------------------------------------------------------------------------------------ 2. GMI cuts behind model edits


def cut_and_certify(gpu, P, M, what):
    """Solve, cut every eligible column in the repaired mode, certify each cut against M; returns the reference and the columns
    that were cut."""
    assert P.simplex() == 0 and P.status == OPT, what
    ref = cf.certify(M, P, what=what)
    cols = es.cut_columns(ref)
    assert cols, what
    pts = cf.integer_points(M)
    vals, rhs, ok = device_cuts(gpu, P, cols)
    done = []
    for t, j in enumerate(cols):
        if ok[t]:
            cf.certify_gmi(ref, j, vals[t, 1:], rhs[t], pts, what="%s, column %d" % (what, j))
            COUNTS[("gmi cut", "-")] += 1
            done.append(j)
    assert done, what
    return ref, done


def gmi_handle(gpu):
    A, b, c, U, M = es.gmi_model()
    return lpgen.load_ilp(gpu, A, b, c, U), M, A


@pytest.mark.parametrize("i", es.GMI_ROWS)
def test_gmi_cuts_follow_a_row_rewritten_twice(gpu, i):
    """No clone of the handle is alive and no GMI call lies between the two rewrites: the second row object may take the address
    the first rewrite freed, which is the address the device matrix was built from.  With a device matrix that compares bare
    addresses all four rows fail on the device: the cuts of the second solve are back-substituted through the coefficients of the
    first model and differ from the formula by 0.004 to 667."""
    P, M, A = gmi_handle(gpu)
    cut_and_certify(gpu, P, M, "row %d, before" % i)
    first, second = es.gmi_rewrites(A, i)
    ind = es.all_indices(P.n)
    P.set_mat_row(i, ind, np.concatenate([[0.0], first]))
    P.set_mat_row(i, ind, np.concatenate([[0.0], second]))
    R = es.gmi_rewritten(M, i)
    es.check_model(P, R, "row %d rewritten" % i)
    ref, done = cut_and_certify(gpu, P, R, "row %d, after" % i)
    assert es.row_feeds_a_cut(ref, i, done)  # a cut above went through the row's new coefficients


def test_gmi_cuts_follow_column_and_row_edits(gpu):
    P, M, A = gmi_handle(gpu)
    m, n = M.m, M.n
    cut_and_certify(gpu, P, M, "before")
    # add_dense_cols: two integer columns
    rng = np.random.default_rng(3)
    cols = 1.0 + np.floor(rng.random((2, m)) * 20.0)
    obj = np.array([7.0, 12.0])
    assert P.add_dense_cols(cols, obj, [DB, DB], [0.0, 0.0], [2.0, 2.0], kinds=[IV, IV]) == 0
    for t in range(2):
        M.add_col(cols[t], DB, 0.0, 2.0, cost=obj[t], kind=IV)
    es.check_model(P, M, "columns appended")
    cut_and_certify(gpu, P, M, "columns appended")
    # del_cols: an original column and an appended one
    gone = [2, n + 1]
    assert P.del_cols(gone) == 0
    es.reduced_cols(M, gone)
    es.check_model(P, M, "columns deleted")
    cut_and_certify(gpu, P, M, "columns deleted")
    # del_rows of an original row
    assert P.del_rows([3]) == 0
    es.reduced_rows(M, [3])
    es.check_model(P, M, "row deleted")
    cut_and_certify(gpu, P, M, "row deleted")
    # add_cut_rows, del_rows of the last row, add_cut_rows: the last row's number is taken twice
    x = P.col_prim()
    for seed in (5, 6):
        v = np.zeros((2, P.n + 1))
        v[:, 1:] = -1.0 - np.floor(np.random.default_rng(seed).random((2, P.n)) * 5.0)
        rhs = np.floor(v[:, 1:] @ x) - 1.0
        assert bnb.add_cut_rows(P, v, rhs) == 0
        for t in range(2):
            M.add_row(v[t, 1:], LO, float(rhs[t]), 0.0)
        if seed == 5:
            assert P.del_rows([P.m]) == 0
            es.reduced_rows(M, [M.m])
    es.check_model(P, M, "rows appended, deleted, appended")
    cut_and_certify(gpu, P, M, "rows appended, deleted, appended")


# ------------------------------------------------------------------------------------------------ 3. rmod behind edits of the root

RMOD_CASE = (12, 24, 5, 3)  # synth.dense_ilp


def rmod_root(api, table=None):
    A, b, c, U = synth.dense_ilp(*RMOD_CASE)
    root = lpgen.load_ilp(api, A, b, c, U)
    nodes = bnb.node_sample(root, 6, table=table)
    assert len(nodes) == 6
    return root, nodes, A, b, c


def rewrite_twice(root, i, first, second):
    ind = es.all_indices(root.n)
    root.set_mat_row(i, ind, np.concatenate([[0.0], first]))
    root.set_mat_row(i, ind, np.concatenate([[0.0], second]))


def picks(root, nodes, table, device):
    """The picks of every (node, rule) pair from the host twin on the root as it stands; with `device`, mvx_dive_pick_many first,
    held to the twin bit for bit (device_vs_host of test_gpu_dive.py, keeping the answers)."""
    hs = [P for P in nodes for _ in RULES]
    rules = [r for _ in nodes for r in RULES]
    want = []
    for P, r in zip(hs, rules):
        rc, w = bnb.dive_pick_node(P, root, r, table=table)
        assert rc == 0
        want.append(w)
    if device:
        rc, got = bnb.dive_pick_many(root, hs, rules)
        assert rc == 0 and got == want, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:3]
    return want


def dive_edits(root, nodes, A, table=None, device=True):
    """Caches the model with a first call, then edits the root and calls again after every edit; every answer is the twin's on the
    edited root, and it changes where the edit must change it."""
    api, h, m = root.api, root.h, root.m

    def of(ans, node, rule):
        return ans[node * len(RULES) + RULES.index(rule)]

    a0 = picks(root, nodes, table, device)
    assert all(of(a0, t, 1)[0] >= 2 for t in range(len(nodes)))  # two candidates at least in every node: a pick can move
    # set_col_kind: the column rule 1 picks in node 0 becomes continuous -- no candidate any more, one fractional column fewer
    j = of(a0, 0, 1)[1]
    api.set_col_kind(h, j, CV)
    a1 = picks(root, nodes, table, device)
    assert all(of(a1, 0, r)[0] == of(a0, 0, r)[0] - 1 and of(a1, 0, r)[1] != j for r in RULES)
    # set_obj_coef: the column rule 4 picks in node 0 becomes a thousand times as expensive -- its key is the largest now
    j = of(a1, 0, 4)[1]
    api.set_obj_coef(h, j, 1000.0 * api.get_obj_coef(h, j))
    a2 = picks(root, nodes, table, device)
    assert of(a2, 0, 4)[1] != j and of(a2, 0, 1) == of(a1, 0, 1)
    # the direction: every cost is positive, so rule 4 now rounds every pick up instead of down
    assert all(of(a2, t, 4)[2] == 0 for t in range(len(nodes)))
    api.set_obj_dir(h, MIN)
    a3 = picks(root, nodes, table, device)
    assert all(of(a3, t, 4)[2] == 1 for t in range(len(nodes)))
    # a row rewritten twice: in the end row 1 enters the column rule 2 picks in node 0 with the other sign -- the only column with a
    # down-lock, so rule 2 turns to another one
    j = of(a3, 0, 2)[1]
    second = A[0].copy()
    second[j - 1] = -second[j - 1]
    rewrite_twice(root, 1, A[0][::-1].copy(), second)
    a4 = picks(root, nodes, table, device)
    assert of(a4, 0, 2)[1] != j and of(a3, 0, 2)[2] == 0
    # set_row_bnds UP -> DB: row 1 now locks every column both ways, one down-lock each -- rule 2 is back at its first pick
    api.set_row_bnds(h, 1, DB, -1.0e6, api.get_row_ub(h, 1))
    a5 = picks(root, nodes, table, device)
    assert of(a5, 0, 2)[1] == j
    # a second call on the unchanged root: the model it kept
    assert picks(root, nodes, table, device) == a5
    return a0, a5


def roundings(root, nodes, table, device):
    """(obj, found, x) of every node in both modes from the host twin on the root as it stands; with `device`, mvx_round_many first,
    held to the twin bit for bit (device_vs_host of test_gpu_heuristic.py, keeping the answers)."""
    out = []
    for mode in (1, 2):
        got = bnb.round_many(root, nodes, mode) if device else None
        assert not device or got[0] == 0
        for t, P in enumerate(nodes):
            hrc, hobj, hf, hx = bnb.round_node(P, root, mode, table=table)
            assert hrc == 0
            if device:
                _rc, obj, fnd, x = got
                assert obj[t] == hobj and fnd[t] == hf and np.array_equal(x[t, 1:], hx[1:]), (mode, t, obj[t], hobj, fnd[t], hf)
            out.append((hobj, hf, hx[1:].copy()))
    return out


def changed(a, b):
    return [k for k, (u, v) in enumerate(zip(a, b)) if not (u[0] == v[0] and u[1] == v[1] and np.array_equal(u[2], v[2]))]


def round_edits(root, nodes, A, table=None, device=True):
    api, h, n = root.api, root.h, root.n
    k = len(nodes)
    r0 = roundings(root, nodes, table, device)
    assert all(f == 1 for _, f, _ in r0[k:])  # the greedy fill of mode 2 finds a point in every node
    # set_obj_coef: a column at 1 or more in node 0's filled point costs 1000 more -- the objective of that point follows
    x0 = r0[k][2]
    j = int(np.argmax(x0)) + 1
    assert x0[j - 1] >= 1.0
    api.set_obj_coef(h, j, api.get_obj_coef(h, j) + 1000.0)
    r1 = roundings(root, nodes, table, device)
    assert k in changed(r0, r1) and r1[k][0] != r0[k][0]
    # the direction: filling up no longer pays, the fill keeps what the rounding left
    api.set_obj_dir(h, MIN)
    r2 = roundings(root, nodes, table, device)
    assert set(range(k, 2 * k)) <= set(changed(r1, r2))
    api.set_obj_dir(h, MAX)
    assert not changed(roundings(root, nodes, table, device), r1)
    # a row rewritten twice: in the end row 1 is a hundred times as heavy -- node 0's filled point breaks it
    rewrite_twice(root, 1, A[0][::-1].copy(), 100.0 * A[0])
    r3 = roundings(root, nodes, table, device)
    assert k in changed(r1, r3)
    rewrite_twice(root, 1, 100.0 * A[0], A[0].copy())
    assert not changed(roundings(root, nodes, table, device), r1)
    # set_row_bnds UP -> DB with a lower bound above every point of the box: no rounding is feasible any more
    api.set_row_bnds(h, 2, DB, 1.0e6, 2.0e6)
    r4 = roundings(root, nodes, table, device)
    assert all(f == 0 for _, f, _ in r4)
    api.set_row_bnds(h, 2, UP, 0.0, float(synth.dense_ilp(*RMOD_CASE)[1][1]))
    assert not changed(roundings(root, nodes, table, device), r1)
    # set_col_kind: the column goes continuous -- it keeps its fractional LP value where it had one
    frac = [(t, j) for t, P in enumerate(nodes) for j, v in enumerate(P.col_prim(), start=1) if abs(v - np.rint(v)) > 1e-6]
    assert frac
    t, j = frac[0]
    api.set_col_kind(h, j, CV)
    r5 = roundings(root, nodes, table, device)
    assert t in changed(r1, r5) or k + t in changed(r1, r5)
    assert not changed(roundings(root, nodes, table, device), r5)  # a second call on the unchanged root: the model it kept
    return r0, r5


def test_dive_picks_follow_edits_of_the_root(gpu):
    root, nodes, A, _b, _c = rmod_root(gpu)
    dive_edits(root, nodes, A)


def test_roundings_follow_edits_of_the_root(gpu):
    root, nodes, A, _b, _c = rmod_root(gpu)
    round_edits(root, nodes, A)


def test_zz_certified_step_counts():
    """The steps certified above, per kind and mode; they go to $MVX_EDIT_SCHEDULES_REPORT when set."""
    out = os.environ.get("MVX_EDIT_SCHEDULES_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump({"%s/%s" % k: v for k, v in sorted(COUNTS.items())}, f, indent=1)
    if COUNTS[("end", "quiet")] == len(es.SCHEDULES):  # the whole file ran
        for kind in es.PAIR_KINDS + es.PLACED_KINDS + ("Cx", "Rx"):
            for mode in es.MODES:
                assert COUNTS[(kind, mode)] >= 1, (kind, mode)
