"""CPU: the independent certificates of tests/certify.py -- first that every check fails on a hand-damaged input, then
the oracle's states under them (dense, general-bounds, degenerate and infeasible LPs, B&B children, cut rows and
repaired GMI cuts against every integer point of small boxes).  A case the certificates reject is a bug in the oracle
and, since the GPU suite holds the engine to the oracle bit for bit, in the engine too."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from mvolps_amd import capi, synth
from mvolps_amd.capi import DB, FX, LO, MAX, NL, NOFEAS, NU, OPT, UNBND, UP

from . import certify as cf
from . import lpgen


def dense(api, m, n, seed):
    A, b, c = synth.dense_lp(m, n, seed)
    P = api.create()
    P.load_dense(A, b, c)
    return P, cf.Model.dense(A, b, c)


def general(api, A, rb, cb, c, d):
    P = api.create()
    P.load_general(A, rb, cb, c, direction=d)
    return P, cf.Model(A, rb, cb, c, direction=d)


def ilp(api, m, n, seed, U):
    A, b, c, U = synth.dense_ilp(m, n, seed, U)
    return lpgen.load_ilp(api, A, b, c, U), cf.Model.ilp(A, b, c, U)


def infeasible_general_lp(rng):
    """random_general_lp plus two rows that contradict each other: r x >= L and r x <= L - 1."""
    A, rb, cb, c, d = lpgen.random_general_lp(rng)
    r = np.round(rng.normal(size=A.shape[1]) * 2)
    r[0] = r[0] or 1.0
    L = float(rng.integers(-3, 4))
    return np.vstack([A, r, r]), rb + [(LO, L, 0.0), (UP, 0.0, L - 1.0)], cb, c, d


def orc_gmi(orc, Q, j):
    n = Q.n
    inds = np.zeros(n + 1, dtype=np.int32)
    vals = np.zeros(n + 1)
    lb, eff = C.c_double(0.0), C.c_double(0.0)
    rc = orc.generateCutGMI(Q.h, j, inds.ctypes.data_as(C.POINTER(C.c_int)), vals.ctypes.data_as(C.POINTER(C.c_double)),
                            C.byref(lb), C.byref(eff))
    return rc, vals[1:], lb.value, eff.value


def append_cut(api, P, model, coef, rhs):
    n = P.n
    r = api.add_rows(P.h, 1)
    P.set_mat_row(r, np.arange(n + 1, dtype=np.int32), np.concatenate([[0.0], coef]))
    api.set_row_bnds(P.h, r, LO, float(rhs), 0.0)
    model.add_row(coef, LO, float(rhs), 0.0)


# ------------------------------------------------------------------------------ every check fails on damage


@pytest.fixture
def solved17(orc):
    P, M = dense(orc, 17, 33, 2)
    assert P.simplex() == 0 and P.status == OPT
    return P, M


def test_clean_state_passes_both_paths(solved17):
    P, M = solved17
    a = cf.certify(M, P)
    b = cf.certify(M, P, exact=True)
    assert np.abs(a.full_tableau() - b.full_tableau()).max() < 1e-15 * a.growth


def test_nudged_tableau_entry_fails(solved17):
    P, M = solved17
    for (i, j) in ((3, 5), (0, 7), (4, 0), (0, 0)):
        S = cf.Snapshot(P)
        S.tab[i, j] += 1e-7
        with pytest.raises(cf.CertError, match="tableau entry"):
            cf.certify(M, S)


def test_flipped_bound_flag_fails(orc):
    P, M = ilp(orc, 10, 20, 4, 3)
    P.simplex()
    S = cf.Snapshot(P)
    t = int(np.nonzero(S.flag[1:] == NL)[0][0]) + 1
    S.flag[t] = NU  # a boxed column said to sit on its upper bound: x_B no longer fits T[:,0]
    with pytest.raises(cf.CertError):
        cf.certify(M, S)
    S = cf.Snapshot(P)
    S.col_stat[S.nb[t] - M.m - 1] = NU if S.nb[t] > M.m else S.col_stat[0]
    with pytest.raises(cf.CertError, match="statuses"):
        cf.certify(M, S)


def test_wrong_signed_dual_fails(solved17):
    P, M = solved17
    S = cf.Snapshot(P)
    j = int(np.nonzero(S.col_dual)[0][0])
    S.col_dual[j] = -S.col_dual[j]
    with pytest.raises(cf.CertError, match="dual"):
        cf.certify(M, S)
    S = cf.Snapshot(P)
    i = int(np.nonzero(S.row_dual)[0][0])
    S.row_dual[i] = -S.row_dual[i]
    with pytest.raises(cf.CertError, match="dual"):
        cf.certify(M, S)


def test_optimality_claimed_too_early_fails(orc):
    P, M = dense(orc, 17, 33, 2)
    P.simplex(it_lim=3)
    cf.certify(M, P)  # FEAS after 3 pivots: tableau and values hold
    with pytest.raises(cf.CertError, match="reduced cost"):
        cf.certify(M, P, status=OPT)


def test_fake_statuses_fail(orc, solved17):
    P, M = solved17
    with pytest.raises(cf.CertError, match="NOFEAS"):
        cf.certify(M, P, status=NOFEAS)
    with pytest.raises(cf.CertError, match="UNBND"):
        cf.certify(M, P, status=UNBND)
    # a true NOFEAS basis is no optimum, and a true UNBND one has no infeasibility certificate
    A, rb, cb, c, d = infeasible_general_lp(np.random.default_rng(3))
    Q, MQ = general(orc, A, rb, cb, c, d)
    Q.simplex()
    assert Q.status == NOFEAS
    cf.certify(MQ, Q)
    with pytest.raises(cf.CertError):
        cf.certify(MQ, Q, status=OPT)
    A, b, c = lpgen.CYCLING["beale"]
    R, MR = general(orc, np.array(A), [(UP, 0.0, v) for v in b], [(LO, 0.0, 0.0)] * 4, -np.array(c), MAX)
    R.simplex()
    if R.status == UNBND:
        with pytest.raises(cf.CertError, match="NOFEAS"):
            cf.certify(MR, R, status=NOFEAS)


def test_damaged_eval_tab_row_fails(solved17):
    P, M = solved17
    ref = cf.certify(M, P)
    cf.certify_eval_tab_row(ref, P)

    class Bad:
        def __init__(self, P):
            self.P = P

        def eval_tab_row(self, k):
            ind, val = self.P.eval_tab_row(k)
            if k == ref.head[2]:
                val = val.copy()
                val[0] *= 1.0 + 1e-6
            return ind, val

    with pytest.raises(cf.CertError, match="eval_tab_row"):
        cf.certify_eval_tab_row(ref, Bad(P))


def test_damaged_cuts_fail(orc):
    P, M = ilp(orc, 6, 10, 3, 2)
    P.simplex()
    pts = cf.integer_points(M)
    ref = cf.certify(M, P)
    done = 0
    for j in range(1, M.n + 1):
        if P.api.get_col_stat(P.h, j) != capi.BS:
            continue
        rc, coef, rhs, eff = orc_gmi(orc, P, j)
        if rc != 0:
            continue
        got = cf.certify_gmi(ref, j, coef, rhs, pts)
        assert abs(got - eff) <= 1e-9 * (1 + abs(eff))
        # (a) a coefficient off in its fifth digit: no longer the formula
        bad = coef.copy()
        bad[np.argmax(np.abs(bad))] *= 1.0 + 1e-5
        with pytest.raises(cf.CertError, match="formula"):
            cf.certify_gmi(ref, j, bad, rhs, pts)
        # (c) the right-hand side moved past the best integer point: cuts one off (checked by the point test alone)
        lhs = pts @ coef
        assert len(cf.cut_cuts_off(coef, rhs, pts)) == 0
        assert len(cf.cut_cuts_off(coef, lhs.min() + 0.5, pts)) > 0
        # (b) a cut the vertex satisfies
        with pytest.raises(cf.CertError):
            cf.certify_gmi(ref, j, coef, rhs - 2.0 * (rhs - coef @ P.col_prim()), ())
        done += 1
    assert done >= 1


# ------------------------------------------------------------------------------ the oracle under the certificates


@pytest.mark.parametrize("m,n,seed", [(3, 5, 1), (17, 33, 2), (64, 128, 12345), (100, 37, 5), (256, 512, 12345)])
def test_oracle_dense_lps(orc, m, n, seed):
    P, M = dense(orc, m, n, seed)
    for lim in (1, 2, 7, 33):
        P.simplex(it_lim=lim)
        cf.certify(M, P, exact=(m <= 17), what="%dx%d it %d" % (m, n, P.it_cnt))
    assert P.simplex() == 0 and P.status == OPT
    ref = cf.certify(M, P)
    cf.certify_eval_tab_row(ref, P)


@pytest.mark.parametrize("seed", [7, 1, 2, 3, 4])
def test_oracle_general_bounds(orc, seed):
    """120 general-bounds LPs per seed (seed 7 is the HiGHS-pinned set), both directions, every bound type; one in four
    gets two contradicting rows (NOFEAS), so all three statuses meet their certificates."""
    rng = np.random.default_rng(seed)
    seen = {}
    for t in range(120):
        A, rb, cb, c, d = infeasible_general_lp(rng) if (seed != 7 and t % 4 == 3) else lpgen.random_general_lp(rng)
        P, M = general(orc, A, rb, cb, c, d)
        assert P.simplex() == 0
        cf.certify(M, P, exact=True, what="seed %d trial %d" % (seed, t))
        seen[P.status] = seen.get(P.status, 0) + 1
    assert seen.get(OPT, 0) > 40 and seen.get(UNBND, 0) > 5
    if seed != 7:
        assert seen.get(NOFEAS, 0) >= 30


def test_oracle_degenerate_and_cycling(orc):
    for (m, n, seed) in ((30, 50, 1), (60, 90, 2), (120, 200, 3)):
        A, b, c = lpgen.degenerate_lp(m, n, seed)
        P = lpgen.load_degenerate(orc, A, b, c)
        assert P.simplex() == 0
        cf.certify(cf.Model(A, [(UP, 0.0, float(x)) for x in b], [(DB, 0.0, 2.0)] * n, c), P)
    for name, (A, b, c) in lpgen.CYCLING.items():
        P, M = general(orc, np.array(A), [(UP, 0.0, v) for v in b], [(LO, 0.0, 0.0)] * 4, np.array(c), MAX)
        assert P.simplex() == 0
        cf.certify(M, P, exact=True, what=name)


def test_oracle_phase1_infeasible_start(orc):
    """x >= 3 on a packing ILP: the slack basis violates every row and phase 1 proves it cannot be repaired; a milder
    lower bound is feasible after phase 1."""
    for lb, want in ((3.0, NOFEAS), (0.25, OPT)):
        A, b, c, U = synth.dense_ilp(20, 30, 5, 3, cap=0.3)
        cols = [(LO, lb, 0.0)] * 30
        P, M = general(orc, A, [(UP, 0.0, float(v)) for v in b], cols, c, MAX)
        assert P.simplex() == 0 and P.status == want
        cf.certify(M, P)


def test_oracle_children_clones_and_bound_edits(orc):
    P, M = ilp(orc, 40, 90, 17, 2)
    P.simplex()
    x = P.col_prim()
    frac = [j + 1 for j in range(len(x)) if abs(x[j] - round(x[j])) > 1e-6]
    assert len(frac) >= 3
    statuses = set()
    for j in frac[:4]:
        for (t, lo, hi) in ((DB, 0.0, float(np.floor(x[j - 1]))), (DB, float(np.ceil(x[j - 1])), 2.0)):
            ch, Mc = P.copy(), M.copy()
            ch.api.set_col_bnds(ch.h, j, t, lo, hi)
            Mc.set_col_bnds(j, t, lo, hi)
            cf.certify(Mc, ch, status=capi.UNDEF, what="child before solve")  # the warm start's shifted x_B
            ch.simplex()
            cf.certify(Mc, ch, what="child %d" % j)
            statuses.add(ch.status)
            gc, Mg = ch.copy(), Mc.copy()  # clone of a clone with more edits, then an infeasible box
            for k in frac[4:12]:
                gc.api.set_col_bnds(gc.h, k, DB, 1.0, 2.0)
                Mg.set_col_bnds(k, DB, 1.0, 2.0)
            gc.simplex()
            cf.certify(Mg, gc, what="grandchild")
            statuses.add(gc.status)
    # every column at its upper bound: no room left
    Q, MQ = P.copy(), M.copy()
    for j in range(1, 91):
        Q.api.set_col_bnds(Q.h, j, FX, 2.0, 2.0)
        MQ.set_col_bnds(j, FX, 2.0, 2.0)
    Q.simplex()
    assert Q.status == NOFEAS
    cf.certify(MQ, Q, what="all fixed")
    assert OPT in statuses


def test_oracle_cut_rows_and_repaired_gmi_against_every_integer_point(orc):
    """Small enumerable ILPs (U = 2, n <= 12): three rounds of repaired GMI cuts; each cut equals the formula on the
    recomputed row, is violated by the vertex, excludes no integer feasible point; the appended row is checked
    right after set_mat_row (before any pivot) and after the dual re-solve."""
    ncuts = 0
    for (m, n, seed) in ((6, 10, 3), (5, 12, 8), (8, 11, 21), (4, 9, 2)):
        P, M = ilp(orc, m, n, seed, 2)
        pts = cf.integer_points(M)
        assert len(pts) > 0
        P.simplex()
        for rnd in range(3):
            ref = cf.certify(M, P, exact=True)
            cands = []
            for j in range(1, n + 1):
                if P.api.get_col_stat(P.h, j) != capi.BS:
                    continue
                rc, coef, rhs, eff = orc_gmi(orc, P, j)
                if rc == 0:
                    cf.certify_gmi(ref, j, coef, rhs, pts, what="%dx%d round %d" % (m, n, rnd))
                    cands.append((eff, coef, rhs))
                    ncuts += 1
            if not cands:
                break
            eff, coef, rhs = max(cands, key=lambda t: t[0])
            append_cut(orc, P, M, coef, rhs)
            cf.certify(M, P, status=capi.UNDEF, exact=True, what="appended row before a pivot")
            P.simplex()
            cf.certify(M, P, exact=True, what="after the re-solve")
    assert ncuts >= 10


def test_oracle_gmi_cuts_keep_the_milp_optimum(orc):
    """Larger ILPs: every repaired cut of three rounds keeps the HiGHS milp optimum point (tests/golden/milp_pins.json,
    objective equal to the pin)."""
    pins = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "milp_pins.json")))
    for pin in pins["points"]:
        if pin["m"] > 128:
            continue
        A, b, c, U = synth.dense_ilp(pin["m"], pin["n"], pin["seed"], pin["U"], pin["cap"])
        xs = np.array(pin["x"])
        assert abs(c @ xs - pin["milp_obj"]) <= 1e-9 * abs(pin["milp_obj"]) and np.all(A @ xs <= b)
        P, M = lpgen.load_ilp(orc, A, b, c, U), cf.Model.ilp(A, b, c, U)
        P.simplex()
        for rnd in range(3):
            ref = cf.certify(M, P)
            best = None
            for j in range(1, M.n + 1):
                if P.api.get_col_stat(P.h, j) != capi.BS:
                    continue
                rc, coef, rhs, eff = orc_gmi(orc, P, j)
                if rc == 0:
                    cf.certify_gmi(ref, j, coef, rhs, xs[None, :], what="pin %d round %d" % (pin["seed"], rnd))
                    if best is None or eff > best[0]:
                        best = (eff, coef, rhs)
            append_cut(orc, P, M, best[1], best[2])
            P.simplex()
