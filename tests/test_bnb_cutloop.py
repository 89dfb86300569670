"""CPU: the root cut rounds (DESIGN.md "Root cut rounds") over the ORACLE's table, so the host side of the definition runs:
mvx_generateCutGMI per candidate column (the oracle's table has no gmi_cuts), the twin mvx_bnb_cut_scores, mvx_bnb_cut_select,
the per-row appends and the oracle's dual simplex.

The rows the loop appends keep the enumerated optimum of every fixture instance and never improve the root LP; every
instance closes on its pin with the loop in front of each single-GPU driver; windows give the serial tree; the selection and
the scores are checked with == against plain-Python restatements of the definition; the refusals return their codes."""
import math
import os
import subprocess

import numpy as np
import pytest

from mvolps_amd import bnb, capi, synth
from mvolps_amd.capi import MAX, OPT

from . import certify as cf
from . import lpgen
from .test_bnb_general import INSTANCES, check_pin, failures, instance, run
from .test_bnb_host import same_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = bnb.CUTLOOP_COUNTERS + ("cutloop_bound0", "cutloop_bound")
OPTIMAL = [r for r in INSTANCES if r["status"] == "optimal"]
PIN_OPTIONS = {
    "serial": dict(cut_rounds=5, window=1),
    "window64": dict(cut_rounds=5, window=64),
    "best_window8": dict(cut_rounds=5, node_strat=1, best_window=8),
    "tree_cuts": dict(cut_rounds=5, cut_strat=1),
    "heur2_rcfix_prop8_window64": dict(cut_rounds=5, heur=2, rc_fix=1, prop=8, window=64),
}


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    assert not t.gmi_cuts and not t.cut_scores and not t.add_cut_rows  # the host side of the definition runs over the oracle
    return t


def rounded_root(orc, tab, inst):
    """The root as the driver hands it to the loop: integer columns' bounds rounded inward (None: no integer in a range)."""
    P = lpgen.load_milp(orc, inst)
    return None if bnb.integral_bounds(P, table=tab) == 2 else P


def rows_behind(api, P, m0):
    out = []
    for i in range(m0 + 1, api.get_num_rows(P.h) + 1):
        ind, val = P.get_mat_row(i)
        coef = np.zeros(P.n)
        coef[np.asarray(ind, dtype=int) - 1] = val
        out.append((coef, api.get_row_lb(P.h, i)))
    return out


# ------------------------------------------------------------------------------------------------ validity


def test_loop_rows_keep_the_optimum_and_never_improve_the_root(orc, tab):
    """R = 1, 3, 8 on every instance with an enumerated optimum: no appended row excludes the pinned point (the margin of
    test_repaired_cuts_on_tree_nodes_keep_the_optimum), the counters agree with the handle, and the root LP after a round is
    not better than before it by more than 1e-7 max(1, |obj|), the margin check_incumbent grants an LP vertex."""
    checked, bad = 0, []
    for rec in OPTIMAL:
        inst = instance(rec)
        x = np.array(rec["x"])
        sg = 1.0 if inst["direction"] == MAX else -1.0
        trail = []
        for R in (1, 3, 8):
            P = rounded_root(orc, tab, inst)
            assert P is not None
            m0 = P.m
            rc, out = bnb.cut_loop(P, rounds=R, table=tab)
            assert rc == 0, (rec["index"], rc)
            rows = rows_behind(orc, P, m0)
            assert len(rows) == out["cutloop_rows"] and out["cutloop_rounds"] <= R and out["cutloop_lps"] == 1 + out["cutloop_rounds"]
            assert out["cutloop_rows"] <= max(64, m0)
            for coef, rhs in rows:
                checked += 1
                if len(cf.cut_cuts_off(coef, rhs, [x])):
                    bad.append("instance %d, R = %d: a row excludes the optimum %s (%.9g < %.9g)" % (rec["index"], R, rec["x"], coef @ x, rhs))
            assert P.status == OPT, (rec["index"], R, P.status)  # valid cuts leave the optimum feasible
            trail.append((out["cutloop_bound0"], out["cutloop_bound"]))
        # rounds 1, 3 and 8 of the same deterministic sequence, then every round on its own
        seq = [trail[0][0]] + [b for _b0, b in trail]
        P = rounded_root(orc, tab, inst)
        for _ in range(8):
            rc, out = bnb.cut_loop(P, rounds=1, table=tab)
            assert rc == 0
            if out["cutloop_rounds"] == 0:
                break
            seq += [out["cutloop_bound0"], out["cutloop_bound"]]
        for before, after in zip(seq[:3], seq[1:4]):
            assert sg * after <= sg * before + 1e-7 * max(1.0, abs(before)), (rec["index"], before, after)
        for before, after in zip(seq[4::2], seq[5::2]):
            assert sg * after <= sg * before + 1e-7 * max(1.0, abs(before)), (rec["index"], before, after)
    assert not bad, "\n".join(bad[:20])
    assert checked >= 30, checked


# ------------------------------------------------------------------------------------------------ whole trees


@pytest.mark.parametrize("name", list(PIN_OPTIONS))
def test_trees_behind_the_loop_close_on_the_enumerated_optimum(orc, tab, name):
    kw = PIN_OPTIONS[name]
    rounds = []

    def one(rec):
        inst = instance(rec)
        r = run(orc, rec, inst, table=tab, **kw)
        check_pin(rec, inst, r)
        rounds.append(r["cutloop_rounds"])
        assert r["cutloop_lps"] in (0, 1 + r["cutloop_rounds"])  # 0: a column's range holds no integer, nothing was solved

    bad = failures(INSTANCES, one)
    assert not bad, "\n".join(bad)
    assert sum(1 for k in rounds if k > 0) >= 30, "the loop ran on %d instances only" % sum(1 for k in rounds if k > 0)


def test_windows_give_the_serial_tree(orc, tab):
    recs = INSTANCES[::10]

    def same(a, b):
        same_result(a, b)
        for k in COUNTERS:
            assert a[k] == b[k], k

    def one(rec):
        inst = instance(rec)
        ref = run(orc, rec, inst, table=tab, window=1, cut_rounds=5)
        for w in (2, 8, 64):
            same(run(orc, rec, inst, table=tab, window=w, cut_rounds=5), ref)
        ref = run(orc, rec, inst, table=tab, node_strat=1, window=1, cut_rounds=5)
        for w in (1, 8):
            same(run(orc, rec, inst, table=tab, node_strat=1, best_window=w, cut_rounds=5), ref)

    bad = failures(recs, one)
    assert not bad, "\n".join(bad)


def test_cut_rounds_0_is_todays_result(orc, tab):
    def one(rec):
        inst = instance(rec)
        for kw in (dict(window=1), dict(window=64, cut_strat=1), dict(window=64, heur=2, rc_fix=1, prop=8)):
            ref = run(orc, rec, inst, table=tab, **kw)
            got = run(orc, rec, inst, table=tab, cut_rounds=0, cut_round_max=-7, cut_maxpar=5.0, **kw)  # not read when off
            assert got == ref
            assert all(got[k] == 0 for k in COUNTERS)

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)


def test_the_callers_handle_is_left_as_it_was(orc, tab):
    rec = next(r for r in OPTIMAL if r["family"] == "a")
    inst = instance(rec)
    P = lpgen.load_milp(orc, inst)
    m0 = P.m
    r = bnb.branch_and_bound(P, quirks=0, table=tab, cut_rounds=5)
    check_pin(rec, inst, r)
    assert P.m == m0 and orc.get_num_rows(P.h) == m0


# ------------------------------------------------------------------------------------------------ the selection twin


def py_select(eff, G, K, maxpar, budget):
    """Step 4 of the definition on Python floats."""
    order = sorted(range(len(eff)), key=lambda t: (-eff[t], t))
    taken = []
    for t in order:
        if len(taken) >= K or len(taken) >= budget:
            break
        if all(float(G[t][s]) <= maxpar * (math.sqrt(float(G[t][t])) * math.sqrt(float(G[s][s]))) for s in taken):
            taken.append(t)
    return taken


def seq_gram(V):
    """G[t][s] = sum_j v_tj v_sj over ascending j from +0.0, product and sum rounded separately, on Python floats."""
    k = len(V)
    G = np.zeros((k, k))
    for t in range(k):
        for s in range(k):
            g = 0.0
            for a, b in zip(V[t], V[s]):
                g = g + float(a) * float(b)
            G[t, s] = g
    return G


def test_cut_select_hand_cases():
    eye = np.eye(4)
    assert bnb.cut_select([1.0, 2.0, 2.0, 1.0], eye) == (0, [1, 2, 0, 3])  # ties in efficacy go to the lower index
    assert bnb.cut_select([1.0, 2.0, 2.0, 1.0], eye, K=1) == (0, [1])
    assert bnb.cut_select([1.0, 2.0, 2.0, 1.0], eye, K=3, budget=2) == (0, [1, 2])  # the row budget ends the round part-way
    assert bnb.cut_select([1.0, 2.0, 2.0, 1.0], eye, budget=0) == (0, [])
    assert bnb.cut_select([], np.zeros((0, 0))) == (0, [])
    # a duplicated candidate is never taken twice under a maxpar below 1, whatever its efficacy
    V = np.array([[1.0, 2.0, -3.0], [0.0, 1.0, 1.0], [1.0, 2.0, -3.0], [0.3, 0.1, 0.7]])
    G = seq_gram(V)
    for mp in (0.9, 0.5, 0.999999, 1e-9):
        rc, got = bnb.cut_select([3.0, 2.0, 3.0, 1.0], G, maxpar=mp)
        assert rc == 0 and got[0] == 0 and 2 not in got and got == py_select([3.0, 2.0, 3.0, 1.0], G, 32, mp, 1 << 30)
    # bad arguments
    for kw in (dict(K=0), dict(maxpar=0.0), dict(maxpar=1.5), dict(maxpar=float("nan")), dict(budget=-1)):
        assert bnb.cut_select([1.0], np.eye(1), **kw)[0] == -1, kw


def test_cut_select_against_the_definition():
    rng = np.random.default_rng(20261019)
    passed_at_1 = 0
    for trial in range(200):
        k, n = int(rng.integers(1, 24)), int(rng.integers(1, 9))
        V = rng.integers(-3, 4, size=(k, n)).astype(np.float64) * rng.choice([1.0, 0.1, 1.0 / 3.0], size=(k, 1))
        for t in range(1, k):  # proportional and duplicated rows
            if rng.random() < 0.3:
                V[t] = V[int(rng.integers(0, t))] * rng.choice([1.0, 2.0, 3.0, 0.7])
        V[np.abs(V).sum(axis=1) == 0, 0] = 1.0
        G = seq_gram(V)
        assert np.array_equal(G, G.T)
        eff = np.round(rng.random(k) * 4) / 4 + 0.25  # many ties
        for mp in (1.0, 0.9, 0.3, 1e-9):
            for K, budget in ((32, 1 << 30), (1, 5), (3, 2), (5, 64)):
                rc, got = bnb.cut_select(eff, G, K=K, maxpar=mp, budget=budget)
                assert rc == 0 and got == py_select(eff, G, K, mp, budget), (trial, mp, K, budget)
                assert len(got) <= min(K, budget) and len(set(got)) == len(got)
                for a in range(len(got)):
                    for b in range(a):
                        t, s = got[a], got[b]
                        assert G[t, s] <= mp * (math.sqrt(G[t, t]) * math.sqrt(G[s, s]))
                if mp == 1.0 and K == 32:
                    # only a cut whose G[t][s] rounds above sqrt(nrm_t) sqrt(nrm_s) is dropped
                    for t in set(range(k)) - set(got):
                        assert any(G[t, s] > math.sqrt(G[t, t]) * math.sqrt(G[s, s]) for s in got)
                    passed_at_1 += sum(1 for a in got for b in got if a < b and abs(G[a, b]) >= 0.999999 * math.sqrt(G[a, a] * G[b, b]))
    assert passed_at_1 > 50, passed_at_1  # proportional cuts usually pass at maxpar = 1


# ------------------------------------------------------------------------------------------------ the scores twin


def gmi_rows(orc, tab, P):
    """The repaired cuts of every candidate column of the solved handle P: (vals (k, n + 1), rhs, eff)."""
    vals, rhs, eff = [], [], []
    for j in range(1, P.n + 1):
        got = bnb.generate_cut_gmi(P, j, table=tab)
        if got is not None:
            vals.append(got[0])
            rhs.append(got[1])
            eff.append(got[2])
    return np.array(vals), np.array(rhs), np.array(eff)


@pytest.mark.parametrize("case", [(8, 16, 3, 2), (24, 48, 5, 3)], ids=lambda c: "%dx%d" % (c[0], c[1]))
def test_cut_scores_twin_against_the_definition(orc, tab, case):
    m, n, seed, U = case
    A, b, c, Ub = synth.dense_ilp(m, n, seed, U)
    P = lpgen.load_ilp(orc, A, b, c, Ub)
    P.simplex()
    assert P.status == OPT
    vals, rhs, eff = gmi_rows(orc, tab, P)
    k = len(vals)
    assert k >= 3
    rc, dot, gram = bnb.cut_scores(P, vals, table=tab)
    assert rc == 0
    x = [orc.get_col_prim(P.h, j) for j in range(1, n + 1)]
    G = seq_gram(vals[:, 1:])
    assert np.array_equal(gram, G) and np.array_equal(gram, gram.T)
    for t in range(k):
        d = 0.0
        for a, xv in zip(vals[t, 1:], x):
            d = d + float(a) * float(xv)
        assert dot[t] == d
        assert eff[t] == (rhs[t] - d) / math.sqrt(G[t, t])  # generateCutGMI's own efficacy is the same arithmetic
    # entry 0 of a row is not read
    v2 = vals.copy()
    v2[:, 0] = 123.0
    rc, dot2, gram2 = bnb.cut_scores(P, v2, table=tab)
    assert rc == 0 and np.array_equal(dot2, dot) and np.array_equal(gram2, gram)
    # a handle that is not OPT, no rows
    Q = lpgen.load_ilp(orc, A, b, c, Ub)
    assert bnb.cut_scores(Q, vals, table=tab)[0] == -1
    assert bnb.cut_scores(P, np.zeros((0, n + 1)), table=tab)[0] == -1


# ------------------------------------------------------------------------------------------------ the loop's own numbers


def test_loop_follows_the_definition_round_by_round(orc, tab):
    """One round restated with the binding's pieces: candidates, efficacy filter and order, C = 4 K, Gram, selection, rows in
    taken order with their bounds."""
    A, b, c, Ub = synth.dense_ilp(24, 48, 5, 3)
    for K, mp in ((32, 0.9), (2, 0.9), (4, 0.1)):
        P = lpgen.load_ilp(orc, A, b, c, Ub)
        P.simplex()
        m0 = P.m
        vals, rhs, eff = gmi_rows(orc, tab, P)
        mag = np.abs(vals[:, 1:])
        wide = [mag[t].max() > 1e9 * mag[t][mag[t] > 0].min() for t in range(len(eff))]  # the coefficient-range safeguard
        live = [t for t in sorted(range(len(eff)), key=lambda t: (-eff[t], t)) if eff[t] > 1e-6 and not wide[t]][: 4 * K]
        _rc, _dot, gram = bnb.cut_scores(P, vals[live], table=tab)
        taken = [live[t] for t in py_select([eff[t] for t in live], gram, K, mp, max(64, m0))]
        Q = lpgen.load_ilp(orc, A, b, c, Ub)
        rc, out = bnb.cut_loop(Q, rounds=1, K=K, maxpar=mp, table=tab)
        assert rc == 0 and out["cutloop_rounds"] == 1 and out["cutloop_rows"] == len(taken) and out["cutloop_candidates"] == len(eff)
        rows = rows_behind(orc, Q, m0)
        assert len(rows) == len(taken) >= 1
        for (coef, lb), t in zip(rows, taken):
            assert np.array_equal(coef, vals[t, 1:]) and lb == rhs[t]
        assert out["cutloop_bound0"] == P.obj and out["cutloop_bound"] == Q.obj and Q.obj <= P.obj + 1e-9
    # the defaults: K = 0 means 32, maxpar = 0.0 means 0.9
    Q1, Q2 = lpgen.load_ilp(orc, A, b, c, Ub), lpgen.load_ilp(orc, A, b, c, Ub)
    assert bnb.cut_loop(Q1, rounds=3, table=tab) == bnb.cut_loop(Q2, rounds=3, K=32, maxpar=0.9, table=tab)


# ------------------------------------------------------------------------------------------------ refusals, CLI


def test_refusals(orc, tab):
    from mvolps_amd import dist_bnb, dist_native

    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    for kw in (dict(cut_rounds=65, quirks=0), dict(cut_rounds=-1, quirks=0), dict(cut_rounds=5, quirks=1), dict(cut_rounds=5),
               dict(cut_rounds=1, quirks=0, cut_round_max=-1), dict(cut_rounds=1, quirks=0, cut_round_max=4097),
               dict(cut_rounds=1, quirks=0, cut_maxpar=-0.1), dict(cut_rounds=1, quirks=0, cut_maxpar=1.1),
               dict(cut_rounds=1, quirks=0, cut_maxpar=float("nan"))):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, **kw)
        assert r["rc"] == -1 and r["n_nodes"] == 0 and r["count"] == 0, kw
    for kw in (dict(cut_rounds=1), dict(cut_rounds=64, cut_round_max=4096, cut_maxpar=1.0), dict(cut_rounds=5, node_strat=1),
               dict(cut_rounds=5, node_strat=1, best_window=8), dict(cut_rounds=5, var_strat=3), dict(cut_rounds=5, dive=7, pump=30)):
        assert bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0, **kw)["rc"] == 0, kw
    # bug-compatible mode never reads the other two fields
    assert bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, cut_round_max=-5, cut_maxpar=7.0)["rc"] == 0
    P = lpgen.load_ilp(orc, A, b, c, U)
    with pytest.raises(ValueError):
        dist_native.branch_and_bound(P, table=tab, cut_rounds=5, quirks=0)
    with pytest.raises(ValueError):
        dist_bnb.branch_and_bound(None, P, cut_rounds=5, quirks=0)
    pr = bnb.make_params(quirks=0, cut_rounds=5)
    L = dist_native._lib()
    res, st = bnb.BnbResult(), dist_native.DistStats()
    tptr = bnb.C.cast(bnb.C.pointer(tab), bnb.C.c_void_p)
    assert L.mvx_branchAndBound_dist(tptr, None, P.h, bnb.C.byref(pr), None, None, bnb.C.byref(res), bnb.C.byref(st)) == capi.EFAIL
    # the loop's own entry
    for kw in (dict(rounds=0), dict(rounds=65), dict(K=-1), dict(K=4097), dict(maxpar=-0.5), dict(maxpar=1.5)):
        assert bnb.cut_loop(lpgen.load_ilp(orc, A, b, c, U), table=tab, **kw)[0] == -1, kw
    # a loop that cannot run: an error with the unsolved root as the tree, not a run without the loop
    bare = bnb.table_from(orc)
    bare.eval_tab_row = None
    assert bnb.cut_loop(lpgen.load_ilp(orc, A, b, c, U), table=bare)[0] == -2
    for kw in (dict(window=1), dict(window=64), dict(node_strat=1, best_window=8)):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=bare, cut_rounds=5, quirks=0, **kw)
        assert r["rc"] == -2 and r["n_nodes"] == 1 and r["count"] == 0 and not r["has_incumbent"], kw


def test_cli_flags_parse():
    """The flags on tests/golden/f1.lp.  Without a device the front end can not solve, so the values are followed up to the
    driver's refusal: without --repaired the driver refuses cut rounds and the message names the flag; values out of range are
    refused by the parser itself."""
    exe = os.path.join(ROOT, "mvolps_amd", "bin", "mvolps")
    f1 = os.path.join(ROOT, "tests", "golden", "f1.lp")

    def cli(*flags):
        return subprocess.run([exe, "-f", f1, *flags], capture_output=True, text=True)

    assert "--cut-rounds" in subprocess.run([exe, "-h"], capture_output=True, text=True).stdout
    for flags in (("--cut-rounds",), ("--cut-rounds", "7"), ("--cut-rounds", "--cut-round-max", "8", "--cut-maxpar", "0.5")):
        r = cli(*flags)
        assert r.returncode != 0 and "/ --cut-rounds are not supported" in r.stderr and "Unknown parameter" not in r.stderr, (flags, r.stderr)
    for flags, name in ((("--repaired", "--cut-rounds", "65"), "--cut-rounds"), (("--repaired", "--cut-rounds", "0"), "--cut-rounds"),
                        (("--repaired", "--cut-rounds", "--cut-round-max", "0"), "--cut-round-max"),
                        (("--repaired", "--cut-rounds", "--cut-round-max", "4097"), "--cut-round-max"),
                        (("--repaired", "--cut-rounds", "--cut-maxpar", "0"), "--cut-maxpar"),
                        (("--repaired", "--cut-rounds", "--cut-maxpar", "1.5"), "--cut-maxpar"),
                        (("--repaired", "--cut-rounds", "--cut-maxpar", "x"), "--cut-maxpar")):
        r = cli(*flags)
        assert r.returncode != 0 and "Unknown parameter value for %s" % name in r.stderr, (flags, r.stderr)
