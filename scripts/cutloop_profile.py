"""Measurements behind DESIGN.md "Root cut rounds" (mvx_bnb_params.cut_rounds).

  --part cpu      no device: the loop over the oracle's table on every fourth general fixture and on small dense_ilp instances,
                  for K in {4, 8, 32, 128} x maxpar in {0.5, 0.9, 1.0} at 5 rounds (and the rounds 1 / 5 / 10 at the defaults):
                  trees' nodes with and without the loop, rows appended, share of the root gap closed.
  --part append   one mvx_add_cut_rows(k) call against k per-row appends on clones of the solved 512x1024 root, k = 8 / 32 / 128,
                  alternating, medians of 7; the rows are the root's own GMI cuts.
  --part scores   mvx_cut_scores against the host twin mvx_bnb_cut_scores at C = 128 and C = 512 rows of the same root.
  --part trees    config 5 to the end and the wide instance to 20 000 nodes at window 64, repaired: cut_rounds 0 / 1 / 5 / 10, plain,
                  with cut_strat = 1 and with heur 2 + rc_fix, two alternating runs each.
One JSON object per line on stdout (and appended to --out when given)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("count", "hit_limit", "has_incumbent", "best_lower", "total_pivots", "cutloop_rounds", "cutloop_candidates", "cutloop_rows",
        "cutloop_lps", "cutloop_pivots", "cutloop_bound0", "cutloop_bound")
WIDE = (512, 1024, 12345, 3, 0.4)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def config5():
    from mvolps_amd import synth

    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "config5.json")))
    return synth.dense_ilp(fx["m"], fx["n"], fx["seed"], fx["U"], fx["cap"])


def part_cpu(out):
    from mvolps_amd import bnb, synth
    from oracle import oracle
    from tests import lpgen
    from tests.test_bnb_general import INSTANCES, instance, max_nodes

    orc = oracle.api()
    tab = bnb.table_from(orc)
    fixtures = [(rec, instance(rec)) for rec in INSTANCES[::4] if rec["status"] == "optimal"]
    dense = [synth.dense_ilp(m, n, seed, U) for (m, n, seed, U) in ((10, 20, 4, 3), (16, 32, 5, 2), (24, 48, 5, 3), (30, 60, 9, 2))]

    def sweep(label, loads, limit, **kw):
        nodes = rows = pivots = loop_pivots = 0
        closed = []
        for load, opt in loads:
            r = bnb.branch_and_bound(load(), quirks=0, table=tab, window=64, max_nodes=limit, **kw)
            assert r["rc"] == 0
            nodes += r["count"]
            pivots += r["total_pivots"]
            rows += r["cutloop_rows"]
            loop_pivots += r["cutloop_pivots"]
            if kw.get("cut_rounds") and opt is not None and abs(r["cutloop_bound0"] - opt) > 1e-9:
                closed.append((r["cutloop_bound0"] - r["cutloop_bound"]) / (r["cutloop_bound0"] - opt))
        emit(dict({"part": "cpu", "set": label, "instances": len(loads), "nodes": nodes, "tree_pivots": pivots, "loop_pivots": loop_pivots,
                   "rows": rows, "mean_gap_closed": statistics.fmean(closed) if closed else None}, **kw), out)

    fl = [((lambda inst=inst: lpgen.load_milp(orc, inst)), rec["optimum"]) for rec, inst in fixtures]
    dl = [((lambda mod=mod: synth.load_ilp(orc, *mod)), None) for mod in dense]
    for label, loads, limit in (("general fixtures", fl, 100000), ("dense_ilp 10x20..30x60", dl, 20000)):
        sweep(label, loads, limit)
        for R in (1, 5, 10):
            sweep(label, loads, limit, cut_rounds=R)
        for K in (4, 8, 32, 128):
            for mp in (0.5, 0.9, 1.0):
                if (K, mp) != (32, 0.9):
                    sweep(label, loads, limit, cut_rounds=5, cut_round_max=K, cut_maxpar=mp)


def wide_root_cuts(count):
    """The solved wide root and `count` of its repaired GMI cuts (further rounds' cuts when one round has too few)."""
    import mvolps_amd
    import numpy as np
    from mvolps_amd import bnb, synth

    gpu = mvolps_amd.api()
    root = synth.load_ilp(gpu, *synth.dense_ilp(*WIDE))
    root.simplex()
    vals, rhs = [], []
    P = root.copy()
    while len(vals) < count:
        got = [g for g in (bnb.generate_cut_gmi(P, j) for j in range(1, P.n + 1)) if g is not None]
        assert got
        vals += [g[0] for g in got]
        rhs += [g[1] for g in got]
        assert bnb.add_cut_rows(P, np.array([g[0] for g in got[:32]]), np.array([g[1] for g in got[:32]])) == 0
        P.simplex()
    return gpu, root, np.array(vals[:count]), np.array(rhs[:count])


def part_append(out):
    import numpy as np
    from mvolps_amd import bnb
    from mvolps_amd.capi import LO

    gpu, root, vals, rhs = wide_root_cuts(128)
    ind = np.arange(root.n + 1, dtype=np.int32)

    def per_row(P, k):
        for t in range(k):
            i = gpu.add_rows(P.h, 1)
            P.set_mat_row(i, ind, vals[t])
            gpu.set_row_bnds(P.h, i, LO, float(rhs[t]), 0.0)

    for k in (8, 32, 128):
        one, each = [], []
        for rep in range(8):
            a, b = root.copy(), root.copy()
            gpu.sync()
            t0 = time.perf_counter()
            assert bnb.add_cut_rows(a, vals[:k], rhs[:k]) == 0
            gpu.sync()
            t1 = time.perf_counter()
            per_row(b, k)
            gpu.sync()
            t2 = time.perf_counter()
            if rep:  # the first repetition warms both paths up
                one.append(t1 - t0)
                each.append(t2 - t1)
            same = bool(np.array_equal(a.tableau().view(np.uint64), b.tableau().view(np.uint64)))
        emit({"part": "append", "instance": "512x1024 cap 0.4 U 3 root", "k": k, "reps": len(one), "add_cut_rows_ms": statistics.median(one) * 1e3,
              "per_row_ms": statistics.median(each) * 1e3, "per_row_us_per_row": statistics.median(each) / k * 1e6, "same_tableau": same}, out)


def part_scores(out):
    import numpy as np
    from mvolps_amd import bnb

    gpu, root, vals, _rhs = wide_root_cuts(512)
    for C_ in (128, 512):
        dev, host = [], []
        for rep in range(6):
            gpu.sync()
            t0 = time.perf_counter()
            rc, dot, gram = bnb.cut_scores(root, vals[:C_])
            t1 = time.perf_counter()
            trc, tdot, tgram = bnb.cut_scores(root, vals[:C_], table=None)
            t2 = time.perf_counter()
            assert rc == 0 and trc == 0
            if rep:
                dev.append(t1 - t0)
                host.append(t2 - t1)
        emit({"part": "scores", "instance": "512x1024 cap 0.4 U 3 root", "C": C_, "reps": len(dev), "mvx_cut_scores_ms": statistics.median(dev) * 1e3,
              "mvx_bnb_cut_scores_ms": statistics.median(host) * 1e3,
              "same_bits": bool(np.array_equal(gram.view(np.uint64), tgram.view(np.uint64)) and np.array_equal(dot.view(np.uint64), tdot.view(np.uint64)))},
             out)


def part_trees(out):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    def tree(model, **kw):
        t0 = time.perf_counter()
        r = bnb.branch_and_bound(synth.load_ilp(mvolps_amd.api(), *model), quirks=0, window=64, **kw)
        return r, time.perf_counter() - t0

    for name, model, limit in (("config-5", config5(), 2 * 15697), ("512x1024 cap 0.4 U 3", synth.dense_ilp(*WIDE), 20000)):
        tree(model, cut_rounds=1, max_nodes=1)  # warm-up
        for rep in range(2):
            for extra in (dict(), dict(cut_strat=1), dict(heur=2, rc_fix=1)):
                for R in (0, 1, 5, 10):
                    r, el = tree(model, cut_rounds=R, max_nodes=limit, **extra)
                    emit(dict({"part": "trees", "instance": name, "window": 64, "max_nodes": limit, "cut_rounds": R, "rep": rep, "rc": r["rc"],
                               "seconds": el}, **extra, **{k: r[k] for k in KEYS}), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["cpu", "append", "scores", "trees"], required=True)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"cpu": part_cpu, "append": part_append, "scores": part_scores, "trees": part_trees}[a.part](a.out)


if __name__ == "__main__":
    main()
