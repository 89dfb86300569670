"""Measurements behind DESIGN.md "Cut purging (cut_purge)" (mvx_del_rows, k_delrows, mvx_bnb_params.cut_purge).

  --part cpu      no device: whole trees over the oracle's table, whose purge is the free-row path (the same LP as a deletion),
                  for the age limit A = 0..4: every fourth general fixture with an optimum at 5 rounds of GMI cuts, and the four
                  binary dense_ilp models of the clique table that take more than one round, at 10 rounds with both families.
                  Work is counted as tree pivots x (rows the tree's root holds + 1), the entries a dense pivot touches per column.
  --part call     the first half of --part device alone: the single calls, no trees.
  --part device   one mvx_del_rows(k) call, k = 8 / 32 / 128, on clones of the solved wide 512x1024 root carrying 128 of its own GMI
                  rows, beside one mvx_add_cut_rows(k) call of the same session: host clocks around calls that end in a
                  synchronise, one warm-up first, medians of 7 (--out).  Then whole trees at window 64 with cut_rounds 5 and
                  A = 0 / 1 / 3, two alternating runs each: config 5 with families 1 and 3, dense_ilp(64,128,7,1,0.025) with families
                  3, and the wide instance cut at 20 000 nodes (--out-trees).
One JSON object per line on stdout (and appended to --out / --out-trees when given)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("count", "n_nodes", "hit_limit", "has_incumbent", "best_lower", "total_pivots", "cutloop_rounds", "cutloop_rows", "cutloop_purged",
        "cutloop_live_rows", "cutloop_lps", "cutloop_pivots", "cutloop_bound0", "cutloop_bound")
BINARY = ((24, 48, 5, 1, 0.06), (32, 64, 7, 1, 0.045), (64, 128, 7, 1, 0.025), (32, 64, 7, 1, 0.05))
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
    from tests.test_bnb_general import INSTANCES, instance

    orc = oracle.api()
    tab = bnb.table_from(orc)
    assert not tab.del_rows
    fixtures = [(rec, instance(rec)) for rec in INSTANCES[::4] if rec["status"] == "optimal"]

    def sweep(label, loads, **kw):
        for A in range(5):
            tot = dict(nodes=0, tree_pivots=0, loop_pivots=0, rows=0, purged=0, work=0, purging_instances=0, missed=0)
            for load, opt in loads:
                P = load()
                m0 = P.m
                r = bnb.branch_and_bound(P, quirks=0, table=tab, window=64, max_nodes=200000, cut_purge=A, **kw)
                assert r["rc"] == 0 and not r["hit_limit"]
                tot["nodes"] += r["n_nodes"]
                tot["tree_pivots"] += r["total_pivots"]
                tot["loop_pivots"] += r["cutloop_pivots"]
                tot["rows"] += r["cutloop_rows"]
                tot["purged"] += r["cutloop_purged"]
                tot["purging_instances"] += r["cutloop_purged"] > 0
                tot["work"] += r["total_pivots"] * (m0 + r["cutloop_live_rows"] + 1)
                tot["missed"] += opt is not None and abs(r["best_lower"] - opt) > 1e-6 * (1 + abs(opt))
            emit(dict({"part": "cpu", "set": label, "instances": len(loads), "cut_purge": A}, **kw, **tot), out)

    sweep("general fixtures, every 4th with an optimum", [((lambda inst=inst: lpgen.load_milp(orc, inst)), rec["optimum"]) for rec, inst in fixtures],
          cut_rounds=5)
    for case in BINARY:
        model = synth.dense_ilp(*case)
        opt = bnb.branch_and_bound(synth.load_ilp(orc, *model), quirks=0, table=tab, window=64, max_nodes=200000)["best_lower"]
        sweep("dense_ilp%r" % (case,), [((lambda model=model: synth.load_ilp(orc, *model)), opt)], cut_rounds=10, cut_families=3)


def part_call(out):
    import numpy as np
    from mvolps_amd import bnb
    from mvolps_amd.capi import BS, OPT

    from scripts.cutloop_profile import wide_root_cuts

    gpu, root, vals, rhs = wide_root_cuts(256)
    base = root.copy()
    m0 = base.m
    assert bnb.add_cut_rows(base, vals[:128], rhs[:128]) == 0
    base.simplex()
    assert base.status == OPT
    stat = np.array(base.row_stat())
    slack = [i for i in range(base.m, 0, -1) if stat[i - 1] == BS]  # the cut rows first
    for k in (8, 32, 128):
        rows = sorted(slack[:k])
        assert len(rows) == k
        dele, app = [], []
        for rep in range(8):
            a, b = base.copy(), base.copy()
            gpu.sync()
            t0 = time.perf_counter()
            assert a.del_rows(rows) == 0
            gpu.sync()
            t1 = time.perf_counter()
            assert bnb.add_cut_rows(b, vals[128:128 + k], rhs[128:128 + k]) == 0
            gpu.sync()
            t2 = time.perf_counter()
            if rep:  # the first repetition warms both paths up
                dele.append(t1 - t0)
                app.append(t2 - t1)
        it0 = a.it_cnt
        a.simplex()
        emit({"part": "del_rows", "instance": "512x1024 cap 0.4 U 3 root + 128 GMI rows", "rows": base.m, "k": k, "cut_rows_among_them":
              sum(1 for i in rows if i > m0), "first_row": rows[0], "reps": len(dele), "del_rows_ms": statistics.median(dele) * 1e3,
              "add_cut_rows_ms": statistics.median(app) * 1e3, "pivots_after": a.it_cnt - it0, "same_objective": bool(a.obj == base.obj)}, out)


def part_device(out, out_trees):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    part_call(out)

    def tree(model, **kw):
        t0 = time.perf_counter()
        r = bnb.branch_and_bound(synth.load_ilp(mvolps_amd.api(), *model), quirks=0, window=64, **kw)
        return r, time.perf_counter() - t0

    cases = (("config-5", config5(), 1, 2 * 15697), ("config-5", config5(), 3, 2 * 15697),
             ("dense_ilp(64,128,7,1,0.025)", synth.dense_ilp(64, 128, 7, 1, 0.025), 3, 200000), ("512x1024 cap 0.4 U 3", synth.dense_ilp(*WIDE), 1, 20000))
    for name, model, fam, limit in cases:
        tree(model, cut_rounds=1, cut_families=fam, cut_purge=1, max_nodes=1)  # warm-up
        for rep in range(2):
            for A in (0, 1, 3):
                r, el = tree(model, cut_rounds=5, cut_families=fam, cut_purge=A, max_nodes=limit)
                emit(dict({"part": "trees", "instance": name, "window": 64, "max_nodes": limit, "cut_rounds": 5, "cut_families": fam, "cut_purge": A,
                           "rep": rep, "rc": r["rc"], "seconds": el}, **{k: r[k] for k in KEYS}), out_trees)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["cpu", "call", "device"], required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--out-trees", default=None)
    a = ap.parse_args()
    if a.part == "cpu":
        part_cpu(a.out)
    elif a.part == "call":
        part_call(a.out)
    else:
        part_device(a.out, a.out_trees)


if __name__ == "__main__":
    main()
