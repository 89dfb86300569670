"""Measurements behind DESIGN.md "Clique cuts (cut_families)" (mvx_bnb_params.cut_families).

  --part cpu      no device: the loop over the oracle's table on the binary dense_ilp models, cut_families 1 / 2 / 3 at 10 rounds:
                  conflict density, root LP by round, rows appended, and the trees' nodes at 5 rounds.
  --part graph    one mvx_conflict_graph call against the host twin mvx_bnb_conflict_graph on the same handle, for the config-5
                  instance (512x1024, cap 0.002) and the 128x256 sample: host clocks around calls that end in a synchronise, one
                  warm-up first, medians of 7.
  --part trees    config 5 to the end at window 64, repaired: plain and heur 2 + rc_fix, cut_rounds 5 under cut_families 1 / 2 / 3,
                  two alternating runs each.
One JSON object per line on stdout (and appended to --out when given)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("count", "n_nodes", "hit_limit", "has_incumbent", "best_lower", "total_pivots", "cutloop_rounds", "cutloop_candidates", "cutloop_rows",
        "cutloop_lps", "cutloop_pivots", "cutloop_bound0", "cutloop_bound", "cutloop_conflicts", "cutloop_clique_cands",
        "cutloop_clique_rows")
BINARY = ((10, 20, 3, 1, 0.1), (32, 64, 7, 1, 0.03), (128, 256, 7, 1, 0.01), (24, 48, 5, 1, 0.06), (32, 64, 7, 1, 0.045),
          (64, 128, 7, 1, 0.025), (32, 64, 7, 1, 0.05), (16, 32, 9, 1, 0.2))


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

    orc = oracle.api()
    tab = bnb.table_from(orc)
    for case in BINARY:
        model = synth.dense_ilp(*case)
        n = case[1]
        _rc, _adj, edges = bnb.conflict_graph(synth.load_ilp(orc, *model), table=tab)
        base = bnb.branch_and_bound(synth.load_ilp(orc, *model), quirks=0, table=tab, window=64, max_nodes=200000)
        for fam in (1, 2, 3):
            bounds, rows = [], 0
            for R in range(1, 11):  # the loop of R rounds from the start, so that the graph is the model's own every time
                rc, o = bnb.cut_loop(synth.load_ilp(orc, *model), rounds=R, table=tab, families=fam)
                assert rc == 0
                bounds = bounds or [o["cutloop_bound0"]]
                if o["cutloop_rounds"] < R:
                    break
                bounds.append(o["cutloop_bound"])
                rows = o["cutloop_rows"]
            r = bnb.branch_and_bound(synth.load_ilp(orc, *model), quirks=0, table=tab, window=64, max_nodes=200000, cut_rounds=5,
                                     cut_families=fam)
            emit({"part": "cpu", "model": list(case), "cut_families": fam, "edges": edges, "density": edges / (n * (n - 1) / 2),
                  "optimum": base["best_lower"], "root_lp_by_round": bounds, "rows_10_rounds": rows, "nodes_without_loop": base["n_nodes"],
                  "nodes_cut_rounds_5": r["n_nodes"], "hit_limit": r["hit_limit"], "best_lower": r["best_lower"]}, out)


def part_graph(out):
    import mvolps_amd
    import numpy as np
    from mvolps_amd import bnb, synth

    gpu = mvolps_amd.api()
    for name, model in (("config-5 512x1024 cap 0.002", config5()), ("128x256 cap 0.01", synth.dense_ilp(128, 256, 7, 1, 0.01))):
        P = synth.load_ilp(gpu, *model)
        dev, host = [], []
        for rep in range(8):
            gpu.sync()
            t0 = time.perf_counter()
            rc, words, edges = bnb.conflict_words(P)  # ends in the entry's own synchronise
            t1 = time.perf_counter()
            trc, twords, tedges = bnb.conflict_words(P, table=None)
            t2 = time.perf_counter()
            assert rc == 0 and trc == 0
            if rep:  # the first repetition uploads the model and warms both paths up
                dev.append(t1 - t0)
                host.append(t2 - t1)
        n = P.n
        emit({"part": "graph", "instance": name, "reps": len(dev), "edges": edges, "density": edges / (n * (n - 1) / 2),
              "mvx_conflict_graph_ms": statistics.median(dev) * 1e3, "mvx_bnb_conflict_graph_ms": statistics.median(host) * 1e3,
              "same_words": bool(np.array_equal(words, twords) and edges == tedges)}, out)


def part_trees(out):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    model = config5()

    def tree(**kw):
        t0 = time.perf_counter()
        r = bnb.branch_and_bound(synth.load_ilp(mvolps_amd.api(), *model), quirks=0, window=64, **kw)
        return r, time.perf_counter() - t0

    tree(cut_rounds=1, cut_families=3, max_nodes=1)  # warm-up
    for rep in range(2):
        for extra in (dict(), dict(heur=2, rc_fix=1)):
            for fam in (1, 2, 3):
                r, el = tree(cut_rounds=5, cut_families=fam, max_nodes=2 * 15697, **extra)
                emit(dict({"part": "trees", "instance": "config-5", "window": 64, "cut_rounds": 5, "cut_families": fam, "rep": rep, "rc": r["rc"],
                           "seconds": el}, **extra, **{k: r[k] for k in KEYS}), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["cpu", "graph", "trees"], required=True)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"cpu": part_cpu, "graph": part_graph, "trees": part_trees}[a.part](a.out)


if __name__ == "__main__":
    main()
