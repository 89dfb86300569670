"""Measurements behind DESIGN.md "Clique cuts in the tree (node_cliques)" (mvx_clique_cuts_many, k_cliquesep,
mvx_bnb_params.node_cliques).

  --part cpu      no device: whole trees over the oracle's table (the twin separates, the rows go in one by one) on the binary
                  dense_ilp models of the clique table, window 64: K = 0 / 1 / 4 / 16, without root rounds and behind cut_rounds = 5
                  with cut_families = 3, without the tree's purge and with node_purge = 2.
  --part device   one mvx_clique_cuts_many call over 64 solved nodes (bnb.node_sample) of config 5 (512x1024, cap 0.002) and of
                  the 128x256 cap 0.01 sample, K = 4 and 16, against the host twin mvx_bnb_clique_masks on the same handles with the
                  graph in hand.  Host clocks around calls that end in a synchronise, one warm-up first, medians of 7.
  --part trees    config 5 and 64x128 cap 0.025 to the end at window 64, repaired, K = 0 (the parent's tree) / 4 / 16, two
                  alternating runs each.
One JSON object per line on stdout (and appended to --out when given)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("count", "n_nodes", "hit_limit", "has_incumbent", "best_lower", "total_pivots", "node_clique_conflicts", "node_clique_calls",
        "node_clique_rows", "node_purge_rows", "node_cut_rows_peak", "cutloop_rows")
BINARY = ((24, 48, 5, 1, 0.06), (32, 64, 7, 1, 0.05), (32, 64, 7, 1, 0.045), (64, 128, 7, 1, 0.025), (32, 64, 7, 1, 0.03),
          (16, 32, 9, 1, 0.2), (10, 20, 3, 1, 0.1))


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
        for rounds in (dict(), dict(cut_rounds=5, cut_families=3)):
            for purge in (0, 2):
                for K in (0, 1, 4, 16):
                    t0 = time.perf_counter()
                    r = bnb.branch_and_bound(synth.load_ilp(orc, *model), quirks=0, table=tab, window=64, max_nodes=200000, node_cliques=K,
                                             node_purge=purge, **rounds)
                    emit(dict({"part": "cpu", "model": list(case), "node_cliques": K, "node_purge": purge, "rc": r["rc"],
                               "seconds": time.perf_counter() - t0}, **rounds, **{k: r[k] for k in KEYS}), out)


def part_device(out):
    import mvolps_amd
    import numpy as np
    from mvolps_amd import bnb, synth

    gpu = mvolps_amd.api()
    for name, model in (("config-5 512x1024 cap 0.002", config5()), ("128x256 cap 0.01", synth.dense_ilp(128, 256, 7, 1, 0.01))):
        root = synth.load_ilp(gpu, *model)
        nodes = bnb.node_sample(root, 64, quirks=0)
        rc, words, edges = bnb.conflict_words(root, table=None)
        assert rc == 0
        for K in (4, 16):
            dev, host = [], []
            for rep in range(8):
                gpu.sync()
                t0 = time.perf_counter()
                d = bnb.clique_cuts_many(root, nodes, K)  # ends in a synchronise
                t1 = time.perf_counter()
                h = bnb.clique_cuts_many(root, nodes, K, table=None, adj=words)
                t2 = time.perf_counter()
                assert d[0] == h[0] == 0
                if rep:  # the first repetition computes the graph on the device and warms both paths up
                    dev.append(t1 - t0)
                    host.append(t2 - t1)
            same = bool(np.array_equal(d[1], h[1]) and np.array_equal(d[2], h[2]) and np.array_equal(d[3].view(np.uint64), h[3].view(np.uint64)))
            n = root.n
            emit({"part": "device", "instance": name, "handles": len(nodes), "n": n, "W": (n + 1 + 63) // 64, "edges": edges,
                  "density": edges / (n * (n - 1) / 2), "max_cuts": K, "reps": len(dev), "kept": int(d[1].sum()),
                  "seeds_per_node": float(np.mean([sum(1 for v in P.col_prim() if v > 1e-6) for P in nodes])),
                  "device_ms": statistics.median(dev) * 1e3, "twin_ms": statistics.median(host) * 1e3, "same_bits": same}, out)


def part_trees(out):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    def tree(model, **kw):
        t0 = time.perf_counter()
        r = bnb.branch_and_bound(synth.load_ilp(mvolps_amd.api(), *model), quirks=0, window=64, **kw)
        return r, time.perf_counter() - t0

    for name, model in (("config 5", config5()), ("64x128 cap 0.025", synth.dense_ilp(64, 128, 7, 1, 0.025))):
        tree(model, max_nodes=20, node_cliques=4)  # warm-up
        for rep in range(2):
            for K in (0, 4, 16):
                r, el = tree(model, node_cliques=K, max_nodes=2 * 15697)
                emit(dict({"part": "trees", "instance": name, "node_cliques": K, "rep": rep, "rc": r["rc"], "seconds": el,
                           "nodes_per_s": r["count"] / el}, **{k: r[k] for k in KEYS}), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["cpu", "device", "trees"], required=True)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"cpu": part_cpu, "device": part_device, "trees": part_trees}[a.part](a.out)


if __name__ == "__main__":
    main()
