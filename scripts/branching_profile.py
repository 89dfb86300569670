"""Measurements behind DESIGN.md "Branching on the node LP" (var_strat 3 / 4).

  --part penalty  k_penalty on a 64-node window of the wide 512 x 1024 ILP (mvx_branch_penalties_many, one launch for every
                  candidate of every node) against the host twin on the same window (mvx_bnb_penalties: one tableau export
                  per node).  Run it under `rocprofv3 --kernel-trace --stats` for the per-launch kernel time.
  --part trees    node count and wall time to close the calibrated config-5 instance under VO, var_strat 3 and var_strat 4
                  (window 64), and how far the wide 512 x 1024 instance gets under var_strat 4 within a node cap.
One JSON object per line on stdout (and appended to --out when given)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def part_penalty(out, reps):
    import mvolps_amd
    from mvolps_amd import bnb
    from tests.test_gpu_branching import node_set

    gpu = mvolps_amd.api()
    nodes, _keep = node_set(gpu, (512, 1024, 12345, 3, 0.4), 64)
    hs, cols = [P for P, _ in nodes], [c for _, c in nodes]
    ncand = sum(len(c) for c in cols)
    bnb.branch_penalties_many(hs, cols)  # warm-up: buffers
    t0 = time.perf_counter()
    for _ in range(reps):
        rc, _ = bnb.branch_penalties_many(hs, cols)
        assert rc == 0
    dev = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    for _ in range(max(1, reps // 10)):
        for P, c in nodes:
            rc, _ = bnb.penalties(P, c)
            assert rc == 0
    host = (time.perf_counter() - t0) / max(1, reps // 10)
    emit({"part": "penalty", "instance": "wide 512x1024 (cap 0.4, U 3)", "nodes": len(nodes), "candidates": ncand,
          "device_call_ms": dev * 1e3, "host_twin_ms": host * 1e3, "reps": reps}, out)


def part_trees(out, wide_cap):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    gpu = mvolps_amd.api()
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "config5.json")))
    A, b, c, U = synth.dense_ilp(fx["m"], fx["n"], fx["seed"], fx["U"], fx["cap"])
    bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), quirks=0, max_nodes=64)  # warm-up
    for vs in (0, 3, 4):
        t0 = time.perf_counter()
        r = bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), var_strat=vs, quirks=0, window=64, max_nodes=200000)
        el = time.perf_counter() - t0
        emit({"part": "trees", "instance": "config-5 (cap %g, U %g)" % (fx["cap"], fx["U"]), "var_strat": vs, "window": 64, "rc": r["rc"],
              "nodes": r["count"], "closed": not r["hit_limit"], "best_lower": r["best_lower"], "seconds": el,
              "total_pivots": r["total_pivots"], "sb_lps": r["sb_lps"], "sb_pivots": r["sb_pivots"]}, out)
    A, b, c, U = synth.dense_ilp(512, 1024, 12345, 3, 0.4)
    for vs in (0, 4):
        t0 = time.perf_counter()
        r = bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), var_strat=vs, quirks=0, window=64, max_nodes=wide_cap)
        el = time.perf_counter() - t0
        emit({"part": "trees", "instance": "wide 512x1024 (cap 0.4, U 3)", "var_strat": vs, "window": 64, "node_cap": wide_cap, "rc": r["rc"],
              "nodes": r["count"], "closed": not r["hit_limit"], "best_lower": r["best_lower"], "seconds": el,
              "total_pivots": r["total_pivots"], "sb_lps": r["sb_lps"], "sb_pivots": r["sb_pivots"]}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["penalty", "trees"], required=True)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--wide-cap", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.part == "penalty":
        part_penalty(a.out, a.reps)
    else:
        part_trees(a.out, a.wide_cap)


if __name__ == "__main__":
    main()
