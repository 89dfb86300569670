"""Measurements behind DESIGN.md "Primal rounding heuristic" (mvx_bnb_params.heur).

  --part window   k_round on a 64-node window of the wide 512 x 1024 ILP (mvx_round_many, one launch for every node) against
                  the host twin on the same window (mvx_bnb_round through the engine's table).  Run it under
                  `rocprofv3 --kernel-trace --stats` for the per-launch kernel time.
  --part trees    config 5 (the calibrated 512 x 1024 instance) closed at heur 0 / 1 / 2 (FIFO, window 64): nodes, seconds,
                  where the final incumbent came from; the wide 512 x 1024 instance at heur 0 / 2 within a node cap:
                  incumbent, its gap to the root LP bound, nodes per second.
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


def part_window(out, reps):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    gpu = mvolps_amd.api()
    A, b, c, U = synth.dense_ilp(512, 1024, 12345, 3, 0.4)
    root = synth.load_ilp(gpu, A, b, c, U)
    nodes = bnb.node_sample(root, 64)
    for mode in (1, 2):
        bnb.round_many(root, nodes, mode)  # warm-up: buffers, the model upload
        t0 = time.perf_counter()
        for _ in range(reps):
            rc, _o, found, _x = bnb.round_many(root, nodes, mode)
            assert rc == 0
        dev = (time.perf_counter() - t0) / reps
        t0 = time.perf_counter()
        for P in nodes:
            assert bnb.round_node(P, root, mode)[0] == 0
        host = time.perf_counter() - t0
        emit({"part": "window", "instance": "wide 512x1024 (cap 0.4, U 3)", "mode": mode, "nodes": len(nodes), "found": int(found.sum()),
              "device_call_ms": dev * 1e3, "host_twin_ms": host * 1e3, "reps": reps}, out)


def part_trees(out, wide_cap):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    gpu = mvolps_amd.api()
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "config5.json")))
    A, b, c, U = synth.dense_ilp(fx["m"], fx["n"], fx["seed"], fx["U"], fx["cap"])
    bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), quirks=0, max_nodes=64, heur=2)  # warm-up
    keys = ("count", "hit_limit", "best_lower", "total_pivots", "incumbent_oid", "incumbent_heur", "heur_calls", "heur_found", "heur_improved")
    for h in (0, 1, 2):
        t0 = time.perf_counter()
        r = bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), quirks=0, window=64, heur=h)
        el = time.perf_counter() - t0
        emit(dict({"part": "trees", "instance": "config-5 (cap %g, U %g)" % (fx["cap"], fx["U"]), "heur": h, "window": 64, "rc": r["rc"],
                   "seconds": el}, **{k: r[k] for k in keys}), out)
    A, b, c, U = synth.dense_ilp(512, 1024, 12345, 3, 0.4)
    root = synth.load_ilp(gpu, A, b, c, U)
    R = root.copy()
    R.simplex()
    lp = R.obj
    for h in (0, 2):
        t0 = time.perf_counter()
        r = bnb.branch_and_bound(synth.load_ilp(gpu, A, b, c, U), quirks=0, window=64, heur=h, max_nodes=wide_cap)
        el = time.perf_counter() - t0
        gap = (lp - r["best_lower"]) / abs(lp) if r["has_incumbent"] else None
        emit(dict({"part": "trees", "instance": "wide 512x1024 (cap 0.4, U 3)", "heur": h, "window": 64, "node_cap": wide_cap, "rc": r["rc"],
                   "seconds": el, "nodes_per_s": r["count"] / el, "root_lp": lp, "has_incumbent": r["has_incumbent"], "gap": gap},
                  **{k: r[k] for k in keys}), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["window", "trees"], required=True)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--wide-cap", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.part == "window":
        part_window(a.out, a.reps)
    else:
        part_trees(a.out, a.wide_cap)


if __name__ == "__main__":
    main()
