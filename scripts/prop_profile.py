"""Measurements behind DESIGN.md "Node bound propagation" (mvx_bnb_params.prop).

  --part trees    config 5 closed plain and with prop 8, then at heur 2 + rc_fix and the same plus prop 8 (FIFO, window 64),
                  twice each, alternating: nodes, pivots, seconds, counters.
  --part window   the unsolved children of a 64-node window of config 5: one mvx_propagate_many call (k_prop) against the host
                  twin per child (mvx_bnb_propagate through the engine's table), and one mvx_set_col_bnds_many call (k_setbnds)
                  with the resulting lists against mvx_set_col_bnds per entry on clones of the same children.
  --part wide     the wide instance (512x1024, cap 0.4, U = 3), 2000 nodes at window 64, plain and with prop 8: what the
                  calls cost where the rows are far from tight.
  --part trace    the prop 8 tree of config 5 alone: run under `rocprofv3 --kernel-trace --stats` for the launch counts and
                  times of k_prop and k_setbnds.
One JSON object per line on stdout (and appended to --out when given)."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("count", "hit_limit", "has_incumbent", "best_lower", "total_pivots", "incumbent_oid", "heur_calls", "heur_improved", "rc_calls",
        "rc_fixed", "prop_calls", "prop_fixed", "prop_tightened", "prop_infeasible")


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


def tree(model, **kw):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    t0 = time.perf_counter()
    r = bnb.branch_and_bound(synth.load_ilp(mvolps_amd.api(), *model), quirks=0, window=64, **kw)
    return r, time.perf_counter() - t0


def part_trees(out):
    model = config5()
    tree(model, prop=8)  # warm-up
    for base in (dict(), dict(heur=2, rc_fix=1)):
        for rep in range(2):
            for prop in (0, 8):
                r, el = tree(model, prop=prop, **base)
                emit(dict({"part": "trees", "instance": "config-5", "options": base, "prop": prop, "window": 64, "rep": rep, "rc": r["rc"],
                           "seconds": el}, **{k: r[k] for k in KEYS}), out)


def part_wide(out):
    from mvolps_amd import synth

    model = synth.dense_ilp(512, 1024, 12345, 3, 0.4)
    tree(model, prop=8, max_nodes=200)  # warm-up
    for rep in range(2):
        for prop in (0, 8):
            r, el = tree(model, prop=prop, max_nodes=2000)
            emit(dict({"part": "wide", "instance": "512x1024 cap 0.4 U 3", "prop": prop, "window": 64, "max_nodes": 2000, "rep": rep, "rc": r["rc"],
                       "seconds": el}, **{k: r[k] for k in KEYS}), out)


def set_bounds(gpu, P, j, lb, ub):
    from mvolps_amd.capi import DB, FX, LO, UP

    hl, hu = math.isfinite(lb), math.isfinite(ub)
    gpu.set_col_bnds(P.h, j, (FX if lb == ub else DB) if hl and hu else LO if hl else UP, lb if hl else 0.0, ub if hu else 0.0)


def part_window(out, reps):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    gpu = mvolps_amd.api()
    root = synth.load_ilp(gpu, *config5())
    nodes = bnb.node_sample(root, 64)

    def children():
        kids = []
        for P in nodes:
            _st, viol = bnb.print_info(P, quirks=0)
            if viol:
                kids += list(bnb.make_children(P, viol[0], quirks=0))
        return kids[:64]

    kids = children()
    rc, res = bnb.propagate_many(root, kids, 8)  # warm-up: the model's second orientation, buffers
    assert rc == 0
    t0 = time.perf_counter()
    for _ in range(reps):
        assert bnb.propagate_many(root, kids, 8)[0] == 0
    dev = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    for S in kids:
        assert bnb.propagate_node(S, root, 8)[0] == 0
    host = time.perf_counter() - t0
    lists = [lst for _inf, _rounds, lst in res]
    emit({"part": "window", "entry": "mvx_propagate_many", "instance": "config-5", "children": len(kids), "entries": sum(len(l) for l in lists),
          "infeasible": sum(r[0] for r in res), "rounds": sorted({r[1] for r in res}), "device_call_ms": dev * 1e3, "host_twin_ms": host * 1e3,
          "reps": reps}, out)
    assert bnb.set_col_bnds_many(children(), lists) == 0  # warm-up
    many, one = [], []
    for _ in range(5):
        kids = children()
        kids[-1].tableau()  # the clones have landed: the timed call starts from an idle stream
        t0 = time.perf_counter()
        assert bnb.set_col_bnds_many(kids, lists) == 0
        many.append(time.perf_counter() - t0)
        kids = children()
        t0 = time.perf_counter()
        for S, l in zip(kids, lists):
            for (j, lb, ub) in l:
                set_bounds(gpu, S, j, lb, ub)
        kids[-1].tableau()  # ends in a device synchronise
        one.append(time.perf_counter() - t0)
    emit({"part": "window", "entry": "mvx_set_col_bnds_many", "instance": "config-5", "children": len(kids), "entries": sum(len(l) for l in lists),
          "one_call_ms": min(many) * 1e3, "set_col_bnds_per_entry_ms": min(one) * 1e3, "runs": 5}, out)


def part_trace(out):
    r, el = tree(config5(), prop=8)
    emit(dict({"part": "trace", "prop": 8, "seconds": el}, **{k: r[k] for k in KEYS}), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["trees", "window", "wide", "trace"], required=True)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.part == "trees":
        part_trees(a.out)
    elif a.part == "window":
        part_window(a.out, a.reps)
    elif a.part == "wide":
        part_wide(a.out)
    else:
        part_trace(a.out)


if __name__ == "__main__":
    main()
