"""Measurements behind DESIGN.md "Reduced-cost tightening" (mvx_bnb_params.rc_fix).

  --part window   a 64-node window of the config-5 instance against the cutoff 20: one mvx_rc_tighten_many call (k_rcfix) against
                  the host twin on every node (mvx_bnb_rc_tighten through the engine's table: a tableau export per node), and
                  one mvx_tighten_cols_many call (k_setbnds) for the two children of every node against mvx_set_col_bnds per
                  entry on clones of the same children.
  --part trees    config 5 closed at heur 2 and at heur 2 + rc_fix (FIFO, window 64), twice each, alternating: nodes, pivots,
                  seconds, counters.
  --part trace    the heur 2 + rc_fix tree alone, then the heur 2 tree alone when --off is given: run under
                  `rocprofv3 --kernel-trace --stats` for the launch counts of k_rcfix, k_setbnds and k_set_nonbasic.
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


def config5():
    from mvolps_amd import synth

    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "config5.json")))
    return synth.dense_ilp(fx["m"], fx["n"], fx["seed"], fx["U"], fx["cap"])


def part_window(out, reps):
    import mvolps_amd
    from mvolps_amd import bnb, synth
    from mvolps_amd.capi import DB, FX

    gpu = mvolps_amd.api()
    A, b, c, U = config5()
    nodes = bnb.node_sample(synth.load_ilp(gpu, A, b, c, U), 64)
    cut = [20.0] * len(nodes)
    rc, lists = bnb.rc_tighten_many(nodes, cut)  # warm-up: buffers
    assert rc == 0
    t0 = time.perf_counter()
    for _ in range(reps):
        assert bnb.rc_tighten_many(nodes, cut)[0] == 0
    dev = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    for P in nodes:
        assert bnb.rc_tighten_node(P, 20.0)[0] == 0
    host = time.perf_counter() - t0
    emit({"part": "window", "entry": "mvx_rc_tighten_many", "instance": "config-5", "nodes": len(nodes), "entries": sum(len(l) for l in lists),
          "device_call_ms": dev * 1e3, "host_twin_ms": host * 1e3, "reps": reps}, out)

    def children():
        kids, kl = [], []
        for P, l in zip(nodes, lists):
            _st, viol = bnb.print_info(P, quirks=0)
            if viol:
                for S in bnb.make_children(P, viol[0], quirks=0):
                    kids.append(S)
                    kl.append(l)
        return kids, kl

    kids, kl = children()
    assert bnb.tighten_cols_many(kids, kl) == 0  # warm-up
    many, one = [], []
    for _ in range(5):
        kids, kl = children()
        kids[-1].tableau()  # the clones have landed: the timed call starts from an idle stream
        t0 = time.perf_counter()
        assert bnb.tighten_cols_many(kids, kl) == 0
        many.append(time.perf_counter() - t0)
        kids, kl = children()
        t0 = time.perf_counter()
        for S, l in zip(kids, kl):
            for (j, lb, ub) in l:
                gpu.set_col_bnds(S.h, j, FX if lb == ub else DB, lb, ub)
        kids[-1].tableau()  # ends in a device synchronise
        one.append(time.perf_counter() - t0)
    emit({"part": "window", "entry": "mvx_tighten_cols_many", "instance": "config-5", "children": len(kids), "entries": sum(len(l) for l in kl),
          "one_call_ms": min(many) * 1e3, "set_col_bnds_per_entry_ms": min(one) * 1e3, "runs": 5}, out)


KEYS = ("count", "hit_limit", "best_lower", "total_pivots", "incumbent_oid", "incumbent_heur", "heur_calls", "heur_improved", "rc_calls", "rc_fixed",
        "rc_tightened")


def tree(rc_fix, heur=2):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    A, b, c, U = config5()
    t0 = time.perf_counter()
    r = bnb.branch_and_bound(synth.load_ilp(mvolps_amd.api(), A, b, c, U), quirks=0, window=64, heur=heur, rc_fix=rc_fix)
    return r, time.perf_counter() - t0


def part_trees(out):
    tree(1)  # warm-up
    for rep in range(2):
        for rc_fix in (0, 1):
            r, el = tree(rc_fix)
            emit(dict({"part": "trees", "instance": "config-5", "heur": 2, "rc_fix": rc_fix, "window": 64, "rep": rep, "rc": r["rc"], "seconds": el},
                      **{k: r[k] for k in KEYS}), out)


def part_trace(out, off):
    r, el = tree(0 if off else 1)
    windows = sum(1 for e in r["events"] if e[0] == 0)  # popped nodes; the rounds are fewer
    emit(dict({"part": "trace", "rc_fix": 0 if off else 1, "seconds": el, "popped": windows}, **{k: r[k] for k in KEYS}), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["window", "trees", "trace"], required=True)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--off", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.part == "window":
        part_window(a.out, a.reps)
    elif a.part == "trees":
        part_trees(a.out)
    else:
        part_trace(a.out, a.off)


if __name__ == "__main__":
    main()
