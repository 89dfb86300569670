"""Measurements behind DESIGN.md "Incumbent polishing (polish)" (mvx_polish_many, k_lsmove, mvx_bnb_params.polish).

  --part cpu      no device: whole trees over the oracle's table, where the host twin mvx_bnb_polish runs, on the six small
                  dense_ilp models of the section's table, with polish 0 and 1000 under heur 2, with and without rc_fix, in FIFO
                  order at window 64 and in best-bound order (node at a time: rc_fix is not in the best-bound window), cut at
                  20 000 nodes: nodes, tree pivots, the incumbent's objective and the oid it arrived at.
  --part device   one mvx_polish_many call on the heur 2 point of the wide 512x1024 root against the twin mvx_bnb_polish through
                  the engine's own table: host clocks around calls that end in a synchronise, one warm-up first, medians of 7.
                  Then the wide tree and config 5 at window 64 with heur 2 and polish 0 / 1000, two alternating runs each, cut at
                  20 000 nodes.  The polish = 0 runs of the same session stand for the code without the feature.
One JSON object per line on stdout (and appended to --out when given)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("count", "n_nodes", "hit_limit", "has_incumbent", "best_lower", "incumbent_oid", "incumbent_heur", "total_pivots", "heur_calls",
        "heur_improved", "polish_calls", "polish_moves", "polish_improved", "rc_calls", "rc_fixed", "rc_tightened")
SMALL = ((10, 20, 3, 3, 0.4), (24, 48, 5, 3, 0.3), (32, 64, 7, 3, 0.4), (64, 128, 7, 3, 0.4), (128, 256, 7, 3, 0.4), (32, 64, 7, 1, 0.2))
WIDE = (512, 1024, 12345, 3, 0.4)
LIMIT = 20000


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
    assert not tab.polish_many
    orders = (("fifo window 64", dict(window=64)), ("best bound", dict(node_strat=1, window=1)))
    for case in SMALL:
        model = synth.dense_ilp(*case)
        for order, okw in orders:
            for rc_fix in (0, 1):
                for polish in (0, 1000):
                    t0 = time.perf_counter()
                    r = bnb.branch_and_bound(synth.load_ilp(orc, *model), quirks=0, table=tab, heur=2, rc_fix=rc_fix, polish=polish,
                                             max_nodes=LIMIT, **okw)
                    assert r["rc"] == 0
                    emit(dict({"part": "cpu", "model": "dense_ilp%r" % (case,), "order": order, "max_nodes": LIMIT, "heur": 2, "rc_fix": rc_fix,
                               "polish": polish, "seconds": time.perf_counter() - t0}, **{k: r[k] for k in KEYS}), out)


def part_device(out):
    import mvolps_amd
    import numpy as np
    from mvolps_amd import bnb, synth
    from mvolps_amd.capi import OPT

    gpu = mvolps_amd.api()
    model = synth.dense_ilp(*WIDE)
    root = synth.load_ilp(gpu, *model)
    node = root.copy()
    node.simplex()
    assert node.status == OPT
    rc, obj, found, x = bnb.round_many(root, [node], 2)
    assert rc == 0 and found[0]
    dev, host, got = [], [], None
    for rep in range(8):
        gpu.sync()
        t0 = time.perf_counter()
        d = bnb.polish_many(root, x, 1000)
        gpu.sync()
        t1 = time.perf_counter()
        h = bnb.polish_many(root, x, 1000, table=None)
        t2 = time.perf_counter()
        assert d[0] == h[0] == 0 and all(np.array_equal(a, b) for a, b in zip(d[1:], h[1:]))
        got = d
        if rep:  # the first repetition warms both paths up (the model's upload among them)
            dev.append(t1 - t0)
            host.append(t2 - t1)
    emit({"part": "polish_many", "instance": "512x1024 cap 0.4 U 3, the root's heur 2 point", "root_lp": node.obj, "entry_obj": float(obj[0]),
          "obj": float(got[2][0]), "moves": int(got[3][0]), "ok": int(got[4][0]), "reps": len(dev), "device_ms": statistics.median(dev) * 1e3,
          "twin_ms": statistics.median(host) * 1e3, "same_bits": True}, out)

    def tree(model, **kw):
        t0 = time.perf_counter()
        r = bnb.branch_and_bound(synth.load_ilp(mvolps_amd.api(), *model), quirks=0, window=64, heur=2, **kw)
        return r, time.perf_counter() - t0

    for name, m in (("512x1024 cap 0.4 U 3", model), ("config-5", config5())):
        tree(m, polish=1000, max_nodes=64)  # warm-up
        for rep in range(2):
            for polish in (0, 1000):
                r, el = tree(m, polish=polish, max_nodes=LIMIT)
                emit(dict({"part": "trees", "instance": name, "window": 64, "max_nodes": LIMIT, "heur": 2, "polish": polish, "rep": rep,
                           "rc": r["rc"], "seconds": el}, **{k: r[k] for k in KEYS}), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["cpu", "device"], required=True)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.part == "cpu":
        part_cpu(a.out)
    else:
        part_device(a.out)


if __name__ == "__main__":
    main()
