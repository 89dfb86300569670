"""Measurements behind DESIGN.md "Feasibility pump" (mvx_bnb_params.pump).

  --part rounds   root pumps of the wide instance (512x1024, cap 0.4, U = 3) written out in Python over the same entries the
                  driver uses, host clocks around the synchronising calls: per round the objective step (mvx_pump_obj_many), the
                  objective apply (mvx_set_obj_many) and the batched solve (mvx_simplex_batch), for the pump of the root and for
                  8 lockstep pumps (the root and seven nodes below it); then one objective of the root applied column by column
                  (mvx_set_obj_coef) against the one call, and the twin's time for the same steps.
  --part trees    config 5 to the end and the wide instance to 20 000 nodes at window 64, repaired, heur 2: pump 30 (alpha 0 and
                  0.9) against its own pump = 0 base from the same run, alternating: nodes, pivots, seconds, the oid of the final
                  incumbent, the pumps' counters.
One JSON object per line on stdout (and appended to --out when given)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("count", "hit_limit", "has_incumbent", "best_lower", "total_pivots", "incumbent_oid", "incumbent_heur", "heur_calls", "heur_improved",
        "pump_calls", "pump_found", "pump_improved", "pump_lps", "pump_pivots")
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


def tree(model, **kw):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    t0 = time.perf_counter()
    r = bnb.branch_and_bound(synth.load_ilp(mvolps_amd.api(), *model), quirks=0, window=64, **kw)
    return r, time.perf_counter() - t0


def part_trees(out):
    from mvolps_amd import synth

    for name, model, limit in (("config-5", config5(), 0), ("512x1024 cap 0.4 U 3", synth.dense_ilp(*WIDE), 20000)):
        tree(model, pump=30, max_nodes=1)  # warm-up
        for rep in range(2):
            for pump, alpha in ((0, 0.0), (30, 0.0), (30, 0.9)):
                r, el = tree(model, heur=2, pump=pump, pump_alpha=alpha, max_nodes=limit)
                emit(dict({"part": "trees", "instance": name, "heur": 2, "pump": pump, "pump_alpha": alpha, "window": 64, "max_nodes": limit,
                           "rep": rep, "rc": r["rc"], "seconds": el}, **{k: r[k] for k in KEYS}), out)


def lockstep(gpu, root, nodes, out, label, iters=30):
    """The driver's rounds (bnb.cpp, class Pump) with a clock around each call; plain pumps (alpha 0)."""
    from mvolps_amd import bnb
    from mvolps_amd.capi import OPT

    jobs = [dict(cur=P.copy(), hist=[], k=0, end=None) for P in nodes]
    t_step = t_apply = t_solve = 0.0
    rounds = lps = 0
    while True:
        live = [jb for jb in jobs if jb["end"] is None]
        if not live:
            break
        t0 = time.perf_counter()
        rc, info, xt, c = bnb.pump_obj_many(root, [jb["cur"] for jb in live], [jb["hist"][-1] if jb["hist"] else None for jb in live])
        t_step += time.perf_counter() - t0
        assert rc == 0
        going = []
        for t, jb in enumerate(live):
            if info[t][0] == 0:
                jb["end"] = "integral"
            elif jb["k"] == iters:
                jb["end"] = "limit"
            elif info[t][2]:
                jb["end"] = "stalled"
            elif info[t][1] > 0 and any((xt[t] == h).all() for h in jb["hist"]):
                jb["end"] = "cycle"
            else:
                jb["hist"].append(xt[t].copy())
                going.append((jb, c[t]))
        if not going:
            continue
        t0 = time.perf_counter()
        assert bnb.set_obj_many([jb["cur"] for jb, _ in going], [cc for _, cc in going]) == 0
        gpu.sync()
        t_apply += time.perf_counter() - t0
        t0 = time.perf_counter()
        arr = (C.c_void_p * len(going))(*[jb["cur"].h for jb, _ in going])
        gpu.simplex_batch(arr, len(going), None, None)
        ok = [jb["cur"].status == OPT for jb, _ in going]
        t_solve += time.perf_counter() - t0
        rounds += 1
        lps += len(going)
        for (jb, _), good in zip(going, ok):
            jb["k"] += 1
            if not good:
                jb["end"] = "failed"
    ends = {}
    for jb in jobs:
        ends[jb["end"]] = ends.get(jb["end"], 0) + 1
    emit({"part": "rounds", "instance": "512x1024 cap 0.4 U 3", "pumps": label, "rounds": rounds, "lps": lps, "ends": ends,
          "objective_step_ms_per_round": t_step / max(1, rounds) * 1e3, "objective_apply_ms_per_round": t_apply / max(1, rounds) * 1e3,
          "batched_solve_ms_per_round": t_solve / max(1, rounds) * 1e3, "total_s": t_step + t_apply + t_solve}, out)


def part_rounds(out):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    gpu = mvolps_amd.api()
    root = synth.load_ilp(gpu, *synth.dense_ilp(*WIDE))
    nodes = bnb.node_sample(root, 8)
    lockstep(gpu, root, nodes[:1], None, "warm-up")
    for rep in range(2):
        lockstep(gpu, root, nodes[:1], out, "1")
        lockstep(gpu, root, nodes, out, "8")
    # one objective on the root's tableau: the one call against n + 1 single-coefficient calls
    rc, _info, _xt, c = bnb.pump_obj_many(root, nodes[:1])
    assert rc == 0
    many, each = nodes[0].copy(), nodes[0].copy()
    gpu.sync()
    t0 = time.perf_counter()
    assert bnb.set_obj_many([many], c) == 0
    gpu.sync()
    t_many = time.perf_counter() - t0
    t0 = time.perf_counter()
    for j in range(root.n + 1):
        gpu.set_obj_coef(each.h, j, float(c[0][j]))
    gpu.sync()
    t_each = time.perf_counter() - t0
    emit({"part": "rounds", "entry": "mvx_set_obj_many", "handles": 1, "one_call_ms": t_many * 1e3, "per_coefficient_ms": t_each * 1e3,
          "same_tableau": bool((many.tableau() == each.tableau()).all())}, out)
    t0 = time.perf_counter()
    for _ in range(50):
        assert bnb.pump_obj_many(root, nodes)[0] == 0
    dev = (time.perf_counter() - t0) / 50
    t0 = time.perf_counter()
    for P in nodes:
        assert bnb.pump_obj_node(P, root)[0] == 0
    emit({"part": "rounds", "entry": "mvx_pump_obj_many", "handles": len(nodes), "device_call_ms": dev * 1e3,
          "host_twin_ms": (time.perf_counter() - t0) * 1e3, "note": "the twin reads the root's rows anew on every call"}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["rounds", "trees"], required=True)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"rounds": part_rounds, "trees": part_trees}[a.part](a.out)


if __name__ == "__main__":
    main()
