"""Measurements behind DESIGN.md "LP diving heuristic" (mvx_bnb_params.dive).

  --part rounds   root dives of the wide instance (512x1024, cap 0.4, U = 3) written out in Python over the same entries the
                  driver uses, host clocks around the synchronising calls: per round the pick call (mvx_dive_pick_many), the
                  clones plus the bound apply (mvx_set_col_bnds_many) and the batched solve (mvx_simplex_batch), for the 3
                  lockstep dives of the root and for 3 x 8 (the root and seven nodes below it); then the twin's time for the
                  same picks (mvx_bnb_dive_pick through the engine's table).
  --part trees    config 5 to the end at window 64, repaired: plain, dive 7 at the root, the same plus heur 2 + rc_fix, and
                  plus prop 8, each against its own dive = 0 base from the same run, alternating: nodes, pivots, seconds, the
                  oid of the final incumbent, the dives' counters.
  --part wide     the wide instance, 20 000 nodes at window 64: heur 2 alone and with dive 7: the incumbent and its gap to
                  the root bound.
  --part trace    24 picks on the wide instance's nodes, 200 times, and nothing else: run under `rocprofv3 --kernel-trace
                  --stats` for k_divepick's time.
One JSON object per line on stdout (and appended to --out when given)."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("count", "hit_limit", "has_incumbent", "best_lower", "total_pivots", "incumbent_oid", "incumbent_heur", "heur_calls", "heur_improved",
        "rc_calls", "rc_fixed", "prop_calls", "prop_fixed", "dive_calls", "dive_found", "dive_improved", "dive_lps", "dive_pivots")
WIDE = (512, 1024, 12345, 3, 0.4)
WIDE_ROOT_BOUND = 7384.26


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
    tree(model, dive=7, max_nodes=200)  # warm-up
    for base in (dict(), dict(heur=2, rc_fix=1), dict(heur=2, rc_fix=1, prop=8)):
        for rep in range(2):
            for dive in (0, 7):
                r, el = tree(model, dive=dive, **base)
                emit(dict({"part": "trees", "instance": "config-5", "options": base, "dive": dive, "window": 64, "rep": rep, "rc": r["rc"],
                           "seconds": el}, **{k: r[k] for k in KEYS}), out)


def part_wide(out):
    from mvolps_amd import synth

    model = synth.dense_ilp(*WIDE)
    tree(model, dive=7, max_nodes=1)  # warm-up
    for rep in range(2):
        for dive in (0, 7):
            r, el = tree(model, heur=2, dive=dive, max_nodes=20000)
            emit(dict({"part": "wide", "instance": "512x1024 cap 0.4 U 3", "heur": 2, "dive": dive, "window": 64, "max_nodes": 20000, "rep": rep,
                       "rc": r["rc"], "seconds": el, "gap_to_root_bound": WIDE_ROOT_BOUND - r["best_lower"]}, **{k: r[k] for k in KEYS}), out)


def lockstep(gpu, root, nodes, out, label):
    """The driver's rounds (bnb.cpp, class Dive) with a clock around each call."""
    from mvolps_amd import bnb
    from mvolps_amd.capi import DB, FX, LO, OPT, UP

    def col_range(P, j):
        t = gpu.get_col_type(P.h, j)
        l = gpu.get_col_lb(P.h, j) if t in (LO, DB, FX) else -math.inf
        u = l if t == FX else gpu.get_col_ub(P.h, j) if t in (UP, DB) else math.inf
        return l, u

    jobs = [dict(cur=P, rule=r, state="pick") for P in nodes for r in (1, 2, 4)]
    t_pick = t_clone = t_solve = 0.0
    rounds = lps = 0
    while True:
        picking = [jb for jb in jobs if jb["state"] == "pick"]
        if picking:
            t0 = time.perf_counter()
            rc, got = bnb.dive_pick_many(root, [jb["cur"] for jb in picking], [jb["rule"] for jb in picking])
            t_pick += time.perf_counter() - t0
            assert rc == 0
            for jb, (nfrac, col, side, val) in zip(picking, got):
                if nfrac == 0:
                    jb["state"] = "integral"
                else:
                    jb.update(col=col, side=side, val=val)
        live = [jb for jb in jobs if jb["state"] in ("pick", "flip")]
        t0 = time.perf_counter()
        kids, lists, owners = [], [], []
        for jb in live:
            l, u = col_range(jb["cur"], jb["col"])
            l, u = (float(math.ceil(jb["val"])), u) if jb["side"] else (l, float(math.floor(jb["val"])))
            if l > u:
                jb["state"] = "ended"  # the timed instance never meets a crossing side
                continue
            kids.append(jb["cur"].copy())
            lists.append([(jb["col"], l, u)])
            owners.append(jb)
        if not kids:
            break
        assert bnb.set_col_bnds_many(kids, lists) == 0
        t_clone += time.perf_counter() - t0
        t0 = time.perf_counter()
        arr = (C.c_void_p * len(kids))(*[k.h for k in kids])
        gpu.simplex_batch(arr, len(kids), None, None)
        ok = [k.status == OPT for k in kids]
        t_solve += time.perf_counter() - t0
        rounds += 1
        lps += len(kids)
        for jb, kid, good in zip(owners, kids, ok):
            if good:
                jb.update(cur=kid, state="pick")
            elif jb["state"] == "pick":
                jb.update(state="flip", side=1 - jb["side"])
            else:
                jb["state"] = "ended"
    emit({"part": "rounds", "instance": "512x1024 cap 0.4 U 3", "dives": label, "lockstep_dives": len(jobs), "rounds": rounds, "lps": lps,
          "integral": sum(jb["state"] == "integral" for jb in jobs), "pick_call_ms_per_round": t_pick / rounds * 1e3,
          "clones_and_bounds_ms_per_round": t_clone / rounds * 1e3, "batched_solve_ms_per_round": t_solve / rounds * 1e3,
          "total_s": t_pick + t_clone + t_solve}, out)


def part_rounds(out):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    gpu = mvolps_amd.api()
    root = synth.load_ilp(gpu, *synth.dense_ilp(*WIDE))
    nodes = bnb.node_sample(root, 8)
    lockstep(gpu, root, nodes[:1], None, "warm-up")
    for rep in range(2):
        lockstep(gpu, root, nodes[:1], out, "3")
        lockstep(gpu, root, nodes, out, "3 x 8")
    hs = [P for P in nodes for _ in range(3)]
    rules = [r for _ in nodes for r in (1, 2, 4)]
    t0 = time.perf_counter()
    for _ in range(50):
        assert bnb.dive_pick_many(root, hs, rules)[0] == 0
    dev = (time.perf_counter() - t0) / 50
    t0 = time.perf_counter()
    for P, r in zip(hs, rules):
        assert bnb.dive_pick_node(P, root, r)[0] == 0
    emit({"part": "rounds", "entry": "mvx_dive_pick_many", "picks": len(hs), "device_call_ms": dev * 1e3,
          "host_twin_ms": (time.perf_counter() - t0) * 1e3, "note": "the twin reads the root's rows anew on every call"}, out)


def part_trace(out):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    gpu = mvolps_amd.api()
    root = synth.load_ilp(gpu, *synth.dense_ilp(*WIDE))
    nodes = bnb.node_sample(root, 8)
    hs = [P for P in nodes for _ in range(3)]
    rules = [r for _ in nodes for r in (1, 2, 4)]
    for _ in range(200):
        assert bnb.dive_pick_many(root, hs, rules)[0] == 0
    emit({"part": "trace", "picks_per_call": len(hs), "calls": 200}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["rounds", "trees", "wide", "trace"], required=True)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"rounds": part_rounds, "trees": part_trees, "wide": part_wide, "trace": part_trace}[a.part](a.out)


if __name__ == "__main__":
    main()
