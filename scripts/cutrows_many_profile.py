"""Measurements behind DESIGN.md "Row append across handles (add_cut_rows_many)" (mvx_add_cut_rows_many, k_cutrows_many).

The config-3 root (dense_ilp 512x1024, cap 0.4, U 3), solved.  W = 8 / 64 / 128 clones of it, each with its own repaired GMI cut
out of ONE mvx_gmi_cuts_many call over the clones (the columns go round when the root has fewer than W fractional ones); the cuts
are appended in three ways:
  (a) add_rows, set_mat_row, set_row_bnds per handle;  (b) mvx_add_cut_rows(k = 1) per handle;  (c) one mvx_add_cut_rows_many.
Fresh clones per repetition.  Series "launched": the clones are made and launched before the clock starts.  Series "recorded":
the clones are only recorded when the clock starts, so their flush is inside the leg.  Host clocks around a leg that ends in
mvx_sync; one warm-up, medians of 7.  "model_only" is leg (a) on clones of a never-solved handle of the same model: the host's
model work alone, which every leg pays per handle.

  --part legs     the table (--out appends the JSON lines)
  --part trace    W = 64, legs (b) and (c) twice each and nothing else: run it under `rocprofv3 --kernel-trace` (nothing else
                  traced) and read the kernels' own times with scripts/kstats.py <dir> k_cutrows k_copy_many
One JSON object per line on stdout."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDE = (512, 1024, 12345, 3, 0.4)
REPS = 7


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def setup():
    import mvolps_amd
    import numpy as np
    from mvolps_amd import bnb, synth
    from mvolps_amd.capi import OPT

    gpu = mvolps_amd.api()
    model = synth.dense_ilp(*WIDE)
    root = synth.load_ilp(gpu, *model)
    root.simplex()
    assert root.status == OPT
    cold = synth.load_ilp(gpu, *model)  # never solved: no tableau
    cols = [j for j in range(1, root.n + 1) if bnb.generate_cut_gmi(root, j) is not None]
    assert cols
    return gpu, np, bnb, root, cold, cols


def own_cuts(gpu, np, clones, cols):
    """One mvx_gmi_cuts_many call: cut t from clone t, column cols[t mod len]."""
    W, n = len(clones), clones[0].n
    vals, rhs, ok = np.zeros((W, n + 1)), np.zeros(W), np.zeros(W, dtype=np.int32)
    arr = np.asarray([cols[t % len(cols)] for t in range(W)], dtype=np.int32)
    hs = (C.c_void_p * W)(*[p.h for p in clones])
    lib = gpu.lib
    lib.mvx_gmi_cuts_many.restype = C.c_int
    lib.mvx_gmi_cuts_many.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.mvx_gmi_cuts_many(hs, 1, arr.ctypes.data, W, vals.ctypes.data, rhs.ctypes.data, ok.ctypes.data) == 0
    assert ok.all()
    return vals, rhs


def leg_a(gpu, np, hs, vals, rhs):
    from mvolps_amd.capi import LO

    ind = np.arange(hs[0].n + 1, dtype=np.int32)
    for t, P in enumerate(hs):
        i = gpu.add_rows(P.h, 1)
        P.set_mat_row(i, ind, vals[t])
        gpu.set_row_bnds(P.h, i, LO, float(rhs[t]), 0.0)


def leg_b(bnb, hs, vals, rhs):
    for t, P in enumerate(hs):
        assert bnb.add_cut_rows(P, vals[t:t + 1], rhs[t:t + 1]) == 0


def leg_c(bnb, hs, vals, rhs):
    assert bnb.add_cut_rows_many(hs, [vals[t:t + 1] for t in range(len(hs))], [rhs[t:t + 1] for t in range(len(hs))]) == 0


def part_legs(out):
    gpu, np, bnb, root, cold, cols = setup()
    for W in (8, 64, 128):
        vals, rhs = own_cuts(gpu, np, [root.copy() for _ in range(W)], cols)
        legs = (("a_three_calls", lambda hs: leg_a(gpu, np, hs, vals, rhs)), ("b_add_cut_rows", lambda hs: leg_b(bnb, hs, vals, rhs)),
                ("c_add_cut_rows_many", lambda hs: leg_c(bnb, hs, vals, rhs)))
        times = {}
        last = {}
        for rep in range(REPS + 1):
            for series in ("launched", "recorded"):
                for name, leg in legs:
                    gpu.sync()
                    if series == "launched":
                        hs = [root.copy() for _ in range(W)]
                        gpu.sync()
                        t0 = time.perf_counter()
                    else:
                        t0 = time.perf_counter()
                        hs = [root.copy() for _ in range(W)]
                    leg(hs)
                    gpu.sync()
                    t1 = time.perf_counter()
                    if rep:  # the first repetition warms every path up
                        times.setdefault((series, name), []).append(t1 - t0)
                    last[name] = hs
            hs = [cold.copy() for _ in range(W)]
            t0 = time.perf_counter()
            leg_a(gpu, np, hs, vals, rhs)
            t1 = time.perf_counter()
            if rep:
                times.setdefault(("host", "model_only"), []).append(t1 - t0)
        same = all(np.array_equal(x.tableau().view(np.uint64), y.tableau().view(np.uint64)) and np.array_equal(x.tableau().view(np.uint64), z.tableau().view(np.uint64))
                   for x, y, z in zip(last["a_three_calls"][::17], last["b_add_cut_rows"][::17], last["c_add_cut_rows_many"][::17]))
        rec = {"part": "legs", "instance": "512x1024 cap 0.4 U 3 root", "W": W, "distinct_cut_columns": min(W, len(cols)), "reps": REPS, "same_bits": bool(same)}
        for (series, name), ts in times.items():
            rec["%s_%s_ms" % (series, name)] = round(statistics.median(ts) * 1e3, 4)
        emit(rec, out)


def part_trace():
    gpu, np, bnb, root, _cold, cols = setup()
    W = 64
    vals, rhs = own_cuts(gpu, np, [root.copy() for _ in range(W)], cols)
    for _ in range(2):
        for leg in (leg_b, leg_c):
            hs = [root.copy() for _ in range(W)]
            gpu.sync()
            leg(bnb, hs, vals, rhs)
            gpu.sync()
    print(json.dumps({"part": "trace", "W": W, "legs": "b, c, b, c"}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["legs", "trace"], default="legs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.part == "legs":
        part_legs(a.out)
    else:
        part_trace()
