"""Measurements behind DESIGN.md "Infeasibility and unboundedness proofs (farkas)" (mvx_farkas, mvx_farkas_many, k_farkas_*,
mvx_bnb_params.farkas).

  --part single   for each shape m x n (default 512x1024, 1024x2048, 4096x8192) a dense_lp root is solved on the engine and a clone
                  of it is made infeasible (its first column pushed past the first row's capacity; the dual simplex ends
                  MVX_NOFEAS); then the median of 7 calls of mvx_farkas (five kernels and the copy back; the call ends in a stream
                  synchronise), of the host twin mvx_bnb_farkas through the engine's own table, and of mvx_kkt on the same handle.
                  The device call is set against (m + 1) ld 8 bytes of tableau plus 2 m n 8 bytes of model -- one tableau pass
                  and two model passes; the column pass alone reads m n 8 -- and the bulk pass's measured stream rate.
  --part window   the children of 64 solved nodes (bnb.node_sample) of config 5 (512x1024), their most fractional column rounded
                  up, solved in one batch; one mvx_farkas_many call over the MVX_NOFEAS ones against one mvx_farkas call each and
                  against the twin on the same handles.
  --part trees    config 5 to the end at window 64, repaired, farkas = 0 and farkas = 1, two alternating runs.  With
                  --flag-off-only the farkas argument is never passed, so that --tree can name a checkout from before the flag:
                  the parent commit's farkas = 0 run.
Host clocks around calls that end in a synchronise, one warm-up first, medians of 7; results are compared bit for bit before
anything is timed.  One JSON object per line on stdout (and appended to --out when given); --label WORD goes into every record."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BULK_STREAM_BYTES_PER_S = 6.6e12  # DESIGN.md section 6, bulk launch with one pivot at 4096x8192

LABEL = None  # --label: written into every record, to tell the runs of one file apart


def emit(rec, out):
    if LABEL is not None:
        rec = dict(rec, label=LABEL)
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def median_ms(fn, reps):
    fn()  # warm-up: buffers, code objects, the device copies of the model
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def config5(tree):
    from mvolps_amd import synth

    fx = json.load(open(os.path.join(tree, "tests", "golden", "config5.json")))
    return synth.dense_ilp(fx["m"], fx["n"], fx["seed"], fx["U"], fx["cap"])


def bits(a):
    import numpy as np

    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def part_single(a):
    import numpy as np

    import mvolps_amd
    from mvolps_amd import bnb, capi, synth

    gpu = mvolps_amd.api()
    for shape in a.shapes.split(","):
        m, n = (int(t) for t in shape.split("x"))
        A, b, c = synth.dense_lp(m, n, a.seed)
        R = gpu.create()
        R.load_dense(A, b, c)
        R.simplex()
        assert R.status == capi.OPT, R.status
        P = R.copy()
        gpu.set_col_bnds(P.h, 1, capi.LO, (float(b[0]) + 1.0) / float(A[0, 0]), 0.0)
        t0 = time.perf_counter()
        P.simplex()
        solve_s = time.perf_counter() - t0
        assert P.status == capi.NOFEAS, P.status
        d = bnb.farkas(P)
        h = bnb.farkas(P, table=None)
        assert d[0] == h[0] == 0
        same = bool(np.array_equal(bits(d[1]), bits(h[1])) and np.array_equal(d[2], h[2]) and np.array_equal(bits(d[3]), bits(h[3])))
        assert same
        dev = median_ms(lambda: bnb.farkas(P, weights=False), a.reps)
        twin = median_ms(lambda: bnb.farkas(P, table=None, weights=False), a.reps)
        kkt = median_ms(lambda: bnb.kkt(P, residuals=False), a.reps)
        ld = gpu.get_tableau_ld(P.h) if hasattr(gpu, "get_tableau_ld") else n + 1
        nbytes = (m + 1) * ld * 8 + 2 * m * n * 8
        emit({"part": "single", "shape": shape, "pivots_to_nofeas": P.it_cnt - R.it_cnt, "solve_s": solve_s, "reps": a.reps, "same_bits": same,
              "val": [float(v) for v in d[1]], "ind": [int(v) for v in d[2]], "device_call_ms": dev[0], "device_call_ms_min": dev[1],
              "device_call_ms_max": dev[2], "ld": ld, "bytes": nbytes, "rate_TBps_of_call": nbytes / (dev[0] * 1e-3) / 1e12,
              "share_of_bulk_stream": nbytes / (dev[0] * 1e-3) / BULK_STREAM_BYTES_PER_S, "kkt_call_ms": kkt[0],
              "kkt_rate_TBps_of_call": 2 * m * n * 8 / (kkt[0] * 1e-3) / 1e12, "host_twin_ms": twin[0], "host_twin_ms_min": twin[1],
              "host_twin_ms_max": twin[2], "twin_over_device": twin[0] / dev[0]}, a.out)


def part_window(a):
    import numpy as np

    import mvolps_amd
    from mvolps_amd import bnb, capi, synth

    gpu = mvolps_amd.api()
    A, b, c, U = config5(ROOT)
    root = synth.load_ilp(gpu, A, b, c, U)
    kids = []
    for P in bnb.node_sample(root, 64, quirks=0):
        x = P.col_prim()
        j = int(np.argmax(np.abs(x - np.round(x))))
        ch = P.copy()
        gpu.set_col_bnds(ch.h, j + 1, capi.DB if np.ceil(x[j]) < U else capi.FX, float(np.ceil(x[j])), float(U))
        kids.append(ch)
    hs = (bnb.C.c_void_p * len(kids))(*[p.h for p in kids])
    gpu.simplex_batch(hs, len(kids), None, None)
    nodes = [p for p in kids if p.status == capi.NOFEAS]
    if not nodes:
        emit({"part": "window", "instance": "config-5 512x1024", "children": len(kids), "handles": 0}, a.out)
        return
    d = bnb.farkas_many(root, nodes)
    h = bnb.farkas_many(root, nodes, table=None)
    assert d[0] == h[0] == 0
    same = bool(np.array_equal(bits(d[1]), bits(h[1])) and np.array_equal(d[2], h[2]))
    assert same

    def one_by_one():
        for P in nodes:
            assert bnb.farkas(P, weights=False)[0] == 0

    many = median_ms(lambda: bnb.farkas_many(root, nodes), a.reps)
    single = median_ms(one_by_one, a.reps)
    twin = median_ms(lambda: bnb.farkas_many(root, nodes, table=None), a.reps)
    emit({"part": "window", "instance": "config-5 512x1024", "children": len(kids), "handles": len(nodes), "m": root.m, "n": root.n,
          "reps": a.reps, "same_bits": same, "found": [int(v) for v in d[2][:, 0]], "rel_min": float(d[1][:, 1].min()),
          "de_max": float(d[1][:, 3].max()), "farkas_many_ms": many[0], "farkas_many_ms_min": many[1], "farkas_many_ms_max": many[2],
          "farkas_each_ms": single[0], "farkas_each_ms_min": single[1], "farkas_each_ms_max": single[2], "twin_ms": twin[0],
          "twin_ms_min": twin[1], "twin_ms_max": twin[2], "twin_over_many": twin[0] / many[0], "each_over_many": single[0] / many[0]}, a.out)


def part_trees(a):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    model = config5(a.tree)

    def tree(**kw):
        t0 = time.perf_counter()
        r = bnb.branch_and_bound(synth.load_ilp(mvolps_amd.api(), *model), quirks=0, window=64, **kw)
        return r, time.perf_counter() - t0

    tree(max_nodes=20)  # warm-up
    for rep in range(2):
        for flag in ((None,) if a.flag_off_only else (0, 1)):
            r, el = tree(**({} if flag is None else {"farkas": flag}))
            rec = {"part": "trees", "tree": "this checkout" if os.path.abspath(a.tree) == ROOT else "--tree checkout", "instance": "config 5",
                   "farkas": flag, "rep": rep, "rc": r["rc"], "seconds": el, "nodes_per_s": r["count"] / el, "count": r["count"],
                   "total_pivots": r["total_pivots"], "best_lower": r["best_lower"]}
            rec.update({k: r.get(k) for k in getattr(bnb, "FARKAS_COUNTERS", ())})
            emit(rec, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["single", "window", "trees"], required=True)
    ap.add_argument("--shapes", default="512x1024,1024x2048,4096x8192")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is measured (--part trees --flag-off-only: the parent commit's)")
    ap.add_argument("--flag-off-only", action="store_true")
    ap.add_argument("--label", default=None, help="a word written into every record of this run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    global LABEL
    LABEL = a.label
    sys.path.insert(0, os.path.abspath(a.tree))
    import mvolps_amd

    mvolps_amd.require_device()
    {"single": part_single, "window": part_window, "trees": part_trees}[a.part](a)


if __name__ == "__main__":
    main()
