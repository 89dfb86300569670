"""Measurements behind DESIGN.md "Sifting (sift)" (mvx_pool_price, mvx_pool_append, mvx_sift; k_poolprice, k_poolsel_*, k_poolgather).

  --part cpu      no device: the loop emulated with the CPU oracle's COLD solves of each round's working set and the host twins
                  of the pricing pass, on three wide dense_lp instances, for K in {m/4, m/2, m, 2m}: rounds, summed pivots and the
                  final width.  The defaults of mvx_init_sift_parm were chosen from these lines (profiles/sift_cpu.jsonl).
  --part price    mvx_pool_price on solved dense_lp roots against pools of m x N in {512 x 65536, 1024 x 131072, 4096 x 262144},
                  K = m: host clocks around the call (it ends in a synchronise), one warm-up, medians of 7; N m 8 bytes over the
                  time; the same call with K = 0, whose difference is the selection's share.
  --part loop     mvx_sift from a working set of m columns against a direct mvx_simplex on the full-width handle, at
                  512 x 65536 and 1024 x 131072: seconds, pivots, rounds, final width, both objectives.
  --part trace    reads the kernel statistics a separate `rocprofv3 --kernel-trace --stats` run of --part price left in --csv and
                  records the sifting kernels' times.
One JSON object per line on stdout (and appended to --out when given)."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CPU_SIZES = ((32, 2048), (64, 4096), (128, 8192))
PRICE_SIZES = ((512, 65536), (1024, 131072), (4096, 262144))
LOOP_SIZES = ((512, 65536), (1024, 131072))
REPS = 7


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def sizes_of(text, default):
    return tuple(tuple(int(v) for v in s.split("x")) for s in text.split(",")) if text else default


def part_cpu(out, sizes):
    import numpy as np
    from mvolps_amd import bnb, capi, synth
    from oracle import oracle

    orc = oracle.api()
    for m, N in sizes:
        A, b, c = synth.dense_lp(m, m + N, 12345)
        F = orc.create()
        F.load_dense(A, b, c)
        t0 = time.perf_counter()
        assert F.simplex() == 0 and F.status == capi.OPT
        emit({"part": "cpu", "m": m, "N": N, "call": "direct", "pivots": F.it_cnt, "n": m + N, "obj": F.obj, "s": time.perf_counter() - t0}, out)
        for K in (m // 4, m // 2, m, 2 * m):
            inside = list(range(m))
            rounds = pivots = 0
            t0 = time.perf_counter()
            while True:
                rounds += 1
                P = orc.create()
                P.load_dense(A[:, inside], b, c[inside])
                assert P.simplex() == 0 and P.status == capi.OPT
                pivots += P.it_cnt
                T = P.tableau()
                _, nb, _ = P.basis()
                y = np.zeros(m + 1)
                for q in range(1, P.n + 1):
                    if nb[q] <= m:
                        y[nb[q]] = T[0, q]
                skip = np.zeros(N + 1, dtype=np.uint8)
                skip[[j - m + 1 for j in inside if j >= m]] = 1
                rc, dj, att = bnb.pool_price_values(A[:, m:].T, c[m:], [capi.LO] * N, y, capi.MAX, 1e-9)
                rc2, pick = bnb.pool_select(dj, att, K, skip)
                assert rc == 0 and rc2 == 0
                if len(pick) == 0:
                    break
                inside += [m + int(j) - 1 for j in pick]
            assert abs(P.obj - F.obj) <= 1e-9 * abs(F.obj)
            emit({"part": "cpu", "m": m, "N": N, "call": "sift, cold solves", "K": K, "rounds": rounds, "pivots": pivots, "n_final": len(inside),
                  "obj": P.obj, "s": time.perf_counter() - t0}, out)


def pool_and_root(gpu, m, N, seed=12345):
    """A solved dense_lp root over the first m columns and the pool of the N others."""
    import numpy as np
    import mvolps_amd
    from mvolps_amd import capi, synth

    A, b, c = synth.dense_lp(m, m + N, seed)
    P = gpu.create()
    P.load_dense(np.ascontiguousarray(A[:, :m]), b, c[:m])
    assert P.simplex() == 0 and P.status == capi.OPT
    S = mvolps_amd.create_pool(m)
    step = max(1, (1 << 27) // (m + 1))  # the bound arrays of a call stay small
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        assert S.add_cols(A[:, m + lo:m + hi].T, c[m + lo:m + hi], [capi.LO] * (hi - lo), np.zeros(hi - lo), np.zeros(hi - lo)) == 0
    return P, S, A, b, c


def part_price(out, sizes):
    import mvolps_amd

    gpu = mvolps_amd.api()
    for m, N in sizes:
        P, S, A, b, c = pool_and_root(gpu, m, N)
        del A
        med = {}
        for K in (m, 0):
            ts = []
            for rep in range(REPS + 1):
                gpu.sync()
                t0 = time.perf_counter()
                rc, _, pick = P.pool_price(S, K, want_dj=False)  # ends in the entry's own synchronise
                ts.append(time.perf_counter() - t0)
                assert rc == 0
            med[K] = statistics.median(ts[1:])
            emit({"part": "price", "call": "mvx_pool_price", "m": m, "N": N, "K": K, "picks": len(pick), "reps": REPS, "ms": med[K] * 1e3,
                  "first_ms": ts[0] * 1e3, "bytes": N * m * 8, "TBps": N * m * 8 / med[K] / 1e12}, out)
        emit({"part": "price", "call": "selection share", "m": m, "N": N, "K": m, "ms": (med[m] - med[0]) * 1e3,
              "share": (med[m] - med[0]) / med[m]}, out)


def part_loop(out, sizes):
    import numpy as np
    import mvolps_amd
    from mvolps_amd import capi

    gpu = mvolps_amd.api()
    for m, N in sizes:
        P, S, A, b, c = pool_and_root(gpu, m, N)
        gpu.sync()
        t0 = time.perf_counter()
        rc, where, info = P.sift(S)
        gpu.sync()
        ts = time.perf_counter() - t0
        emit({"part": "loop", "call": "mvx_sift", "m": m, "N": N, "rc": rc, "end": info.end, "s": ts, "pivots": info.pivots, "rounds": info.rounds,
              "appended": info.appended, "n_final": info.n_final, "obj": P.obj}, out)
        z = P.obj
        del P, S
        F = gpu.create()
        F.load_dense(A, b, c)
        gpu.sync()
        t0 = time.perf_counter()
        assert F.simplex() == 0 and F.status == capi.OPT
        gpu.sync()
        td = time.perf_counter() - t0
        emit({"part": "loop", "call": "mvx_simplex, all columns", "m": m, "N": N, "s": td, "pivots": F.it_cnt, "n": F.n, "obj": F.obj,
              "sift_over_direct": ts / td, "same_objective_1e-9": bool(abs(z - F.obj) <= 1e-9 * abs(F.obj))}, out)


def part_trace(out, path):
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if "k_pool" in name or "k_addcols" in name:
                emit({"part": "trace", "kernel": name.split("(")[0], "calls": int(row["Calls"]), "total_us": float(row["TotalDurationNs"]) / 1e3,
                      "avg_us": float(row["AverageNs"]) / 1e3}, out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["cpu", "price", "loop", "trace"], required=True)
    ap.add_argument("--sizes", default="", help="e.g. 512x65536,1024x131072")
    ap.add_argument("--csv", default="", help="--part trace: rocprofv3's kernel_stats.csv")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.part == "cpu":
        part_cpu(a.out, sizes_of(a.sizes, CPU_SIZES))
    elif a.part == "price":
        part_price(a.out, sizes_of(a.sizes, PRICE_SIZES))
    elif a.part == "loop":
        part_loop(a.out, sizes_of(a.sizes, LOOP_SIZES))
    else:
        part_trace(a.out, a.csv)
