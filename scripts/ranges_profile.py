"""Measurements behind DESIGN.md "Sensitivity ranges (ranges)".

For each shape m x n (default 512x1024, 1024x2048, 4096x8192) a dense_lp root is solved on the engine; then, after one warm-up
call each, the median of 7 calls of
  mvx_ranges      the three kernels and the copy back of both tables (the call ends in a stream synchronise), and
  mvx_bnb_ranges  the host twin through the engine's own table on the same handle (one tableau export, then host loops),
both by a host clock around the call.  The device call is also set against one read of the tableau ((m + 1) ld doubles): the
rate that read would have had if the call were nothing else, and its share of the bulk pass's measured stream rate (DESIGN.md
section 6: 6.6 TB/s at 4096x8192).  The results are compared bit for bit before anything is timed.  Run it under
`rocprofv3 --kernel-trace --stats` (with --reps 3) for the three kernels' own times.
One JSON object per line on stdout (and appended to --out when given)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BULK_STREAM_BYTES_PER_S = 6.6e12  # DESIGN.md section 6, bulk launch with one pivot at 4096x8192


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def median_ms(fn, reps):
    fn()  # warm-up: buffers, code objects
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x1024,1024x2048,4096x8192")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--no-twin", action="store_true", help="time the device call only (profiler runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np

    import mvolps_amd
    from mvolps_amd import bnb, capi, synth

    mvolps_amd.require_device()
    gpu = mvolps_amd.api()
    for shape in a.shapes.split(","):
        m, n = (int(t) for t in shape.split("x"))
        P = gpu.create()
        P.load_dense(*synth.dense_lp(m, n, a.seed))
        t0 = time.perf_counter()
        P.simplex()
        solve_s = time.perf_counter() - t0
        assert P.status == capi.OPT, P.status
        rc, val, var = bnb.ranges(P)
        assert rc == 0
        rec = {"shape": shape, "pivots": P.it_cnt, "solve_s": solve_s, "chunk": bnb.ranges_chunk(), "reps": a.reps}
        if not a.no_twin:
            trc, tval, tvar = bnb.ranges(P, table=None)
            assert trc == 0
            rec["same_bits"] = bool(np.array_equal(val.view(np.int64), tval.view(np.int64)) and np.array_equal(var, tvar))
            assert rec["same_bits"]
        dev = median_ms(lambda: bnb.ranges(P), a.reps)
        ld = gpu.get_tableau_ld(P.h)
        read_bytes = (m + 1) * ld * 8
        rec.update({"device_call_ms": dev[0], "device_call_ms_min": dev[1], "device_call_ms_max": dev[2], "tableau_read_bytes": read_bytes,
                    "read_rate_TBps_of_call": read_bytes / (dev[0] * 1e-3) / 1e12,
                    "share_of_bulk_stream": read_bytes / (dev[0] * 1e-3) / BULK_STREAM_BYTES_PER_S})
        if not a.no_twin:
            twin = median_ms(lambda: bnb.ranges(P, table=None), a.reps)
            rec.update({"host_twin_ms": twin[0], "host_twin_ms_min": twin[1], "host_twin_ms_max": twin[2], "twin_over_device": twin[0] / dev[0]})
        emit(rec, a.out)


if __name__ == "__main__":
    main()
