"""Measurements behind DESIGN.md "Column append (add_cols)" (mvx_add_dense_cols, mvx_price_cols, k_addcols).

  --part call     one call on solved dense_lp roots of 512x1024, 1024x2048 and 4096x8192: mvx_price_cols for 32 candidates with and
                  without images, mvx_add_dense_cols for k = 1, 8 in place and k = 1, 8, 32 with a relayout (a row stride has
                  room for at most 31 more columns, so 32 always move the handle; the relayout handles have one column less, which
                  fills their stride), each on a fresh clone.  Host clocks around calls that end in a synchronise, one warm-up
                  first, medians of 7.  Beside each: the bytes the pass must move ((m+1) x ld x 8 read, the same again written on a
                  relayout), the resulting TB/s, the same call on a clone without a tableau (the host's model edit alone, which
                  rewrites every row of the row-major model) and the host twin mvx_bnb_price_cols on the same handle (one run).
  --part cycle    at the same sizes: the 32 most attractive of 256 further columns of the same generator appended and the LP solved
                  again warm, against the only route without the live append: mvx_add_cols, mvx_set_mat_row on every row, a cold
                  solve.  Seconds and pivots of both.
One JSON object per line on stdout (and appended to --out when given)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((512, 1024), (1024, 2048), (4096, 8192))
REPS = 7


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def ld_of(n):
    return (n + 1 + 31) // 32 * 32


def solved_root(gpu, m, n, seed=12345, extra=0):
    from mvolps_amd import capi, synth

    A, b, c = synth.dense_lp(m, n + extra, seed)
    P = gpu.create()
    P.load_dense(A[:, :n], b, c[:n])
    assert P.simplex() == 0 and P.status == capi.OPT
    return P, A, b, c


def part_call(out, sizes):
    import mvolps_amd
    import numpy as np
    from mvolps_amd import bnb, capi

    gpu = mvolps_amd.api()
    rng = np.random.default_rng(1)
    for m, n in sizes:
        for layout, n0, ks in (("in place", n, (1, 8)), ("relayout", n - 1, (1, 8, 32))):
            P, A, b, c = solved_root(gpu, m, n0)
            U = gpu.create()  # the same model without a tableau
            U.load_dense(A, b, c)
            ld = P.api.get_tableau_ld(P.h)
            read = (m + 1) * ld * 8
            if layout == "in place":  # pricing is measured once per size
                for kp, images in ((32, False), (1, True), (8, True), (32, True)):
                    cols = np.hstack([np.zeros((kp, 1)), rng.random((kp, m))])
                    obj = rng.random(kp)
                    ts = []
                    for rep in range(REPS + 1):
                        gpu.sync()
                        t0 = time.perf_counter()
                        res = P.price_cols(cols, obj, images=images)  # ends in the entry's own synchronise
                        t1 = time.perf_counter()
                        assert res[0] == 0
                        if rep:
                            ts.append(t1 - t0)
                    sec = statistics.median(ts)
                    must = read if images else ld * 8
                    emit({"part": "call", "call": "mvx_price_cols", "m": m, "n": n0, "ld": ld, "k": kp, "images": images, "reps": REPS,
                          "ms": sec * 1e3, "bytes": must, "TBps": must / sec / 1e12}, out)
                t0 = time.perf_counter()
                trc, tdj, timg = bnb.price_cols(P, cols, obj, table=None)
                twin = time.perf_counter() - t0
                rc, dj, img = P.price_cols(cols, obj, images=True)
                emit({"part": "call", "call": "mvx_bnb_price_cols", "m": m, "n": n0, "k": 32, "images": True, "reps": 1, "ms": twin * 1e3,
                      "same_bits": bool(trc == 0 and rc == 0 and np.array_equal(img.view(np.int64), timg.view(np.int64)))}, out)
            for k in ks:
                cols = np.hstack([np.zeros((k, 1)), rng.random((k, m))])
                obj = rng.random(k)
                ty, lb, ub = [capi.LO] * k, [0.0] * k, [0.0] * k
                ts = []
                for rep in range(REPS + 1):
                    Q = P.copy()
                    gpu.sync()  # the clone has landed
                    t0 = time.perf_counter()
                    rc = Q.add_dense_cols(cols, obj, ty, lb, ub)  # ends in a synchronise
                    t1 = time.perf_counter()
                    assert rc == 0 and (Q.api.get_tableau_ld(Q.h) != ld) == (layout == "relayout")
                    if rep:
                        ts.append(t1 - t0)
                    del Q
                sec = statistics.median(ts)
                hs = []
                for rep in range(REPS + 1):  # the same call on a clone without a tableau: the host's model edit alone
                    Q = U.copy()
                    t0 = time.perf_counter()
                    rc = Q.add_dense_cols(cols, obj, ty, lb, ub)
                    t1 = time.perf_counter()
                    assert rc == 0
                    if rep:
                        hs.append(t1 - t0)
                    del Q
                host = statistics.median(hs)
                must = read * (2 if layout == "relayout" else 1)
                emit({"part": "call", "call": "mvx_add_dense_cols", "layout": layout, "m": m, "n": n0, "ld": ld, "ld_new": ld_of(n0 + k), "k": k,
                      "reps": REPS, "ms": sec * 1e3, "model_edit_ms": host * 1e3, "bytes": must, "TBps": must / sec / 1e12}, out)
            del P


def part_cycle(out, sizes):
    import mvolps_amd
    import numpy as np
    from mvolps_amd import capi

    gpu = mvolps_amd.api()
    for m, n in sizes:
        P, A, b, c = solved_root(gpu, m, n, extra=256)
        rc, dj = P.price_cols(A[:, n:].T, c[n:])
        assert rc == 0
        take = n + np.argsort(-dj, kind="stable")[:32]
        attractive = int((dj[take - n] > 1e-9).sum())
        cols = np.ascontiguousarray(np.hstack([np.zeros((32, 1)), A[:, take].T]))
        obj = np.ascontiguousarray(c[take])
        first = P.it_cnt
        # the live route
        gpu.sync()
        t0 = time.perf_counter()
        assert P.add_dense_cols(cols, obj, [capi.LO] * 32, [0.0] * 32, [0.0] * 32) == 0
        t1 = time.perf_counter()
        assert P.simplex() == 0 and P.status == capi.OPT
        gpu.sync()
        t2 = time.perf_counter()
        warm = {"append_s": t1 - t0, "solve_s": t2 - t1, "pivots": P.it_cnt - first, "obj": P.obj}
        # the route without it: add_cols, every row rewritten, a cold solve
        Q, _A, _b, _c = solved_root(gpu, m, n, extra=256)
        assert Q.it_cnt == first
        B = np.hstack([A[:, :n], A[:, take]])
        ind = np.arange(n + 33, dtype=np.int32)
        rows = [np.concatenate([[0.0], B[i]]) for i in range(m)]
        gpu.sync()
        t0 = time.perf_counter()
        Q.api.add_cols(Q.h, 32)
        for i in range(m):
            Q.set_mat_row(i + 1, ind, rows[i])
        for t in range(32):
            Q.api.set_col_bnds(Q.h, n + 1 + t, capi.LO, 0.0, 0.0)
            Q.api.set_obj_coef(Q.h, n + 1 + t, float(obj[t]))
        t1 = time.perf_counter()
        assert Q.simplex() == 0 and Q.status == capi.OPT
        gpu.sync()
        t2 = time.perf_counter()
        cold = {"edit_s": t1 - t0, "solve_s": t2 - t1, "pivots": Q.it_cnt - first, "obj": Q.obj}
        emit({"part": "cycle", "m": m, "n": n, "k": 32, "attractive": attractive, "first_solve_pivots": first, "live": warm, "cold": cold,
              "obj_rel_diff": abs(warm["obj"] - cold["obj"]) / abs(cold["obj"])}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["call", "cycle"], required=True)
    ap.add_argument("--sizes", default=None, help="comma-separated m x n, e.g. 512x1024,1024x2048 (default: all three)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = SIZES if not a.sizes else tuple(tuple(int(v) for v in s.split("x")) for s in a.sizes.split(","))
    {"call": part_call, "cycle": part_cycle}[a.part](a.out, sizes)


if __name__ == "__main__":
    main()
