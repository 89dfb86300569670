"""Measurements behind DESIGN.md "Column deletion (del_cols)" (mvx_del_cols, k_delcols).

  --part call     one call on solved dense_lp roots of 512x1023, 1024x2047 and 4096x8191 (one column short of the sizes of the
                  append's measurements: a stride of 32 then has room for 31 deletions in place): mvx_del_cols of the last 1, 8
                  and 31 non-basic structural positions and of 8 scattered ones in place, of the last 32 and of 32 scattered
                  ones with a relayout (32 deletions always change the row stride), each on a fresh clone.  Host clocks around
                  calls that end in a synchronise, one warm-up first, medians of 7.  Beside each: the entries that move, the
                  bytes the pass must move (read and written), the resulting TB/s of the whole call, and the same call on a
                  clone without a tableau (the host's model edit alone, which rewrites every row of the row-major model).
  --part cycle    column generation from the same roots with 256 further columns of the same generator outside: rounds of
                  pricing everything outside, appending the 32 most attractive, solving warm, until nothing prices out -- once
                  with every non-basic structural column deleted after each solve (they go back outside and are priced again),
                  once with the columns left in.  Pivots and seconds of the re-solves, the pricing, the appends and the purges.
One JSON object per line on stdout (and appended to --out when given)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((512, 1023), (1024, 2047), (4096, 8191))
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


def structural_positions(P):
    _, nb, _ = P.basis()
    return [q for q in range(1, P.n + 1) if nb[q] > P.m]


def part_call(out, sizes):
    import mvolps_amd

    gpu = mvolps_amd.api()
    for m, n in sizes:
        P, A, b, c = solved_root(gpu, m, n)
        U = gpu.create()  # the same model without a tableau
        U.load_dense(A, b, c)
        _, nb, _ = P.basis()
        s = structural_positions(P)
        ld = P.api.get_tableau_ld(P.h)
        m_cap = m + 64
        step = len(s) // 32
        cases = [("last", 1, s[-1:]), ("last", 8, s[-8:]), ("last", 31, s[-31:]), ("scattered", 8, s[:: len(s) // 8][:8]), ("last", 32, s[-32:]),
                 ("scattered", 32, s[::step][:32])]
        for where, k, positions in cases:
            cols = [int(nb[q]) - m for q in positions]
            first, n_new = positions[0], n - k
            nmove = n_new - first + 1
            relayout = ld_of(n_new) != ld
            if relayout:  # the kept entries of rows 0..m are read, every row of the new slab is written over its stride
                must_r, must_w = (m + 1) * (n_new + 1) * 8, (m_cap + 1) * ld_of(n_new) * 8
            else:  # the moved entries of every row are read and written, the vacated ones zeroed
                must_r, must_w = (m_cap + 1) * nmove * 8, (m_cap + 1) * (nmove + k) * 8
            ts = []
            for rep in range(REPS + 1):
                Q = P.copy()
                gpu.sync()  # the clone has landed
                t0 = time.perf_counter()
                rc = Q.del_cols(cols)  # ends in a synchronise
                t1 = time.perf_counter()
                assert rc == 0 and Q.n == n_new and Q.api.get_tableau_ld(Q.h) == ld_of(n_new)
                if rep:
                    ts.append(t1 - t0)
                del Q
            sec = statistics.median(ts)
            hs = []
            for rep in range(REPS + 1):  # the same call on a clone without a tableau: the host's model edit alone
                Q = U.copy()
                t0 = time.perf_counter()
                rc = Q.del_cols(cols)
                t1 = time.perf_counter()
                assert rc == 0
                if rep:
                    hs.append(t1 - t0)
                del Q
            host = statistics.median(hs)
            emit({"part": "call", "call": "mvx_del_cols", "layout": "relayout" if relayout else "in place", "where": where, "m": m, "n": n,
                  "ld": ld, "ld_new": ld_of(n_new), "k": k, "first": first, "moved_per_row": nmove, "reps": REPS, "ms": sec * 1e3,
                  "model_edit_ms": host * 1e3, "bytes_read": must_r, "bytes_written": must_w, "call_TBps": (must_r + must_w) / sec / 1e12}, out)
        del P


def part_cycle(out, sizes, max_rounds):
    import mvolps_amd
    import numpy as np
    from mvolps_amd import capi

    gpu = mvolps_amd.api()
    for m, n in sizes:
        for purge in (True, False):
            P, A, b, c = solved_root(gpu, m, n, extra=256)
            inside = list(range(n))  # generator column of model column j + 1
            outside = list(range(n, n + 256))
            first = P.it_cnt
            tot = {"price_s": 0.0, "append_s": 0.0, "solve_s": 0.0, "purge_s": 0.0, "pivots": 0, "purged": 0, "appended": 0}
            rounds, done = 0, False
            widths = []
            while rounds < max_rounds:
                if purge:
                    _, nb, _ = P.basis()
                    gone = [int(nb[q]) - m for q in range(1, P.n + 1) if nb[q] > m]
                    if gone and len(gone) < P.n:
                        gpu.sync()
                        t0 = time.perf_counter()
                        assert P.del_cols(gone) == 0
                        tot["purge_s"] += time.perf_counter() - t0
                        tot["purged"] += len(gone)
                        dead = set(gone)
                        outside += [inside[j - 1] for j in gone]
                        inside = [g for j, g in enumerate(inside, start=1) if j not in dead]
                cand = np.ascontiguousarray(A[:, outside].T)
                gpu.sync()
                t0 = time.perf_counter()
                rc, dj = P.price_cols(cand, c[outside])
                tot["price_s"] += time.perf_counter() - t0
                assert rc == 0
                pick = [i for i in np.argsort(-dj, kind="stable")[:32] if dj[i] > 1e-9]
                if not pick:
                    done = True
                    break
                take = [outside[i] for i in pick]
                k = len(take)
                cols = np.ascontiguousarray(np.hstack([np.zeros((k, 1)), A[:, take].T]))
                gpu.sync()
                t0 = time.perf_counter()
                assert P.add_dense_cols(cols, c[take], [capi.LO] * k, [0.0] * k, [0.0] * k) == 0
                t1 = time.perf_counter()
                before = P.it_cnt
                assert P.simplex() == 0 and P.status == capi.OPT
                gpu.sync()
                t2 = time.perf_counter()
                tot["append_s"] += t1 - t0
                tot["solve_s"] += t2 - t1
                tot["pivots"] += P.it_cnt - before
                tot["appended"] += k
                widths.append(P.n)
                inside += take
                took = set(take)
                outside = [g for g in outside if g not in took]
                rounds += 1
            rec = {"part": "cycle", "m": m, "n": n, "outside_at_start": 256, "purge": purge, "rounds": rounds, "ended": done,
                   "first_solve_pivots": first, "columns_at_end": P.n, "widest": max(widths) if widths else P.n, "obj": P.obj}
            rec.update(tot)
            rec["ms_per_pivot"] = 1e3 * tot["solve_s"] / max(1, tot["pivots"])
            emit(rec, out)
            del P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["call", "cycle"], required=True)
    ap.add_argument("--sizes", default=None, help="comma-separated m x n, e.g. 512x1023,1024x2047 (default: all three)")
    ap.add_argument("--max-rounds", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = SIZES if not a.sizes else tuple(tuple(int(v) for v in s.split("x")) for s in a.sizes.split(","))
    if a.part == "call":
        part_call(a.out, sizes)
    else:
        part_cycle(a.out, sizes, a.max_rounds)


if __name__ == "__main__":
    main()
