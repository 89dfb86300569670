"""Measurements behind DESIGN.md "Cut purging in the tree (node_purge)" (mvx_del_rows_many, k_delrows_many, mvx_bnb_params.node_purge).

  --part cpu      no device: whole trees over the oracle's table, whose purge is the free-row path (the same LP as a deletion), for
                  the age limit A = 0..4 at window 64: every fourth general fixture with an optimum with cut_strat = 1 (one cut per
                  node), the same with cut_select = 1, and the four binary dense_ilp models of the clique table with cut_strat = 1
                  and cut_select = 1.  Work is the driver's own count (MVX_BNB_WORK): the sum over the booked solves of pivots x
                  (live rows of the handle + 1), the entries a dense pivot touches per column; a free row does not count as live.
  --part call     one mvx_del_rows_many call over 128 clones of the solved wide 512x1024 root carrying 32 of its own GMI rows, the
                  last k = 4 / 16 / 32 slack rows leaving, beside 128 mvx_del_rows calls on twin clones, and beside the same two on
                  clones of a handle with the same model and no tableau (the host share: the model edit and the row list's head
                  copies).  Host clocks around calls that end in a synchronise, one warm-up first, medians of 7 (--out).
  --part trees    whole trees, A = 0 / 1 / 2 / 3, two alternating runs each (--out-trees): the BASELINE config-3 cut modes (512x1024,
                  600 nodes, repaired one cut per node and efficacy-selected, window 64), config 5 with cut_strat = 1, and
                  dense_ilp(128,256,7,3) in best-bound order node at a time with cut_select = 1 to 2 500 nodes.  --only N runs
                  the N-th of them alone.
One JSON object per line on stdout (and appended to --out / --out-trees when given)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("count", "n_nodes", "hit_limit", "has_incumbent", "best_lower", "total_pivots", "node_purge_calls", "node_purge_rows", "node_cut_rows_peak")
BINARY = ((24, 48, 5, 1, 0.06), (32, 64, 7, 1, 0.045), (64, 128, 7, 1, 0.025), (32, 64, 7, 1, 0.05))
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


def counted(call):
    """call() with the driver's work line (stderr, MVX_BNB_WORK) read back: (result, work)."""
    os.environ["MVX_BNB_WORK"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            r = call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["MVX_BNB_WORK"]
        tmp.seek(0)
        text = tmp.read().decode()
    work = [int(l.split(":")[1]) for l in text.splitlines() if l.startswith("bnb work:")]
    assert len(work) == 1, text
    return r, work[0]


def part_cpu(out):
    from mvolps_amd import bnb, synth
    from oracle import oracle
    from tests import lpgen
    from tests.test_bnb_general import INSTANCES, instance

    orc = oracle.api()
    tab = bnb.table_from(orc)
    assert not tab.del_rows and not tab.del_rows_many
    fixtures = [(rec, instance(rec)) for rec in INSTANCES[::4] if rec["status"] == "optimal"]

    def sweep(label, loads, **kw):
        for A in range(5):
            tot = dict(nodes=0, tree_pivots=0, purged=0, peak=0, work=0, purging_instances=0, missed=0)
            for load, opt in loads:
                r, work = counted(lambda: bnb.branch_and_bound(load(), quirks=0, table=tab, window=64, max_nodes=200000, cut_strat=1, node_purge=A, **kw))
                assert r["rc"] == 0 and not r["hit_limit"]
                tot["nodes"] += r["n_nodes"]
                tot["tree_pivots"] += r["total_pivots"]
                tot["purged"] += r["node_purge_rows"]
                tot["peak"] = max(tot["peak"], r["node_cut_rows_peak"])
                tot["purging_instances"] += r["node_purge_rows"] > 0
                tot["work"] += work
                tot["missed"] += opt is not None and abs(r["best_lower"] - opt) > 1e-6 * (1 + abs(opt))
            emit(dict({"part": "cpu", "set": label, "instances": len(loads), "cut_strat": 1, "node_purge": A}, **kw, **tot), out)

    loads = [((lambda inst=inst: lpgen.load_milp(orc, inst)), rec["optimum"]) for rec, inst in fixtures]
    sweep("general fixtures, every 4th with an optimum", loads)
    sweep("general fixtures, every 4th with an optimum", loads, cut_select=1)
    for case in BINARY:
        model = synth.dense_ilp(*case)
        opt = bnb.branch_and_bound(synth.load_ilp(orc, *model), quirks=0, table=tab, window=64, max_nodes=200000)["best_lower"]
        sweep("dense_ilp%r" % (case,), [((lambda model=model: synth.load_ilp(orc, *model)), opt)], cut_select=1)


def part_call(out):
    import numpy as np
    from mvolps_amd import bnb
    from mvolps_amd.capi import BS, LO, OPT

    from scripts.cutloop_profile import wide_root_cuts

    gpu, root, vals, rhs = wide_root_cuts(32)
    base = root.copy()
    m0 = base.m
    assert bnb.add_cut_rows(base, vals, rhs) == 0
    base.simplex()
    assert base.status == OPT
    # the same model on a handle that was never solved: no tableau, so a deletion is the host share alone
    from mvolps_amd import synth

    cold = synth.load_ilp(gpu, *synth.dense_ilp(*WIDE))
    ind = np.arange(cold.n + 1, dtype=np.int32)
    for t in range(32):
        i = gpu.add_rows(cold.h, 1)
        cold.set_mat_row(i, ind, vals[t])
        gpu.set_row_bnds(cold.h, i, LO, float(rhs[t]), 0.0)
    stat = np.array(base.row_stat())
    slack = [i for i in range(base.m, 0, -1) if stat[i - 1] == BS]  # the cut rows first
    H = 128
    for k in (4, 16, 32):
        rows = sorted(slack[:k])
        assert len(rows) == k
        t_many, t_each, h_many, h_each = [], [], [], []
        for rep in range(8):
            a, b = [base.copy() for _ in range(H)], [base.copy() for _ in range(H)]
            ca, cb = [cold.copy() for _ in range(H)], [cold.copy() for _ in range(H)]
            gpu.sync()
            t0 = time.perf_counter()
            assert bnb.del_rows_many(a, [rows] * H) == 0
            gpu.sync()
            t1 = time.perf_counter()
            for P in b:
                assert P.del_rows(rows) == 0
            gpu.sync()
            t2 = time.perf_counter()
            assert bnb.del_rows_many(ca, [rows] * H) == 0
            t3 = time.perf_counter()
            for P in cb:
                assert P.del_rows(rows) == 0
            t4 = time.perf_counter()
            if rep:  # the first repetition warms every path up
                t_many.append(t1 - t0)
                t_each.append(t2 - t1)
                h_many.append(t3 - t2)
                h_each.append(t4 - t3)
        same = all(np.array_equal(x.tableau().view(np.uint64), y.tableau().view(np.uint64)) for x, y in zip(a[::37], b[::37]))
        it0 = a[0].it_cnt
        a[0].simplex()
        emit({"part": "call", "instance": "512x1024 cap 0.4 U 3 root + 32 GMI rows", "handles": H, "rows": base.m, "k": k,
              "cut_rows_among_them": sum(1 for i in rows if i > m0), "first_row": rows[0], "reps": len(t_many),
              "del_rows_many_ms": statistics.median(t_many) * 1e3, "del_rows_x128_ms": statistics.median(t_each) * 1e3,
              "host_share_many_ms": statistics.median(h_many) * 1e3, "host_share_x128_ms": statistics.median(h_each) * 1e3,
              "same_bits": bool(same), "pivots_after": a[0].it_cnt - it0, "same_objective": bool(a[0].obj == base.obj)}, out)


def part_trees(out, only):
    import mvolps_amd
    from mvolps_amd import bnb, synth

    def tree(model, **kw):
        t0 = time.perf_counter()
        r = bnb.branch_and_bound(synth.load_ilp(mvolps_amd.api(), *model), quirks=0, **kw)
        return r, time.perf_counter() - t0

    wide = synth.dense_ilp(512, 1024, 12345, 3)
    cases = (("config 3, one cut per node", wide, dict(window=64, cut_strat=1, max_nodes=600)),
             ("config 3, efficacy-selected", wide, dict(window=64, cut_strat=1, cut_select=1, cut_chance=0.05, max_nodes=600)),
             ("config 5, one cut per node", config5(), dict(window=64, cut_strat=1, max_nodes=2 * 15697)),
             ("dense_ilp(128,256,7,3) best-bound, node at a time, efficacy-selected", synth.dense_ilp(128, 256, 7, 3),
              dict(node_strat=1, window=1, cut_strat=1, cut_select=1, cut_chance=0.05, max_nodes=2500)))
    for idx, (name, model, kw) in enumerate(cases):
        if only is not None and idx != only:
            continue
        tree(model, **dict(kw, max_nodes=20, node_purge=1))  # warm-up
        for rep in range(2):
            for A in (0, 1, 2, 3):
                r, el = tree(model, node_purge=A, **kw)
                emit(dict({"part": "trees", "instance": name, "node_purge": A, "rep": rep, "rc": r["rc"], "seconds": el,
                           "nodes_per_s": r["count"] / el}, **kw, **{k: r[k] for k in KEYS}), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["cpu", "call", "trees"], required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--out-trees", default=None)
    ap.add_argument("--only", type=int, default=None)
    a = ap.parse_args()
    if a.part == "cpu":
        part_cpu(a.out)
    elif a.part == "call":
        part_call(a.out)
    else:
        part_trees(a.out_trees, a.only)


if __name__ == "__main__":
    main()
