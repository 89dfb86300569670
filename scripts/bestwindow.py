"""Best-bound B&B on the 512x1024 ILP: node at a time against the speculative window (best_window 8 / 32 / 64), without
and with GMI cuts.  Every window run must reproduce the node-at-a-time tree (asserted); one JSON line per run with
nodes/s, rounds and speculated nodes.  MVX_BNB_TIMING=1 in the environment adds the window's phase times on stderr."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvolps_amd
from mvolps_amd import bnb, synth
from tests import lpgen

m, n = 512, 1024
nodes = int(sys.argv[1]) if len(sys.argv) > 1 else 1500
api = mvolps_amd.api()
A, b, c, U = synth.dense_ilp(m, n, 12345, 3)
bnb.branch_and_bound(lpgen.load_ilp(api, A, b, c, U), quirks=0, node_strat=1, max_nodes=20, best_window=8)  # warm-up
KEYS = ("events", "prune", "parent", "count", "total_pivots", "node_bound", "x", "incumbent_oid", "best_lower")
for mode in (dict(quirks=0), dict(quirks=1), dict(quirks=0, cut_strat=1), dict(quirks=1, cut_strat=1)):
    ref = None
    for W in (0, 8, 32, 64):
        print("mode %s best_window %d" % (mode, W), file=sys.stderr, flush=True)
        t = time.perf_counter()
        r = bnb.branch_and_bound(lpgen.load_ilp(api, A, b, c, U), node_strat=1, max_nodes=nodes, best_window=W, **mode)
        dt = time.perf_counter() - t
        if ref is None:
            ref = r
        same = all(repr(r[k]) == repr(ref[k]) for k in KEYS)
        print(json.dumps({"mode": mode, "best_window": W, "nodes": r["count"], "pivots": r["total_pivots"], "rounds": r["rounds"],
                          "speculated": r["speculated"], "ms": dt * 1e3, "nodes_per_s": r["count"] / dt, "same_tree": same}), flush=True)
        assert same, (mode, W)
