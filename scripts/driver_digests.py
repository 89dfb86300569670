"""CPU-only record of what the three C++ B&B drivers compute: the drivers over the oracle's LP table on a fixed grid of
instances, node limits, option sets and window sizes.  Two builds that print the same lines took the same decisions with the
same bits (profiles/driver_digests_cpu.jsonl is the committed record).

--full prints one JSON line per run: the options, the return code, treedigest.summary, sha256 of x and of node_bound, and every
counter (11 200 lines, 10 MB).  Without it the runs of one instance, mode (bug-compatible / repaired) and driver share a line:
how many runs, how many of them refused, the nodes they counted, and the sha256 of their --full lines.  A line that differs
names the group to look at with --full.  usage: driver_digests.py [--full]"""
import ctypes as C
import hashlib
import itertools
import json
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvolps_amd import bnb, synth, treedigest
from oracle import oracle
from tests import lpgen

COUNTERS = ("rounds", "speculated", "sb_lps", "sb_pivots", "heur_calls", "heur_found", "heur_improved", "incumbent_heur", "rc_calls",
            "rc_fixed", "rc_tightened", "prop_calls", "prop_fixed", "prop_tightened", "prop_infeasible")
# (window, node_strat, best_window): the serial driver in both node orders, the FIFO window, the best-bound window
DRIVERS = ((1, 0, 0), (7, 0, 0), (64, 0, 0), (1, 1, 0), (1, 1, 8))


def instances(orc):
    """(name, loader) pairs; a loader makes a fresh handle, since a run may edit the one it is given."""
    out = []
    for m, n, seed, U in ((6, 12, 2, 3), (10, 20, 4, 3), (16, 32, 5, 2)):
        A, b, c, UU = synth.dense_ilp(m, n, seed, U)
        out.append(("dense_%dx%d_s%d_U%d" % (m, n, seed, U), lambda A=A, b=b, c=c, UU=UU: lpgen.load_ilp(orc, A, b, c, UU)))
    golden = json.load(open(os.path.join(os.path.dirname(lpgen.__file__), "golden", "general_milp.json")))
    seen = set()
    for rec in golden["instances"] + golden["named_instances"]:  # the first instance of each family
        if rec["family"] in seen:
            continue
        seen.add(rec["family"])
        inst = lpgen.random_general_milp(rec.get("seed", golden["header"]["seed"]), rec["index"])
        out.append(("milp_%s_%d" % (rec["family"], rec["index"]), lambda inst=inst: lpgen.load_milp(orc, inst)))
    A, c = lpgen.setcover_ilp(40, 60, 3)
    out.append(("setcover_40x60_s3", lambda A=A, c=c: lpgen.load_setcover(orc, A, c)))
    return out


def option_sets():
    for cut, var in itertools.product((0, 1), range(5)):
        yield dict(quirks=1, cut_strat=cut, var_strat=var)
    for cut, var, heur, rc, prop in itertools.product((0, 1), range(5), (0, 2), (0, 1), (0, 4)):
        yield dict(quirks=0, cut_strat=cut, var_strat=var, heur=heur, rc_fix=rc, prop=prop)


def hexes(v):
    return hashlib.sha256(b"".join(struct.pack("<d", float(t)) for t in v)).hexdigest()


def run(load, tab, loop_limit=None, **kw):
    pr = bnb.make_params(**kw)
    if loop_limit is not None:
        pr.loop_limit = loop_limit
    res = bnb.BnbResult()
    L = bnb.lib()
    prob = load()  # held until the call has returned
    rc = L.mvx_branchAndBound(C.cast(C.pointer(tab), C.c_void_p), prob.h, C.byref(pr), C.byref(res))
    r = bnb.result_to_dict(res)
    L.mvx_bnb_free_result(C.byref(res))
    line = dict(kw, loop_limit=loop_limit, rc=rc, summary=treedigest.summary(r), x=hexes(r["x"]), node_bound=hexes(r["node_bound"]))
    line.update({k: r[k] for k in COUNTERS})
    return line


def main():
    full = "--full" in sys.argv[1:]
    orc = oracle.api()
    tab = bnb.table_from(orc)
    for name, load in instances(orc):
        groups = {}  # (quirks, driver) -> [runs, refused, nodes, sha256 of the full lines]
        for opt in option_sets():
            for window, node_strat, best_window in DRIVERS:
                # no limit, and the limit met at the root and inside a tree; bug-compatible trees need not close (a child
                # drops its parent's opposite bound), so there "no limit" is 300 nodes
                limits = [(mx, None) for mx in (0 if opt["quirks"] == 0 else 300, 1, 7)]
                if opt["var_strat"] == 0 and not opt.get("prop"):
                    limits.append((0, 3))  # bs.cpp:320 trips once count passes it
                g = groups.setdefault((opt["quirks"], window, node_strat, best_window), [0, 0, 0, hashlib.sha256()])
                for max_nodes, loop_limit in limits:
                    line = run(load, tab, loop_limit=loop_limit, max_nodes=max_nodes, window=window, node_strat=node_strat,
                               best_window=best_window, **opt)
                    text = json.dumps(dict(instance=name, **line), sort_keys=True)
                    if full:
                        print(text)
                    g[0] += 1
                    g[1] += line["rc"] == -1
                    g[2] += line["summary"]["count"]
                    g[3].update(text.encode() + b"\n")
        for (quirks, window, node_strat, best_window), g in ({} if full else groups).items():
            print(json.dumps(dict(instance=name, quirks=quirks, window=window, node_strat=node_strat, best_window=best_window, runs=g[0],
                                  refused=g[1], nodes=g[2], sha256=g[3].hexdigest())))


if __name__ == "__main__":
    main()
