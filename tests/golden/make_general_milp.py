#!/usr/bin/env python3
"""Pins for whole B&B trees on general mixed-integer models: tests/golden/general_milp.json.

The models are lpgen.random_general_milp(SEED, index), index = 0 .. DRAWN - 1 (regenerated from the seed by the tests, not
stored; a SHA-256 of the generated arrays is).  The pin of every instance is decided by enumeration (tests/milp_enum.py);
scipy's HiGHS `milp`, with presolve on and off, is a second opinion whose disagreements are listed in the header.  An
instance is dropped only when it cannot be enumerated (unbounded relaxation, an integer column with an infinite LP range, a
box beyond the limits) -- never because of what a solver or the project's driver answers.

    python tests/golden/make_general_milp.py          # rewrites the file and prints the kept / dropped table
"""
import collections
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import lpgen, milp_enum  # noqa: E402
from mvolps_amd.capi import DB, FR, FX, LO, MAX, MIN, UP  # noqa: E402

SEED = 1000
DRAWN = 480
OUT = os.path.join(HERE, "general_milp.json")
TYPES = {LO: "LO", UP: "UP", DB: "DB", FX: "FX", FR: "FR"}

# Members of the same family from other seeds, kept by name: (name, seed, index).  Of 2000 draws of sub-family a from each of
# the seeds 20000 and 30000, five trees change their answer when a down child loses a negative lower bound (the bug-compatible
# form `UP 0 floor(x)` applied to a LO column); these are the two of them that can be enumerated.  On most trees that mistake
# is invisible: a child's LP optimum sits at floor(x), not at the far bound.
EXTRA = [("down-child-keeps-a-negative-lower-bound-1", 20000, 640), ("down-child-keeps-a-negative-lower-bound-2", 20000, 3763)]

# defects the family exposed in the driver, by name (their instances are ordinary members of sub-family b)
REGRESSIONS = {
    "fractional-lower-bound-branches-forever": "sub-family b: an integer LO column resting on lb = k + 0.5 is branched on; the down "
                                               "child got crossed bounds [k + 0.5, k] and solved to the parent's value",
    "fractional-bound-gmi-cuts-off-optimum": "sub-family b with cut_strat=1: a repaired GMI cut measured from a fractional bound of an "
                                             "integer column is not valid",
}


def conditions(head, insts):
    """The fixture's conditions (the CPU test asserts them again from the header)."""
    kept = head["kept"]
    assert kept >= 240, kept
    for f in "bcd":
        assert head["kept_by_family"][f] >= 25, (f, head["kept_by_family"])
    for d in ("min", "max"):
        assert head["kept_by_direction"][d] >= 0.4 * kept, head["kept_by_direction"]
    assert head["kept_pure"] >= 60 and head["kept_mixed"] >= 100, (head["kept_pure"], head["kept_mixed"])
    for t in TYPES.values():
        assert head["kept_with_col_type"][t] >= 30 and head["kept_with_row_type"][t] >= 30, (t, head)
    a_drawn = head["drawn_by_family"]["a"]
    a_dropped = sum(v for k, v in head["dropped_by_family_and_reason"].items() if k.startswith("a:"))
    assert a_dropped <= 0.5 * a_drawn, (a_dropped, a_drawn)
    assert head["kept_d_with_feasible_relaxation"] >= 25
    assert len(insts) == kept


def main():
    t0 = time.time()
    insts = []
    C = collections.Counter
    drawn_f, kept_f, kept_dir, dropped, colt, rowt, status = C(), C(), C(), C(), C(), C(), C()
    pure = mixed = d_feasible = large = 0
    disagree = []
    extra = []
    for name, seed, index in [(None, SEED, i) for i in range(DRAWN)] + EXTRA:
        inst = lpgen.random_general_milp(seed, index)
        arr = lpgen.milp_arrays(inst)
        e = milp_enum.enumerate_milp(*arr)
        if name is not None:
            assert e["status"] == "optimal", (name, e["status"], e["reason"])
            extra.append({"name": name, "seed": seed, "index": index, "family": inst["family"], "size_class": inst["size_class"],
                          "m": int(arr[0].shape[0]), "n": int(arr[0].shape[1]), "n_int": int(arr[7].sum()),
                          "sha256": lpgen.milp_sha256(inst), "relaxation": e["relaxation"], "status": e["status"],
                          "optimum": e["optimum"], "x": e["x"], "points": e["points"],
                          "highs_presolve_on": list(milp_enum.highs_milp(*arr, presolve=True)),
                          "highs_presolve_off": list(milp_enum.highs_milp(*arr, presolve=False))})
            continue
        drawn_f[inst["family"]] += 1
        if e["status"] == "dropped":
            dropped["%s:%s" % (inst["family"], e["reason"])] += 1
            continue
        hs = [milp_enum.highs_milp(*arr, presolve=p) for p in (True, False)]
        rec = {"index": index, "family": inst["family"], "size_class": inst["size_class"], "m": int(arr[0].shape[0]),
               "n": int(arr[0].shape[1]), "n_int": int(arr[7].sum()), "sha256": lpgen.milp_sha256(inst), "relaxation": e["relaxation"],
               "status": e["status"], "optimum": e["optimum"], "x": e["x"], "points": e["points"],
               "highs_presolve_on": list(hs[0]), "highs_presolve_off": list(hs[1])}
        for name, (st, val) in zip(("presolve on", "presolve off"), hs):
            same = st == e["status"] and (val is None or abs(val - e["optimum"]) <= 1e-6 * (1 + abs(e["optimum"])))
            if not same:
                # "worse point" / "false infeasible": the enumerated point is feasible and better, a certificate the CPU test
                # re-checks; "inconclusive": HiGHS stops at "unbounded or infeasible" on an infeasible model
                kind = "inconclusive" if st.startswith("other") else ("worse point" if st == "optimal" else "false infeasible")
                assert kind == "inconclusive" or e["status"] == "optimal", (index, st, e["status"])
                disagree.append({"index": index, "family": inst["family"], "highs": name, "kind": kind, "highs_answer": [st, val],
                                 "enumerated": [e["status"], e["optimum"]]})
        insts.append(rec)
        kept_f[inst["family"]] += 1
        kept_dir["max" if inst["direction"] == MAX else "min"] += 1
        status[e["status"]] += 1
        large += inst["size_class"]
        pure += int(arr[7].all())
        mixed += int(not arr[7].all())
        d_feasible += int(inst["family"] == "d" and e["relaxation"] == "optimal")
        for t in {t for t, _, _ in inst["col_b"]}:
            colt[TYPES[t]] += 1
        for t in {t for t, _, _ in inst["row_b"]}:
            rowt[TYPES[t]] += 1
    head = {
        "generator": "tests/golden/make_general_milp.py", "family": "tests/lpgen.py random_general_milp(seed, index)",
        "reference": "tests/milp_enum.py (enumeration); HiGHS via scipy %s milp as a second opinion" % __import__("scipy").__version__,
        "seed": SEED, "drawn": DRAWN, "kept": len(insts), "drawn_by_family": dict(sorted(drawn_f.items())),
        "kept_by_family": dict(sorted(kept_f.items())), "dropped_by_family_and_reason": dict(sorted(dropped.items())),
        "kept_by_direction": dict(sorted(kept_dir.items())), "kept_by_status": dict(sorted(status.items())), "kept_pure": pure,
        "kept_mixed": mixed, "kept_large_size_class": large, "kept_d_with_feasible_relaxation": d_feasible,
        "kept_with_col_type": dict(sorted(colt.items())), "kept_with_row_type": dict(sorted(rowt.items())),
        "named": len(extra), "highs_disagreements": disagree, "regressions": REGRESSIONS,
    }
    conditions(head, insts)
    with open(OUT, "w") as f:
        f.write("{\n \"header\": %s,\n \"instances\": [\n" % json.dumps(head, indent=1).replace("\n", "\n "))
        f.write(",\n".join("  " + json.dumps(r) for r in insts))
        f.write("\n ],\n \"named_instances\": [\n")
        f.write(",\n".join("  " + json.dumps(r) for r in extra))
        f.write("\n ]\n}\n")
    print("drawn %d kept %d in %.0f s" % (DRAWN, len(insts), time.time() - t0))
    for k in ("drawn_by_family", "kept_by_family", "dropped_by_family_and_reason", "kept_by_direction", "kept_by_status",
              "kept_with_col_type", "kept_with_row_type"):
        print("%-30s %s" % (k, head[k]))
    print("pure %d mixed %d large %d; d with a feasible relaxation %d; HiGHS disagreements %d" % (pure, mixed, large, d_feasible, len(disagree)))
    for d in disagree:
        print("  ", d)


if __name__ == "__main__":
    main()
