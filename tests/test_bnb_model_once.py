"""The host twins of one tree share one model: however many rules are on, the tree reads the matrix through get_mat_row once
(DESIGN.md "Host model, device flags and adoption").  The oracle's table has none of the batched device entries, so every rule
of these trees runs its twin; with cut_strat = 0 and no root cut rounds nothing else in the driver reads a matrix row."""
import ctypes as C

import pytest

from mvolps_amd import bnb

from . import lpgen
from .test_bnb_general import DRAWN, instance, max_nodes
from .test_bnb_host import same_result

DEVICE_ENTRIES = ("round_many", "polish_many", "propagate_many", "dive_pick_many", "pump_obj_many", "conflict_graph")
RULES = dict(heur=2, pump=20, dive=7, polish=1000, rc_fix=1)
# name -> the driver's keywords and the rules it admits (the best-bound window takes the heuristic and polishing only)
DRIVERS = {
    "serial": dict(window=1, **RULES),
    "window64": dict(window=64, **RULES),
    "best_window8": dict(node_strat=1, best_window=8, heur=2, polish=1000),
}
COUNTERS = bnb.POLISH_COUNTERS + (
    "heur_calls", "heur_found", "heur_improved", "incumbent_heur", "rc_calls", "rc_fixed", "rc_tightened", "prop_calls", "prop_fixed",
    "prop_tightened", "prop_infeasible", "dive_calls", "dive_found", "dive_improved", "dive_lps", "dive_pivots", "pump_calls",
    "pump_found", "pump_improved", "pump_lps", "pump_pivots")
GET_MAT_ROW = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double))


def tree(orc, rec, inst, table, **kw):
    return bnb.branch_and_bound(lpgen.load_milp(orc, inst), quirks=0, table=table, max_nodes=max_nodes(rec), cut_strat=0, cut_rounds=0,
                                **kw)


@pytest.fixture(scope="module")
def plain(orc):
    tab = bnb.table_from(orc)
    for name in DEVICE_ENTRIES:
        assert not getattr(tab, name), name
    return tab


@pytest.fixture(scope="module")
def chosen(orc, plain):
    """The first optimal drawn fixture whose serial tree pumps, dives and polishes at least once each."""
    for rec in DRAWN:
        if rec["status"] != "optimal":
            continue
        inst = instance(rec)
        r = tree(orc, rec, inst, plain, **DRIVERS["serial"])
        if r["rc"] == 0 and r["pump_calls"] >= 1 and r["dive_calls"] >= 1 and r["polish_calls"] >= 1:
            return rec, inst
    raise AssertionError("no general fixture whose tree pumps, dives and polishes")


@pytest.fixture()
def counted(orc):
    """The oracle's table with get_mat_row behind a counter: (table, calls); the callback lives as long as the pair."""
    tab = bnb.table_from(orc)
    inner = GET_MAT_ROW(tab.get_mat_row)
    calls = []

    def get_mat_row(P, i, ind, val):
        calls.append(i)
        return inner(P, i, ind, val)

    cb = GET_MAT_ROW(get_mat_row)
    tab.get_mat_row = C.cast(cb, C.c_void_p).value
    yield tab, calls
    del cb


# the best-bound window refuses prop
@pytest.mark.parametrize("driver,prop", [("serial", 0), ("serial", 8), ("window64", 0), ("window64", 8), ("best_window8", 0)])
def test_one_tree_reads_the_matrix_once(orc, plain, chosen, counted, driver, prop):
    rec, inst = chosen
    tab, calls = counted
    kw = dict(DRIVERS[driver], prop=prop)
    ref = tree(orc, rec, inst, plain, **kw)
    got = tree(orc, rec, inst, tab, **kw)
    assert ref["rc"] == got["rc"] == 0
    if driver != "best_window8":
        assert got["pump_calls"] >= 1 and got["dive_calls"] >= 1
    assert got["heur_calls"] >= 1 and got["polish_calls"] >= 1
    m0 = rec["m"]
    print("%s prop=%d: %d get_mat_row calls, m0 = %d" % (driver, prop, len(calls), m0))
    # the tree's model once; with prop the root's own propagation, which runs before the root's bounds are final, once more
    assert 0 < len(calls) <= (2 * m0 if prop else m0), (len(calls), m0)
    same_result(got, ref)
    for k in COUNTERS:
        assert got[k] == ref[k], k
