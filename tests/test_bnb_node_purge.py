"""CPU: purging of slack cut rows in the tree (DESIGN.md "Cut purging in the tree (node_purge)") over the ORACLE's table.  That
table has neither del_rows nor del_rows_many, so a purged row becomes a free row: the host side of the definition -- the ages a
node inherits, the age step in front of the cut step, the lists both children take, dead rows, the counters -- runs, and a
child's LP is the one a deletion leaves.

Every fixture instance closes on its enumerated pin with cut_strat = 1 and node_purge = 1 under each node-at-a-time and window
driver, with one cut per node and with efficacy-selected cuts; the purge removes rows on the pinned number of instances; windows
give the serial tree and counters; node_purge = 0 is the result without the keyword; the refusals return their codes.  The age
step is checked from numbers alone, and mvx_del_rows_many on the model layer of the product's library, which needs no device."""
import os
import subprocess

import numpy as np
import pytest

import mvolps_amd
from mvolps_amd import bnb, capi, synth

from . import lpgen
from .test_bnb_general import INSTANCES, check_pin, failures, instance, run
from .test_bnb_host import same_result
from .test_bnb_purge import model, read_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    assert not t.del_rows and not t.del_rows_many  # the free-row path of the definition runs over the oracle
    return t


def check_counters(r):
    assert 0 <= r["node_purge_calls"] <= r["node_purge_rows"]
    assert r["node_purge_calls"] % 2 == 0  # both children of a node lose the same rows
    assert r["node_cut_rows_peak"] >= 0


# ------------------------------------------------------------------------------------------------ whole trees

DRIVERS = {"window1": dict(window=1), "window64": dict(window=64), "best": dict(node_strat=1, window=1)}
# instances on which node_purge_rows > 0, from the run of this test with the finished driver over the oracle's table (the trees
# are deterministic: the same counts on every machine); (driver, cut_select) -> count
PURGED_ON = {("window1", 0): 61, ("window64", 0): 61, ("best", 0): 58, ("window1", 1): 71, ("window64", 1): 71, ("best", 1): 70}


@pytest.mark.parametrize("cut_select", [0, 1])
@pytest.mark.parametrize("name", list(DRIVERS))
def test_trees_close_on_the_enumerated_optimum(orc, tab, name, cut_select):
    purged = []

    def one(rec):
        inst = instance(rec)
        r = run(orc, rec, inst, table=tab, cut_strat=1, cut_select=cut_select, node_purge=1, **DRIVERS[name])
        check_pin(rec, inst, r)
        check_counters(r)
        purged.append(r["node_purge_rows"])

    bad = failures(INSTANCES, one)
    assert not bad, "\n".join(bad)
    on = sum(1 for k in purged if k > 0)
    assert PURGED_ON[name, cut_select] >= 10
    assert on >= PURGED_ON[name, cut_select], "the purge removed rows on %d instances only" % on


def test_windows_give_the_serial_tree(orc, tab):
    def one(rec):
        inst = instance(rec)
        for extra in (dict(), dict(cut_select=1), dict(cut_rounds=5), dict(heur=2, rc_fix=1, prop=4)):
            ref = run(orc, rec, inst, table=tab, window=1, cut_strat=1, node_purge=1, **extra)
            check_counters(ref)
            for w in (2, 8, 64):
                got = run(orc, rec, inst, table=tab, window=w, cut_strat=1, node_purge=1, **extra)
                same_result(got, ref)
                for k in bnb.NODE_PURGE_COUNTERS:
                    assert got[k] == ref[k], (k, w, extra)

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)


def test_node_purge_0_is_the_result_without_the_keyword(orc, tab):
    def one(rec):
        inst = instance(rec)
        for kw in (dict(window=1, cut_strat=1), dict(window=64, cut_strat=1, cut_select=1), dict(node_strat=1, window=1, cut_strat=1),
                   dict(window=64, cut_strat=1, cut_rounds=5, cut_purge=1), dict(window=64)):
            ref = run(orc, rec, inst, table=tab, **kw)
            got = run(orc, rec, inst, table=tab, node_purge=0, **kw)
            assert got == ref, kw
            assert got["node_purge_calls"] == 0 and got["node_purge_rows"] == 0
        # no tree cut rows at all: the plain tree, whatever the age limit
        for kw in (dict(window=1), dict(window=64), dict(node_strat=1, window=1)):
            ref = run(orc, rec, inst, table=tab, **kw)
            got = run(orc, rec, inst, table=tab, node_purge=3, cut_strat=0, cut_rounds=0, **kw)
            assert got == ref and got["node_purge_calls"] == 0 and got["node_cut_rows_peak"] == 0, kw

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)


def test_peak_counts_live_rows_with_and_without_the_purge(orc, tab):
    """node_cut_rows_peak is computed at A = 0 too, so the two can be compared: with one cut per node it is the depth of the
    deepest node at the most (a node adds one row or none), with the purge on or off; an age limit that no row of the tree can
    reach purges nothing and leaves the tree and the peak alone."""

    def deepest(r):
        depth = {1: 0}
        for oid in range(2, r["n_nodes"] + 1):
            depth[oid] = depth[r["parent"][oid - 1]] + 1
        return max(depth.values())

    deep = 0
    for rec in [r for r in INSTANCES if r["status"] == "optimal"][::6]:
        inst = instance(rec)
        r0 = run(orc, rec, inst, table=tab, window=64, cut_strat=1)
        assert 0 <= r0["node_cut_rows_peak"] <= deepest(r0) < 64
        r64 = run(orc, rec, inst, table=tab, window=64, cut_strat=1, node_purge=64)
        same_result(r64, r0)
        assert r64["node_purge_rows"] == 0 and r64["node_cut_rows_peak"] == r0["node_cut_rows_peak"]
        r1 = run(orc, rec, inst, table=tab, window=64, cut_strat=1, node_purge=1)
        assert 0 <= r1["node_cut_rows_peak"] <= deepest(r1)
        deep += deepest(r0) >= 3
    assert deep >= 3  # the sample has trees in which a row can age at all


# ------------------------------------------------------------------------------------------------ the age step


def ages_restated(basic, A, age):
    age, out = list(age), []
    for t, b in enumerate(basic):
        if age[t] == 255:
            continue
        age[t] = min(age[t] + 1, 254) if b else 0
        if age[t] >= A:
            out.append(t)
    return age, out


def test_purge_ages_against_a_restatement():
    rng = np.random.default_rng(11)
    for _ in range(300):
        k = int(rng.integers(0, 40))
        A = int(rng.integers(1, 65))
        age = rng.choice([0, 1, 2, 3, A - 1, A, 63, 64, 253, 254, 255], size=k).astype(np.uint8)
        basic = rng.integers(0, 2, size=k)
        rc, got_age, got_out = bnb.purge_ages(basic, A, age)
        want_age, want_out = ages_restated(basic.tolist(), A, age.tolist())
        assert rc == 0 and got_age == want_age and got_out == want_out, (k, A)


def test_purge_ages_by_hand():
    assert bnb.purge_ages([0, 1, 0], 2, [1, 0, 0]) == (0, [0, 1, 0], [])  # a non-basic row starts again
    assert bnb.purge_ages([1, 1, 1], 2, [1, 0, 2]) == (0, [2, 1, 3], [0, 2])  # reaching A exactly, and a row beyond it
    assert bnb.purge_ages([1, 1], 64, [63, 62]) == (0, [64, 63], [0])  # A = 64
    assert bnb.purge_ages([1, 1, 0], 64, [254, 253, 254]) == (0, [254, 254, 0], [0, 1])  # saturation at 254
    assert bnb.purge_ages([1, 0, 1], 1, [255, 255, 0]) == (0, [255, 255, 1], [2])  # dead rows are skipped
    assert bnb.purge_ages([], 1, []) == (0, [], [])
    # bad arguments
    L = bnb.lib()
    IP, UP = bnb.C.POINTER(bnb.C.c_int), bnb.C.POINTER(bnb.C.c_ubyte)
    b = np.ones(2, dtype=np.int32)
    a = np.zeros(2, dtype=np.uint8)
    o = np.zeros(2, dtype=np.int32)
    n = bnb.C.c_int(7)
    args = lambda: (b.ctypes.data_as(IP), a.ctypes.data_as(UP), o.ctypes.data_as(IP))  # noqa: E731
    bp, ap, op = args()
    for A in (0, -1, 65):
        assert L.mvx_bnb_purge_ages(2, bp, A, ap, op, bnb.C.byref(n)) == -1
    assert L.mvx_bnb_purge_ages(-1, bp, 1, ap, op, bnb.C.byref(n)) == -1
    assert L.mvx_bnb_purge_ages(2, None, 1, ap, op, bnb.C.byref(n)) == -1
    assert L.mvx_bnb_purge_ages(2, bp, 1, None, op, bnb.C.byref(n)) == -1
    assert L.mvx_bnb_purge_ages(2, bp, 1, ap, None, bnb.C.byref(n)) == -1
    assert L.mvx_bnb_purge_ages(2, bp, 1, ap, op, None) == -1
    assert a.tolist() == [0, 0] and n.value == 7  # and nothing was written
    assert L.mvx_bnb_purge_ages(0, None, 1, None, None, bnb.C.byref(n)) == 0 and n.value == 0


# ------------------------------------------------------------------------------------------------ mvx_del_rows_many, model layer


def test_del_rows_many_on_the_model():
    """Never-solved handles lose different rows in one call; the clones taken before keep theirs (the row list is
    copy-on-write), a handle with an empty list keeps even its status word, and every handle ends as mvx_del_rows leaves it."""
    api = mvolps_amd.api()
    lists = [[1], [6], [4, 3], [2, 3, 4, 5, 6], [], [1, 2, 3, 4, 5, 6]]
    base, _A, _rows = model(api)
    before = read_model(api, base)
    hs = [base.copy() for _ in lists]
    twins = [base.copy() for _ in lists]
    clones = [h.copy() for h in hs]
    own = api.add_rows(hs[1].h, 2)  # two rows of its own behind the shared ones: the list's tail
    api.add_rows(twins[1].h, 2)
    lists[1] = [6, own + 1]
    assert bnb.del_rows_many(hs, lists) == 0
    for h, tw, cl, l in zip(hs, twins, clones, lists):
        if l:
            assert tw.del_rows(l) == 0
        assert h.m == tw.m == api.get_num_rows(h.h) and read_model(api, h) == read_model(api, tw), l
        assert api.get_status(h.h) == api.get_status(tw.h) == capi.UNDEF
        assert cl.m == 6 and read_model(api, cl) == before
    keep = [i for i in range(1, 7) if i not in (3, 4)]
    assert read_model(api, hs[2]) == [before[i - 1] for i in keep] and hs[4].m == 6 and hs[5].m == 0
    assert read_model(api, base) == before
    # one handle is a batch too, and rows can go again behind a batch
    assert bnb.del_rows_many([hs[0]], [[1, hs[0].m]]) == 0 and read_model(api, hs[0]) == before[2:5]


def test_del_rows_many_refusals_change_nothing():
    api = mvolps_amd.api()
    base, _A, _rows = model(api)
    before = read_model(api, base)
    hs = [base.copy() for _ in range(3)]
    other, _A2, _r2 = model(api)
    api.add_cols(other.h, 1)  # another column count

    def untouched():
        return all(h.m == 6 and read_model(api, h) == before for h in hs)

    for lists in ([[1], [2], [2, 2]], [[1], [2], [7]], [[1], [2], [0]], [[1], [2], [-1]], [[0], [2], [3]], [[1], [3, 1, 3], [2]]):
        assert bnb.del_rows_many(hs, lists) == -1 and untouched(), lists  # the last handle's list is checked before the first is edited
    assert bnb.del_rows_many([hs[0], hs[1], hs[0]], [[1], [2], [3]]) == -1 and untouched()  # a handle listed twice
    assert bnb.del_rows_many([hs[0], other], [[1], [2]]) == -1 and untouched() and other.m == 6  # column counts differ
    L = bnb.lib()
    IP = bnb.C.POINTER(bnb.C.c_int)
    arr = (bnb.C.c_void_p * 3)(*[h.h for h in hs])
    off = np.array([0, 1, 2, 3], dtype=np.int32)
    rows = np.array([1, 2, 3], dtype=np.int32)
    op, rp = off.ctypes.data_as(IP), rows.ctypes.data_as(IP)
    assert L.mvx_del_rows_many(None, 3, op, rp) == -1 and L.mvx_del_rows_many(arr, 0, op, rp) == -1
    assert L.mvx_del_rows_many(arr, -1, op, rp) == -1 and L.mvx_del_rows_many(arr, 3, None, rp) == -1
    assert L.mvx_del_rows_many(arr, 3, op, None) == -1 and untouched()
    bad_off = np.array([0, 2, 1, 3], dtype=np.int32)  # descending
    assert L.mvx_del_rows_many(arr, 3, bad_off.ctypes.data_as(IP), rp) == -1 and untouched()
    null_in = (bnb.C.c_void_p * 3)(hs[0].h, None, hs[2].h)
    assert L.mvx_del_rows_many(null_in, 3, op, rp) == -1 and untouched()
    assert L.mvx_del_rows_many(arr, 3, op, rp) == 0 and [h.m for h in hs] == [5, 5, 5]


# ------------------------------------------------------------------------------------------------ refusals, front end


def test_refusals(orc, tab):
    from mvolps_amd import dist_bnb, dist_native

    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    for kw in (dict(quirks=0, node_purge=-1), dict(quirks=0, node_purge=65), dict(quirks=1, node_purge=1), dict(node_purge=1),
               dict(quirks=1, cut_strat=1, node_purge=2), dict(quirks=0, node_strat=1, best_window=8, node_purge=1),
               dict(quirks=0, node_strat=1, best_window=1, node_purge=1), dict(quirks=1, node_purge=-1)):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, **kw)
        assert r["rc"] == -1 and r["n_nodes"] == 0 and r["count"] == 0, kw
    for kw in (dict(node_purge=0), dict(node_purge=1), dict(node_purge=64, cut_strat=1), dict(node_purge=1, cut_strat=1, node_strat=1),
               dict(node_purge=2, cut_rounds=5, cut_purge=1), dict(node_purge=1, cut_strat=1, heur=2, rc_fix=1, prop=4, dive=7, pump=30, polish=10)):
        assert bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0, **kw)["rc"] == 0, kw
    P = lpgen.load_ilp(orc, A, b, c, U)
    with pytest.raises(ValueError):
        dist_native.branch_and_bound(P, table=tab, node_purge=1, quirks=0)
    with pytest.raises(ValueError):
        dist_bnb.branch_and_bound(None, P, node_purge=1, quirks=0)
    pr = bnb.make_params(quirks=0, node_purge=1)
    L = dist_native._lib()
    res, st = bnb.BnbResult(), dist_native.DistStats()
    tptr = bnb.C.cast(bnb.C.pointer(tab), bnb.C.c_void_p)
    assert L.mvx_branchAndBound_dist(tptr, None, P.h, bnb.C.byref(pr), None, None, bnb.C.byref(res), bnb.C.byref(st)) == capi.EFAIL
    # without tree cut rows there is nothing to age: a table that cannot tell a row's status still runs the plain tree.  (With
    # cut rows such a table gets -2 from the age step; no test reaches it, because the cut generation reads get_row_stat first.)
    bare = bnb.table_from(orc)
    bare.get_row_stat = None
    A2, b2, c2, U2 = synth.dense_ilp(10, 20, 4, 3)
    for kw in (dict(window=1), dict(window=64), dict(node_strat=1, window=1)):
        ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A2, b2, c2, U2), table=tab, quirks=0, **kw)
        assert ref["n_nodes"] >= 3
        assert bnb.branch_and_bound(lpgen.load_ilp(orc, A2, b2, c2, U2), table=bare, quirks=0, node_purge=1, **kw) == ref


def test_python_front_end_lists_the_new_names():
    assert bnb._OPTIONAL[-1] == "del_rows_many"
    assert bnb.BnbParams._fields_[-1][0] == "node_purge"
    assert tuple(f[0] for f in bnb.BnbResult._fields_[-3:]) == bnb.NODE_PURGE_COUNTERS
    t = bnb.LpApiTable.from_address(bnb.lib().mvx_hip_lp_api())
    assert t.del_rows_many and t.del_rows and t.polish_many


def test_cli_flag_parses():
    """--node-purge on tests/golden/f1.lp.  Without a device the front end can not solve, so the value is followed up to the
    driver's refusal: without --repaired the driver refuses it and the message names the flag; values out of range are refused by
    the parser itself."""
    exe = os.path.join(ROOT, "mvolps_amd", "bin", "mvolps")
    f1 = os.path.join(ROOT, "tests", "golden", "f1.lp")

    def cli(*flags):
        return subprocess.run([exe, "-f", f1, *flags], capture_output=True, text=True)

    assert "--node-purge" in subprocess.run([exe, "-h"], capture_output=True, text=True).stdout
    for flags in (("--node-purge",), ("--node-purge", "1"), ("--node-purge", "64", "-cm", "1"), ("--node-purge", "-cm", "1")):
        r = cli(*flags)
        assert r.returncode != 0 and "/ --node-purge are not supported" in r.stderr and "Unknown parameter" not in r.stderr, (flags, r.stderr)
    for bad in ("0", "65", "x", "1x"):
        r = cli("--repaired", "--node-purge", bad)
        assert r.returncode != 0 and "Unknown parameter value for --node-purge" in r.stderr, (bad, r.stderr)
