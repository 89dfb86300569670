"""CPU: purging of slack cut rows in the root cut rounds (DESIGN.md "Cut purging (cut_purge)") over the ORACLE's table.  That table
has no del_rows entry, so a purged row becomes a free row: the host side of the definition -- ages, the one purge call per round,
the extra solve, the live-row budget, the counters -- runs, and the LP stays the one a deletion leaves.

Every fixture instance closes on its enumerated pin with the purge in front of each single-GPU driver; the purge removes rows on
at least 30 of them; windows give the serial tree; cut_purge = 0 is the result without the keyword; the refusals return their
codes.  mvx_del_rows itself is checked on the model layer of the product's library, which needs no device."""
import numpy as np
import pytest

import mvolps_amd
from mvolps_amd import bnb, capi, synth

from . import lpgen
from .test_bnb_cutloop import COUNTERS, PIN_OPTIONS
from .test_bnb_general import INSTANCES, check_pin, failures, instance, run
from .test_bnb_host import same_result

LOOP_COUNTERS = COUNTERS + bnb.CLIQUE_COUNTERS + bnb.PURGE_COUNTERS


@pytest.fixture(scope="module")
def tab(orc):
    t = bnb.table_from(orc)
    assert not t.del_rows and not t.add_cut_rows  # the free-row path of the definition runs over the oracle
    return t


def check_counters(r):
    assert r["cutloop_live_rows"] == r["cutloop_rows"] - r["cutloop_purged"] and 0 <= r["cutloop_purged"] <= r["cutloop_rows"]
    assert r["cutloop_lps"] in (0, 1 + r["cutloop_rounds"])  # the solve behind a purge is not one of the loop's LPs


# ------------------------------------------------------------------------------------------------ whole trees


@pytest.mark.parametrize("name", list(PIN_OPTIONS))
def test_trees_behind_the_purge_close_on_the_enumerated_optimum(orc, tab, name):
    kw = dict(PIN_OPTIONS[name], cut_purge=1)
    assert kw["cut_rounds"] == 5
    purged = []

    def one(rec):
        inst = instance(rec)
        r = run(orc, rec, inst, table=tab, **kw)
        check_pin(rec, inst, r)
        check_counters(r)
        purged.append(r["cutloop_purged"])

    bad = failures(INSTANCES, one)
    assert not bad, "\n".join(bad)
    assert sum(1 for k in purged if k > 0) >= 30, "the purge removed rows on %d instances only" % sum(1 for k in purged if k > 0)


def test_windows_give_the_serial_tree(orc, tab):
    def same(a, b):
        same_result(a, b)
        for k in LOOP_COUNTERS:
            assert a[k] == b[k], k

    def one(rec):
        inst = instance(rec)
        ref = run(orc, rec, inst, table=tab, window=1, cut_rounds=5, cut_purge=1)
        check_counters(ref)
        for w in (2, 8, 64):
            same(run(orc, rec, inst, table=tab, window=w, cut_rounds=5, cut_purge=1), ref)

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)


def test_cut_purge_0_is_the_result_without_the_keyword(orc, tab):
    def one(rec):
        inst = instance(rec)
        for kw in (dict(window=1), dict(window=64, cut_strat=1), dict(window=64, cut_families=3)):
            ref = run(orc, rec, inst, table=tab, cut_rounds=5, **kw)
            got = run(orc, rec, inst, table=tab, cut_rounds=5, cut_purge=0, **kw)
            same_result(got, ref)
            for k in LOOP_COUNTERS:
                assert got[k] == ref[k], k
            assert got["cutloop_purged"] == 0 and got["cutloop_live_rows"] == got["cutloop_rows"]

    bad = failures(INSTANCES[::10], one)
    assert not bad, "\n".join(bad)


def test_the_loops_own_entry(orc, tab):
    """mvx_bnb_cut_loop_purge on the handle: purge = 0 is mvx_bnb_cut_loop_families; with a purge the free rows stay in the
    handle (the oracle's table deletes nothing), are MVX_FR, and the handle is left OPT on the bound the loop reports."""
    purged_somewhere = 0
    for rec in [r for r in INSTANCES if r["status"] == "optimal"][::8]:
        inst = instance(rec)

        def root():
            P = lpgen.load_milp(orc, inst)
            assert bnb.integral_bounds(P, table=tab) != 2
            return P

        P0, P1 = root(), root()
        rc0, out0 = bnb.cut_loop(P0, rounds=5, table=tab, families=1)
        rc1, out1 = bnb.cut_loop(P1, rounds=5, table=tab, families=1, purge=0)
        assert rc0 == rc1 == 0 and all(out0[k] == out1[k] for k in out0) and out1["cutloop_purged"] == 0
        for A in (1, 2, 64):
            P = root()
            m0 = P.m
            rc, out = bnb.cut_loop(P, rounds=5, table=tab, purge=A)
            assert rc == 0
            check_counters(out)
            assert P.m == m0 + out["cutloop_rows"]  # free rows stay
            free = [i for i in range(m0 + 1, P.m + 1) if orc.get_row_type(P.h, i) == capi.FR]
            assert len(free) == out["cutloop_purged"]
            assert P.status == capi.OPT and P.obj == out["cutloop_bound"]
            if A == 64:
                assert out["cutloop_purged"] == 0  # five rounds never reach that age
            purged_somewhere += out["cutloop_purged"] > 0
    assert purged_somewhere >= 3


# ------------------------------------------------------------------------------------------------ refusals


def test_refusals(orc, tab):
    A, b, c, U = synth.dense_ilp(8, 16, 3, 2)
    for kw in (dict(cut_rounds=5, quirks=0, cut_purge=-1), dict(cut_rounds=5, quirks=0, cut_purge=65),
               dict(cut_rounds=5, quirks=1, cut_purge=1), dict(cut_rounds=5, cut_purge=1)):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, **kw)
        assert r["rc"] == -1 and r["n_nodes"] == 0 and r["count"] == 0, kw
    for kw in (dict(cut_rounds=5, cut_purge=0), dict(cut_rounds=5, cut_purge=1), dict(cut_rounds=5, cut_purge=64),
               dict(cut_rounds=0, cut_purge=-1), dict(cut_rounds=0, cut_purge=65), dict(cut_rounds=0, cut_purge=7)):
        assert bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0, **kw)["rc"] == 0, kw
    # not read when the loop is off: the result is that of leaving it out, in bug-compatible mode too
    ref = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0)
    assert bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, quirks=0, cut_purge=99) == ref
    assert bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), table=tab, cut_purge=-3)["rc"] == 0
    for kw in (dict(purge=-1), dict(purge=65)):
        assert bnb.cut_loop(lpgen.load_ilp(orc, A, b, c, U), table=tab, **kw)[0] == -1, kw
    # a table without get_row_stat cannot age a row: an error, not a loop without the purge
    bare = bnb.table_from(orc)
    bare.get_row_stat = None
    assert bnb.cut_loop(lpgen.load_ilp(orc, A, b, c, U), table=bare, purge=1)[0] == -2


# ------------------------------------------------------------------------------------------------ mvx_del_rows, model layer


def model(api):
    """A 6 x 5 model with every row type, no two rows alike."""
    rng = np.random.default_rng(7)
    A = rng.integers(-4, 5, size=(6, 5)).astype(np.float64)
    A[np.arange(6), np.arange(6) % 5] += 10.0 + np.arange(6)
    rows = [(capi.UP, 0.0, 11.0), (capi.LO, -2.0, 0.0), (capi.DB, -3.0, 13.0), (capi.FX, 4.0, 4.0), (capi.FR, 0.0, 0.0), (capi.UP, 0.0, 16.0)]
    cols = [(capi.LO, 0.0, 0.0)] * 5
    P = api.create()
    P.load_general(A, rows, cols, np.arange(1.0, 6.0))
    return P, A, rows


def read_model(api, P):
    out = []
    for i in range(1, P.m + 1):
        ind, val = P.get_mat_row(i)
        coef = np.zeros(P.n)
        coef[np.asarray(ind, dtype=int) - 1] = val
        out.append((coef.tolist(), api.get_row_type(P.h, i), api.get_row_lb(P.h, i), api.get_row_ub(P.h, i)))
    return out


@pytest.mark.parametrize("dele", [[1], [6], [3, 4], [4, 3], [2, 3, 4, 5, 6], [1, 2, 3, 5, 6], [1, 2, 3, 4, 5, 6]], ids=str)
def test_del_rows_on_the_model(dele):
    api = mvolps_amd.api()
    P, _A, _rows = model(api)
    before = read_model(api, P)
    clone = P.copy()
    assert P.del_rows(dele) == 0
    keep = [i for i in range(1, 7) if i not in dele]
    assert P.m == len(keep) == api.get_num_rows(P.h) and P.n == 5
    assert read_model(api, P) == [before[i - 1] for i in keep]
    assert api.get_status(P.h) == capi.UNDEF
    assert all(api.get_row_stat(P.h, i) == capi.BS for i in range(1, P.m + 1))
    # the clone taken before shares the rows and the list: it keeps all six
    assert clone.m == 6 and read_model(api, clone) == before
    # rows can be appended behind a deletion, and deleted again
    first = api.add_rows(P.h, 2)
    assert first == len(keep) + 1 and P.m == len(keep) + 2
    assert P.del_rows([first]) == 0 and P.m == len(keep) + 1
    assert read_model(api, P)[: len(keep)] == [before[i - 1] for i in keep]
    assert read_model(api, clone) == before


def test_del_rows_in_the_tail_and_in_a_shared_head():
    """Rows a handle appended itself (its list's tail) and rows of a frozen head shared with a clone: either way only the
    handle that deletes changes."""
    api = mvolps_amd.api()
    P, _A, _rows = model(api)
    Q = P.copy()
    first = api.add_rows(Q.h, 3)  # Q's own tail
    for t in range(3):
        Q.set_mat_row(first + t, [0, 1 + t], [0.0, 5.0 + t])
        api.set_row_bnds(Q.h, first + t, capi.LO, float(t), 0.0)
    R = Q.copy()
    full = read_model(api, Q)
    assert Q.del_rows([first + 1]) == 0
    assert read_model(api, Q) == full[: first] + full[first + 1:]
    assert read_model(api, R) == full and read_model(api, P) == full[:6]
    assert Q.del_rows([2, Q.m]) == 0  # one in the shared head, one in the tail
    assert read_model(api, Q) == [full[0]] + full[2:6] + [full[6]]
    assert read_model(api, R) == full and read_model(api, P) == full[:6]


def test_del_rows_refusals_change_nothing():
    api = mvolps_amd.api()
    P, _A, _rows = model(api)
    before = read_model(api, P)
    for bad in ([2, 2], [0], [7], [1, 7], [-1], [3, 1, 3]):
        assert P.del_rows(bad) == -1, bad
        assert P.m == 6 and read_model(api, P) == before
    assert P.del_rows([]) == -1  # nrs = 0
    num = np.array([0, 1], dtype=np.int32)
    assert api.del_rows(None, 1, num.ctypes.data_as(capi._IP)) == -1 and api.del_rows(P.h, 1, None) == -1
    assert api.del_rows(P.h, -2, num.ctypes.data_as(capi._IP)) == -1
    assert P.m == 6 and read_model(api, P) == before
    # num[0] is not read
    num = np.array([99, 6], dtype=np.int32)
    assert api.del_rows(P.h, 1, num.ctypes.data_as(capi._IP)) == 0 and read_model(api, P) == before[:5]
