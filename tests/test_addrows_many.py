"""CPU: mvx_add_cut_rows_many (DESIGN.md "Row append across handles (add_cut_rows_many)") as far as it is decided before the
device is needed.  The symbol is exported, declared and bound; every refusal returns -1 and leaves every accessor of every
handle as it was, whichever handle of the call it concerns; a call that gives no handle a row returns 0 and changes nothing.
The handles are never solved, so none of them has a tableau: one that is given rows is itself a refusal, as it is for
mvx_add_cut_rows."""
import os
import re

import numpy as np

import mvolps_amd
from mvolps_amd import bnb, capi

from .test_bnb_purge import model, read_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = bnb.C
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


def accessors(api, P):
    cols = [(api.get_col_type(P.h, j), api.get_col_lb(P.h, j), api.get_col_ub(P.h, j), api.get_obj_coef(P.h, j)) for j in range(1, P.n + 1)]
    stats = [api.get_row_stat(P.h, i) for i in range(1, P.m + 1)] + [api.get_col_stat(P.h, j) for j in range(1, P.n + 1)]
    return (P.m, P.n, api.get_num_rows(P.h), api.get_status(P.h), read_model(api, P), cols, stats)


def test_symbol_is_exported_declared_and_bound():
    L = bnb.lib()
    assert L.mvx_add_cut_rows_many.restype is C.c_int
    assert L.mvx_add_cut_rows_many.argtypes == [C.c_void_p, C.c_int, IP, DP, DP]
    assert "add_cut_rows_many" in mvolps_amd._EXTRA and mvolps_amd.api().add_cut_rows_many is not None
    hdr = open(os.path.join(ROOT, "include", "mvx.h")).read()
    decl = r"int\s+mvx_add_cut_rows_many\(mvx_prob \*const \*Ps, int count, const int \*off,\s*const double \*vals, const double \*rhs\);"
    assert re.search(decl, hdr)
    # the B&B table, parameters and result are what they were: the drivers do not adopt the entry here
    assert "add_cut_rows_many" not in bnb._OPTIONAL and not hasattr(bnb.LpApiTable, "add_cut_rows_many")


def test_refusals_change_nothing():
    api = mvolps_amd.api()
    base, _A, _rows = model(api)
    hs = [base.copy() for _ in range(3)]
    other, _A2, _r2 = model(api)
    api.add_cols(other.h, 1)  # another column count
    everyone = hs + [other, base]
    before = [accessors(api, h) for h in everyone]
    n1 = base.n + 1

    def untouched():
        return [accessors(api, h) for h in everyone] == before

    L = bnb.lib()
    arr = (C.c_void_p * 3)(*[h.h for h in hs])
    off = np.array([0, 1, 3, 4], dtype=np.int32)
    vals = np.arange(4.0 * n1).reshape(4, n1) + 1.0
    rhs = np.array([-1.0, -2.0, -3.0, -4.0])
    op, vp, rp = off.ctypes.data_as(IP), vals.ctypes.data_as(DP), rhs.ctypes.data_as(DP)
    # nulls and counts
    assert L.mvx_add_cut_rows_many(None, 3, op, vp, rp) == -1 and L.mvx_add_cut_rows_many(arr, 3, None, vp, rp) == -1
    assert L.mvx_add_cut_rows_many(arr, 3, op, None, rp) == -1 and L.mvx_add_cut_rows_many(arr, 3, op, vp, None) == -1
    assert L.mvx_add_cut_rows_many(arr, 0, op, vp, rp) == -1 and L.mvx_add_cut_rows_many(arr, -1, op, vp, rp) == -1
    null_in = (C.c_void_p * 3)(hs[0].h, None, hs[2].h)
    assert L.mvx_add_cut_rows_many(null_in, 3, op, vp, rp) == -1 and untouched()
    # the lists
    for bad in ([0, 2, 1, 4], [0, 0, 3, 2], [1, 2, 3, 4], [0, -1, 3, 4]):  # descending, or not from 0
        bo = np.array(bad, dtype=np.int32)
        assert L.mvx_add_cut_rows_many(arr, 3, bo.ctypes.data_as(IP), vp, rp) == -1 and untouched(), bad
    zero = [np.zeros((0, n1))] * 3, [np.zeros(0)] * 3
    assert bnb.add_cut_rows_many([hs[0], hs[1], hs[0]], *zero) == -1 and untouched()  # a handle listed twice, even without rows
    assert bnb.add_cut_rows_many([hs[0], other], zero[0][:2], zero[1][:2]) == -1 and untouched()  # column counts differ
    # a NaN that would be read, in the last handle's rows: checked before the first handle is edited
    for where in ((3, 2), (1, n1 - 1)):
        nv = vals.copy()
        nv[where] = np.nan
        assert L.mvx_add_cut_rows_many(arr, 3, op, nv.ctypes.data_as(DP), rp) == -1 and untouched(), where
    nr = rhs.copy()
    nr[3] = np.nan
    assert L.mvx_add_cut_rows_many(arr, 3, op, vp, nr.ctypes.data_as(DP)) == -1 and untouched()
    # a handle without a tableau that is given rows (these rows hold no NaN; a NaN in entry 0 of a row is not read, so it is
    # not what refuses this call either)
    assert L.mvx_add_cut_rows_many(arr, 3, op, vp, rp) == -1 and untouched()
    nv = vals.copy()
    nv[:, 0] = np.nan
    assert L.mvx_add_cut_rows_many(arr, 3, op, nv.ctypes.data_as(DP), rp) == -1 and untouched()
    assert bnb.add_cut_rows_many(hs, [[], vals[:1], []], [[], rhs[:1], []]) == -1 and untouched()
    # the front end refuses lists that do not fit before the library sees them
    assert bnb.add_cut_rows_many(hs, [vals[:1]] * 2, [rhs[:1]] * 2) == -1
    assert bnb.add_cut_rows_many(hs, [vals[:2]] * 3, [rhs[:1]] * 3) == -1 and untouched()


def test_a_call_without_rows_returns_0_and_changes_nothing():
    api = mvolps_amd.api()
    base, _A, _rows = model(api)
    hs = [base.copy() for _ in range(3)]
    before = [accessors(api, h) for h in hs]
    n1 = base.n + 1
    assert bnb.add_cut_rows_many(hs, [np.zeros((0, n1))] * 3, [np.zeros(0)] * 3) == 0
    assert bnb.add_cut_rows_many(hs[:1], [[]], [[]]) == 0
    L = bnb.lib()
    arr = (C.c_void_p * 3)(*[h.h for h in hs])
    off = np.zeros(4, dtype=np.int32)
    nan = np.full(n1, np.nan)  # nothing of vals / rhs is read
    assert L.mvx_add_cut_rows_many(arr, 3, off.ctypes.data_as(IP), nan.ctypes.data_as(DP), nan.ctypes.data_as(DP)) == 0
    assert [accessors(api, h) for h in hs] == before
    assert all(api.get_status(h.h) == capi.UNDEF for h in hs)
