"""CPU: column deletion (DESIGN.md "Column deletion (del_cols)") without a device.

The model layer of mvx_del_cols runs on handles that have no tableau, so it is checked here against a second handle that is
built from scratch without the deleted columns, accessor by accessor; a clone taken before keeps what it has; appending k
columns and deleting exactly those gives the model back; and every refusal returns -1 with every accessor unchanged."""
import ctypes as C

import numpy as np
import pytest

import mvolps_amd
from mvolps_amd import capi
from mvolps_amd.capi import CV, IV

from . import general_at_size as gs
from .test_addcols import NEW_COLS, columns_of, draw_cols, general_handle, rows_of

IP = C.POINTER(C.c_int)


def names_of(P):
    return [P.api.get_col_name(P.h, j) for j in range(1, P.n + 1)]


def everything(P):
    api = P.api
    return (P.m, P.n, rows_of(P), columns_of(P), api.get_num_int(P.h), names_of(P), api.get_obj_dir(P.h), api.get_obj_coef(P.h, 0),
            api.get_status(P.h), [(api.get_row_type(P.h, i), api.get_row_lb(P.h, i), api.get_row_ub(P.h, i)) for i in range(1, P.m + 1)])


def reduced_handle(api, gone, seed=5, m=6, n=9):
    """general_handle's model built from scratch without the columns `gone` (1-based)."""
    inst = gs.general_lp(m, n, seed)
    keep = [j for j in range(n) if j + 1 not in gone]
    kinds = [IV if j % 3 == 0 else CV for j in range(n)]
    P = api.create()
    P.load_general(inst["A"][:, keep], inst["row_b"], [inst["col_b"][j] for j in keep], inst["c"][keep], kinds=[kinds[j] for j in keep],
                   direction=inst["direction"])
    return P, keep


@pytest.mark.parametrize("gone", [[1], [9], [4, 5], [8, 6, 3, 1]], ids=["first", "last", "adjacent", "scattered descending"])
def test_model_edit_equals_a_handle_built_without_the_columns(gone):
    api = mvolps_amd.api()
    P, inst = general_handle(api)
    m, n = P.m, P.n
    api.set_col_name(P.h, 2, b"second")
    api.set_col_name(P.h, 7, b"seventh")
    api.set_obj_coef(P.h, 0, 2.5)
    clone = P.copy()
    before = everything(P)
    assert P.del_cols(gone) == 0
    Q, keep = reduced_handle(api, gone)
    for j in (2, 7):
        if j in gone:
            continue
        api.set_col_name(Q.h, keep.index(j - 1) + 1, {2: b"second", 7: b"seventh"}[j])
    api.set_obj_coef(Q.h, 0, 2.5)
    assert (P.m, P.n) == (Q.m, Q.n) == (m, n - len(gone))
    assert rows_of(P) == rows_of(Q)
    assert columns_of(P) == columns_of(Q)
    assert api.get_num_int(P.h) == api.get_num_int(Q.h) == sum(1 for j in keep if j % 3 == 0)
    assert names_of(P) == names_of(Q)
    assert api.get_obj_dir(P.h) == api.get_obj_dir(Q.h) == inst["direction"]
    assert api.get_obj_coef(P.h, 0) == 2.5
    assert api.get_status(P.h) == capi.UNDEF
    assert everything(P)[9] == before[9]  # the rows' bounds stay
    # the clone taken before keeps its n, its rows and its names
    assert everything(clone) == before


def test_append_then_delete_gives_the_model_back():
    api = mvolps_amd.api()
    P, _ = general_handle(api, seed=7)
    m, n = P.m, P.n
    api.set_col_name(P.h, 3, b"third")
    before = everything(P)
    k = len(NEW_COLS)
    cols, obj = draw_cols(np.random.default_rng(3), k, m)
    assert P.add_dense_cols(cols, obj, [t for t, _, _, _ in NEW_COLS], [l for _, l, _, _ in NEW_COLS], [u for _, _, u, _ in NEW_COLS],
                            [kd for _, _, _, kd in NEW_COLS]) == 0
    assert P.n == n + k and everything(P) != before
    assert P.del_cols(list(range(n + k, n, -1))) == 0  # exactly those, in descending order
    assert everything(P) == before


def test_every_refusal_leaves_the_model_alone():
    api = mvolps_amd.api()
    P, _ = general_handle(api, seed=9)
    n = P.n
    api.set_col_name(P.h, 1, b"first")
    before = everything(P)

    def call(ncs, nums, null=False):
        num = np.array([0] + list(nums), dtype=np.int32)
        return api.del_cols(P.h, ncs, None if null else num.ctypes.data_as(IP))

    refusals = [
        dict(ncs=1, nums=[1], null=True), dict(ncs=0, nums=[1]), dict(ncs=-2, nums=[1]), dict(ncs=1, nums=[0]), dict(ncs=1, nums=[n + 1]),
        dict(ncs=2, nums=[3, n + 1]), dict(ncs=2, nums=[4, 4]), dict(ncs=3, nums=[2, 5, 2]), dict(ncs=n, nums=list(range(1, n + 1))),
    ]
    for r in refusals:
        assert call(**r) == -1, r
        assert everything(P) == before, r
    assert api.del_cols(None, 1, np.array([0, 1], dtype=np.int32).ctypes.data_as(IP)) == -1
    # num[0] is not read, and all but one column may leave
    num = np.array([-77] + list(range(2, n + 1)), dtype=np.int32)
    assert api.del_cols(P.h, n - 1, num.ctypes.data_as(IP)) == 0 and P.n == 1
    assert names_of(P) == [b"first"]
    assert call(1, [1]) == -1 and P.n == 1  # the last column cannot leave


def test_span_is_exported():
    assert mvolps_amd.api().del_cols_span() % 64 == 0 and mvolps_amd.api().del_cols_span() >= 64
