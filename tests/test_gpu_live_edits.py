"""GPU: one handle walked through a fixed schedule of live tableau edits (DESIGN.md "Live edits").

The edit tests of their own features start every edit from a freshly solved handle.  Here each edit meets what the one before
left behind -- a slab that has moved, bound edits that are still pending, mirrors that are only partly current -- and nothing
is solved in between: cut rows, a bound on an old basic row, a column append that changes the row stride, a row append that
grows the row capacity, the deletion of those rows, a column deletion that takes the stride back, and only then the solve.
A tests/certify.py model is edited alongside; after every edit the tableau is held to the independent reference of that model
and the handle's basis (certify_tableau <= 1.0, the bound of the edit tests), and the final state to cf.certify.

with_cut_rows of test_gpu_delcols.py solves behind its append, which this schedule must not: cut_rows below draws the rows the
same way and leaves the handle unsolved."""
import numpy as np
import pytest

from mvolps_amd import bnb
from mvolps_amd.capi import BS, DB, LO, OPT, UNDEF, UP

from . import certify as cf
from .test_addcols import draw_cols, same_bits
from .test_gpu_delcols import cols_at, dense, ld_of, reduced, structural_positions

pytestmark = pytest.mark.gpu

M0, N0 = 12, 30


def cut_rows(P, M, k, seed):
    """k MVX_LO rows the current vertex satisfies with a slack of 5, appended by one mvx_add_cut_rows call; no solve."""
    n = P.n
    rng = np.random.default_rng(seed)
    x = P.col_prim()
    vals = np.zeros((k, n + 1))
    vals[:, 1:] = -np.abs(np.round(rng.normal(size=(k, n)) * 2)) - 1.0
    rhs = vals[:, 1:] @ x - 5.0
    assert bnb.add_cut_rows(P, vals, rhs) == 0
    for t in range(k):
        M.add_row(vals[t, 1:], LO, float(rhs[t]), 0.0)


def check_state(P, M, m, n, what):
    """What every edit must leave: the counts, the stride, an unknown status, and a tableau the model's reference agrees with."""
    assert (P.m, P.n) == (m, n) == (M.m, M.n), what
    assert P.api.get_tableau_ld(P.h) == ld_of(n), what
    assert P.status == UNDEF, what
    assert cf.certify_tableau(cf.Ref(M, P.basis()), P.tableau(), what) <= 1.0


def front_rows_keep_their_values(P, before, what):
    """row_prim of the rows in front of an append keeps its bits without a solve: the basic ones first, then all of them.  This
    pins the values only: a handle that exported its solution anew would return the same bits, so the test does not tell
    whether the mirrors were read as they stood."""
    m0 = len(before)
    stat = P.row_stat()
    basic = [i for i in range(1, m0 + 1) if stat[i - 1] == BS]
    assert basic, what
    now = [P.api.get_row_prim(P.h, i) for i in basic]
    assert same_bits(now, [before[i - 1] for i in basic]), what
    assert same_bits(P.row_prim()[:m0], before), what


def test_one_handle_through_a_schedule_of_edits(gpu):
    # 1. solve: 31 of the 32 columns of the stride are in use
    P, M = dense(gpu, M0, N0, 21)
    assert ld_of(N0) == 32 and P.api.get_tableau_ld(P.h) == 32
    m, n = M0, N0

    # 2. two cut rows the vertex satisfies
    before = P.row_prim()
    cut_rows(P, M, 2, seed=7)
    m += 2
    check_state(P, M, m, n, "2: cut rows")
    front_rows_keep_their_values(P, before, "2: cut rows")

    # 3. a bound on an old basic row, below its activity: a pending edit keyed by the row
    stat, act = P.row_stat(), P.row_prim()
    i_edit = next(i for i in range(1, M0 + 1) if stat[i - 1] == BS and act[i - 1] > 1.0)
    ub_edit = 0.75 * float(act[i_edit - 1])
    P.api.set_row_bnds(P.h, i_edit, UP, 0.0, ub_edit)
    M.set_row_bnds(i_edit, UP, 0.0, ub_edit)
    check_state(P, M, m, n, "3: row bound")

    # 4. three bounded columns, two of them resting off zero: n = 33, the stride goes from 32 to 64 with the edit outstanding
    types = [(DB, -1.0, 1.0), (DB, 0.0, 2.0), (DB, -2.0, 0.5)]
    cols, obj = draw_cols(np.random.default_rng(4), 3, m)
    assert P.add_dense_cols(cols, obj, [t for t, _, _ in types], [l for _, l, _ in types], [u for _, _, u in types]) == 0
    for t, (ty, l, u) in enumerate(types):
        M.add_col(cols[t, 1:], ty, l, u, cost=obj[t])
    n += 3
    assert ld_of(n) == 64
    check_state(P, M, m, n, "4: column append")

    # 5. forty slack rows in one call: more than the spare rows, the row capacity grows
    before = P.row_prim()
    m_front = m
    cut_rows(P, M, 40, seed=8)
    m += 40
    check_state(P, M, m, n, "5: forty rows")
    front_rows_keep_their_values(P, before, "5: forty rows")

    # 6. those forty leave again: their auxiliaries are basic, nothing has been solved
    gone_rows = list(range(m_front + 1, m + 1))
    assert all(s == BS for s in P.row_stat()[m_front:])
    assert P.del_rows(gone_rows) == 0
    M.A = np.delete(M.A, [i - 1 for i in gone_rows], axis=0)
    del M.rows[m_front:]
    m = m_front
    check_state(P, M, m, n, "6: row deletion")

    # 7. three non-basic structurals leave, two of them appended columns off zero: the stride goes back to 32
    s = structural_positions(P)
    gone_cols = cols_at(P, [s[0], N0 + 1, N0 + 2])
    assert sorted(gone_cols)[1:] == [N0 + 1, N0 + 2] and gone_cols[0] <= N0
    assert P.del_cols(gone_cols) == 0
    M = reduced(M, gone_cols)
    n -= 3
    assert ld_of(n) == 32
    check_state(P, M, m, n, "7: column deletion")

    # 8. the solve: the bound of step 3 is applied, the state certifies against the model that was edited alongside
    assert P.simplex() == 0 and P.status == OPT
    assert P.api.get_row_prim(P.h, i_edit) <= ub_edit + 1e-9
    assert M.rows[i_edit - 1] == (UP, 0.0, ub_edit)
    cf.certify(M, P, status=OPT, what="8: solved")
