"""CPU, the oracle and certify.py alone: every (state, base) pair of tests/images.py builds, has the property its GPU test
(tests/test_gpu_images.py) relies on, and passes the whole check of images.roundtrip on the oracle's own pack code -- so a failure on
the GPU is the engine's, not the case's or the check's.  The states that need a call the oracle lacks (mvx_del_rows,
mvx_add_dense_cols, mvx_del_cols) are held to what can be said without it: the state they start from and the edit's targets."""
import collections

import numpy as np
import pytest

from mvolps_amd.capi import BS, DB, FEAS, FR, FX, MIN, NF, NOFEAS, NU, OPT, UNDEF

from . import images as im

ORACLE_CASES = [c for c in im.CASES if not im.STATES[c[0]][3]]


@pytest.fixture(scope="module")
def okit(orc):
    return im.Kit(orc)


def ld_of(n):
    return (n + 1 + im.LD_ALIGN - 1) // im.LD_ALIGN * im.LD_ALIGN


def test_bases_sit_on_the_edges_of_the_layout(orc):
    shapes = {b: im.BASES[b][1][:2] for b in im.ILP_BASES}
    assert shapes == {"ilp-12x31": (12, 31), "ilp-24x48": (24, 48), "ilp-8x64": (8, 64)}
    assert 31 + 1 == im.LD_ALIGN and 64 + 1 == 2 * im.LD_ALIGN + 1
    # the column edits of state 15 cross a stride in both directions
    assert (ld_of(31), ld_of(32)) == (32, 64) and (ld_of(64), ld_of(62)) == (96, 64)
    assert len(im.GEN_BASES) == 2
    rows, cols, dirs, flags = [], [], [], []
    for b in im.GEN_BASES:
        A, row_b, col_b, c, direction = im.general_instance(im.BASES[b][1])
        rows += [t for t, _, _ in row_b]
        cols += [t for t, _, _ in col_b]
        dirs.append(direction)
        _, P = im.solved(orc, b)
        im.certify_handle(P, im.DEFAULT_TOL, b)
        flags += P.basis()[2][1:].tolist()
    assert DB in rows and FR in cols and FX in cols and DB in cols and MIN in dirs
    assert NU in flags and NF in flags  # at the optima: a non-basic at its upper bound, a free one


def test_every_continuation_step_is_used_twice():
    used = collections.Counter(s for st in im.STATES.values() for s in st[4])
    for step in ("branch", "gmi", "gmi_rows", "del", "ranges", "many", "repack"):
        assert used[step] >= 2, (step, used)
    assert all(b in im.BASES for st in im.STATES.values() for b in st[1])
    for s in ("2-opt", "3-one-pending", "5-nofeas", "6-limit-primal", "6-limit-dual", "8-gmi-rows-solved"):
        assert set(im.GEN_BASES) <= set(im.STATES[s][1]), s
    assert all(set(im.ILP_BASES) <= set(im.STATES[s][1]) for s in im.STATES if s not in ("4-nine-pending", "15-cols-added", "15-cols-deleted"))


def has_tableau(P):
    try:
        P.basis()
        return True
    except RuntimeError:
        return False


@pytest.mark.parametrize("case", ORACLE_CASES, ids=im.case_id)
def test_case_has_its_property_and_passes_the_check_on_the_oracle(okit, orc, case):
    state, base = case
    s = im.build(orc, state, base, orc)
    try:
        root, P = s.root, s.handles[0]
        m0 = root.m
        _, parent = im.solved(orc, base)
        if s.tableau:
            for H in s.handles:
                im.certify_handle(H, s.tol, "%s/%s sender" % case)
        if state == "1-unsolved":
            assert not has_tableau(P) and P.status == UNDEF
            assert sum(im.col_bounds(P, j) != im.col_bounds(root, j) for j in range(1, P.n + 1)) == 2
        elif state == "2-opt":
            assert P.status == OPT
        elif state in ("3-one-pending", "4-nine-pending"):
            want = 1 if state == "3-one-pending" else im.MAX_EDITS + 1
            edited = [j for j in range(1, P.n + 1) if im.col_bounds(P, j) != im.col_bounds(root, j)]
            assert len(edited) == want and set(edited) <= set(im.basic_cols(P)) and P.status == UNDEF
            K = P.copy()
            assert K.simplex() == 0 and K.it_cnt > P.it_cnt  # the edits are not idle: the vertex was cut off
        elif state == "5-nofeas":
            assert P.status == NOFEAS and P.it_cnt > parent.it_cnt
        elif state in ("6-limit-primal", "6-limit-dual"):
            at = P.it_cnt
            assert at > (0 if state == "6-limit-primal" else parent.it_cnt)
            if state == "6-limit-primal":
                assert P.status == FEAS and 2 * at <= parent.it_cnt + 1  # phase 2, about half-way
            else:
                assert P.status != OPT
            K = P.copy()
            assert K.simplex() == 0 and K.status == OPT and K.it_cnt > at  # the limit cut the solve short
        elif state == "7-gmi-row":
            assert P.m == m0 + 1 and P.status == UNDEF and has_tableau(P)
        elif state == "8-gmi-rows-solved":
            assert P.m == m0 + 2 and P.status == OPT and P.it_cnt > parent.it_cnt
        elif state == "9-grown":
            assert P.m == m0 + im.GROW > m0 + im.ROW_SLACK - im.ROW_SPARE
            # what state 11 deletes: appended rows whose auxiliaries are basic, the first, a middle and the last one
            stat = P.row_stat()
            assert all(stat[i - 1] == BS for i in (m0 + 1, m0 + im.GROW // 2, P.m)) and m0 + 1 < m0 + im.GROW // 2 < P.m
        elif state == "10-rows-many":
            assert [H.m for H in s.handles] == [m0 + 2, m0 + 3]
        elif state == "12-batch":
            assert P.status == OPT and P.it_cnt == parent.it_cnt
        elif state == "13-tolerances":
            assert P.status == OPT and s.tol == im.GLPK_TOL != im.DEFAULT_TOL
        elif state == "14-refresh":
            stop = s.extra["stopped_at"]
            K = P.copy()
            before = orc.get_refresh_cnt(K.h)
            assert K.simplex() == 0 and K.status == OPT
            assert orc.get_refresh_cnt(K.h) > before  # the countdown ran out in the second leg ...
            assert 0 < K.it_cnt - stop <= stop  # ... which alone is too short for it
        else:
            raise AssertionError("no property written down for %s" % state)
    finally:
        if s.cleanup:
            s.cleanup()
    im.run_case(okit, state, base, orc)


def test_the_bases_of_the_column_edits_have_what_the_edits_need(orc):
    """State 15 on the oracle's side of the edit: solved bases, two non-basic columns to delete, a column to append that is
    an integer column with a finite box (so that the continuation's cuts see it)."""
    for b in ("ilp-12x31", "ilp-8x64"):
        _, P = im.solved(orc, b)
        assert P.n - len(im.basic_cols(P)) >= 2
    assert [c for c in im.CASES if im.STATES[c[0]][3]] == [("11-rows-deleted", b) for b in im.ILP_BASES] + \
        [("15-cols-added", "ilp-12x31"), ("15-cols-deleted", "ilp-8x64")]
