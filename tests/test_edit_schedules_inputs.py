"""CPU, the oracle and the reference of tests/certify.py alone: the schedules of tests/edit_schedules.py have the properties that
tests/test_gpu_edit_schedules.py relies on.  The oracle solves each base; warm edits never change the basis, so the bookkeeping
walks every schedule from the oracle's optimal basis with no engine, and the GPU file carries the proof over by asserting that the
engine's optimal basis of each base is the oracle's.  A step whose precondition fails is an assertion of the planner
(edit_schedules.plan): a failure, never a skip."""
import itertools

import numpy as np
import pytest

from mvolps_amd.capi import OPT

from . import certify as cf
from . import edit_schedules as es
from . import lpgen

NAMES = list(es.SCHEDULES)


def kinds(name):
    return [s[0] for s in es.SCHEDULES[name][1]]


def adjacent(name):
    k = kinds(name)
    return list(zip(k, k[1:]))


def test_every_ordered_pair_occurs_as_two_adjacent_steps():
    seen = {p for name in NAMES for p in adjacent(name)}
    missing = [p for p in itertools.product(es.PAIR_KINDS, repeat=2) if p not in seen]
    assert len(list(itertools.product(es.PAIR_KINDS, repeat=2))) == 36 and not missing, missing


def test_the_other_kinds_stand_behind_a_column_edit_and_in_front_of_a_compaction():
    pairs = [p for name in NAMES for p in adjacent(name)]
    for kind in es.PLACED_KINDS:
        assert any(a in ("C+", "C-") and b == kind for a, b in pairs), kind  # the stride has just moved
        assert any(a == kind and b in ("R-", "C-") for a, b in pairs), kind  # a compaction follows
    go_on = {s[1] for name in NAMES for s in es.SCHEDULES[name][1] if s[0] == "K"}
    assert go_on == {"source", "clone"}


def test_bases_have_the_geometry():
    m, n, seed = es.BASES["A"]
    assert (m, n, seed) == (12, 30, 21) and es.ld_of(31) == 32 and es.ld_of(32) == 64
    m, n, seed = es.BASES["B"]
    assert 65 <= n + 1 <= 95 and es.ld_of(n) == 96 and es.ld_of(n - 1) == 64
    assert all(len(es.SCHEDULES[name][1]) <= 13 for name in NAMES)
    assert {b for b, _ in es.SCHEDULES.values()} == {"A", "B"}


@pytest.fixture(scope="module")
def bases(orc):
    """name -> (the certify model, the oracle's optimal basis, its pivot count)"""
    out = {}
    for name in es.BASES:
        A, b, c = es.base_lp(name)
        o = orc.create()
        o.load_dense(A, b, c)
        assert o.simplex() == 0 and o.status == OPT
        out[name] = (cf.Model.dense(A, b, c), o.basis(), o.it_cnt)
    return out


def sensitivity(st):
    ref = st.ref()
    return cf.RTOL * ref.growth * (1.0 + float(np.abs(ref.full_tableau()).max()))


def walk(bases, name):
    """Yields (spec, op, the reference before a step that claims to move column 0, the state afterwards, the walker)."""
    base, steps = es.SCHEDULES[name]
    M, basis, _ = bases[base]
    w = es.Walker(es.State(M.copy(), basis), name=name)
    for spec in steps:
        op, before, st = w.step(spec)
        yield spec, op, before, st, w


@pytest.mark.parametrize("name", NAMES)
def test_every_step_holds_in_the_reference(orc, bases, name):
    """The planner's preconditions (deleted rows basic, deleted columns non-basic or, in the give-up schedules, basic; Bb targets
    basic, Bn targets non-basic with a resting value that changes), the sensitivity of the certificate at every state the GPU file
    certifies, the moves of column 0, and an optimum for every final model."""
    base = es.SCHEDULES[name][0]
    assert bases[base][2] >= 8  # the forced refresh at the end looks after 8 pivots: the base's own solve has them
    last = None
    for spec, op, before, st, w in walk(bases, name):
        last = w
        states = [st] + [sq for _, _, sq in w.kept]
        for s in states:
            if s.valid:
                assert sensitivity(s) <= es.SENSITIVITY, (spec, sensitivity(s))
            assert s.M.m < 100 and s.M.n < 130
        if op["moves"] and before is not None:
            # far above ref.tol: a stale mirror cannot pass.  The basic variables keep their tableau rows through these steps
            after = st.ref()
            assert len(after.xB) == len(before.xB)
            assert float(np.abs(after.xB - before.xB).max()) > es.MOVE, spec
            assert abs(float(after.z - before.z)) > es.MOVE, spec
            assert es.MOVE > 100.0 * float(np.max(after.tol(after.x)))
    for M in [last.st.M] + [sq.M for _, _, sq in last.kept]:
        o = orc.create()
        o.load_general(M.A, M.rows, M.cols, M.c, c0=M.c0, direction=M.dir)
        assert o.simplex() == 0 and o.status == OPT


def test_the_schedules_meet_the_states_they_are_named_after(bases):
    grows, overflow, renumbered, gave_up = set(), set(), set(), set()
    for name in NAMES:
        base, steps = es.SCHEDULES[name]
        pending = {}  # basic variable -> outstanding bound edit, as the engine books them (appended rows leave theirs pending)
        grown = False
        for spec, op, before, st, w in walk(bases, name):
            kind = op["kind"]
            m = st.M.m
            if kind in ("R+", "R+1", "R+m"):
                k = len(op["rhs"])
                # the slab was sized for the base's rows at its solve and keeps ROW_SPARE rows behind row m (grow_rows)
                if kind == "R+" and st.valid and m + es.ROW_SPARE > es.BASES[base][0] + es.ROW_SLACK and k > es.ROW_SLACK - es.ROW_SPARE:
                    assert any(v[0] == "Bb" for v in pending.values()) and not grown, name
                    grows.add(base)
                    grown = True
                for t in range(k):
                    pending[m - k + 1 + t] = ("row",)
            elif kind == "Bb":
                for side, j, new in op["edits"]:
                    pending[j if side == "row" else m + j] = ("Bb",)
                if sum(1 for v in pending.values() if v[0] == "Bb") >= 9:
                    overflow.add(base)
            elif kind in ("R-", "R-m"):
                rows = op["rows"]
                hit = [i for i in rows if pending.get(i, ("",))[0] == "Bb"]
                lower = [i for i in rows if hit and i < max(hit)]
                moved = [k for k, v in pending.items() if v[0] == "Bb" and k not in rows and k > min(rows)]
                if hit and lower and moved:
                    renumbered.add(base)
                pending = {(k - m_shift(rows, k, m + len(rows))): v for k, v in pending.items() if k not in rows}
            elif kind in ("Cx", "Rx"):
                assert any(v[0] == "Bb" for v in pending.values()), name  # a Bb is outstanding when the tableau is given up
                gave_up.add(kind)
                pending = {}
            elif kind == "C-":
                cols = op["cols"]
                m_ = st.M.m
                pending = {(k if k <= m_ else k - sum(1 for j in cols if j < k - m_)): v for k, v in pending.items()}
    assert grows == {"A", "B"} and overflow == {"A", "B"} and renumbered == {"A", "B"} and gave_up == {"Cx", "Rx"}


def m_shift(rows, k, m_old):
    """How far variable k moves down when the model rows `rows` of m_old leave (mvx.h)."""
    return len(rows) if k > m_old else sum(1 for i in rows if i < k)


def test_give_up_schedules_go_on_with_model_edits():
    for name in ("give-up-col", "give-up-row"):
        k = kinds(name)
        at = next(i for i, x in enumerate(k) if x in ("Cx", "Rx"))
        assert at >= 2 and "Bb" in k[:at] and set(k[at + 1:]) == {"R+1", "C+", "C-", "Bn"}


def test_gmi_rows_feed_a_cut_after_their_second_rewrite(orc):
    """The GMI case of the GPU file: at the optimum of the model with row i rewritten, the row's auxiliary is non-basic and has a
    non-zero entry in the tableau row of a cut column -- the cut's back-substitution reads the row's new coefficients -- and the
    two rewrites differ from each other and from the original row."""
    A, b, c, U, M = es.gmi_model()
    found = []
    for i in range(1, M.m + 1):
        first, second = es.gmi_rewrites(A, i)
        assert not np.array_equal(first, second) and not np.array_equal(second, A[i - 1]) and not np.array_equal(first, A[i - 1])
        R = es.gmi_rewritten(M, i)
        o = lpgen.load_ilp(orc, R.A, b, c, U)
        assert o.simplex() == 0 and o.status == OPT
        if es.row_feeds_a_cut(cf.Ref(R, o.basis()), i):
            found.append(i)
    assert tuple(found) == es.GMI_ROWS and len(found) >= 3
