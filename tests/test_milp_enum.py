"""CPU: the enumeration reference (tests/milp_enum.py) against certify.integer_points on the three enumerated GMI ILPs of
test_gpu_certify.py and against hand-written two-variable models whose answers are known."""
import numpy as np

from mvolps_amd import synth

from . import certify as cf
from . import milp_enum as me

INF = np.inf


def test_matches_integer_points_on_the_gmi_ilps():
    for (m, n, seed, U) in [(6, 10, 3, 2), (5, 12, 8, 2), (8, 11, 21, 2)]:
        A, b, c, U = synth.dense_ilp(m, n, seed, U, 0.4)
        pts = cf.integer_points(cf.Model.ilp(A, b, c, U))
        assert len(pts) > 0
        want = float((pts @ np.asarray(c, dtype=float)).max())
        args = (A, np.full(m, -INF), np.asarray(b, dtype=float), np.zeros(n), np.full(n, float(U)), c, 0.0, np.ones(n, bool), True)
        for ranges in (None, [(0, U)] * n):  # the box from the relaxation, and the whole column box without any LP
            e = me.enumerate_milp(*args, ranges=ranges)
            assert e["status"] == "optimal" and e["optimum"] == want, (m, n, e["optimum"], want)
            assert any(np.array_equal(np.array(e["x"]), p) for p in pts)
            assert e["points"] <= (U + 1) ** n
        assert me.enumerate_milp(*args, ranges=[(0, U)] * n)["points"] == (U + 1) ** n


def two(rows, cols, c, c0, isint, maximize, **kw):
    A = np.array([r[0] for r in rows], dtype=float)
    return me.enumerate_milp(A, [r[1] for r in rows], [r[2] for r in rows], [b[0] for b in cols], [b[1] for b in cols], c, c0, isint,
                             maximize, **kw)


def test_integer_infeasible_with_a_feasible_relaxation():
    e = two([([2, 2], 3, 3)], [(0, 3), (0, 3)], [1, 1], 0.0, [True, True], True)   # 2 x1 + 2 x2 = 3
    assert e["relaxation"] == "optimal" and e["status"] == "infeasible" and e["points"] > 0 and e["x"] is None


def test_lp_infeasible():
    e = two([([1, 1], 5, INF), ([1, 1], -INF, 4)], [(0, 9), (0, 9)], [1, 0], 0.0, [True, False], False)
    assert e["relaxation"] == "infeasible" and e["status"] == "infeasible" and e["points"] == 0


def test_optimum_on_the_inward_rounding_of_fractional_bounds():
    """x1 in [0.5, 2.5], x2 in [-1.5, 1.5], both integer, x1 + x2 <= 3.5: the relaxation's optimum 3.5 sits on the bounds;
    the integer optimum is x = (2, 1), on floor(2.5) and floor(1.5).  Minimising, it is (1, -1): ceil(0.5), ceil(-1.5)."""
    rows, cols = [([1, 1], -INF, 3.5)], [(0.5, 2.5), (-1.5, 1.5)]
    e = two(rows, cols, [1, 1], 0.0, [True, True], True)
    assert (e["status"], e["optimum"], e["x"], e["points"]) == ("optimal", 3.0, [2.0, 1.0], 6)
    e = two(rows, cols, [1, 1], 0.0, [True, True], False)
    assert (e["status"], e["optimum"], e["x"]) == ("optimal", 0.0, [1.0, -1.0])
    e = two(rows, [(0.5, 0.75), (0, 1)], [1, 1], 0.0, [True, True], True)  # no integer in [0.5, 0.75]
    assert e["status"] == "infeasible" and e["points"] == 0


def test_mixed_minimisation_maximisation_and_the_constant():
    """x integer in [0, 10], y continuous in [0, 1.5], x + y <= 3.7.  max 2 x + y + 4 = 10.7 at (3, 0.7);
    min -x - 3 y - 1 = -7.5 at (2, 1.5) (x = 3 leaves y 0.7: -6.1)."""
    rows, cols = [([1, 1], -INF, 3.7)], [(0, 10), (0, 1.5)]
    e = two(rows, cols, [2, 1], 4.0, [True, False], True)
    assert e["status"] == "optimal" and abs(e["optimum"] - 10.7) < 1e-9 and np.allclose(e["x"], [3, 0.7], atol=1e-9)
    e = two(rows, cols, [-1, -3], -1.0, [True, False], False)
    assert e["status"] == "optimal" and abs(e["optimum"] + 7.5) < 1e-9 and np.allclose(e["x"], [2, 1.5], atol=1e-9)
    assert e["points"] == 4


def test_ties_equalities_and_ranged_rows():
    """1 <= x1 - x2 <= 2 and x1 + x2 = 5 over 0..5: (3, 2) only."""
    e = two([([1, -1], 1, 2), ([1, 1], 5, 5)], [(0, 5), (0, 5)], [1, 3], 2.0, [True, True], False)
    assert (e["status"], e["optimum"], e["x"]) == ("optimal", 11.0, [3.0, 2.0])


def test_what_cannot_be_enumerated_is_dropped_with_its_reason():
    e = two([([1, -1], -INF, 5)], [(0, INF), (0, INF)], [1, 1], 0.0, [True, True], True)
    assert (e["status"], e["reason"], e["relaxation"]) == ("dropped", me.UNBOUNDED, "unbounded")
    e = two([([0, 1], -INF, 1)], [(0, INF), (0, 5)], [0, 1], 0.0, [True, True], True)  # x1 costs nothing and has no end
    assert (e["status"], e["reason"]) == ("dropped", me.INF_RANGE)
    e = two([([1, 1], -INF, 150)], [(0, 100), (0, 100)], [1, 1], 0.0, [True, True], True, pure_limit=1000)
    assert (e["status"], e["reason"]) == ("dropped", me.BOX) and e["points"] == 101 * 101
    e = two([([1, 1], -INF, 150)], [(0, 100), (0, 100)], [1, 1], 0.0, [True, False], True, mixed_limit=100)
    assert (e["status"], e["reason"]) == ("dropped", me.BOX)
