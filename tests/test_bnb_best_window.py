"""CPU: the speculative best-bound window (mvx_bnb_params.best_window) of the C++ driver, run over the ORACLE's
LP-engine table, against the oracle's own node-at-a-time restatement of bs.cpp in best-bound order
(node_strat = 1).  Each round solves, classifies and branches the top W open nodes together and keeps the prefix
the serial loop would also have popped: the tree, oids, events, pivot counts and incumbent must be the serial
ones, bit for bit, whatever W."""
import pytest

from mvolps_amd import bnb, synth

from . import lpgen
from .test_bnb_host import oracle_table, same_result

WINDOWS = [2, 8, 64]


def run_both(orc, load, best_window, **kw):
    from oracle import oracle

    ref = oracle.branch_and_bound(load(), node_strat=1, **kw)
    got = bnb.branch_and_bound(load(), node_strat=1, table=oracle_table(orc), best_window=best_window, **kw)
    same_result(got, ref)
    assert 0 < got["rounds"] <= got["count"] + 1
    assert got["rounds"] <= got["speculated"] <= best_window * got["rounds"]
    return got, ref


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("quirks", [0, 1])
@pytest.mark.parametrize("case", [(16, 32, 5, 2), (40, 80, 7, 2)], ids=lambda c: "%dx%d" % (c[0], c[1]))
def test_best_window_matches_serial_best_bound(orc, case, quirks, W):
    m, n, seed, U = case
    A, b, c, U = synth.dense_ilp(m, n, seed, U)
    got, _ = run_both(orc, lambda: lpgen.load_ilp(orc, A, b, c, U), W, quirks=quirks, max_nodes=4000)
    assert got["count"] > 20


def test_best_window_takes_several_nodes_per_round(orc):
    """The point of the window: on the repaired 16x32 tree W = 64 commits about ten nodes a round."""
    A, b, c, U = synth.dense_ilp(16, 32, 5, 2)
    got, _ = run_both(orc, lambda: lpgen.load_ilp(orc, A, b, c, U), 64, quirks=0)
    assert not got["hit_limit"]
    assert got["rounds"] * 4 < got["count"], (got["rounds"], got["count"])


@pytest.mark.parametrize("W", WINDOWS)
def test_best_window_minimisation_repaired(orc, W):
    """Direction-aware keys (reference_quirks = 0 on a minimisation problem): the smallest bound is popped first."""
    A, c = lpgen.setcover_ilp(40, 60, 3)
    got, _ = run_both(orc, lambda: lpgen.load_setcover(orc, A, c), W, quirks=0, max_nodes=5000)
    assert abs(got["best_lower"] - 22.0) < 1e-9 and got["count"] > 3


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("mode", ["quirks-lazy", "quirks-all", "repaired", "repaired-select"])
def test_best_window_with_gmi_cuts(orc, mode, W):
    """cut_strat = 1: cut rows go onto clones of speculated nodes; the bug-compatible pool that persists from node to node
    (bs.cpp:73, cut.cpp:16-21) is rolled back to where each round's replay stopped."""
    kw = {
        "quirks-lazy": dict(quirks=1, lazy_pool=1),
        "quirks-all": dict(quirks=1, lazy_pool=0),
        "repaired": dict(quirks=0),
        "repaired-select": dict(quirks=0, cut_select=1, cut_chance=0.5),
    }[mode]
    A, b, c, U = synth.dense_ilp(16, 32, 5, 2)
    from oracle import oracle

    ref = oracle.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), node_strat=1, cut_strat=1, max_nodes=1500,
                                  quirks=kw["quirks"], cut_select=kw.get("cut_select", 0), cut_chance=kw.get("cut_chance", 1.0))
    got = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), node_strat=1, cut_strat=1, max_nodes=1500, table=oracle_table(orc),
                               best_window=W, **kw)
    same_result(got, ref)
    assert got["count"] > 20 and got["rounds"] > 0


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("var_strat", [1, 2])
def test_best_window_var_strategies(orc, var_strat, W):
    A, b, c, U = synth.dense_ilp(16, 32, 5, 2)
    got, _ = run_both(orc, lambda: lpgen.load_ilp(orc, A, b, c, U), W, quirks=1, var_strat=var_strat, max_nodes=3000)
    assert got["count"] > 20


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("max_nodes", [1, 7, 50])
def test_best_window_stops_at_the_serial_node(orc, max_nodes, W):
    A, b, c, U = synth.dense_ilp(40, 80, 7, 2)
    got, _ = run_both(orc, lambda: lpgen.load_ilp(orc, A, b, c, U), W, quirks=0, max_nodes=max_nodes)
    assert got["hit_limit"] == 1 and got["count"] == max_nodes


def test_default_is_node_at_a_time(orc):
    """best_window defaults to 0: best-bound runs take the node-at-a-time driver, which reports no rounds."""
    A, b, c, U = synth.dense_ilp(16, 32, 5, 2)
    pr = bnb.make_params(node_strat=1)
    assert pr.best_window == 0
    for W in (None, 0, 1):
        r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), node_strat=1, quirks=0, max_nodes=200, table=oracle_table(orc),
                                 best_window=W)
        assert r["rounds"] == 0 and r["speculated"] == 0
    # FIFO order ignores best_window
    r = bnb.branch_and_bound(lpgen.load_ilp(orc, A, b, c, U), node_strat=0, quirks=0, max_nodes=200, table=oracle_table(orc), best_window=8)
    assert r["rounds"] == 0
