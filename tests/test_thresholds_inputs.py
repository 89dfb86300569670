"""CPU, oracle alone: every instance of test_gpu_thresholds.py has the property its GPU test relies on, so that no GPU
test there can pass without meeting the limit or threshold it is named after."""
import numpy as np
import pytest

from mvolps_amd import capi, synth

from . import thresholds as th


# ------------------------------------------------------------------------------------------------ A: GMI cuts
@pytest.mark.parametrize("case", th.GMI_CASES, ids=th.gmi_id)
def test_gmi_instances_cut_every_column_on_both_sides_of_a_pass(orc, case):
    """Root: a cut in both modes from every basic column; later rounds: the repaired twin may decline at most a quarter.
    Past 1024 columns every cut row has non-zeros in the first pass and after it (the carried right-hand side, `temp`
    and flag all matter); the back-substitution shapes leave a tail in the 64-row group and the 256-column block."""
    m, n = case[:2]
    Q = th.load_gmi_case(orc, case)
    assert Q.simplex() == 0 and Q.status == capi.OPT
    for rnd in range(th.GMI_ROUNDS):
        basic, cuts = th.oracle_round(orc, Q)
        assert len(basic) > th.GMI_CT + 1
        if rnd == 0 and case[:2] in ((24, 1100), (70, 2100)):
            assert len(basic) == (23 if m == 24 else 52)
        assert all(rc == 0 for rc, _, _ in cuts[0])
        skipped = sum(rc != 0 for rc, _, _ in cuts[1])
        assert skipped == 0 if rnd == 0 else 4 * skipped <= len(basic), (rnd, skipped, len(basic))
        if n > th.GMI_CH:
            rows, _ = th.basic_rows(Q, basic)
            assert np.all((rows[:, :th.GMI_CH] != 0).any(axis=1)) and np.all((rows[:, th.GMI_CH:] != 0).any(axis=1))
        assert th.append_cut(orc, Q, cuts[0][-1][1], cuts[0][-1][2]) == 0


def test_gmi_shapes_meet_every_edge():
    shapes = [c[:2] for c in th.GMI_CASES]
    ns = [n for _, n in shapes]
    assert th.GMI_CH - 1 in ns and th.GMI_CH + 1 in ns  # one position short of a pass, one position into the second
    assert any(th.GMI_CH + 1 < n < 2 * th.GMI_CH for n in ns) and any(n > 2 * th.GMI_CH for n in ns)  # two passes, three
    assert (65, 300) in shapes and (63, 257) in shapes  # 64-row groups: one row over, one short; 256-column blocks: one over
    assert th.GMI_TAIL_CASE in th.GMI_CASES and all(c in th.GMI_CASES and c[1] > th.GMI_CH for c in th.GMI_CERT_CASES)


def test_mixed_model_opens_the_second_pass_on_a_binary_position(orc):
    """Position 1025, the first of the second pass, holds a non-basic column that reads as GLP_BV, with a non-zero in
    every cut row: its coefficient is the `temp` the first pass left."""
    Q = th.load_mixed(orc)
    assert Q.simplex() == 0 and Q.status == capi.OPT
    head, nb, flag = Q.basis()
    k = int(nb[th.GMI_CH + 1]) - Q.m
    assert k >= 1 and orc.get_col_kind(Q.h, k) == capi.BV
    basic = [j for j in th.basic_columns(Q) if orc.get_col_kind(Q.h, j) == capi.IV]
    rows, _ = th.basic_rows(Q, basic)
    assert len(basic) > th.GMI_CT and np.all(rows[:, th.GMI_CH] != 0) and np.all((rows[:, :th.GMI_CH] != 0).any(axis=1))
    for mode in (0, 1):
        assert all(th.oracle_cut(orc, Q, j, mode)[0] == 0 for j in basic)


def test_free_model_has_the_three_classes_of_columns(orc):
    """Stopped by its pivot limit with free columns still non-basic: basic integer columns whose first free non-basic
    non-zero lies in the first pass, ones that meet theirs only after it, and ones that meet none."""
    Q = th.load_free(orc)
    assert Q.n > th.GMI_CH
    assert Q.simplex(it_lim=th.FREE_LIMIT) == capi.EITLIM
    kinds = th.free_model()[4]
    basic = [j for j in th.basic_columns(Q) if kinds[j - 1] == capi.IV]
    pos = th.free_positions(Q, basic)
    first_pass = [j for j, p in zip(basic, pos) if p and p[0] <= th.GMI_CH]
    later_only = [j for j, p in zip(basic, pos) if p and p[0] > th.GMI_CH]
    none = [j for j, p in zip(basic, pos) if not p]
    assert first_pass and later_only and none, (first_pass, later_only, none)
    assert any(p and p[0] <= th.GMI_CH < p[-1] for p in pos)  # a flag raised in the first pass and again later
    # the oracle declines exactly where such a position exists or the basic value is integral
    accepted = 0
    for j, p in zip(basic, pos):
        rc = th.oracle_cut(orc, Q, j, 1)[0]
        assert rc != 0 if p else True
        accepted += rc == 0
    assert accepted >= 1


# ------------------------------------------------------------------------------------------------ B: k_dsel
@pytest.mark.parametrize("case", th.DSEL_CASES, ids=th.dsel_id)
def test_dsel_children_pivot_past_one_chain(orc, case):
    """Every child takes more dual pivots than the one chain k_select itself can take at the start of a call
    (DCH_MAX), so k_dsel gets its turn wherever it applies."""
    m, n = case[:2]
    o, x, kids = th.dsel_children(orc, case)
    assert len(kids) == 4
    for key, k in kids.items():
        assert k.status == capi.OPT and k.it_cnt - o.it_cnt > th.DCH_MAX, (key, k.it_cnt - o.it_cnt)
    assert n <= th.DSEL_MAX and (m in (th.DSEL_MAX - 1, th.DSEL_MAX, th.DSEL_MAX + 1))


def test_growth_rounds_pivot_on_both_sides_of_the_row_limit(orc):
    m, n = th.DSEL_GROW[:2]
    Q = th.load_gmi_case(orc, th.DSEL_GROW)
    assert Q.simplex() == 0
    seen = []
    for rnd in range(th.DSEL_GROW_ROUNDS):
        it0 = Q.it_cnt
        assert th.grow_apply(orc, Q, th.grow_plan(orc, Q)) == 0 and Q.status == capi.OPT
        assert Q.m == m + rnd + 1
        pivots = Q.it_cnt - it0
        assert pivots >= 2, (rnd, pivots)
        if Q.m <= th.DSEL_MAX:
            assert pivots > th.DCH_MAX, (rnd, pivots)  # more than k_select's own first chain: k_dsel gets a turn
        seen.append(Q.m)
    assert th.DSEL_MAX in seen and th.DSEL_MAX + 1 in seen and n <= th.DSEL_MAX


# ------------------------------------------------------------------------------------------------ C: k_persist
@pytest.mark.parametrize("cus", [256, 304])
def test_persist_shapes_lie_on_their_side_of_each_threshold(cus):
    S = th.persist_shapes(cus)
    for name, (m, n, seed, taken) in S.items():
        assert (th.persist_plan(m, n, cus) is not None) == taken, (name, m, n)
    m, n = S["cpw3-short-last-strip"][:2]
    cpw, nw, _ = th.persist_plan(m, n, cus)
    assert cpw == 3 and n - cpw * (nw - 1) == 1
    m, n = S["cpw4-under-the-area-cap"][:2]
    assert th.persist_plan(m, n, cus)[0] == 4 and (m + 1) * (n + 1) > 0.98 * th.PERSIST_AREA_MAX
    # the LDS ceiling, not the area cap, is what declines one row more
    m, n = S["lds-ceiling"][:2]
    cpw, _, lds = th.persist_plan(m, n, cus)
    assert cpw == 1 and lds <= th.PERSIST_LDS_MAX < th.persist_lds_bytes(m + 1, cpw) and (m + 2) * (n + 1) <= th.PERSIST_AREA_MAX
    assert S["lds-ceiling+1"][:2] == (m + 1, n)
    # the area thresholds, met from both sides with everything else admissible
    m, n = S["area-min"][:2]
    assert (m + 1) * n < th.PERSIST_AREA_MIN <= (m + 1) * (n + 1) and S["area-min-1"][:2] == (m, n - 1)
    m, n = S["area-max"][:2]
    assert (m + 1) * (n + 1) <= th.PERSIST_AREA_MAX < (m + 1) * (n + 2) and S["area-max+1"][:2] == (m, n + 1)
    # more columns per workgroup than the four the workload sizes reach, up to the kernel's own limit and one past it
    m, n = S["widest-strips"][:2]
    cpw = th.persist_plan(m, n, cus)[0]
    assert cpw > 4 and (cpw == th.PERSIST_MAX_CPW or cus > 256) and (m + 1) * (n + 1) > 0.98 * th.PERSIST_AREA_MAX
    m, n = S["strips-too-wide"][:2]
    assert (n + cus - 1) // cus == th.PERSIST_MAX_CPW + 1 and th.PERSIST_AREA_MIN <= (m + 1) * (n + 1) <= th.PERSIST_AREA_MAX
    for name in ("area-min-1", "area-max+1"):
        m, n = S[name][:2]
        cpw = (n + cus - 1) // cus
        assert cpw <= th.PERSIST_MAX_CPW and (n + cpw - 1) // cpw <= 256 and th.persist_lds_bytes(m, cpw) <= th.PERSIST_LDS_MAX


def test_persist_shapes_on_256_units_are_the_documented_ones():
    S = th.persist_shapes(256)
    assert [S[k][:2] for k in S] == [(500, 601), (690, 1000), (3488, 199), (3489, 199), (127, 255), (127, 254), (699, 999), (699, 1000),
                                    (173, 4000), (100, 4097)]


# ------------------------------------------------------------------------------------------------ D: clones
@pytest.mark.parametrize("case", th.CLONE_CASES, ids=th.clone_id)
def test_clone_slabs_fall_in_their_copy_regime(orc, case):
    m, n, seed, lim1, lim2, regime = case
    g = th.slab_geometry(m, n)
    assert th.copy_regime(m, n) == regime
    path, ranges, looped = regime
    assert g["total"] > th.COPY_ONE_PASS and looped
    assert (g["total"] <= th.COPY_KERNEL_MAX) == (path == "kernel")
    assert (g["spare"] > th.COPY_WHOLE_SPARE) == (ranges == 2)
    if path == "memcpy":
        assert g["total"] < th.COPY_KERNEL_MAX + 2 * th.MIB  # just over the switch
    # the limits stop the source inside its primal phase with a basis, statuses and bounds that are not the initial ones
    o = th.load_clone_case(orc, case)
    assert o.simplex(it_lim=lim1) == capi.EITLIM and o.it_cnt == lim1
    head, nb, flag = o.basis()
    assert np.count_nonzero(head[1:] > m) >= 5 and np.count_nonzero(flag[1:] == capi.NU) >= 5
    assert o.simplex(it_lim=lim2) == capi.EITLIM and o.it_cnt == lim1 + lim2


# ------------------------------------------------------------------------------------------------ E: objective row
@pytest.mark.parametrize("m,n,seed", th.ROWCOMB_CASES)
def test_objective_rows_weigh_the_rows_at_the_chunk_edges(orc, m, n, seed):
    """The rows on both sides of every 64-row chunk edge, and the last row, hold basic structural columns with a cost:
    their weights in the recomputed objective row are non-zero, the partial sum of a short last chunk counts."""
    A, b, c = synth.dense_lp(m, n, seed)
    o = orc.create()
    o.load_dense(A, b, c)
    assert o.simplex() == 0
    head = o.basis()[0]
    edges = [i for i in (64, 65, 128, 129) if i <= m] + [m]
    for i in edges:
        assert head[i] > m and c[head[i] - m - 1] != 0.0, (m, i)
    assert (m + th.ROWCOMB_CHUNK - 1) // th.ROWCOMB_CHUNK == (1 if m <= 64 else 2 if m <= 128 else 3)
    it0 = o.it_cnt
    th.change_objective(o)
    assert o.simplex() == 0 and o.it_cnt > it0  # the changed objective moves the optimum: the re-solve pivots
