"""GPU: whole B&B trees of the gfx950 engine on the general mixed-integer family (tests/golden/general_milp.json, pinned by
enumeration), on the default path and on the forced streamed paths; the engine's state on tree nodes and on both children of
each certified against the model (tests/certify.py); and the batched per-node entries against their host twins on windows of
tree nodes with continuous, free, upper-resting and fixed columns.

Status: written against the CPU results (the same loops pass over the oracle's table, and the certificate loop passes on the
oracle's handles); not yet run on a device, so its wall time, the device's tree sizes and whether the forced streamed paths
agree with the oracle on these models are unmeasured.  If it takes longer than the longest existing GPU file, thin the
instance loops by index (every second instance), never by outcome."""
import collections
import ctypes as C

import numpy as np
import pytest

from mvolps_amd import bnb, capi
from mvolps_amd.capi import NOFEAS, OPT

from . import certify as cf
from . import lpgen
from .test_bnb_branching import basic_fractional
from .test_bnb_general import INSTANCES, OPTIONS, check_pin, failures, instance, node_box, run, sampled
from .test_bnb_host import same_result
from .test_bnb_rcfix import same_counters
from .test_gpu_branching import device_vs_host as penalties_device_vs_host
from .test_gpu_certify import device_cuts_many, paths  # noqa: F401  (paths: the fixture that restores the engine's settings)
from .test_gpu_heuristic import device_vs_host as round_device_vs_host
from .test_gpu_rcfix import device_vs_twin as rc_device_vs_twin

pytestmark = pytest.mark.gpu

GPU_OPTIONS = ["serial", "window64", "best_window8", "heur2_rcfix_window64", "cuts_heur2_rcfix_window64", "var3", "var4"]
COUNTS = collections.Counter()  # (what, sub-family, status) -> certified states; (path, option set) -> trees compared


def tree_check(gpu, orc, tab, rec, name):
    inst = instance(rec)
    r = run(gpu, rec, inst, **OPTIONS[name])
    check_pin(rec, inst, r)
    ref = run(orc, rec, inst, table=tab, **OPTIONS[name])
    same_result(r, ref)
    same_counters(r, ref)
    assert (r["sb_lps"], r["sb_pivots"]) == (ref["sb_lps"], ref["sb_pivots"])


def tree_loop(gpu, orc, recs, name, path):
    tab = bnb.table_from(orc)

    def one(rec):
        tree_check(gpu, orc, tab, rec, name)
        COUNTS[("trees", path, name)] += 1

    bad = failures(recs, one)
    assert not bad, "%s, %s: %d of %d fail:\n%s" % (path, name, len(bad), len(recs), "\n".join(bad))


@pytest.mark.parametrize("name", GPU_OPTIONS)
def test_trees_close_on_the_enumerated_optimum_and_match_the_oracle_table(gpu, orc, name):
    tree_loop(gpu, orc, INSTANCES, name, "default")


@pytest.mark.parametrize("cluster", [1, 0], ids=["cluster", "two-launch"])
@pytest.mark.parametrize("name", GPU_OPTIONS)
def test_trees_on_the_forced_streamed_paths(paths, orc, name, cluster):
    """These models fit the resident-tableau kernel; with it switched off the streamed update, k_chain (cluster) or the
    two-launch path, and k_dsel's dual chains meet FR / NU / FX variables and ranged rows below a branching."""
    paths.set_persist(0)
    paths.set_cluster(cluster)
    paths.set_dual_chain(8)
    tree_loop(paths, orc, INSTANCES[::4], name, "cluster" if cluster else "two-launch")


# ------------------------------------------------------------------------------------------------ node LPs, certified


def node_model(api, inst, P):
    """cf.Model from the test's arrays with the column bounds of the node copied in from the handle."""
    M = cf.Model(inst["A"], inst["row_b"], inst["col_b"], inst["c"], c0=inst["c0"], direction=inst["direction"], kinds=inst["kinds"])
    for j in range(1, P.n + 1):
        M.set_col_bnds(j, api.get_col_type(P.h, j), api.get_col_lb(P.h, j), api.get_col_ub(P.h, j))
    return M


def rounded_root(api, inst):
    root = lpgen.load_milp(api, inst)
    return root, bnb.integral_bounds(root)


def cert(api, inst, P, what, family, status=None):
    cf.certify(node_model(api, inst, P), P, status=status, exact=True, what=what)
    COUNTS[(what, family, P.status if status is None else status)] += 1


def test_node_lps_and_their_children_are_certified(gpu):
    recs = [r for r in INSTANCES[::5]]
    for rec in recs:
        inst = instance(rec)
        root, code = rounded_root(gpu, inst)
        if code == 2:
            continue
        first = root.copy()
        first.simplex()
        if first.status != OPT:  # the LP-infeasible members: the root's own certificate
            cert(gpu, inst, first, "root", rec["family"])
            continue
        for P in bnb.node_sample(root, 8, quirks=0):
            cert(gpu, inst, P, "node", rec["family"])
            _st, viol = bnb.print_info(P, quirks=0)
            if not viol:
                continue
            for S in bnb.make_children(P, viol[0], quirks=0):
                cert(gpu, inst, S, "child before solve", rec["family"], status=capi.UNDEF)
                S.simplex()
                cert(gpu, inst, S, "child", rec["family"])
    kids = collections.Counter()
    for (what, _family, status), k in COUNTS.items():
        if what == "child":
            kids[status] += k
    assert kids[OPT] > 0 and kids[NOFEAS] > 0, kids
    assert {f for (what, f, _s) in COUNTS if what in ("node", "root")} == set("abcd")


# ------------------------------------------------------------------------------------------------ batched entries on mixed windows


def host_gmi(gpu, host_tab, P, j):
    """mvx_generateCutGMI through a table without the device cut entries: the driver's host loop for one column."""
    lib = bnb.lib()
    lib.mvx_generateCutGMI.restype = C.c_int
    lib.mvx_generateCutGMI.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    n = P.n
    inds, vals = np.zeros(n + 1, dtype=np.int32), np.zeros(n + 1)
    lb, eff = C.c_double(0.0), C.c_double(0.0)
    rc = lib.mvx_generateCutGMI(C.cast(C.pointer(host_tab), C.c_void_p), P.h, j, inds.ctypes.data, vals.ctypes.data, C.byref(lb), C.byref(eff))
    coef = np.zeros(n + 1)
    for k in range(1, n + 1):
        if inds[k] > 0:
            coef[inds[k]] = vals[k]
    return rc, coef[1:], lb.value


def test_batched_entries_match_host_twins_on_tree_nodes(gpu):
    """The sampled nodes of one instance in one call each of mvx_round_many, mvx_rc_tighten_many, mvx_branch_penalties_many and
    mvx_gmi_cuts_many, bit for bit against the host twins; every device cut keeps the enumerated optimum where it lies in the
    node's box."""
    recs = sampled([r for r in INSTANCES if r["status"] == "optimal" and r["family"] in "ab"], 30)
    assert len(recs) == 30 and {r["family"] for r in recs} == {"a", "b"}
    host_tab = bnb.table_from(gpu)
    host_tab.gmi_cuts = None
    host_tab.gmi_cuts_many = None
    nodes = found = entries = cands = cuts = inside = 0
    for rec in recs:
        inst = instance(rec)
        root, code = rounded_root(gpu, inst)
        assert code != 2
        sample = bnb.node_sample(root, 12, quirks=0)
        if not sample:
            continue
        nodes += len(sample)
        sg = -1.0 if inst["direction"] == capi.MIN else 1.0
        found += round_device_vs_host(root, sample)
        for delta in (0.25, 2.0, 9.0):
            entries += rc_device_vs_twin(sample, [P.obj - sg * delta for P in sample])
        entries += rc_device_vs_twin(sample, [rec["optimum"]] * len(sample))
        with_cols = [(P, basic_fractional(P, None)) for P in sample]
        with_cols = [(P, [j for j in cols if inst["kinds"][j - 1] != capi.CV]) for P, cols in with_cols]
        with_cols = [(P, cols) for P, cols in with_cols if cols]
        if not with_cols:
            continue
        penalties_device_vs_host(with_cols)
        cands += sum(len(cols) for _, cols in with_cols)
        x = np.array(rec["x"])
        for pos in (0, -1):  # one column per handle and call: the first candidates, then the last
            Ps, cols = [P for P, _ in with_cols], [c[pos] for _, c in with_cols]
            vals, rhs, ok = device_cuts_many(gpu, Ps, cols)
            for t, (P, j) in enumerate(zip(Ps, cols)):
                rc, coef, lb = host_gmi(gpu, host_tab, P, j)
                if rc != 0:  # rejected on the host side (fractional part, norm); the engine reports the free non-basic only
                    continue
                assert ok[t] == 1
                assert np.array_equal(vals[t, 1:].view(np.uint64), coef.view(np.uint64)) and rhs[t] == lb, (rec["index"], j)
                cuts += 1
                lo, hi = node_box(gpu, P)
                if np.all(x >= lo - 1e-9) and np.all(x <= hi + 1e-9):
                    inside += 1
                    assert len(cf.cut_cuts_off(vals[t, 1:], rhs[t], [x])) == 0, (rec["index"], j, rec["x"])
    assert nodes >= 60 and found > 20 and entries >= 100 and cands >= 60 and cuts >= 40 and inside >= 15, (
        nodes, found, entries, cands, cuts, inside)
    COUNTS[("batched", "nodes", OPT)] += nodes


def test_zz_general_counts():
    """Last in the file: what was certified and compared, per sub-family and status, and per forced path."""
    names = {capi.OPT: "OPT", capi.NOFEAS: "NOFEAS", capi.UNDEF: "UNDEF", capi.UNBND: "UNBND"}
    print()
    for key in sorted(COUNTS, key=str):
        a, b, c = key
        print("general: %-20s %-12s %-28s %d" % (a, b, names.get(c, c), COUNTS[key]))
    trees = collections.Counter()
    for (what, path, _name), k in COUNTS.items():
        if what == "trees":
            trees[path] += k
    assert trees["default"] == len(INSTANCES) * len(GPU_OPTIONS)
    assert trees["cluster"] == trees["two-launch"] == len(INSTANCES[::4]) * len(GPU_OPTIONS)
