"""GPU: the batched node entries (mvx_classify_many, mvx_branch_penalties_many, mvx_round_many, mvx_dive_pick_many,
mvx_rc_tighten_many, mvx_propagate_many, mvx_gmi_cuts_many, and the two that apply bound lists, mvx_tighten_cols_many and
mvx_set_col_bnds_many) share one device + pinned scratch arena.  Called in turn in one process, small batches around full
ones so that the arena grows under different entries, each must give the same bits whatever ran in between.  (What
each entry computes is checked against its host twin in the entry's own test file.)"""
import ctypes as C

import numpy as np
import pytest

from mvolps_amd import bnb, synth
from mvolps_amd.capi import DB, FX

from . import lpgen
from .test_bnb_prop import set_bounds
from .test_gpu_rcfix import state

pytestmark = pytest.mark.gpu

TOL = 1e-9


def gmi_cuts_many(gpu, Ps, cols):
    lib = gpu.lib
    k, n = len(cols), Ps[0].n
    vals, rhs, ok = np.zeros((k, n + 1)), np.zeros(k), np.zeros(k, dtype=np.int32)
    arr = np.asarray(cols, dtype=np.int32)
    hs = (C.c_void_p * k)(*[p.h for p in Ps])
    lib.mvx_gmi_cuts_many.restype = C.c_int
    lib.mvx_gmi_cuts_many.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.mvx_gmi_cuts_many(hs, 1, arr.ctypes.data, k, vals.ctypes.data, rhs.ctypes.data, ok.ctypes.data) == 0
    return vals, rhs, ok


def same(got, want):
    """Bit equality of two results of one entry: np.array_equal on arrays, == on everything else."""
    if isinstance(want, np.ndarray):
        assert np.array_equal(got, want)
    elif isinstance(want, (list, tuple)) and len(want) and isinstance(want[0], (np.ndarray, list, tuple)):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            same(g, w)
    else:
        assert got == want


def head(r):
    """The first two handles' part of a full batch's result (a list per handle, or a tuple of arrays by handle)."""
    return tuple(a[:2] for a in r) if isinstance(r, tuple) else r[:2]


def test_entries_share_one_arena(gpu):
    A, b, c, U = synth.dense_ilp(512, 1024, 12345, 3, 0.4)
    root = lpgen.load_ilp(gpu, A, b, c, U)
    nodes = bnb.node_sample(root, 64)
    assert len(nodes) == 64
    cand = [bnb.print_info(P, quirks=0)[1] for P in nodes]  # fractional integer columns (basic), from the host mirrors
    assert cand[0] and cand[1]
    cut = [t for t in range(64) if cand[t]]  # a cut needs a basic fractional column
    assert cut[:2] == [0, 1] and len(cut) >= 32
    cutoffs = [P.obj - (3.0, 25.0, 70.0, 400.0)[t % 4] for t, P in enumerate(nodes)]

    def classify(k):
        rc, out = bnb.classify_many(nodes[:k], quirks=0)
        assert rc == 0
        return out

    def penalties(k):
        rc, out = bnb.branch_penalties_many(nodes[:k], cand[:k], TOL)
        assert rc == 0
        return out

    def rounding(k):
        rc, obj, found, x = bnb.round_many(root, nodes[:k], 2)
        assert rc == 0
        return obj, found, x

    def rcfix(k):
        rc, lists = bnb.rc_tighten_many(nodes[:k], cutoffs[:k], TOL)
        assert rc == 0
        return lists

    def cuts(k):
        ts = cut[:2] if k == 2 else cut
        return gmi_cuts_many(gpu, [nodes[t] for t in ts], [cand[t][0] for t in ts])

    kids = [S for t in cut for S in bnb.make_children(nodes[t], cand[t][0], quirks=0)][:64]  # unsolved: a pending branching edit
    assert len(kids) == 64
    rules = [(1, 2, 4)[t % 3] for t in range(64)]

    def dive(k):
        rc, out = bnb.dive_pick_many(root, nodes[:k], rules[:k])
        assert rc == 0
        return out

    def prop(k):
        rc, out = bnb.propagate_many(root, kids[:k])
        assert rc == 0
        return out

    applied = []  # (clone, twin, list, per-entry edit)

    def tighten_entry(R, e):
        gpu.set_col_bnds(R.h, e[0], FX if e[1] == e[2] else DB, e[1], e[2])

    def apply(k, res):
        """The two apply entries on clones of the first k nodes / children, one call each: a node takes its reduced-cost
        list, a child its parent's and, over it, the bounds propagation found for the child (what a child of the rc_fix +
        prop driver takes; on this sample propagation finds nothing).  nodes and kids themselves stay untouched."""
        def kid_list(t):
            lst = {e[0]: e for e in res["rcfix"][cut[t // 2]]}
            lst.update((e[0], e) for e in res["prop"][t][2])
            return [lst[j] for j in sorted(lst)]

        live = [t for t in range(k) if not res["prop"][t][0]]
        tc, pc = [P.copy() for P in nodes[:k]], [kids[t].copy() for t in live]
        tl, pl = res["rcfix"][:k], [kid_list(t) for t in live]
        applied.extend((S, P.copy(), l, tighten_entry) for S, P, l in zip(tc, nodes[:k], tl))
        applied.extend((S, kids[t].copy(), l, lambda R, e: set_bounds(gpu, R, *e)) for S, t, l in zip(pc, live, pl))
        assert bnb.tighten_cols_many(tc, tl) == 0
        assert bnb.set_col_bnds_many(pc, pl) == 0
        return sum(len(l) for l in tl), sum(len(l) for l in pl)

    entries = dict(classify=classify, penalties=penalties, rounding=rounding, rcfix=rcfix, cuts=cuts, dive=dive, prop=prop)
    small = {name: entries[name](2) for name in ("classify", "penalties", "rounding", "dive", "rcfix", "prop", "cuts")}
    assert small["rcfix"][0] or small["rcfix"][1]
    assert small["cuts"][2].any() and all(len(p[0]) > 0 for p in small["penalties"])
    assert all(r[1] > 0 for r in small["dive"])
    apply(2, small)
    full = {name: entries[name](64) for name in ("penalties", "cuts", "prop", "classify", "rcfix")}
    counts = apply(64, full)  # between two full read-only calls
    print("entries applied to 64 clones: %d tighten, %d set-bounds" % counts)
    assert counts[0] > 0 and counts[1] > 0
    full.update({name: entries[name](64) for name in ("rounding", "dive")})
    for name in ("rcfix", "rounding", "dive", "cuts"):
        same(entries[name](2), small[name])
    apply(2, small)
    for name in ("penalties", "prop", "classify"):
        same(entries[name](2), small[name])
    for name in entries:
        same(head(full[name]), small[name])
    # the clones against clones edited one entry at a time (mvx_set_col_bnds)
    for S, R, lst, edit in applied:
        for e in lst:
            edit(R, e)
        assert state(S) == state(R)
        assert np.array_equal(S.tableau(), R.tableau())
