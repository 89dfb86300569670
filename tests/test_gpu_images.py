"""GPU: node images (mvx_pack / mvx_pack_from / mvx_unpack) of the engine in every state a handle can take.

tests/images.py names the bases, builds the sender states and holds the one check every state goes through (`roundtrip`); this file
gives it the engine's side -- images in device memory with guard bytes around them, a used receiver whose DevMatrix and rounding
model were built for another model, the batched node entries, mvx_ranges, mvx_del_rows -- and, for the states the oracle can build
and the suite already compares bitwise between the two, holds the engine's receiver to the oracle's after the unpack and after every
continuation step.  tests/test_images_inputs.py proves on the oracle and certify.py that every (state, base) pair has the property its
test here relies on.  The refusals are one test: each is an argument check that returns a code.

What this file found.  (i) On its first device run: the image of a handle without a tableau carried the slab geometry (ld, m_cap) its fields still
held from an earlier life: state 1 unpacked into the used receiver packed to other bytes than the sender (engine_pack writes zeros
there now).  (ii) By reading, pinned in test_refusals: a refused mvx_unpack left dst with the status, pivot count and pending edits of whatever it held before, so a
used dst did not cold-solve to the base's bits (mvx_unpack resets them before it looks at the image).  (iii) Likewise: images against a base
of another column count were built in full and refused only by the receiver; the pack refuses them now.

First device run that passed (MI355X): 59 tests in 5.3 s, the slowest case 0.25 s.  Mutation check (scratch copies, never committed,
each run once against this file): (a) engine_pack without flush_edits fails states 3 and 7 on every base at the first continuation
step (the receiver's re-solve does not see the pending bound: it_cnt); (b) the first appended row left zero in engine_unpack fails
states 7 to 11 at "matrix rows" of the receiver; (c) last_tol and (d) piv_since_check not restored fail every state with a tableau
at the image of the image (24 bytes and 1 byte of the header), in front of the checks of states 13 and 14 that are written for
them; (e) mvx_unpack keeping dst's upper bounds fails test_refusals at a receiver that held a sibling node ("column bounds")."""
import numpy as np
import pytest
import torch

from mvolps_amd import bnb
from mvolps_amd.capi import OPT

from . import images as im

pytestmark = pytest.mark.gpu


class EngineKit(im.Kit):
    name = "engine"
    pad_bytes = im.IMAGE_ALIGN - 1  # between the live tableau rows and the slab tail (engine.cpp: engine_pack)

    def buffer(self, size, fill=im.PATTERN):
        store = torch.full((size + 2 * im.GUARD + im.IMAGE_ALIGN,), fill, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # the engine writes on its own stream: the fill has to be over first
        off = im.GUARD + (-(store.data_ptr() + im.GUARD)) % im.IMAGE_ALIGN
        return (store, off, size), store.data_ptr() + off

    def read(self, buf):
        store, off, size = buf
        torch.cuda.synchronize()
        host = store.cpu().numpy()
        return host[:off].copy(), host[off:off + size].copy(), host[off + size:].copy()

    def write(self, buf, image):
        store, off, size = buf
        store[off:off + size] = torch.from_numpy(np.ascontiguousarray(image)).to("cuda")
        torch.cuda.synchronize()

    def used(self):
        """Solved on a 6x10 model, has answered mvx_gmi_cuts (its DevMatrix is built) and been the root of an mvx_round_many call
        (its rounding model is built)."""
        Q = super().used()
        vals, rhs, ok = im.gmi(Q, im.basic_cols(Q))
        assert ok.any()
        node = Q.copy()
        assert bnb.round_many(Q, [node], 2)[0] == 0
        return Q

    def can_delete(self):
        return True

    def step_ranges(self, group):
        return [H.ranges() for H in group]

    def step_many(self, group):
        """mvx_classify_many, mvx_branch_penalties_many and mvx_rc_tighten_many over all handles in one call each."""
        lead = group[0]
        rc, cls = bnb.classify_many(group, quirks=0)
        if lead.status != OPT and rc != 0:  # not a state the entry takes: the code is all there is to compare
            return [(np.int64(rc),)] * len(group)
        assert rc == 0
        cols = [c[1] for c in cls]
        rp, pen = bnb.branch_penalties_many(group, cols)
        sign = 1.0 if self.api.get_obj_dir(lead.h) == 2 else -1.0
        rt, fix = bnb.rc_tighten_many(group, [lead.obj - sign * 2.0] * len(group))
        if lead.status == OPT:
            assert rp == 0 and rt == 0
        out = []
        for t in range(len(group)):
            entry = [np.int64(cls[t][0]), np.array(cls[t][1], dtype=np.int64), np.array(cls[t][2], dtype=np.float64), np.int64(rp), np.int64(rt)]
            if rp == 0:
                entry += [np.asarray(a) for a in pen[t]]
            if rt == 0:
                entry += [np.array([e[0] for e in fix[t]], dtype=np.int64), np.array([e[1:] for e in fix[t]], dtype=np.float64).reshape(-1, 2)]
            out.append(tuple(entry))
        return out

    def short_cut(self, group):
        """State 13: the tolerances travel with the image, so the same tolerances again are answered from the state at hand
        (last_solve_ms == 0, as test_gpu_tolerances.py pins it) and other tolerances are a solve."""
        out = []
        for H in group:
            rc1 = H.simplex(tol=im.GLPK_TOL)
            again = self.api.last_solve_ms(H.h) == 0.0
            rc2 = H.simplex(tol=im.DEFAULT_TOL)
            real = self.api.last_solve_ms(H.h) > 0.0
            assert rc1 == 0 and again and real, ("short cut", rc1, again, rc2, real)
            out.append((np.int64(rc1), np.int64(rc2)))
        return out


@pytest.fixture(scope="module")
def kit(gpu):
    return EngineKit(gpu)


@pytest.fixture(scope="module")
def okit(orc):
    return im.Kit(orc)


@pytest.mark.parametrize("case", im.CASES, ids=im.case_id)
def test_image_roundtrip(kit, okit, orc, case):
    state, base = case
    trace = []
    sender = im.run_case(kit, state, base, orc, trace)
    if state == "9-grown":  # the sender's slab had to grow for the rows
        assert sender.handles[0].m > sender.root.m + im.ROW_SLACK - im.ROW_SPARE
    if state not in im.ORACLE_PARITY:
        return
    want = []
    im.run_case(okit, state, base, orc, want)
    got = dict(trace)
    assert want and want[0][0] == "received"
    for label, snap in want:
        im.same_snapshots(got[label], snap, "%s/%s: the engine's receiver against the oracle's, %s" % (state, base, label), only=im.PARITY)


def model_part(P):
    keep = ("m", "n", "dir", "row types", "row bounds", "column types", "column bounds", "objective", "kinds", "matrix rows")
    return [e for e in im.snapshot(P) if e[0] in keep]


def test_refusals(kit, gpu):
    """Every refusal returns its code, writes nothing outside (or into) the image, leaves the base and the sender as they were, and
    -- where mvx_unpack refuses -- leaves dst a model-only copy of the base that cold-solves to the base's bits."""
    api = gpu
    root, P = im.solved(api, "ilp-24x48")
    tall = root.copy()
    api.add_rows(tall.h, 1)
    j, x = im.first_fractional(P)
    im.set_col(P, j, im.cut_bound(P, j, x))  # one pending edit, as a node carries it
    before = {id(H): im.snapshot(H) for H in (root, P, tall)}
    cold = root.copy()
    assert cold.simplex() == 0
    cold_bits = im.snapshot(cold)

    def unchanged(what):
        for H in (root, P, tall):
            im.same_snapshots(im.snapshot(H), before[id(H)], what)

    def refused_pack(S, base, what):
        assert api.pack_size_from(S.h, base.h) == -1, what
        buf, addr = kit.buffer(1 << 16)
        assert api.pack_from(S.h, base.h, addr) == -1, what
        assert np.all(im.guards_intact(kit, buf) == im.PATTERN), (what, "a refused pack wrote")

    def refused_unpack(dst, base, image, what):
        buf, addr = kit.buffer(len(image))
        kit.write(buf, image)
        assert api.unpack(dst.h, base.h, addr) == -1, what
        assert np.array_equal(im.guards_intact(kit, buf), image), what
        if dst is base:
            return
        fresh = base.copy()
        im.same_snapshots(model_part(dst), model_part(fresh), what + ": dst is not a copy of the base's model")
        assert [e for e in im.snapshot(dst) if e[0] == "has a tableau"][0][2] == 0, what
        im.same_snapshots(im.snapshot(dst), im.snapshot(fresh), what + ": dst against a model-only copy of the base")
        assert dst.simplex() == fresh.simplex(), what
        im.same_snapshots(im.snapshot(dst), im.snapshot(fresh), what + ": dst solved against the base solved")

    # a base with more rows than the sender
    refused_pack(P, tall, "base taller than the sender")
    unchanged("base taller than the sender")
    image = im.pack(kit, P, root, "the sender of the refusals")
    # dst == base
    refused_unpack(root, root, image, "dst == base")
    unchanged("dst == base")
    def sibling():
        """A handle that held another node of the same base: same sizes, other column bounds, solved."""
        K = root.copy()
        for c in (1, 2, 3):
            im.set_col(K, c, (im.DB, 0.0, 1.0))
        assert K.simplex() == 0
        return K

    for make, name in ((kit.fresh, "fresh"), (kit.used, "used"), (sibling, "sibling's")):
        # wrong magic
        refused_unpack(make(), root, np.zeros(len(image), dtype=np.uint8), "zeros into a %s handle" % name)
        # a base whose m differs from the image's m_base
        refused_unpack(make(), tall, image, "base of another row count into a %s handle" % name)
        unchanged(name)
    im.same_snapshots(im.snapshot(cold), cold_bits, "cold")
    # a base of another column count: the sender has gained or lost columns since, the base has not
    for state, bname in (("15-cols-added", "ilp-12x31"), ("15-cols-deleted", "ilp-8x64")):
        s = im.build(api, state, bname, None)
        S, base = s.handles[0], s.root
        assert S.n != base.n and S.m == base.m
        marks = im.snapshot(S), im.snapshot(base)
        refused_pack(S, base, state + ": packed against the unedited base")
        own = im.pack(kit, S, None, state + ": its own base")  # the same handle does travel as its own base
        for make, name in ((kit.fresh, "fresh"), (kit.used, "used")):
            refused_unpack(make(), base, own, "%s: unpacked against the unedited base into a %s handle" % (state, name))
        im.same_snapshots(im.snapshot(S), marks[0], state + ": sender")
        im.same_snapshots(im.snapshot(base), marks[1], state + ": base")
