"""Held commitments on the GPU (csrc/prover.hip zkh_commit_data / zkh_prove_begin_held; SegmentProver.commit_data,
seal_with_accum(held=...); page_seal.seal_tied_group's hold_bytes).  A commitment's root against zkh_data_root and against the seal; a
begin from a held commitment against zkh_prove_begin byte for byte; that a commitment is shared and aliases no trace; every refusal by
its message; the device bytes a commitment and a whole tied group hold, a refused group included; and four tied groups at three
budgets each, byte for byte.

Every seal is small: SYN-A at po2 12, and the tiny tied segment of tied_cases (po2 8 over an image of 64 words, h = 3) with its page-out
as P2-TREE-tied at (8, 40), two parts, and at (10, 500), one part, and as P2-PAGE-tied at tied_cases' page shape, three parts."""
import ctypes as C
import gc
import re

import numpy as np
import pytest

import tied_cases as host
from args_gpu import image_buf, upload
from zeth_amd import hal as zhal, page_seal
from zeth_amd.circuits import logup, p2_page_tied, p2_tree_tied as TT, syn_air, syn_lookup as sl
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver, seal_tied, seal_tied_tree, verify_tied, verify_tied_tree

pytestmark = pytest.mark.gpu
P, ONE = host.P, host.ONE
NOISE = 0x7EED
SEG_PO2, SEG_ZK = host.SEG_PO2, host.SEG_ZK
H = 3
TWO_PARTS, ONE_PART, PATHS = (8, 40), (10, 500), (host.PAGE_PO2, host.PAGE_ZK)
PO2 = 12
EVERYTHING = 1 << 40


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _zero(hal, buf):
    """every word INVALID, then zkh_eltwise_zeroize_elem, which turns exactly those into 0: the buffer holds nothing of the trace"""
    buf.write(np.full(buf.size(), 0xFFFFFFFF, dtype=np.uint32))
    hal.eltwise_zeroize_elem(buf)


def _live(hal):
    gc.collect()
    return hal.memory()["live"]


class Syn:
    """a SYN-A segment at po2 12 on the device, and its seal through zkh_prove_begin"""

    def __init__(self, hal, **kw):
        self.hal, self.desc = hal, syn_air.syn_a()
        self.prover = SegmentProver(hal, self.desc, **kw)
        self.seg = Segment(index=0, po2=PO2, seed=0x5EED0001, noise_seed=NOISE)
        self.code, self.data, self.out = SegmentProver(hal, self.desc).witgen(self.seg)
        self.plain = self.seal()

    def seal(self, held=None, seg=None, out=None, accumulate=None):
        seg = seg or self.seg
        return self.prover.seal_with_accum(seg, self.code, self.data, self.out if out is None else out, accumulate or self.prover.syn_accumulate(seg, self.data), held=held)


class Tied:
    """the tiny tied segment on the device, paged out twice from the same image: once keeping the tree before, once the dirty nodes"""

    def __init__(self, hal):
        s = host.segment()
        self.hal, self.desc, self.table = hal, s["desc"], s["table"]
        self.seg_prover = SegmentProver(hal, s["desc"], arguments=s["blob"])
        self.tree_prover = SegmentProver(hal, TT.p2_tree_tied_circuit(), arguments=TT.arguments())
        self.path_prover = SegmentProver(hal, p2_page_tied.p2_page_tied_circuit(), arguments=p2_page_tied.arguments())
        self.seg = Segment(index=0, po2=SEG_PO2, zk_cycles=SEG_ZK, noise_seed=NOISE)
        code, bare, _ = sl.witness(sl.TINY, SEG_PO2, SEG_ZK, seed=3, link=False, reads=True, pages=False, image=s["image"])
        self.code, self.data = upload(hal, code, bare)
        hal.derive_all_paged(self.seg_prover.circuit, SEG_PO2, SEG_ZK, self.code, self.data, image_buf(hal, s["image"]))
        hal.reduce_elem(self.code)
        hal.reduce_elem(self.data)
        self.image = image_buf(hal, s["image"])
        self.after = hal.image_commit(self.image)
        self.proof, self.before = self.seg_prover.page_out(self.seg, self.data, self.image, tree=self.after, proof=True, keep_before=True)
        image2 = image_buf(hal, s["image"])
        _, self.dirty = self.seg_prover.page_out(self.seg, self.data, image2, tree=hal.image_commit(image2), proof=True, dirty=True)
        assert int(self.proof[4]) == H
        image_after = np.array(s["image"], dtype=np.uint32)
        for a, _, w_out in self.table:
            image_after[a] = w_out
        self.root_before, self.root_after = logup.reference_image_root(s["image"]), logup.reference_image_root(image_after)

    def segs(self, shape, parts):
        return [Segment(index=1 + p, po2=shape[0], zk_cycles=shape[1], noise_seed=NOISE + 1 + p) for p in range(parts)]

    def seal_tree(self, shape=TWO_PARTS, parts=2, dirty=None, proof=None, after=None, **kw):
        proof = self.proof if proof is None else proof
        before, after = (self.before, self.after if after is None else after) if dirty is None else (None, None)
        return seal_tied_tree(self.seg_prover, self.seg, self.code, self.data, np.zeros(4, dtype=np.uint32), self.tree_prover, self.segs(shape, parts), proof, proof.size,
                              before, after, dirty=dirty, **kw)

    def seal_paths(self, **kw):
        return seal_tied(self.seg_prover, self.seg, self.code, self.data, np.zeros(4, dtype=np.uint32), self.path_prover, self.segs(PATHS, 3), self.proof, self.proof.size,
                         self.before, self.after, **kw)

    def open_seal(self, held=None):
        """the segment's seal alone through accumulate_open under tied_cases' fixed challenge"""
        accum = self.hal.alloc_elem("accum", self.seg_prover.group_sizes()[0] << SEG_PO2)
        total = self.hal.accumulate_open(self.seg_prover.circuit, SEG_PO2, SEG_ZK, NOISE, self.code, self.data, host.CHALLENGE, accum)
        out = np.concatenate([np.zeros(4, dtype=np.uint32), host.CHALLENGE, total]).astype(np.uint32)
        return self.seg_prover.seal_with_accum(self.seg, self.code, self.data, out, lambda _mix: accum, held=held)


@pytest.fixture(scope="module")
def syn(hal):
    return Syn(hal)


@pytest.fixture(scope="module")
def tied(hal):
    return Tied(hal)


# ------------------------------------------------------------------------------------------------ 1. the roots
def test_a_commitments_root_is_the_data_root_and_the_seals(hal, syn, tied):
    for prover, data, po2, desc, seal in ((syn.prover, syn.data, PO2, syn.desc, syn.plain.seal), (tied.seg_prover, tied.data, SEG_PO2, tied.desc, tied.open_seal().seal)):
        com = prover.commit_data(data, po2)
        assert np.array_equal(com.root, prover.data_root(data, po2))
        assert np.array_equal(com.root, zhal.HostCircuit(desc).seal_data_root(seal))
        assert com.bytes == 4 * (5 * prover.group_sizes()[2] + 64) << po2 == page_seal.commitment_bytes(prover.group_sizes()[2], po2)
        com.release()


# ------------------------------------------------------------------------------------------------ 2. the begin
def test_a_begin_from_a_held_commitment_gives_the_seal_of_prove_begin(hal, syn, tied):
    com = syn.prover.commit_data(syn.data, PO2)
    held = syn.seal(held=com)
    assert np.array_equal(held.seal, syn.plain.seal), "SYN-A: the seal from the held commitment differs"
    held.verify(syn.desc, syn.prover.control_root(PO2))
    # the same with the code group resident: code == NULL in both arms
    resident = Syn(hal, resident_code_group=True)
    assert resident.prover._resident == {PO2: syn.seg.zk_cycles} and resident.prover._code_handle(resident.seg, resident.code) is None
    assert np.array_equal(resident.plain.seal, syn.plain.seal)
    assert np.array_equal(resident.seal(held=resident.prover.commit_data(resident.data, PO2)).seal, syn.plain.seal), "resident code group: the seal differs"
    assert np.array_equal(resident.seal(held=com).seal, syn.plain.seal), "a commitment of another prover of this context and circuit"
    # the tied segment through accumulate_open
    com = tied.seg_prover.commit_data(tied.data, SEG_PO2)
    assert np.array_equal(tied.open_seal(held=com).seal, tied.open_seal().seal), "the tied segment: the seal from the held commitment differs"


# ------------------------------------------------------------------------------------------------ 3. sharing
def test_a_commitment_is_shared_not_consumed_and_aliases_no_trace(hal, syn):
    data = hal.alloc_elem("data", syn.data.size())
    hal.eltwise_copy_elem(data, syn.data)
    com = syn.prover.commit_data(data, PO2)
    assert np.array_equal(syn.seal(held=com).seal, syn.plain.seal) and np.array_equal(syn.seal(held=com).seal, syn.plain.seal)      # two jobs, one commitment
    inner = syn.prover.syn_accumulate(syn.seg, data)

    def accumulate(mix):
        """the accum from the trace, then the commitment goes and the trace is zeroed, all between the begin and the finish"""
        accum = inner(mix)
        com.release()
        _zero(hal, data)
        return accum
    late = syn.seal(held=com, accumulate=accumulate)
    assert com.h is None and not data.to_vec().any()
    assert np.array_equal(late.seal, syn.plain.seal), "the job read the released commitment or the zeroed trace"
    # and a commitment made before its trace was zeroed still seals the trace it committed
    hal.eltwise_copy_elem(data, syn.data)
    com = syn.prover.commit_data(data, PO2)
    _zero(hal, data)
    assert np.array_equal(syn.seal(held=com).seal, syn.plain.seal)


def test_a_commitment_outlives_the_prover_that_made_it(hal, syn):
    """include/zkhal.h, DESTRUCTION ORDER: released after zkh_prover_destroy, before the context"""
    start = _live(hal)
    maker = SegmentProver(hal, syn.desc)
    com = maker.commit_data(syn.data, PO2)
    maker.__del__()
    assert maker.h is None and _live(hal) == start + com.bytes
    assert np.array_equal(syn.seal(held=com).seal, syn.plain.seal)
    com.release()
    assert _live(hal) == start


# ------------------------------------------------------------------------------------------------ 4. the refusals
def _refuses(text):
    return pytest.raises(HalError, match=f"^{text}$")


def test_every_refusal_by_its_message_and_the_commitment_is_still_usable(hal, syn, tied):
    lib, prover = zhal.load_library(), syn.prover
    com = prover.commit_data(syn.data, PO2)
    job, mix = C.c_void_p(), np.zeros(max(1, int(prover.circuit.desc[8])), dtype=np.uint32)
    begin = lambda p, po2, code, held, out, j=C.byref(job): zhal._check(lib.zkh_prove_begin_held(p, po2, code, held, None if out is None else _u32p(out), j, _u32p(mix)))
    for operands in ((None, PO2, syn.code.h, com.h, syn.out), (prover.h, PO2, syn.code.h, None, syn.out), (prover.h, PO2, syn.code.h, com.h, None)):
        with _refuses("prove_begin_held: null argument"):
            begin(*operands)
    with _refuses("prove_begin_held: null argument"):
        begin(prover.h, PO2, syn.code.h, com.h, syn.out, None)
    with _refuses(re.escape(f"prove_begin_held: no code trace and no resident code group for po2 {PO2} (zkh_prover_cache_code)")):
        begin(prover.h, PO2, None, com.h, syn.out)
    other = zhal.HipHal(0)
    try:
        foreign = SegmentProver(other, syn.desc)
        fdata = other.alloc_elem("data", syn.data.size())
        fdata.write(syn.data.to_vec())
        fcom = foreign.commit_data(fdata, PO2)
        assert np.array_equal(fcom.root, com.root)
        with _refuses(f"prove_begin_held: the commitment was made by a prover of context 0x0*{other.ctx.value:x}, this prover's is 0x0*{hal.ctx.value:x}"):
            syn.seal(held=fcom)
        fcom.release()                                                          # everything of the other context goes while it lives
        fdata.release()
        foreign.__del__()
        h, foreign.circuit.h = foreign.circuit.h, None
        lib.zkh_circuit_destroy(h)
    finally:
        other.close()
    narrow = tied.seg_prover.commit_data(tied.data, SEG_PO2)
    with _refuses(f"prove_begin_held: the commitment holds {tied.seg_prover.group_sizes()[2]} columns, the circuit's data group has {prover.group_sizes()[2]}"):
        syn.seal(held=narrow, seg=Segment(index=0, po2=SEG_PO2, noise_seed=NOISE, zk_cycles=SEG_ZK))
    with _refuses(f"prove_begin_held: the commitment was made at po2 {PO2}, the call's is {PO2 - 1}"):
        syn.seal(held=com, seg=Segment(index=0, po2=PO2 - 1, noise_seed=NOISE))
    # what zkh_prove_begin refuses of po2 and out_global, in its words after the prefix
    bad = syn.out.copy()
    bad[1] = P
    for who, call in (("prove_begin_held", lambda **kw: syn.seal(held=com, **kw)), ("prove_begin", lambda **kw: syn.seal(**kw))):
        with _refuses(f"{who}: output global 1 is not a reduced element"):
            call(out=bad)
        with _refuses(re.escape(f"{who}: po2 25 too large (max 24)")):
            call(seg=Segment(index=0, po2=25, noise_seed=NOISE))
    assert not job.value, "a refusal made a job"
    # after all of them the same commitment begins a seal that verifies
    receipt = syn.seal(held=com)
    receipt.verify(syn.desc, syn.prover.control_root(PO2))
    assert np.array_equal(receipt.seal, syn.plain.seal)
    lib.zkh_commitment_release(None)
    com.release()
    com.release()
    narrow.release()
    with _refuses("prove_begin_held: null argument"):                            # a released commitment is no commitment
        syn.seal(held=com)


# ------------------------------------------------------------------------------------------------ 5. memory
def test_live_bytes_rise_by_the_commitments_bytes_and_come_back(hal, syn):
    start = _live(hal)
    com = syn.prover.commit_data(syn.data, PO2)
    assert com.bytes == 4 * (5 * syn.prover.group_sizes()[2] + 64) << PO2
    assert _live(hal) == start + com.bytes
    receipt = syn.seal(held=com)
    assert _live(hal) == start + com.bytes
    com.release()
    assert _live(hal) == start and np.array_equal(receipt.seal, syn.plain.seal)
    # released between the begin and the finish: the job's references keep the buffers, the finish gives them back
    com = syn.prover.commit_data(syn.data, PO2)
    inner, seen = syn.prover.syn_accumulate(syn.seg, syn.data), []

    def accumulate(mix):
        com.release()
        seen.append(_live(hal))
        return inner(mix)
    syn.seal(held=com, accumulate=accumulate)
    assert seen[0] >= start + com.bytes and _live(hal) == start


def _forged_page_out(hal, tied):
    """a consistent page-out of ANOTHER table: one `out` word of row 1 altered in the proof's table, and the tree after it committed over
    the image with that word"""
    proof = tied.proof.copy()
    at = 5 + H + 3 * 1 + 2
    proof[at] = (int(proof[at]) + ONE) % P
    image = tied.image.to_vec()
    image[int(proof[5 + H + 3])] = proof[at]
    return proof, hal.image_commit(image_buf(hal, image))


def test_a_whole_tied_group_gives_back_what_it_held_a_refused_one_included(hal, tied):
    start = _live(hal)
    receipts = tied.seal_tree(hold_bytes=EVERYTHING)
    assert _live(hal) == start
    del receipts
    proof, after = _forged_page_out(hal, tied)
    start = _live(hal)
    with pytest.raises(HalError, match=r"^seal_tied_tree: the proof's table is not the segment's page table: "):
        tied.seal_tree(proof=proof, after=after, hold_bytes=EVERYTHING)
    assert _live(hal) == start, "a refused group left a held commitment or trace behind"


# ------------------------------------------------------------------------------------------------ 6. the groups
def _budget_for_the_segment_and_one_part(tied, page_prover, po2):
    wd = page_prover.group_sizes()[2]
    return page_seal.commitment_bytes(tied.seg_prover.group_sizes()[2], SEG_PO2) + page_seal.commitment_bytes(wd, po2) + 4 * (wd << po2)


GROUPS = {"two_trees": (lambda t, **kw: t.seal_tree(**kw), "tree_prover", TWO_PARTS, 2),
          "dirty": (lambda t, **kw: t.seal_tree(dirty=t.dirty, **kw), "tree_prover", TWO_PARTS, 2),
          "device_plan": (lambda t, **kw: t.seal_tree(ONE_PART, 1, plan="device", **kw), "tree_prover", ONE_PART, 1),
          "paths": (lambda t, **kw: t.seal_paths(**kw), "path_prover", PATHS, 3)}


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_a_tied_group_is_the_same_seals_at_every_budget(hal, tied, name, monkeypatch):
    seal, prover, shape, parts = GROUPS[name]
    calls = []
    for method in ("commit_data", "data_root"):
        inner = getattr(SegmentProver, method)
        monkeypatch.setattr(SegmentProver, method, lambda self, data, po2, inner=inner, method=method: (calls.append(method), inner(self, data, po2))[1])
    some = _budget_for_the_segment_and_one_part(tied, getattr(tied, prover), shape[0])
    sealed = {}
    for budget, held in ((0, 0), (EVERYTHING, 1 + parts), (some, 2)):
        del calls[:]
        sealed[budget] = seal(tied, check=True, hold_bytes=budget)
        assert (calls.count("commit_data"), calls.count("data_root")) == (held, 1 + parts - held), f"hold_bytes {budget}"
    seg0, parts0 = sealed[0]
    assert len(parts0) == parts
    for budget in (EVERYTHING, some):
        seg_b, parts_b = sealed[budget]
        assert np.array_equal(seg_b.seal, seg0.seal) and np.array_equal(seg_b.control_root, seg0.control_root), f"hold_bytes {budget}: the segment's seal differs"
        for p, (a, b) in enumerate(zip(parts0, parts_b)):
            assert np.array_equal(a.seal, b.seal) and np.array_equal(a.control_root, b.control_root), f"hold_bytes {budget}: part {p} differs"
    for seg_r, part_rs in sealed.values():
        if name == "paths":
            linked = verify_tied(seg_r, tied.desc, seg_r.control_root, part_rs, part_rs[0].control_root, root_before=tied.root_before)
        else:
            linked = verify_tied_tree(seg_r, tied.desc, seg_r.control_root, part_rs, part_rs[0].control_root, H, root_before=tied.root_before)
        assert np.array_equal(linked[0], tied.root_before) and np.array_equal(linked[1], tied.root_after)
        assert np.array_equal(linked[1], hal.image_root(tied.after)), "the group does not reach the updated tree's root"
