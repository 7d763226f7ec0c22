"""Sealing a page-out from (proof, dirty nodes) alone, end to end (SegmentProver.page_out(..., proof=True, dirty=True),
page_seal.seal_tied_tree(dirty=...), SegmentProver.seal_page_out_tree(dirty=...)): the tied group of tests/test_tree_tied_gpu.py, the tiny
segment over an image of 64 words (h = 3) with its page-out at (8, 40), two parts, and at (10, 500), one part, sealed once from the two
trees and once from the dirty-node table with the same noise seeds.  Every seal must be byte-identical, the verifiers must return the
same roots and hi, and the new keyword combinations are refused, one message each."""
import re

import numpy as np
import pytest

import tied_cases as host
from args_gpu import image_buf, upload
from zeth_amd.circuits import logup, p2_page_ordered, p2_tree, p2_tree_tied as TT, syn_lookup as sl
from zeth_amd.hal import Buffer, HalError
from zeth_amd.prover import Segment, SegmentProver, seal_tied_tree, verify_page_tree_chain, verify_tied_tree

pytestmark = pytest.mark.gpu
NOISE = 0x7EED
SEG_PO2, SEG_ZK, W = host.SEG_PO2, host.SEG_ZK, host.W
H = 3
TWO_PARTS, ONE_PART = (8, 40), (10, 500)


class Group:
    """the tied segment on the device, paged out twice from the same image: once keeping the tree before (the two-tree operands), once
    keeping the dirty nodes (no copy of the tree)"""

    def __init__(self, hal):
        s = host.segment()
        self.hal, self.desc, self.table = hal, s["desc"], s["table"]
        self.seg_prover = SegmentProver(hal, s["desc"], arguments=s["blob"])
        self.page_prover = SegmentProver(hal, TT.p2_tree_tied_circuit(), arguments=TT.arguments())
        self.seg = Segment(index=0, po2=SEG_PO2, zk_cycles=SEG_ZK, noise_seed=NOISE)
        code, bare, _ = sl.witness(sl.TINY, SEG_PO2, SEG_ZK, seed=3, link=False, reads=True, pages=False, image=s["image"])
        self.code, self.data = upload(hal, code, bare)
        hal.derive_all_paged(self.seg_prover.circuit, SEG_PO2, SEG_ZK, self.code, self.data, image_buf(hal, s["image"]))
        hal.reduce_elem(self.code)
        hal.reduce_elem(self.data)
        self.host_image = s["image"]
        image = image_buf(hal, s["image"])
        self.after = hal.image_commit(image)
        self.proof, self.before = self.seg_prover.page_out(self.seg, self.data, image, tree=self.after, proof=True, keep_before=True)
        image2 = image_buf(hal, s["image"])
        self.after2 = hal.image_commit(image2)
        self.proof2, self.dirty = self.seg_prover.page_out(self.seg, self.data, image2, tree=self.after2, proof=True, dirty=True)
        self.root_before = logup.reference_image_root(s["image"])

    def segs(self, shape, parts, first=1):
        return [Segment(index=first + p, po2=shape[0], zk_cycles=shape[1], noise_seed=NOISE + 1 + p) for p in range(parts)]

    def seal(self, shape, parts, dirty=None, **kw):
        before, after = (self.before, self.after) if dirty is None else (None, None)
        return seal_tied_tree(self.seg_prover, self.seg, self.code, self.data, np.zeros(4, dtype=np.uint32), self.page_prover, self.segs(shape, parts),
                              self.proof, self.proof.size, kw.pop("before", before), kw.pop("after", after), dirty=dirty, **kw)


@pytest.fixture(scope="module")
def group(hal):
    return Group(hal)


def test_page_out_hands_back_the_proof_and_its_dirty_nodes_without_a_copy_of_the_tree(hal, group):
    assert isinstance(group.dirty, Buffer) and np.array_equal(group.proof2, group.proof)
    assert np.array_equal(group.after2.to_vec(), group.after.to_vec())
    root_after, want = logup.reference_page_out_nodes(group.proof, group.root_before)
    assert np.array_equal(group.dirty.to_vec()[:want.size], want) and np.array_equal(root_after, hal.image_root(group.after))
    image = image_buf(hal, group.host_image)
    tree = hal.image_commit(image)
    with pytest.raises(HalError, match=r"^page_out: dirty=True needs proof=True \(the dirty nodes are read off the proof\)$"):
        group.seg_prover.page_out(group.seg, group.data, image, tree=tree, dirty=True)
    with pytest.raises(HalError, match=r"^page_out: dirty=True with keep_before=True "):
        group.seg_prover.page_out(group.seg, group.data, image, tree=tree, proof=True, keep_before=True, dirty=True)
    assert np.array_equal(image.to_vec(), group.host_image) and np.array_equal(tree.to_vec(), group.before.to_vec()), "a refused page_out wrote"


@pytest.mark.parametrize("shape,parts,plan", [(TWO_PARTS, 2, "host"), (ONE_PART, 1, "device")], ids=["two_parts", "one_part"])
def test_the_tied_group_from_the_dirty_nodes_is_the_group_from_the_two_trees_byte_for_byte(hal, group, shape, parts, plan):
    seg_a, parts_a = group.seal(shape, parts, check=True, plan=plan)
    seg_b, parts_b = group.seal(shape, parts, dirty=group.dirty, check=True, plan=plan)
    assert len(parts_a) == len(parts_b) == parts
    assert np.array_equal(seg_a.seal, seg_b.seal), "the segment's seal differs"
    for p, (a, b) in enumerate(zip(parts_a, parts_b)):
        assert np.array_equal(a.seal, b.seal), f"part {p}: the seal from the dirty nodes is not the seal from the two trees"
        assert np.array_equal(a.control_root, b.control_root)
    verify = lambda s, ps: verify_tied_tree(s, group.desc, s.control_root, ps, ps[0].control_root, H, root_before=group.root_before)
    (rb_a, ra_a, hi_a), (rb_b, ra_b, hi_b) = verify(seg_a, parts_a), verify(seg_b, parts_b)
    assert np.array_equal(rb_a, rb_b) and np.array_equal(ra_a, ra_b) and hi_a == hi_b == 1 << H
    assert np.array_equal(ra_b, hal.image_root(group.after))


def test_the_untied_chain_from_the_dirty_nodes_is_the_chain_from_the_two_trees(hal, group):
    prover = SegmentProver(hal, p2_tree.p2_tree_circuit(), arguments=p2_tree.arguments())
    segs = group.segs(TWO_PARTS, 2, first=0)
    recs_a = prover.seal_page_out_tree(segs, group.proof, group.proof.size, group.before, group.after, check=True)
    recs_b = prover.seal_page_out_tree(segs, group.proof, group.proof.size, None, None, check=True, dirty=group.dirty)
    assert len(recs_a) == len(recs_b) == 2
    for a, b in zip(recs_a, recs_b):
        assert np.array_equal(a.seal, b.seal)
    root = prover.code_root(hal.page_tree_code(prover.circuit, *TWO_PARTS), TWO_PARTS[0])
    got_a, got_b = verify_page_tree_chain(recs_a, root, H, group.root_before), verify_page_tree_chain(recs_b, root, H, group.root_before)
    assert all(np.array_equal(x, y) for x, y in zip(got_a[:2], got_b[:2])) and got_a[2] == got_b[2] == 1 << H


def test_the_new_keyword_combinations_are_refused(hal, group):
    with pytest.raises(HalError, match=r"^seal_tied_tree: dirty nodes stand in place of the two trees: nodes_before and nodes_after must be None$"):
        group.seal(TWO_PARTS, 2, dirty=group.dirty, before=group.before, after=group.after)
    with pytest.raises(HalError, match=r"^seal_tied_tree: dirty nodes stand in place of the two trees"):
        group.seal(TWO_PARTS, 2, dirty=group.dirty, after=group.after)
    prover = SegmentProver(hal, p2_tree.p2_tree_circuit(), arguments=p2_tree.arguments())
    with pytest.raises(HalError, match=r"^seal_page_out_tree: dirty nodes stand in place of the two trees"):
        prover.seal_page_out_tree(group.segs(TWO_PARTS, 2, first=0), group.proof, group.proof.size, group.before, group.after, dirty=group.dirty)
    ordered = SegmentProver(hal, p2_page_ordered.p2_page_ordered_circuit())
    from zeth_amd import page_seal
    with pytest.raises(HalError, match=re.escape("seal_page_out_ordered: dirty nodes seal the tree kinds (7, 9); kind 6 lays out paths, which read the two trees")):
        page_seal.seal_chain("seal_page_out_ordered", ordered, 6, group.segs(TWO_PARTS, 1), group.proof, group.proof.size, None, None, False, dirty=group.dirty)
