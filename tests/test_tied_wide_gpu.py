"""THE TIE of a wide memory on the GPU, end to end (SYN-LOOKUP-tied-wide; page_seal.seal_tied, seal_tied_tree, seal_tied_tree_from_proof,
preflight_paged_run / seal_paged_step and their host-only verifiers).  The tiny tied-wide segment of flat_cases (po2 8, zk 40, seed 3 over a
flat image of 64 words: 32 addresses of two value words, h = 3): the device proof's table is the FLAT one of 64 rows and its fingerprint
is the segment's open total; the group seals with P2-TREE-tied parts at (8, 40), two parts, and at (10, 500), one part planned on the
device, and with P2-PAGE-tied parts, three; the group from the proof alone is byte for byte the group of the rank that holds the image; two
segments over one image are sealed in reverse order and verified from root_0 to root_2.  No page-out circuit knows V.  Then the refusals,
one message each."""
import numpy as np
import pytest

import flat_cases as fc
from args_gpu import image_buf, upload
from zeth_amd.circuits import logup, p2_page_tied, p2_tree_tied as TT, syn_lookup as sl
from zeth_amd.hal import Buffer, HalError
from zeth_amd.page_seal import (PagedStep, preflight_paged_run, seal_paged_step, seal_tied, seal_tied_tree, seal_tied_tree_from_proof, verify_paged_run, verify_tied,
                                verify_tied_tree)
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu
P, ONE, CHALLENGE = fc.P, fc.ONE, fc.CHALLENGE
NOISE = 0x7EED
SEG_PO2, SEG_ZK, WORDS, H = fc.SEG_PO2, fc.SEG_ZK, fc.WORDS, fc.H
TWO_PARTS, ONE_PART = fc.TWO_PARTS, fc.ONE_PART
PREFIX = np.zeros(4, dtype=np.uint32)
WIT = dict(reads=True, wide=True, flat=True)


def _page_segs(shape, parts, first=1):
    return [Segment(index=first + p, po2=shape[0], zk_cycles=shape[1], noise_seed=NOISE + first + p) for p in range(parts)]


def _paged_out(image, table):
    """the flat image after the flat table's page-out"""
    after = np.array(image, dtype=np.uint32)
    for a, _, w_out in table:
        after[a] = w_out
    return after


class Group:
    """one tied group of a WIDE segment on the device: its traces derived from the flat image, its page-out's proof, the two trees, the
    dirty nodes"""

    def __init__(self, hal):
        s = fc.segment()
        self.hal, self.desc, self.table = hal, s["desc"], s["table"]
        self.seg_prover = SegmentProver(hal, s["desc"], arguments=s["blob"])
        assert self.seg_prover.circuit.page_words() == 2 and self.seg_prover.circuit.page_flats() == 2
        self.page_prover = SegmentProver(hal, TT.p2_tree_tied_circuit(), arguments=TT.arguments())
        self.seg = Segment(index=0, po2=SEG_PO2, zk_cycles=SEG_ZK, noise_seed=NOISE)
        self.host_code, self.host_data, _ = sl.witness(sl.TINY, SEG_PO2, SEG_ZK, seed=3, link=False, pages=False, image=s["image"], **WIT)
        self.code, self.data = upload(hal, self.host_code, self.host_data)
        self.image = image_buf(hal, s["image"])
        hal.derive_all_paged(self.seg_prover.circuit, SEG_PO2, SEG_ZK, self.code, self.data, self.image)
        hal.reduce_elem(self.code)
        hal.reduce_elem(self.data)
        n, A = 1 << SEG_PO2, (1 << SEG_PO2) - SEG_ZK
        assert np.array_equal(self.data.to_vec().reshape(-1, n)[:, :A], s["data"].reshape(-1, n)[:, :A]), "the derive is not the host-made witness"
        self.after = hal.image_commit(self.image)                             # the page-out turns the image, and this tree, into the ones after
        self.proof, self.before = self.seg_prover.page_out(self.seg, self.data, self.image, tree=self.after, proof=True, keep_before=True)
        self.root_before = logup.reference_image_root(s["image"])
        self.root_after = logup.reference_image_root(_paged_out(s["image"], s["table"]))
        _, self.dirty = hal.image_proof_nodes(hal.copy_from("image_proof", self.proof), self.root_before, words=self.proof.size)

    def seal(self, shape=TWO_PARTS, parts=2, proof=None, after=None, **kw):
        proof = self.proof if proof is None else proof
        return seal_tied_tree(self.seg_prover, self.seg, self.code, self.data, PREFIX, self.page_prover, _page_segs(shape, parts), proof, proof.size,
                              self.before, self.after if after is None else after, **kw)

    def verify(self, seg_receipt, parts, h=H, **kw):
        return verify_tied_tree(seg_receipt, self.desc, seg_receipt.control_root, parts, parts[0].control_root, h, **kw)


@pytest.fixture(scope="module")
def group(hal):
    g = Group(hal)
    g.receipts = g.seal(check=True)
    return g


def test_the_proofs_table_is_the_flat_one_and_its_fingerprint_is_the_open_total(hal, group):
    proof = group.proof
    assert (int(proof[1]), int(proof[2]), int(proof[4])) == (WORDS, 64, H)   # (V W, V D): 64 flat rows over the flat image, h = 3
    table = proof[5 + H:5 + H + 3 * 64].reshape(-1, 3)
    want = np.array(group.table, dtype=np.uint64)
    assert np.array_equal(table[:, 0], want[:, 0]) and np.array_equal(table[:, 1:], (want[:, 1:] % P))
    _, total = fc.segment_total()
    assert np.array_equal(hal.table_fingerprint(hal.copy_from("image_proof", proof), 5 + H, 64, CHALLENGE), total)
    assert np.array_equal(hal.image_root(group.after), group.root_after) and np.array_equal(group.image.to_vec() % P, _paged_out(fc.segment()["image"], group.table) % P)


def test_a_tied_wide_group_seals_and_verifies_from_root_to_root(hal, group):
    seg_receipt, parts = group.receipts
    assert len(parts) == 2
    for given in (group.root_before, None):
        root_before, root_after, hi = group.verify(seg_receipt, parts, root_before=given)
        assert np.array_equal(root_before, group.root_before) and np.array_equal(root_after, group.root_after) and hi == 1 << H
    assert not np.array_equal(group.root_before, group.root_after)
    for r in parts:                                                          # every part carries the segment's challenge
        r.verify(TT.p2_tree_tied_circuit(), r.control_root)
        assert np.array_equal(r.seal[TT.OUT_ALPHA:TT.OUT_TOTAL], seg_receipt.seal[sl.OUT_ALPHA:sl.OUT_TOTAL]) and int(r.seal[TT.OUT_BASE]) == TT.out_base(H)
    seg_receipt.verify(group.desc, seg_receipt.control_root)
    seg1, parts1 = group.seal(ONE_PART, 1, check=True, plan="device")        # one part, planned where the table lies
    assert len(parts1) == 1
    root_before, root_after, hi = group.verify(seg1, parts1, root_before=group.root_before)
    assert np.array_equal(root_before, group.root_before) and np.array_equal(root_after, group.root_after) and hi == 1 << H
    # from the dirty nodes, and with what pass one may hold: the same seals
    seg2, parts2 = seal_tied_tree(group.seg_prover, group.seg, group.code, group.data, PREFIX, group.page_prover, _page_segs(TWO_PARTS, 2), group.proof,
                                  group.proof.size, None, None, dirty=group.dirty, hold_bytes=1 << 30)
    assert np.array_equal(seg2.seal, seg_receipt.seal) and all(np.array_equal(a.seal, b.seal) for a, b in zip(parts, parts2))


def test_p2_page_tied_seals_the_flat_table_in_three_parts(hal, group):
    pager = SegmentProver(hal, p2_page_tied.p2_page_tied_circuit(), arguments=p2_page_tied.arguments())
    seg_p, parts_p = seal_tied(group.seg_prover, group.seg, group.code, group.data, PREFIX, pager, _page_segs((fc.PAGE_PO2, fc.PAGE_ZK), 3), group.proof,
                               group.proof.size, group.before, group.after)
    assert len(parts_p) == 3
    root_before, root_after, hi = verify_tied(seg_p, group.desc, seg_p.control_root, parts_p, parts_p[0].control_root, root_before=group.root_before)
    assert np.array_equal(root_before, group.root_before) and np.array_equal(root_after, group.root_after) and hi == 64       # the last flat address is 63


def test_the_group_from_the_proof_alone_is_byte_for_byte_the_same(hal, group):
    seg_a, parts_a = group.receipts
    seg_b, parts_b, root_after = seal_tied_tree_from_proof(group.seg_prover, group.seg, group.host_code, group.host_data, PREFIX, group.page_prover,
                                                           _page_segs(TWO_PARTS, 2), group.proof, group.root_before, check=True, plan="host")
    assert np.array_equal(root_after, group.root_after) and len(parts_b) == 2
    assert np.array_equal(seg_a.seal, seg_b.seal), "the segment's seal differs"
    for p, (a, b) in enumerate(zip(parts_a, parts_b)):
        assert np.array_equal(a.seal, b.seal), f"part {p}: the seal differs"


def test_a_run_of_two_wide_segments_over_one_image(hal):
    desc, blob = sl.syn_lookup_tiny_tied_wide()
    args = logup.Arguments.parse(blob)
    n, A = 1 << SEG_PO2, (1 << SEG_PO2) - SEG_ZK
    image = fc.flat_image()
    images, witnesses, rows = [image], [], []
    for seed in (3, 4):                                                      # the second segment's image is the first one's page-out
        code, bare, _ = sl.witness(sl.TINY, SEG_PO2, SEG_ZK, seed=seed, link=False, pages=False, image=image, **WIT)
        _, full, _ = sl.witness(sl.TINY, SEG_PO2, SEG_ZK, seed=seed, link=True, pages=True, image=image, **WIT)
        d, pg = full.reshape(-1, n), args.pages
        on = d[pg.p_on, :A] == ONE
        addrs = logup._dec(d[pg.p_addr, :A][on]).astype(np.int64)
        image = image.copy()
        for j in range(2):
            image[2 * addrs + j] = d[pg.p_outs[j], :A][on]
        witnesses.append((code, bare))
        rows.append(2 * int(on.sum()))
        images.append(image)
    roots = [logup.reference_image_root(i) for i in images]
    assert all(r > 0 for r in rows) and not np.array_equal(roots[0], roots[1]) and not np.array_equal(roots[1], roots[2])
    segs = [Segment(index=10 * k, po2=SEG_PO2, zk_cycles=SEG_ZK, noise_seed=NOISE + 100 * k) for k in range(2)]
    seg_prover = SegmentProver(hal, desc, arguments=blob)
    page_prover = SegmentProver(hal, TT.p2_tree_tied_circuit(), arguments=TT.arguments())
    dimage = image_buf(hal, images[0])
    tree = hal.image_commit(dimage)
    steps = preflight_paged_run(seg_prover, segs, witnesses, dimage, tree)
    assert np.array_equal(dimage.to_vec() % P, images[2] % P) and np.array_equal(tree.to_vec(), logup.reference_image_tree(images[2]).reshape(-1))
    assert [int(s.proof[2]) for s in steps] == rows                          # the proofs' tables are the flat ones
    for k, s in enumerate(steps):
        assert np.array_equal(s.root_before, roots[k]) and np.array_equal(s.root_after, roots[k + 1])
        assert not any(isinstance(v, Buffer) for v in vars(s).values()), "a step ships no device buffer"
    del dimage, tree
    groups = [None] * 2
    for k in (1, 0):
        groups[k] = seal_paged_step(steps[k], seg_prover, PREFIX, page_prover, lambda p, k=k: Segment(index=10 * k + 1 + p, po2=TWO_PARTS[0], zk_cycles=TWO_PARTS[1],
                                                                                                        noise_seed=NOISE + 100 * k + 1 + p))
    seg_root, page_root = groups[0][0].control_root, groups[0][1][0].control_root
    for given in (None, roots[0]):
        first, last = verify_paged_run(groups, desc, seg_root, page_root, H, root_before=given)
        assert np.array_equal(first, roots[0]) and np.array_equal(last, roots[2])
    with pytest.raises(HalError, match=r"^verify_paged_run: group 1 opens root [0-9a-f ]+, but group 0 left root [0-9a-f ]+$"):
        verify_paged_run(groups[::-1], desc, seg_root, page_root, H)


# ------------------------------------------------------------------------------------------------ refusals
def _forged_page_out(hal, group):
    """a consistent page-out of ANOTHER table: one `out` word of flat row 1 altered in the proof's table, and the tree after it committed
    over the image with that word"""
    proof = group.proof.copy()
    at = 5 + H + 3 * 1 + 2
    proof[at] = (int(proof[at]) + ONE) % P
    image = group.image.to_vec()
    image[int(proof[5 + H + 3])] = proof[at]
    return proof, hal.image_commit(image_buf(hal, image))


def test_a_proof_of_another_table_is_refused_before_a_part_is_sealed_and_by_the_verifier_without_the_check(hal, group):
    proof, after = _forged_page_out(hal, group)
    with pytest.raises(HalError, match=r"^seal_tied_tree: the proof's table is not the segment's page table: the segment's open total is [0-9a-f ]+, the fingerprint of "
                                       r"the proof's 64 rows is [0-9a-f ]+$"):
        group.seal(proof=proof, after=after)
    seg_receipt, parts = group.seal(proof=proof, after=after, check_table=False)       # all seals are made: the forged page-out is consistent
    with pytest.raises(HalError, match=r"^verify_tied_tree: the totals do not cancel: the segment's F plus the parts' is [0-9a-f ]+, not zero"):
        group.verify(seg_receipt, parts)


def test_a_wide_prover_without_flat_columns_is_refused_by_every_entry_point(hal, group):
    desc, blob = sl.build_syn_lookup(sl.TINY, link=True, reads=True, pages=True, wide=True)
    sp = SegmentProver(hal, desc, arguments=blob)
    assert sp.circuit.page_words() == 2 and sp.circuit.page_flats() == 0
    msg = r"^{}: the segment's memory holds 2 value words per address \(ZKA1 version 10\): the tie of a wide memory is not built without flat-address columns"
    pager = group.page_prover
    with pytest.raises(HalError, match=msg.format("seal_tied")):
        seal_tied(sp, group.seg, group.code, group.data, PREFIX, pager, _page_segs(TWO_PARTS, 2), group.proof, group.proof.size, group.before, group.after)
    with pytest.raises(HalError, match=msg.format("seal_tied_tree")):
        seal_tied_tree(sp, group.seg, group.code, group.data, PREFIX, pager, _page_segs(TWO_PARTS, 2), group.proof, group.proof.size, group.before, group.after)
    with pytest.raises(HalError, match=msg.format("seal_tied_tree_from_proof")):
        seal_tied_tree_from_proof(sp, group.seg, group.host_code, group.host_data, PREFIX, pager, _page_segs(TWO_PARTS, 2), group.proof, group.root_before)
    with pytest.raises(HalError, match=msg.format("preflight_paged_run")):
        preflight_paged_run(sp, [group.seg], [(group.host_code, group.host_data)], group.image, group.after)
    step = PagedStep(group.seg, group.host_code, group.host_data, group.proof, group.root_before, group.root_after)
    with pytest.raises(HalError, match=msg.format("seal_tied_tree_from_proof")):
        seal_paged_step(step, sp, PREFIX, pager, _page_segs(TWO_PARTS, 2))
