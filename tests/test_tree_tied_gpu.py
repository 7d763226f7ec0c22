"""P2-TREE-tied on the GPU (zkh_page_tree_code / zkh_page_tree_witgen serving kind 9, csrc/page_tree.hip k_tree_words; prover.seal_tied_tree /
verify_tied_tree).  The device witness against p2_tree_tied's reference word for word, all 138 columns, the blinding rows and `out`; the
open accumulate of a part against the reference's accum and total; one tied group end to end at two page shapes, planned on the host and
on the device; and what the prover and the group verifier refuse, one message each.

Shapes, the smallest at which the new code can go wrong: page_tree_cases' (10, 500, 64), a tree of 7 blocks, with no row, with two words
of one pair in different leaves, with three words of one leaf, and with every word; (12, 1994, 8 * 17 + 3), whose last pair of leaves
reaches past the image; (10, 500, 512) with every word, several parts; (12, 200, 2048) with 40 random addresses: 250 lanes of the block
kernel in workgroups of 64, and 3875 rows of the new kernel in 16 workgroups of 256, the last partial.  End to end: the tiny tied segment
of tied_cases (po2 8 over an image of 64 words, h = 3) with its page-out at (8, 40), 6 block slots and so two parts, and at (10, 500),
one part."""
import ctypes as C

import numpy as np
import pytest

import page_circuit_cases as pcases
import page_tree_cases as tc
import tied_cases as host
import tree_tied_cases as cases
from args_gpu import image_buf, upload
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, p2_page_tied, p2_tree, p2_tree_tied as TT, syn_lookup as sl
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver, seal_tied, seal_tied_tree, verify_tied_tree

pytestmark = pytest.mark.gpu
P, ONE, CHALLENGE = cases.P, cases.ONE, cases.CHALLENGE
NOISE = 0x7EED
SEG_PO2, SEG_ZK, W = host.SEG_PO2, host.SEG_ZK, host.W
H = 3                                                                             # the height of the tree of the segment's image
TWO_PARTS, ONE_PART = (8, 40), (10, 500)                                          # the page shapes of the end-to-end runs: (po2, zk_cycles)


@pytest.fixture(scope="module")
def prover(hal):
    return SegmentProver(hal, TT.p2_tree_tied_circuit(), arguments=TT.arguments())


_on_device = {}


def _device(hal, s, what):
    """the table on the device -> (proof buffer, proof words, nodes_before, nodes_after): the trees of the WHOLE page-out, once per table"""
    if (s, what) not in _on_device:
        t = tc.table(*s, what)
        before = hal.image_commit(image_buf(hal, t["image"]))
        after = hal.image_commit(image_buf(hal, t["image_after"]))
        proof = pcases.host_proof(t["image"], t["addrs"], t["outs"], before.to_vec())
        _on_device[s, what] = (hal.copy_from("proof", proof), proof.size, before, after)
    return _on_device[s, what]


@pytest.mark.parametrize("g", cases.grid(cases.TABLES + [(cases.H8, "random")]), ids=cases.grid_id)
def test_the_generator_is_the_reference_word_for_word(hal, prover, g):
    (po2, zk, W_), what, p = g
    t = tc.table(po2, zk, W_, what)
    first, count = t["plan"][p]
    want_data, _, want_out, want_code = cases.part(po2, zk, W_, what, p)
    n, A = 1 << po2, (1 << po2) - zk
    proof, words, before, after = _device(hal, (po2, zk, W_), what)
    code = hal.page_tree_code(prover.circuit, po2, zk)
    assert np.array_equal(code.to_vec().reshape(TT.WC, n), want_code), "the code group is not P2-TREE's"
    data = hal.alloc_elem("data", TT.WD << po2)
    data.write(np.full(TT.WD << po2, 0xdeadbeef, dtype=np.uint32))                 # every cell has a writer
    noise = NOISE + p
    out = hal.page_tree_witgen(prover.circuit, po2, zk, code, proof, words, before, after, first, count, data, noise)
    got = data.to_vec().reshape(TT.WD, n)
    bad = np.argwhere(got[:, :A] != want_data[:, :A])
    assert bad.size == 0, f"data: {len(bad)} cells differ, the first at (column, row) {tuple(bad[0])}"
    lib = zhal.load_library()
    kp = zhal.noise_key(noise).ctypes.data_as(C.POINTER(C.c_uint32))
    rows = sorted({A, A + 1, n - 1, *range(A, n, 97)})
    for col in (0, 95, p2_tree.D_ID, p2_tree.D_GACC, TT.D_CH, TT.D_WA - 1, TT.D_WA, TT.WD - 1):
        assert [int(got[col, r]) for r in rows] == [lib.zkh_noise_cell_host(kp, 2, col, r) for r in rows], f"blinding rows of column {col}"
    assert out.size == 18 and np.array_equal(out, want_out[:TT.PREFIX_WORDS]), "out is not the reference's first 18 words"


def _noise(seed, po2, zk):
    """the accum group's blinding rows as the library draws them: noise(column) -> rows [A, n)"""
    key, lib = zhal.noise_key(seed), zhal.load_library()
    n, A = 1 << po2, (1 << po2) - zk
    return lambda col: np.array([lib.zkh_noise_cell_host(zhal._ptr(key), 0, col, r) for r in range(A, n)], dtype=np.uint32)


def test_accumulate_open_is_the_reference_on_a_tied_tree_part(hal, prover):
    s, what, p = cases.H6, "all", 1                                               # a middle part: both of its edges are other parts'
    po2, zk, W_ = s
    data, want_accum, want_out, code = cases.part(po2, zk, W_, what, p)
    dcode, ddata = upload(hal, np.ascontiguousarray(code).reshape(-1), np.ascontiguousarray(data).reshape(-1))
    accum = hal.alloc_elem("accum", TT.WA << po2)
    total = hal.accumulate_open(prover.circuit, po2, zk, NOISE, dcode, ddata, CHALLENGE, accum)
    got = accum.to_vec().reshape(TT.WA, 1 << po2)
    A = (1 << po2) - zk
    bad = np.argwhere(got[:, :A] != want_accum[:, :A])
    assert bad.size == 0, f"{len(bad)} accum words differ, the first at (column, row) {tuple(bad[0])}"
    noise = _noise(NOISE, po2, zk)
    for col in (0, 23, 24, TT.WA - 1):
        assert np.array_equal(got[col, A:], noise(col)), f"blinding rows of accum column {col}"
    assert np.array_equal(total, want_out[TT.OUT_TOTAL:]) and total.any()
    first, count = tc.table(po2, zk, W_, what)["plan"][p]
    rows = tc.table(po2, zk, W_, what)["table"][first:first + count]
    assert not host.f4_add(total, logup.table_fingerprint(rows, CHALLENGE[:4], CHALLENGE[4:])).any()
    # the witness with the reference's `out` satisfies the circuit's own constraints on the device; the digest bus balances inside the part
    mix = np.zeros(TT.MIX_WORDS, dtype=np.uint32)
    assert hal.check_rows(prover.circuit, po2, accum, dcode, ddata, want_out, mix)["row"] == -1
    assert hal.check_bus(prover.circuit, po2, zk, dcode, ddata)["row"] == -1


# ------------------------------------------------------------------------------------------------ end to end
class Group:
    """one tied group on the device: the segment's traces derived from the image, the page-out's proof and trees, the provers"""

    def __init__(self, hal, page_prover):
        s = host.segment()
        self.hal, self.desc, self.table, self.page_prover = hal, s["desc"], s["table"], page_prover
        self.seg_prover = SegmentProver(hal, s["desc"], arguments=s["blob"])
        self.seg = Segment(index=0, po2=SEG_PO2, zk_cycles=SEG_ZK, noise_seed=NOISE)
        code, bare, _ = sl.witness(sl.TINY, SEG_PO2, SEG_ZK, seed=3, link=False, reads=True, pages=False, image=s["image"])
        self.host_code, self.host_data, self.host_image = code, bare, s["image"]
        self.code, self.data = self.traces(bare)
        self.image = image_buf(hal, s["image"])                                   # the page-out turns it, and its tree, into the image after
        self.after = hal.image_commit(self.image)
        self.proof, self.before = self.seg_prover.page_out(self.seg, self.data, self.image, tree=self.after, proof=True, keep_before=True)
        assert int(self.proof[4]) == H
        image_after = np.array(s["image"], dtype=np.uint32)
        for a, _, w_out in self.table:
            image_after[a] = w_out
        self.root_before, self.root_after = logup.reference_image_root(s["image"]), logup.reference_image_root(image_after)

    def traces(self, host_data):
        code, data = upload(self.hal, self.host_code, host_data)
        self.hal.derive_all_paged(self.seg_prover.circuit, SEG_PO2, SEG_ZK, code, data, image_buf(self.hal, self.host_image))
        self.hal.reduce_elem(code)
        self.hal.reduce_elem(data)
        return code, data

    def segs(self, shape, parts):
        return [Segment(index=1 + p, po2=shape[0], zk_cycles=shape[1], noise_seed=NOISE + 1 + p) for p in range(parts)]

    def seal(self, shape=TWO_PARTS, parts=2, data=None, proof=None, after=None, page_prover=None, **kw):
        proof = self.proof if proof is None else proof
        return seal_tied_tree(self.seg_prover, self.seg, self.code, self.data if data is None else data, np.zeros(4, dtype=np.uint32),
                              page_prover or self.page_prover, self.segs(shape, parts), proof, proof.size, self.before, self.after if after is None else after, **kw)

    def verify(self, seg_receipt, parts, h=H, **kw):
        return verify_tied_tree(seg_receipt, self.desc, seg_receipt.control_root, parts, parts[0].control_root, h, **kw)


@pytest.fixture(scope="module")
def group(hal, prover):
    # on the CPU, before anything is sealed: the segment's table touches all four pairs of leaves, 7 nodes, and (8, 40) has 6 block slots
    addrs = [a for a, _, _ in host.segment()["table"]]
    assert {a >> 4 for a in addrs} == {0, 1, 2, 3} and p2_tree.block_slots(*TWO_PARTS) == 6
    assert len(p2_tree.parts(*TWO_PARTS, W, addrs)) == 2 and len(p2_tree.parts(*ONE_PART, W, addrs)) == 1
    g = Group(hal, prover)
    g.receipts = g.seal(check=True)
    return g


def test_a_tied_tree_group_seals_and_verifies_from_root_to_root(hal, group):
    seg_receipt, parts = group.receipts
    assert len(parts) == 2 and any(i == o for _, i, o in group.table)
    for given in (group.root_before, None):
        root_before, root_after, hi = group.verify(seg_receipt, parts, root_before=given)
        assert np.array_equal(root_before, group.root_before) and np.array_equal(root_after, group.root_after) and hi == 1 << H
    assert not np.array_equal(group.root_before, group.root_after)
    page_hc = zhal.HostCircuit(TT.p2_tree_tied_circuit())
    for r in parts:                                                               # every seal also verifies alone, and states the group's challenge and h's base
        r.verify(TT.p2_tree_tied_circuit(), r.control_root)
        assert np.array_equal(r.seal[TT.OUT_ALPHA:TT.OUT_TOTAL], seg_receipt.seal[sl.OUT_ALPHA:sl.OUT_TOTAL]) and int(r.seal[TT.OUT_BASE]) == TT.out_base(H)
    roots = [zhal.HostCircuit(group.desc).seal_data_root(seg_receipt.seal)] + [page_hc.seal_data_root(r.seal) for r in parts]
    assert np.array_equal(zhal.tie_challenge(np.concatenate(roots)), seg_receipt.seal[sl.OUT_ALPHA:sl.OUT_TOTAL])
    # the same group in one part, planned where the table lies
    seg1, parts1 = group.seal(ONE_PART, 1, check=True, plan="device")
    assert len(parts1) == 1
    root_before, root_after, hi = group.verify(seg1, parts1, root_before=group.root_before)
    assert np.array_equal(root_before, group.root_before) and np.array_equal(root_after, group.root_after) and hi == 1 << H
    with pytest.raises(HalError, match=r"^verify_page_tree_chain: part 0 starts at lo 4, not 2\^3 = 8"):
        group.verify(seg1, parts1, h=H + 1)
    with pytest.raises(HalError, match=r"^seal_tied_tree: 1 segments, but a table of \d+ rows takes 2 parts of 6 block slots at po2 8$"):
        group.seal(TWO_PARTS, 1)


def _forged_page_out(hal, group):
    """a consistent page-out of ANOTHER table: one `out` word of row 1 altered in the proof's table, and the tree after it committed over
    the image with that word"""
    proof = group.proof.copy()
    at = 5 + H + 3 * 1 + 2
    proof[at] = (int(proof[at]) + ONE) % P
    image = group.image.to_vec()
    image[int(proof[5 + H + 3])] = proof[at]
    return proof, hal.image_commit(image_buf(hal, image))


def test_a_proof_of_another_table_is_refused_before_a_part_is_sealed_and_by_the_verifier_without_the_check(hal, group):
    proof, after = _forged_page_out(hal, group)
    with pytest.raises(HalError, match=r"^seal_tied_tree: the proof's table is not the segment's page table: the segment's open total is [0-9a-f ]+, the fingerprint of "
                                       rf"the proof's {len(group.table)} rows is [0-9a-f ]+$"):
        group.seal(proof=proof, after=after)
    seg_receipt, parts = group.seal(proof=proof, after=after, check_table=False)       # all seals are made: the forged page-out is consistent
    with pytest.raises(HalError, match=r"^verify_tied_tree: the totals do not cancel: the segment's F plus the parts' is [0-9a-f ]+, not zero"):
        group.verify(seg_receipt, parts)


def test_the_verifier_names_a_part_of_another_group_by_its_challenge(hal, group):
    seg_receipt, parts = group.receipts
    # the same group with one blinding word of the segment's data another: another data root, so another challenge; the parts' traces, and
    # so their data roots, are the same
    other = group.host_data.copy().reshape(-1, 1 << SEG_PO2)
    other[0, -1] = (int(other[0, -1]) + 1) % P
    _, data2 = group.traces(other.reshape(-1))
    seg2, parts2 = group.seal(data=data2)
    assert not np.array_equal(seg2.seal[sl.OUT_ALPHA:sl.OUT_TOTAL], seg_receipt.seal[sl.OUT_ALPHA:sl.OUT_TOTAL])
    group.verify(seg2, parts2)
    with pytest.raises(HalError, match=r"^verify_tied_tree: part 1: its challenge [0-9a-f ]+ is not the one the data roots give, [0-9a-f ]+$"):
        group.verify(seg_receipt, [parts[0], parts2[1]])


def test_the_parts_of_a_p2_page_tied_group_are_rejected(hal, group):
    seg_receipt, parts = group.receipts
    pager = SegmentProver(hal, p2_page_tied.p2_page_tied_circuit(), arguments=p2_page_tied.arguments())
    po2, zk = host.PAGE_PO2, host.PAGE_ZK
    seg_p, parts_p = seal_tied(group.seg_prover, group.seg, group.code, group.data, np.zeros(4, dtype=np.uint32), pager, group.segs((po2, zk), 3), group.proof,
                               group.proof.size, group.before, group.after)
    with pytest.raises(HalError, match="^verify_segment: "):
        group.verify(seg_p, parts_p)
    with pytest.raises(HalError, match="^verify_segment: "):                       # whichever control root the caller hands over
        verify_tied_tree(seg_p, group.desc, seg_p.control_root, parts_p, parts[0].control_root, H)


def test_a_p2_tree_prover_is_refused_for_having_no_open_bus(hal, group):
    plain = SegmentProver(hal, p2_tree.p2_tree_circuit(), arguments=p2_tree.arguments())
    with pytest.raises(HalError, match=r"^seal_tied_tree: the page-out prover's circuit has no open bus \(its arguments hold no OPEN record\)$"):
        group.seal(page_prover=plain)
    with pytest.raises(HalError, match=r'^seal_tied_tree: plan="gpu" \(the plan is made on the "host" or on the "device"\)$'):
        group.seal(plan="gpu")
