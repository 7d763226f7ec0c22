"""A tied group from the proof alone, and a paged run (page_seal.seal_tied_tree_from_proof, preflight_paged_run, seal_paged_step,
verify_paged_run).  The tiny tied segment of tied_cases (po2 8 over an image of 64 words, h = 3) with its page-out at (8, 40), two parts,
and at (10, 500), one part: the group sealed from (the underived traces, the proof, root_before), by calls that are handed no image and
no tree, must be byte for byte the group that `seal_tied_tree` makes on the path that holds the image.  Then three such segments over
one image: preflight once, the steps sealed in reverse order, and the host-only verifier takes the groups from root_0 to root_3."""
import re

import numpy as np
import pytest

import tied_cases as host
from args_gpu import image_buf, upload
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, p2_tree_tied as TT, syn_lookup as sl
from zeth_amd.hal import Buffer, HalError
from zeth_amd.prover import (Segment, SegmentProver, preflight_paged_run, seal_paged_step, seal_tied_tree, seal_tied_tree_from_proof, verify_paged_run,
                             verify_tied_tree)

pytestmark = pytest.mark.gpu
P, ONE = host.P, host.ONE
NOISE = 0x7EED
SEG_PO2, SEG_ZK, W = host.SEG_PO2, host.SEG_ZK, host.W
H = 3
TWO_PARTS, ONE_PART = (8, 40), (10, 500)
PREFIX = np.zeros(4, dtype=np.uint32)


def _page_segs(shape, parts, first=1):
    return [Segment(index=first + p, po2=shape[0], zk_cycles=shape[1], noise_seed=NOISE + first + p) for p in range(parts)]


class Group:
    """the tied segment on the rank that holds the image: its traces derived from the image, its page-out's proof and dirty nodes"""

    def __init__(self, hal):
        s = host.segment()
        self.hal, self.desc = hal, s["desc"]
        self.seg_prover = SegmentProver(hal, s["desc"], arguments=s["blob"])
        self.page_prover = SegmentProver(hal, TT.p2_tree_tied_circuit(), arguments=TT.arguments())
        self.seg = Segment(index=0, po2=SEG_PO2, zk_cycles=SEG_ZK, noise_seed=NOISE)
        self.host_code, self.host_data, _ = sl.witness(sl.TINY, SEG_PO2, SEG_ZK, seed=3, link=False, reads=True, pages=False, image=s["image"])
        self.code, self.data = upload(hal, self.host_code, self.host_data)
        image = image_buf(hal, s["image"])
        hal.derive_all_paged(self.seg_prover.circuit, SEG_PO2, SEG_ZK, self.code, self.data, image)
        hal.reduce_elem(self.code)
        hal.reduce_elem(self.data)
        self.tree = hal.image_commit(image)
        self.proof, self.dirty = self.seg_prover.page_out(self.seg, self.data, image, tree=self.tree, proof=True, dirty=True)
        self.root_before = logup.reference_image_root(s["image"])

    def from_proof(self, shape, parts, proof=None, root_before=None, **kw):
        return seal_tied_tree_from_proof(self.seg_prover, self.seg, self.host_code, self.host_data, PREFIX, self.page_prover, _page_segs(shape, parts),
                                         self.proof if proof is None else proof, self.root_before if root_before is None else root_before, **kw)


@pytest.fixture(scope="module")
def group(hal):
    return Group(hal)


@pytest.mark.parametrize("shape,parts,plan", [(TWO_PARTS, 2, "host"), (ONE_PART, 1, "device")], ids=["two_parts", "one_part"])
def test_the_group_from_the_proof_alone_is_the_group_of_the_rank_that_holds_the_image(hal, group, shape, parts, plan):
    seg_a, parts_a = seal_tied_tree(group.seg_prover, group.seg, group.code, group.data, PREFIX, group.page_prover, _page_segs(shape, parts), group.proof,
                                    group.proof.size, None, None, check=True, plan=plan, dirty=group.dirty)
    seg_b, parts_b, root_after = group.from_proof(shape, parts, check=True, plan=plan)
    assert len(parts_a) == len(parts_b) == parts
    assert np.array_equal(seg_a.seal, seg_b.seal), "the segment's seal differs"
    for p, (a, b) in enumerate(zip(parts_a, parts_b)):
        assert np.array_equal(a.seal, b.seal), f"part {p}: the seal differs"
        assert np.array_equal(a.control_root, b.control_root)
    rb, ra, hi = verify_tied_tree(seg_b, group.desc, seg_b.control_root, parts_b, parts_b[0].control_root, H, root_before=group.root_before)
    assert np.array_equal(rb, group.root_before) and np.array_equal(ra, root_after) and np.array_equal(ra, hal.image_root(group.tree)) and hi == 1 << H
    # the segments of the parts as a callable, asked once per part of the plan
    asked = []
    segs = _page_segs(shape, parts)
    seg_c, parts_c, _ = seal_tied_tree_from_proof(group.seg_prover, group.seg, group.host_code, group.host_data, PREFIX, group.page_prover,
                                                  lambda p: asked.append(p) or segs[p], group.proof, group.root_before, plan=plan)
    assert asked == list(range(parts)) and np.array_equal(seg_c.seal, seg_a.seal) and all(np.array_equal(a.seal, c.seal) for a, c in zip(parts_a, parts_c))


def test_a_proof_that_does_not_open_the_root_is_refused_before_anything_is_derived(hal, group):
    proof = group.proof.copy()
    proof[5 + H + 3 * 1 + 1] = (int(proof[5 + H + 3 * 1 + 1]) + ONE) % P      # the `in` word of row 1
    with pytest.raises(HalError) as e:
        zhal.image_proof_verify(proof, group.root_before)
    said = str(e.value).split(": ", 1)[1]
    hal.prof_enable(True)
    hal.prof_reset()
    with pytest.raises(HalError, match="^" + re.escape("image_proof_nodes: " + said) + "$"):
        group.from_proof(TWO_PARTS, 2, proof=proof)
    other = group.root_before.copy()
    other[0] = (int(other[0]) + 1) % P
    with pytest.raises(HalError, match=r"^image_proof_nodes: the proof opens root .+, not root_before"):
        group.from_proof(TWO_PARTS, 2, root_before=other)
    ran = {r["name"] for r in hal.prof_get() if r["calls"]}
    hal.prof_enable(False)
    assert not ran & {"sort_keys", "links_check", "links_write"}, ran


# ------------------------------------------------------------------------------------------------ a run
class Run:
    """three segments over one image of 64 words, on the CPU: the witnesses, and the image before and after every segment"""

    def __init__(self):
        self.desc, self.blob = sl.syn_lookup_tiny_tied()
        args = logup.Arguments.parse(self.blob)
        n, A = 1 << SEG_PO2, (1 << SEG_PO2) - SEG_ZK
        image = np.random.default_rng(3).integers(1, P, W, dtype=np.uint64).astype(np.uint32)
        self.images, self.witnesses, self.rows = [image], [], []
        for seed in (3, 4, 5):
            code, bare, _ = sl.witness(sl.TINY, SEG_PO2, SEG_ZK, seed=seed, link=False, reads=True, pages=False, image=image)
            _, full, _ = sl.witness(sl.TINY, SEG_PO2, SEG_ZK, seed=seed, link=True, reads=True, pages=True, image=image)
            d, pg = full.reshape(-1, n), args.pages
            on = d[pg.p_on, :A] == ONE
            addrs = logup._dec(d[pg.p_addr, :A][on]).astype(np.int64)
            image = image.copy()
            image[addrs] = d[pg.p_out, :A][on]
            self.witnesses.append((code, bare))
            self.rows.append(int(on.sum()))
            self.images.append(image)
        self.roots = [logup.reference_image_root(i) for i in self.images]
        self.segs = [Segment(index=10 * k, po2=SEG_PO2, zk_cycles=SEG_ZK, noise_seed=NOISE + 100 * k) for k in range(3)]


def test_a_run_of_three_segments_over_one_image(hal):
    run = Run()
    assert all(D > 0 for D in run.rows) and run.rows == [63, 61, 64]
    assert all(not np.array_equal(run.roots[k], run.roots[k + 1]) for k in range(3))
    seg_prover = SegmentProver(hal, run.desc, arguments=run.blob)
    page_prover = SegmentProver(hal, TT.p2_tree_tied_circuit(), arguments=TT.arguments())
    image = image_buf(hal, run.images[0])
    tree = hal.image_commit(image)
    steps = preflight_paged_run(seg_prover, run.segs, run.witnesses, image, tree)
    assert np.array_equal(image.to_vec() % P, run.images[3] % P) and np.array_equal(tree.to_vec(), logup.reference_image_tree(run.images[3]).reshape(-1))
    assert [int(s.proof[2]) for s in steps] == run.rows
    for k, s in enumerate(steps):
        assert np.array_equal(s.root_before, run.roots[k]) and np.array_equal(s.root_after, run.roots[k + 1])
        assert not any(isinstance(v, Buffer) for v in vars(s).values()), "a step ships no device buffer"
    del image, tree                                                          # the seals are handed neither
    groups = [None] * 3
    for k in (2, 1, 0):
        groups[k] = seal_paged_step(steps[k], seg_prover, PREFIX, page_prover, lambda p, k=k: Segment(index=10 * k + 1 + p, po2=TWO_PARTS[0], zk_cycles=TWO_PARTS[1],
                                                                                                        noise_seed=NOISE + 100 * k + 1 + p))
    seg_root, page_root = groups[0][0].control_root, groups[0][1][0].control_root
    verify = lambda gs, **kw: verify_paged_run(gs, run.desc, seg_root, page_root, H, **kw)
    for given in (None, run.roots[0]):
        first, last = verify(groups, root_before=given)
        assert np.array_equal(first, run.roots[0]) and np.array_equal(last, run.roots[3])
    with pytest.raises(HalError, match=r"^verify_paged_run: group 1 opens root [0-9a-f ]+, but group 0 left root [0-9a-f ]+$"):
        verify([groups[1], groups[0], groups[2]])
    with pytest.raises(HalError, match=r"^verify_paged_run: group 1 opens root [0-9a-f ]+, but group 0 left root [0-9a-f ]+$"):
        verify([groups[0], groups[2]])
    with pytest.raises(HalError, match=r"^verify_paged_run: group 0 opens root [0-9a-f ]+, not root_before [0-9a-f ]+$"):
        verify(groups, root_before=run.roots[1])
    with pytest.raises(HalError, match=r"^verify_paged_run: no group$"):
        verify([])
