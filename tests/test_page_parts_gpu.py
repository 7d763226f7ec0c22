"""P2-PAGE's parts on the GPU (zkh_page_circuit_witgen_part, csrc/page_circuit.hip; SegmentProver.seal_page_out_parts,
prover.verify_page_out_chain): a page table of D > N rows sealed as a chain of traces.  Per part: the device witness against
p2_page.reference_page_part word for word, its two roots against the reference's and against the committed tree of the image with the
updates before the part, and through the part, applied (hal.image_commit), and the witness against the circuit's constraints on the
device.  Then the chain of seals, the existing entry point as the part at 0, the whole flow from a paging segment, and the refusals.

The yardstick applies the updates before the part to the image in numpy and then one update at a time to one tree; the device reads
both trees of the WHOLE page-out for every part and walks the root before the part as h bare hash_pairs (k_page_root).

Shapes, the smallest at which the new code can go wrong:
  (10, 900, 16)        h = 1, N = 4,  every word: 4 full parts; the leaf block is the top, every boundary splits one pair of leaves
  (12, 1994, 8*17+3)   h = 5, N = 13, 30 random addresses: 13, 13, 4; a partial last leaf, no-ops only in the last part
  (12, 1994, 64)       h = 3, N = 22, every word: 22, 22, 20; updates first - 1 and first share a leaf
  (12, 200, 64)        h = 3, N = 41, every word: 41, 23; two workgroups of the path kernel
and at the h = 5 shape a table of D = 3 rows at first = 1 (a part that is not on a multiple of N) and at first = 0 (the existing entry
point's witness word for word).

Mutants these are meant to catch: slot 0's `cur` taken from `nodes_before` when first > 0 (every part after the first); `slot < D` for
`first + slot < D` in the path or the bookkeeping kernel (the last part at h = 5: slots 4 .. 12 are no-ops); the table's row taken as
`slot` (every part after the first); `<` for `<=` in the root walk's choice of tree (the update's own word must be the new one); a
sibling from the wrong tree in the root walk (every word paged: each left sibling has been written, each right one will be).  Each of
these was built and run against this file, but the path kernel's `slot < D` (it would index a tree with a word that is no address):
between 6 and 8 of the 8 tests fail on every one of them."""
import ctypes as C
import re

import numpy as np
import pytest

import page_circuit_cases as cases
import page_parts_cases as pp
import pages_cases as pc
from args_gpu import image_buf, upload
from zeth_amd import hal as zhal
from zeth_amd.circuits import p2_page as G
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver, SegmentReceipt, verify_page_out_chain

pytestmark = pytest.mark.gpu
P = cases.P
BLOCK = G.BLOCK_ROWS
GRID = [((10, 900, 16), "all", [4, 4, 4, 4]), (pp.H5, 30, [13, 13, 4]), ((12, 1994, 64), "all", [22, 22, 20]), ((12, 200, 64), "all", [41, 23])]


@pytest.fixture(scope="module")
def prover(hal):
    p = SegmentProver(hal, G.p2_page_circuit())
    assert p.circuit.has_compiled_kernel()
    return p


def _device(hal, t):
    """the table on the device -> (proof buffer, proof words, nodes_before, nodes_after): the trees of the WHOLE page-out"""
    before = hal.image_commit(image_buf(hal, t["image"]))
    after = hal.image_commit(image_buf(hal, t["image_after"]))
    proof = cases.host_proof(t["image"], t["addrs"], t["outs"], before.to_vec())
    assert int(proof[2]) == len(t["addrs"])
    return hal.copy_from("proof", proof), proof.size, before, after


def _root_of(hal, image):
    return hal.image_root(hal.image_commit(image_buf(hal, image)))


def _check_part(hal, prover, t, dev, code, data, first, want_data, want_out, noise):
    """one part on the device against the reference: witness, blinding rows, roots, constraints"""
    po2, zk = t["po2"], t["zk"]
    n, A = 1 << po2, (1 << po2) - zk
    proof, words, before, after = dev
    out = hal.page_circuit_witgen_part(prover.circuit, po2, zk, code, proof, words, before, after, first, data, noise)
    got = data.to_vec().reshape(G.WD, n)
    bad = np.argwhere(got[:, :A] != want_data[:, :A])
    assert bad.size == 0, f"first {first}: {len(bad)} cells differ, the first at (column, row) {tuple(bad[0])}"
    lib = zhal.load_library()
    kp = zhal.noise_key(noise).ctypes.data_as(C.POINTER(C.c_uint32))
    rows = sorted({A, A + 1, n - 1, *range(A, n, 97)})
    for col in (0, 47, 48, 95, 96, 112, 116, 124):
        assert [int(got[col, r]) for r in rows] == [lib.zkh_noise_cell_host(kp, 2, col, r) for r in rows], f"first {first}: blinding rows of column {col}"
    count = min(t["N"], len(t["addrs"]) - first)
    assert np.array_equal(out, want_out), f"first {first}: out_roots are not the reference's"
    assert np.array_equal(out[:8], _root_of(hal, pp.image_at(t, first))), f"first {first}: the root before the part"
    assert np.array_equal(out[8:], _root_of(hal, pp.image_at(t, first + count))), f"first {first}: the root after the part"
    mix = np.random.default_rng(5).integers(0, P, 4, dtype=np.uint64).astype(np.uint32)
    accum = hal.alloc_elem("accum", G.WA << po2)
    hal.syn_accum(prover.circuit, po2, zk, noise, data, mix, accum)
    r = hal.check_rows(prover.circuit, po2, accum, code, data, out, mix)
    assert r["row"] == -1 and r["failing_rows"] == 0, (first, r)
    return out


@pytest.mark.parametrize("shape,what,counts", GRID, ids=[f"{s[0]}-{s[1]}-{s[2]}" for s, _, _ in GRID])
def test_every_part_is_the_reference_word_for_word(hal, prover, shape, what, counts):
    po2, zk, W = shape
    t = pp.table(po2, zk, W, what)
    assert [c for _, c in t["plan"]] == counts and hal.page_circuit_slots(po2, zk, W) == t["N"] == counts[0]
    dev = _device(hal, t)
    code = hal.page_circuit_code(prover.circuit, po2, zk, W)
    assert np.array_equal(code.to_vec().reshape(G.WC, 1 << po2), G.reference_page_code(po2, zk, t["h"]))
    data = hal.alloc_elem("data", G.WD << po2)                                # one buffer for every part, as seal_page_out_parts uses it
    outs = []
    for p, (first, _) in reversed(list(enumerate(t["plan"]))):               # in any order: here the last part first
        want_data, want_out = pp.part(po2, zk, W, what, first)
        outs.append(_check_part(hal, prover, t, dev, code, data, first, want_data, want_out, cases.NOISE + p))
    outs.reverse()
    assert all(np.array_equal(outs[p][8:], outs[p + 1][:8]) for p in range(len(outs) - 1))
    assert np.array_equal(outs[0][:8], hal.image_root(dev[2])) and np.array_equal(outs[-1][8:], hal.image_root(dev[3]))


def test_a_part_that_is_not_on_a_multiple_of_n_and_the_part_at_0(hal, prover):
    po2, zk, W = pp.H5
    c = cases.case(po2, zk, W, 3)                                            # D = 3 < N = 13
    t = {k: c[k] for k in ("po2", "zk", "W", "h", "N", "image", "addrs", "outs", "image_after")}
    dev = _device(hal, t)
    proof, words, before, after = dev
    n = 1 << po2
    code = hal.page_circuit_code(prover.circuit, po2, zk, W)
    data = hal.alloc_elem("data", G.WD * n)
    # first = 1: updates 1 and 2, then eleven no-ops; it opens the tree with update 0 applied
    active, root_before, root_after = G.reference_page_part(po2, zk, W, c["table"], c["image"], 1)
    want = np.zeros((G.WD, n), dtype=np.uint32)
    want[:, :n - zk] = active
    out = _check_part(hal, prover, t, dev, code, data, 1, want, np.concatenate([root_before, root_after]).astype(np.uint32), cases.NOISE)
    assert not np.array_equal(out[:8], hal.image_root(before)) and np.array_equal(out[8:], hal.image_root(after))
    # first = 0 is the existing entry point, word for word: active rows, blinding rows and roots
    whole = hal.alloc_elem("data", G.WD * n)
    out_whole = hal.page_circuit_witgen(prover.circuit, po2, zk, code, proof, words, before, after, whole, cases.NOISE)
    out_part = hal.page_circuit_witgen_part(prover.circuit, po2, zk, code, proof, words, before, after, 0, data, cases.NOISE)
    assert np.array_equal(out_part, out_whole) and np.array_equal(out_whole, c["out"])
    assert np.array_equal(data.to_vec(), whole.to_vec())
    assert np.array_equal(whole.to_vec().reshape(G.WD, n)[:, :n - zk], c["data"][:, :n - zk])


def _fmt(r):
    return " ".join(f"{int(w):08x}" for w in r)


def test_the_chain_of_seals_gives_the_two_trees_roots(hal, prover):
    po2, zk, W = pp.H5
    t = pp.table(po2, zk, W, 30)
    proof, words, before, after = _device(hal, t)
    segs = [Segment(index=p, po2=po2, zk_cycles=zk, noise_seed=cases.NOISE + p) for p in range(3)]
    recs = prover.seal_page_out_parts(segs, proof, words, before, after, check=True)
    assert len(recs) == 3 and [r.index for r in recs] == [0, 1, 2]
    for r, (first, _) in zip(recs, t["plan"]):
        assert np.array_equal(r.output, pp.part(po2, zk, W, 30, first)[1]) and np.array_equal(r.seal[:16], r.output)
    root = prover.code_root(hal.page_circuit_code(prover.circuit, po2, zk, W), po2)
    assert all(np.array_equal(r.control_root, root) for r in recs)
    root_before, root_after = hal.image_root(before), hal.image_root(after)
    got = verify_page_out_chain(recs, root, root_before)
    assert np.array_equal(got[0], root_before) and np.array_equal(got[1], root_after)
    got = verify_page_out_chain(recs, root)
    assert np.array_equal(got[0], root_before) and np.array_equal(got[1], root_after)
    assert np.array_equal(zhal.image_proof_verify(proof.to_vec()[:words], root_before), root_after)
    # two receipts swapped: every seal is good, the chain is not
    with pytest.raises(HalError, match=re.escape(f"part 1 opens root {_fmt(recs[0].seal[:8])}, but part 0 left root {_fmt(recs[1].seal[8:16])}")):
        verify_page_out_chain([recs[1], recs[0], recs[2]], root)
    with pytest.raises(HalError, match=re.escape(f"part 1 opens root {_fmt(recs[2].seal[:8])}, but part 0 left root {_fmt(recs[0].seal[8:16])}")):
        verify_page_out_chain([recs[0], recs[2], recs[1]], root)
    with pytest.raises(HalError, match=re.escape(f"part 0 opens root {_fmt(root_before)}, not root_before {_fmt(root_after)}")):
        verify_page_out_chain(recs, root, root_after)
    # one seal's `out` tampered with: the verifier of that seal refuses; so does another control root
    bad = recs[1].seal.copy()
    bad[8] = (int(bad[8]) + 1) % P
    tampered = [recs[0], SegmentReceipt(seal=bad, index=1, po2=po2), recs[2]]
    with pytest.raises(HalError):
        verify_page_out_chain(tampered, root)
    with pytest.raises(HalError):
        verify_page_out_chain(recs, prover.code_root(hal.page_circuit_code(prover.circuit, po2, zk, 64), po2))
    with pytest.raises(HalError, match="no receipt"):
        verify_page_out_chain([], root)
    # a `segs` of the wrong length names both numbers; so does one of mixed sizes
    with pytest.raises(HalError, match=re.escape("seal_page_out_parts: 2 segments, but a table of 30 rows takes 3 parts of 13 slots")):
        prover.seal_page_out_parts(segs[:2], proof, words, before, after)
    with pytest.raises(HalError, match=re.escape("seal_page_out_parts: 4 segments, but a table of 30 rows takes 3 parts")):
        prover.seal_page_out_parts(segs + [Segment(index=3, po2=po2, zk_cycles=zk, noise_seed=9)], proof, words, before, after)
    with pytest.raises(HalError, match="the same"):
        prover.seal_page_out_parts(segs[:2] + [Segment(index=2, po2=po2 + 1, zk_cycles=zk, noise_seed=9)], proof, words, before, after)
    # the one-seal entry point still refuses this table
    with pytest.raises(HalError, match=re.escape(f"page_circuit_witgen: D 30 updates, but h 5 at po2 {po2} leaves N 13 path slots")):
        prover.seal_page_out(segs[0], proof, words, before, after)


def test_the_whole_flow_from_a_paging_segment_in_parts(hal, prover):
    """image -> image_commit -> a paging circuit's derived data -> page_out(proof, keep_before) -> seal_page_out_parts -> the chain"""
    po2, zk = 8, 40
    desc, blob, code, data, image = pc.case("range5", 11, po2, zk)
    paged = SegmentProver(hal, desc, arguments=blob)
    dcode, ddata = upload(hal, code.reshape(-1), data.reshape(-1))
    dimage = image_buf(hal, image)
    tree = hal.image_commit(dimage)
    root_before = hal.image_root(tree)
    hal.derive_all_paged(paged.circuit, po2, zk, dcode, ddata, dimage)
    words, before = paged.page_out(Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=1), ddata, dimage, tree=tree, proof=True, keep_before=True)
    W, D = int(words[1]), int(words[2])
    ppo2, pzk = 12, 3100                                                     # W = 1000: h = 7; 996 active rows: N = 4 < D = 5
    assert D == 5 and G.parts(ppo2, pzk, W, D) == [(0, 4), (4, 1)] == [(f, min(4, D - f)) for f in range(0, D, hal.page_circuit_slots(ppo2, pzk, W))]
    segs = [Segment(index=1 + p, po2=ppo2, zk_cycles=pzk, noise_seed=cases.NOISE + p) for p in range(2)]
    recs = prover.seal_page_out_parts(segs, words, words.size, before, tree, check=True)
    got = verify_page_out_chain(recs, recs[0].control_root, root_before)
    assert np.array_equal(got[0], root_before) and np.array_equal(got[1], hal.image_root(tree))
    assert np.array_equal(got[1], zhal.image_proof_verify(words, root_before))
    assert np.array_equal(recs[0].output[:8], root_before) and np.array_equal(recs[0].output[8:], recs[1].output[:8])


def test_refusals(hal, prover):
    po2, zk, W = pp.H5
    t = pp.table(po2, zk, W, 30)
    N, h, n = t["N"], t["h"], 1 << po2
    proof, words, before, after = _device(hal, t)
    code = hal.page_circuit_code(prover.circuit, po2, zk, W)
    data = hal.alloc_elem("data", G.WD * n)
    data.write(np.full(G.WD * n, 0xdeadbeef, dtype=np.uint32))
    call = lambda first, **kw: hal.page_circuit_witgen_part(prover.circuit, po2, zk, code, kw.get("proof", proof), kw.get("words", words), before,
                                                            kw.get("after", after), first, kw.get("data", data), cases.NOISE)
    for first in (30, 31):
        with pytest.raises(HalError, match=re.escape(f"page_circuit_witgen_part: first {first}, but the table has 30 rows")):
            call(first)
    # an empty table has one part, at 0; first = 1 is past it
    empty = cases.host_proof(t["image"], t["addrs"][:0], t["outs"][:0], before.to_vec())
    with pytest.raises(HalError, match=re.escape("page_circuit_witgen_part: first 1, but the table has 0 rows")):
        call(1, proof=hal.copy_from("proof", empty), words=empty.size, after=before)
    # the shared refusals carry this entry point's name
    with pytest.raises(HalError, match=re.escape("page_circuit_witgen_part: buffer shape mismatch")):
        call(13, data=hal.alloc_elem("data", G.WD * n - 1))
    with pytest.raises(HalError, match=re.escape(f"page_circuit_witgen_part: nodes of {before.size()} and {2 * before.size()} words")):
        call(13, after=hal.alloc("nodes", 2 * before.size()))
    assert bool((data.to_vec() == 0xdeadbeef).all()), "a refusal before any launch wrote into the data group"
    # two rows swapped in part 0, the call lays out part 1: the check pass covers the whole table and names the row by its index there
    host = proof.to_vec()
    t0 = 5 + h
    swapped = host.copy()
    swapped[t0], swapped[t0 + 3] = host[t0 + 3], host[t0]
    a0, a1 = int(host[t0]), int(host[t0 + 3])
    with pytest.raises(HalError, match=re.escape(f"page_circuit_witgen_part: row 1: address {a0} does not follow a smaller one (row 0: address {a1})")):
        call(13, proof=hal.copy_from("proof", swapped))
    outside = host.copy()
    outside[t0 + 3 * 29] = 0xfffffff0                                        # the last row, in part 2
    with pytest.raises(HalError, match=re.escape(f"page_circuit_witgen_part: row 29: address {0xfffffff0} outside the image of {W} words")):
        call(13, proof=hal.copy_from("proof", outside))
    assert (data.to_vec().reshape(G.WD, n)[:G.D_E, :BLOCK * h * N] == 0xdeadbeef).all(), "a path was walked after the check pass refused"
    # and the good calls right after them: the empty table's part, then the middle part
    out = call(0, proof=hal.copy_from("proof", empty), words=empty.size, after=before)
    assert np.array_equal(out[:8], hal.image_root(before)) and np.array_equal(out[8:], out[:8])
    assert np.array_equal(call(13), pp.part(po2, zk, W, 30, 13)[1])
