"""P2-PAGE on the GPU (zkh_page_circuit_code / zkh_page_circuit_witgen, csrc/page_circuit.hip; SegmentProver.seal_page_out): the device
generator against the Python reference word for word, its roots against the trees and the walk of the proof, the witness against the
circuit's constraints on the device, a seal that the host verifier accepts with out = both roots, and every refusal by its message.

The yardstick, p2_page.reference_page_trace, applies the updates one at a time to one tree; the device generator reads the memory an
update opens from the tree before and the tree after the page-out.  Shapes (page_circuit_cases.SHAPES): h = 1 (the leaf block is the
top, N = W = 16), h = 5 with a partial last leaf and padding leaves, h = 3; D in {0, 1, 3, N}; tables with two addresses in one leaf,
two in one pair of leaves, the last word of the image, a word of the partial leaf.  k_page_paths runs 2 N lanes in workgroups of 64:
N = 41 at (12, 200, 64) takes two workgroups, the other shapes one.

Mutants these cases are meant to catch: `<` for `<=` in the new side's choice of tree (one_leaf, one_pair: a later word of the same pair
must still be the old one); a sibling from the wrong tree (D = N: every sibling on a path lies between two updates); a no-op slot opened
under the tree before the page-out (D = 1, 3: the slots after the last update); `cur` of a slot taken from the wrong row; the partial
leaf's padding."""
import ctypes as C
import re

import numpy as np
import pytest

import page_circuit_cases as cases
import pages_cases as pc
from args_gpu import image_buf, upload
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, p2_join, p2_page as G
from zeth_amd.hal import HalError, HostCircuit
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu
P = cases.P
ONE = cases.ONE
BLOCK = G.BLOCK_ROWS
WIDE = (12, 200, 64)                                                         # N = 41: 82 lanes, two workgroups of the path kernel
GRID = [(s, d) for s in cases.SHAPES for d in (0, 1, 3, "N")] + [(cases.SHAPES[1], w) for w in ("one_leaf", "one_pair", "last", "first_last")] + [(WIDE, "N")]


@pytest.fixture(scope="module")
def prover(hal):
    p = SegmentProver(hal, G.p2_page_circuit())
    assert p.circuit.has_compiled_kernel()
    return p


def _device(hal, c):
    """the case on the device -> (proof buffer, proof words, nodes_before, nodes_after): the proof built on the host and uploaded, the
    two trees committed from the two images (word for word what zkh_page_out_tree leaves: tests/test_image_tree_gpu.py)"""
    before = hal.image_commit(image_buf(hal, c["image"]))
    after = hal.image_commit(image_buf(hal, c["image_after"]))
    proof = cases.host_proof(c["image"], c["addrs"], c["outs"], before.to_vec())
    return hal.copy_from("proof", proof), proof.size, before, after


def _witgen(hal, prover, c, dev=None):
    proof, words, before, after = dev or _device(hal, c)
    n = 1 << c["po2"]
    code = hal.page_circuit_code(prover.circuit, c["po2"], c["zk"], c["W"])
    data = hal.alloc_elem("data", G.WD * n)
    out = hal.page_circuit_witgen(prover.circuit, c["po2"], c["zk"], code, proof, words, before, after, data, cases.NOISE)
    return code, data, out


def _check_rows(hal, prover, c, code, data, out, seed=5):
    mix = np.random.default_rng(seed).integers(0, P, 4, dtype=np.uint64).astype(np.uint32)
    accum = hal.alloc_elem("accum", G.WA << c["po2"])
    hal.syn_accum(prover.circuit, c["po2"], c["zk"], cases.NOISE, data, mix, accum)
    return hal.check_rows(prover.circuit, c["po2"], accum, code, data, out, mix)


@pytest.mark.parametrize("shape,what", GRID, ids=[f"{s[0]}-{s[2]}-{d}" for s, d in GRID])
def test_witness_is_the_reference_word_for_word(hal, prover, shape, what):
    po2, zk, W = shape
    c = cases.case(po2, zk, W, what)
    n, A = 1 << po2, (1 << po2) - zk
    dev = _device(hal, c)
    code, data, out = _witgen(hal, prover, c, dev)
    assert np.array_equal(code.to_vec().reshape(G.WC, n), c["code"])
    got = data.to_vec().reshape(G.WD, n)
    bad = np.argwhere(got[:, :A] != c["data"][:, :A])
    assert bad.size == 0, f"{len(bad)} cells differ, the first at (column, row) {tuple(bad[0])}"
    # the blinding rows: the host twin of the noise generator, on the first and last rows and on a stride between them
    lib = zhal.load_library()
    key = zhal.noise_key(cases.NOISE)
    kp = key.ctypes.data_as(C.POINTER(C.c_uint32))
    rows = sorted({A, A + 1, n - 1, *range(A, n, 97)})
    for col in (0, 47, 48, 95, 96, 112, 116, 124):
        assert [int(got[col, r]) for r in rows] == [lib.zkh_noise_cell_host(kp, 2, col, r) for r in rows], f"blinding rows of column {col}"
    # the roots: the reference's, the trees', and what the walk of the proof gives
    proof, words, before, after = dev
    assert np.array_equal(out, c["out"])
    assert np.array_equal(out[:8], hal.image_root(before)) and np.array_equal(out[8:], hal.image_root(after))
    assert np.array_equal(hal.image_proof_walk(proof, out[:8], words=words), out[8:])
    r = _check_rows(hal, prover, c, code, data, out)
    assert r["row"] == -1 and r["failing_rows"] == 0, r


def test_seal_is_accepted_with_both_roots_and_rejected_with_another(hal, prover):
    c = cases.case(*cases.SHAPES[1], 3)
    proof, words, before, after = _device(hal, c)
    seg = Segment(index=0, po2=c["po2"], zk_cycles=c["zk"], noise_seed=cases.NOISE)
    rec = prover.seal_page_out(seg, proof, words, before, after, check=True)
    assert np.array_equal(rec.output, c["out"]) and np.array_equal(rec.seal[:16], c["out"])
    hc = HostCircuit(G.p2_page_circuit())
    hc.verify_segment(rec.seal, rec.control_root)
    bad = rec.seal.copy()
    bad[8] = (int(bad[8]) + 1) % P
    with pytest.raises(HalError):
        hc.verify_segment(bad, rec.control_root)
    # the control root is the code group's: another tree height is another circuit instance
    other = prover.code_root(hal.page_circuit_code(prover.circuit, c["po2"], c["zk"], 64), c["po2"])
    with pytest.raises(HalError):
        hc.verify_segment(rec.seal, other)


def test_the_whole_flow_on_the_device_from_a_paging_segment(hal, prover):
    """image -> image_commit -> a paging circuit's derived data -> page_out(proof, walk, keep_before) -> seal_page_out"""
    po2, zk = 8, 40
    desc, blob, code, data, image = pc.case("range5", 11, po2, zk)
    paged = SegmentProver(hal, desc, arguments=blob)
    dcode, ddata = upload(hal, code.reshape(-1), data.reshape(-1))
    dimage = image_buf(hal, image)
    tree = hal.image_commit(dimage)
    root_before = hal.image_root(tree)
    hal.derive_all_paged(paged.circuit, po2, zk, dcode, ddata, dimage)
    words, before = paged.page_out(Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=1), ddata, dimage, tree=tree, proof=True, walk=True, keep_before=True)
    assert np.array_equal(hal.image_root(before), root_before) and int(words[2]) == 5
    seg = Segment(index=1, po2=12, zk_cycles=1994, noise_seed=cases.NOISE)          # W = 1000: h = 7, N = 9 >= D = 5
    rec = prover.seal_page_out(seg, words, words.size, before, tree, check=True)
    assert np.array_equal(rec.output[:8], root_before) and np.array_equal(rec.output[8:], hal.image_root(tree))
    assert np.array_equal(rec.output[8:], zhal.image_proof_verify(words, root_before))
    HostCircuit(G.p2_page_circuit()).verify_segment(rec.seal, rec.control_root)
    with pytest.raises(HalError, match="keep_before=True needs proof=True"):
        paged.page_out(Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=1), ddata, dimage, tree=tree, keep_before=True)


def test_a_flipped_cell_is_named_inside_its_block(hal, prover):
    c = cases.case(*cases.SHAPES[1], 3)
    code, data, out = _witgen(hal, prover, c)
    n = 1 << c["po2"]
    block = c["h"] * 2 + 3                                                   # slot 2, block 3
    row, col = BLOCK * block + 12, G.D_SN + 7                                # a partial-round row of the new path
    cell = data.slice(col * n + row, 1)
    cell.write(np.array([(int(cell.to_vec()[0]) + 1) % P], dtype=np.uint32))
    r = _check_rows(hal, prover, c, code, data, out)
    assert BLOCK * block <= r["row"] < BLOCK * (block + 1) and r["row"] in (row, row + 1), r
    assert G.family_of(r["step"]) == "rounds"
    # a table that does not match the trees: the generator trusts it, the check names the opening
    proof, words, before, after = _device(hal, c)
    host = proof.to_vec()
    host[5 + c["h"] + 3 * 1 + 1] = (int(host[5 + c["h"] + 3 * 1 + 1]) + 1) % P         # row 1's `in`
    code, data, out = _witgen(hal, prover, c, (hal.copy_from("proof", host), words, before, after))
    r = _check_rows(hal, prover, c, code, data, out)
    assert r["row"] == BLOCK * c["h"] * 1 and G.family_of(r["step"]) == "leaf_in", r


def test_refusals(hal, prover):
    c = cases.case(*cases.SHAPES[1], 3)
    po2, zk, W, N, h = c["po2"], c["zk"], c["W"], c["N"], c["h"]
    n = 1 << po2
    proof, words, before, after = _device(hal, c)
    code = hal.page_circuit_code(prover.circuit, po2, zk, W)
    data = hal.alloc_elem("data", G.WD * n)
    data.write(np.full(G.WD * n, 0xdeadbeef, dtype=np.uint32))
    call = lambda **kw: hal.page_circuit_witgen(kw.get("circuit", prover.circuit), po2, zk, kw.get("code", code), kw.get("proof", proof), kw.get("words", words),
                                                before, kw.get("after", after), kw.get("data", data), cases.NOISE)
    untouched = lambda: bool((data.to_vec() == 0xdeadbeef).all())
    # D = N + 1
    image = c["image"]
    addrs = np.arange(N + 1, dtype=np.int64) * 2
    many = cases.host_proof(image, addrs, image[addrs] % np.uint32(P), before.to_vec())
    with pytest.raises(HalError, match=re.escape(f"page_circuit_witgen: D {N + 1} updates, but h {h} at po2 {po2} leaves N {N} path slots")):
        call(proof=hal.copy_from("proof", many), words=many.size)
    # W = 8
    img8 = np.arange(1, 9, dtype=np.uint32)
    nodes8 = hal.image_commit(image_buf(hal, img8))
    one = cases.host_proof(img8, np.array([3]), np.array([7], dtype=np.uint32), nodes8.to_vec())
    with pytest.raises(HalError, match=re.escape("page_circuit_witgen: an image of 8 words has a single leaf")):
        call(proof=hal.copy_from("proof", one), words=one.size)
    with pytest.raises(HalError, match=re.escape("page_circuit_code: an image of 8 words has a single leaf")):
        hal.page_circuit_code(prover.circuit, po2, zk, 8)
    # a wrong-sized nodes_after
    with pytest.raises(HalError, match=re.escape(f"page_circuit_witgen: nodes of {before.size()} and {2 * before.size()} words; an image of {W} words has a tree of {before.size()}")):
        call(after=hal.alloc("nodes", 2 * before.size()))
    # buffer shapes; a proof whose header does not fit its length (the walk's message)
    with pytest.raises(HalError, match=re.escape("page_circuit_witgen: buffer shape mismatch")):
        call(data=hal.alloc_elem("data", G.WD * n - 1))
    with pytest.raises(HalError, match=re.escape(f"page_circuit_witgen: a proof of {words - 1} words, but the header describes {words}")):
        call(words=words - 1)
    # a circuit that is not P2-PAGE
    join = hal.load_circuit(p2_join.p2_join_circuit())
    with pytest.raises(HalError, match=re.escape("page_circuit_witgen: the circuit does not have P2-PAGE's shape")):
        call(circuit=join)
    assert untouched(), "a refusal before any launch wrote into the data group"
    # a code group built for another h (h = 3: W = 64): reported after the launches, which read nothing out of bounds
    with pytest.raises(HalError, match=re.escape(f"page_circuit_witgen: the code group was not built for h {h}")):
        call(code=hal.page_circuit_code(prover.circuit, po2, zk, 64))
    # addresses that do not increase / lie outside the image: the check pass refuses, no path is walked
    host = proof.to_vec()
    t0 = 5 + h
    swapped = host.copy()
    swapped[t0], swapped[t0 + 3] = host[t0 + 3], host[t0]
    a0, a1 = int(host[t0]), int(host[t0 + 3])
    with pytest.raises(HalError, match=re.escape(f"page_circuit_witgen: row 1: address {a0} does not follow a smaller one (row 0: address {a1})")):
        call(proof=hal.copy_from("proof", swapped))
    outside = host.copy()
    outside[t0 + 6] = 0xfffffff0
    data.write(np.full(G.WD * n, 0xdeadbeef, dtype=np.uint32))
    with pytest.raises(HalError, match=re.escape(f"page_circuit_witgen: row 2: address {0xfffffff0} outside the image of {W} words")):
        call(proof=hal.copy_from("proof", outside))
    assert (data.to_vec().reshape(G.WD, n)[:G.D_E, :BLOCK * h * N] == 0xdeadbeef).all(), "a path was walked after the check pass refused"
    # and the good call right after them
    assert np.array_equal(call(), c["out"])
