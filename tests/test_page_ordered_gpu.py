"""P2-PAGE-ordered on the GPU (zkh_page_ordered_code / zkh_page_ordered_witgen, csrc/page_circuit.hip; SegmentProver.seal_page_out_ordered,
prover.verify_page_ordered_chain).  The device code group and witness against p2_page_ordered's references word for word over
page_ordered_cases.GRID and a shape whose path kernel takes two workgroups, the blinding rows of the new columns, `out`, and the witness
against the circuit's constraints on the device; a chain of three seals and what its verifier refuses; and the refusals of the two
calls, by message, with the good call right after them.

The yardstick applies the updates one at a time to one tree and fills the new columns in plain numpy over the table; the device reads
both trees of the whole page-out and writes the new columns with one lane per (path row, column).

Shapes, the smallest at which the new code can go wrong: (10, 500, 16) has 496 path rows, two workgroups of k_page_order, the second
partial; (12, 1994, 2^14 + 3) reaches gap bits up to 2^13; `adjacent` has gaps of 0; the parts at first = 13 and 26 of a table of 29 rows
take lo from the row before the part, and the last has dead slots, whose lo is one more than the table's last address."""
import ctypes as C
import re

import numpy as np
import pytest

import page_circuit_cases as cases
import page_ordered_cases as oc
from args_gpu import image_buf
from zeth_amd import hal as zhal
from zeth_amd.circuits import p2_page, p2_page_ordered as G
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver, SegmentReceipt, verify_page_ordered_chain

pytestmark = pytest.mark.gpu
P = cases.P
BLOCK = p2_page.BLOCK_ROWS
GRID = oc.GRID + [(oc.WIDE, "N", 0), (oc.WIDE, 3, 0)]
H5 = cases.SHAPES[1]


@pytest.fixture(scope="module")
def prover(hal):
    p = SegmentProver(hal, G.p2_page_ordered_circuit())
    assert p.circuit.has_compiled_kernel()
    return p


def _device(hal, t):
    """the table on the device -> (proof buffer, proof words, nodes_before, nodes_after): the trees of the WHOLE page-out"""
    before = hal.image_commit(image_buf(hal, t["image"]))
    after = hal.image_commit(image_buf(hal, t["image_after"]))
    proof = cases.host_proof(t["image"], t["addrs"], t["outs"], before.to_vec())
    assert int(proof[2]) == len(t["addrs"])
    return hal.copy_from("proof", proof), proof.size, before, after


@pytest.mark.parametrize("g", GRID, ids=oc.grid_id)
def test_the_generator_is_the_reference_word_for_word(hal, prover, g):
    (po2, zk, W), what, first = g
    t = oc.table(po2, zk, W, what)
    want_data, want_out, want_code = oc.part(po2, zk, W, what, first)
    n, A = 1 << po2, (1 << po2) - zk
    proof, words, before, after = _device(hal, t)
    code = hal.page_ordered_code(prover.circuit, po2, zk, W)
    got_code = code.to_vec().reshape(G.WC, n)
    bad = np.argwhere(got_code != want_code)
    assert bad.size == 0, f"code: {len(bad)} cells differ, the first at (column, row) {tuple(bad[0])}"
    data = hal.alloc_elem("data", G.WD << po2)
    noise = cases.NOISE + first
    out = hal.page_ordered_witgen(prover.circuit, po2, zk, code, proof, words, before, after, first, data, noise)
    got = data.to_vec().reshape(G.WD, n)
    bad = np.argwhere(got[:, :A] != want_data[:, :A])
    assert bad.size == 0, f"data: {len(bad)} cells differ, the first at (column, row) {tuple(bad[0])}"
    lib = zhal.load_library()
    kp = zhal.noise_key(noise).ctypes.data_as(C.POINTER(C.c_uint32))
    rows = sorted({A, A + 1, n - 1, *range(A, n, 97)})
    for col in (0, 124, G.D_LIVE, G.D_LO, G.D_GBIT, G.D_GACC):
        assert [int(got[col, r]) for r in rows] == [lib.zkh_noise_cell_host(kp, 2, col, r) for r in rows], f"blinding rows of column {col}"
    assert out.size == 18 and np.array_equal(out, want_out), "out is not the reference's 18 words"
    assert [G.decode(out[16]), G.decode(out[17])] == list(oc.bounds(t, first))
    mix = np.random.default_rng(5).integers(0, P, 4, dtype=np.uint64).astype(np.uint32)
    accum = hal.alloc_elem("accum", G.WA << po2)
    hal.syn_accum(prover.circuit, po2, zk, noise, data, mix, accum)
    r = hal.check_rows(prover.circuit, po2, accum, code, data, out, mix)
    assert r["row"] == -1 and r["failing_rows"] == 0, r


def _fmt(r):
    return " ".join(f"{int(w):08x}" for w in r)


def test_the_chain_of_ordered_seals(hal, prover):
    po2, zk, W = H5
    t = oc.table(po2, zk, W, "2N+3")
    assert len(t["addrs"]) == 29 and t["plan"] == [(0, 13), (13, 13), (26, 3)]
    proof, words, before, after = _device(hal, t)
    segs = [Segment(index=p, po2=po2, zk_cycles=zk, noise_seed=cases.NOISE + p) for p in range(3)]
    recs = prover.seal_page_out_ordered(segs, proof, words, before, after, check=True)
    assert len(recs) == 3 and [r.index for r in recs] == [0, 1, 2]
    root = prover.code_root(hal.page_ordered_code(prover.circuit, po2, zk, W), po2)
    hc = zhal.HostCircuit(G.p2_page_ordered_circuit())
    for r, (first, _) in zip(recs, t["plan"]):
        assert np.array_equal(r.output, oc.part(po2, zk, W, "2N+3", first)[1]) and np.array_equal(r.seal[:18], r.output)
        assert np.array_equal(r.control_root, root)
        hc.verify_segment(r.seal, root)
    root_before, root_after = hal.image_root(before), hal.image_root(after)
    hi = int(t["addrs"][-1]) + 1
    for given in (root_before, None):
        got = verify_page_ordered_chain(recs, root, given)
        assert np.array_equal(got[0], root_before) and np.array_equal(got[1], root_after) and got[2] == hi
    # every seal is good, the chain is not: two parts swapped, a part dropped
    with pytest.raises(HalError, match=re.escape(f"part 0 starts at lo {int(t['addrs'][12]) + 1}, not 0")):
        verify_page_ordered_chain([recs[1], recs[0], recs[2]], root)
    with pytest.raises(HalError, match=re.escape(f"part 1 opens root {_fmt(recs[2].seal[:8])}, but part 0 left root {_fmt(recs[0].seal[8:16])}")):
        verify_page_ordered_chain([recs[0], recs[2], recs[1]], root)
    with pytest.raises(HalError, match=re.escape(f"part 1 opens root {_fmt(recs[2].seal[:8])}, but part 0 left root {_fmt(recs[0].seal[8:16])}")):
        verify_page_ordered_chain([recs[0], recs[2]], root)
    with pytest.raises(HalError, match=re.escape(f"part 0 opens root {_fmt(root_before)}, not root_before {_fmt(root_after)}")):
        verify_page_ordered_chain(recs, root, root_after)
    with pytest.raises(HalError, match="no receipt"):
        verify_page_ordered_chain([], root)
    # a seal with `lo` altered: the verifier of that seal refuses it, whatever the chain says
    bad = recs[1].seal.copy()
    bad[16] = recs[0].seal[16]
    with pytest.raises(HalError, match="verify_segment: "):
        verify_page_ordered_chain([recs[0], SegmentReceipt(seal=bad, index=1, po2=po2), recs[2]], root)
    with pytest.raises(HalError):
        verify_page_ordered_chain(recs, prover.code_root(hal.page_ordered_code(prover.circuit, po2, zk, 64), po2))
    # a `segs` of the wrong length names both numbers
    with pytest.raises(HalError, match=re.escape("seal_page_out_ordered: 2 segments, but a table of 29 rows takes 3 parts of 13 slots")):
        prover.seal_page_out_ordered(segs[:2], proof, words, before, after)


def test_refusals(hal, prover):
    po2, zk, W = H5
    t = oc.table(po2, zk, W, "2N+3")
    N, h, n = t["N"], t["h"], 1 << po2
    proof, words, before, after = _device(hal, t)
    page = SegmentProver(hal, p2_page.p2_page_circuit())
    code = hal.page_ordered_code(prover.circuit, po2, zk, W)
    data = hal.alloc_elem("data", G.WD * n)
    data.write(np.full(G.WD * n, 0xdeadbeef, dtype=np.uint32))
    call = lambda first, **kw: hal.page_ordered_witgen(kw.get("circuit", prover.circuit), po2, zk, kw.get("code", code), kw.get("proof", proof), words, before,
                                                       after, first, kw.get("data", data), cases.NOISE)
    # a P2-PAGE (kind 5) circuit passed to the ordered calls
    shape = "the circuit does not have P2-PAGE-ordered's shape (kind 6, 42 / 129 / 4 columns, 18 outputs)"
    with pytest.raises(HalError, match=re.escape(f"page_ordered_code: {shape}")):
        hal.page_ordered_code(page.circuit, po2, zk, W, code=code)
    with pytest.raises(HalError, match=re.escape(f"page_ordered_witgen: {shape}")):
        call(0, circuit=page.circuit)
    # an ordered circuit passed to P2-PAGE's generator: its existing message
    with pytest.raises(HalError, match=re.escape("page_circuit_witgen: the circuit does not have P2-PAGE's shape (kind 5, 39 / 125 / 4 columns, 16 outputs)")):
        hal.page_circuit_witgen(prover.circuit, po2, zk, code, proof, words, before, after, data, cases.NOISE)
    # h = 27: refused from the image's size alone, before anything of that size exists (P2-PAGE takes this size)
    with pytest.raises(HalError, match=re.escape(f"page_ordered_code: an image of {(1 << 29) + 1} words has h 27; the gap between two addresses is decomposed into "
                                                 "29 bits, which takes addresses below 2^29: h <= 26")):
        hal.page_ordered_code(prover.circuit, po2, zk, (1 << 29) + 1, code=code)
    assert hal.page_circuit_slots(po2, zk, (1 << 29) + 1) == (n - zk) // BLOCK // 27 > 0
    # the shared refusals carry this entry point's name
    with pytest.raises(HalError, match=re.escape("page_ordered_witgen: buffer shape mismatch")):
        call(13, data=hal.alloc_elem("data", p2_page.WD * n))
    with pytest.raises(HalError, match=re.escape("page_ordered_witgen: first 29, but the table has 29 rows")):
        call(29)
    assert bool((data.to_vec() == 0xdeadbeef).all()), "a refusal before any launch wrote into the data group"
    # a table out of order: the check pass's message, and no path column written, old or new
    host = proof.to_vec()
    t0 = 5 + h
    swapped = host.copy()
    swapped[t0], swapped[t0 + 3] = host[t0 + 3], host[t0]
    a0, a1 = int(host[t0]), int(host[t0 + 3])
    with pytest.raises(HalError, match=re.escape(f"page_ordered_witgen: row 1: address {a0} does not follow a smaller one (row 0: address {a1})")):
        call(13, proof=hal.copy_from("proof", swapped))
    got = data.to_vec().reshape(G.WD, n)
    assert (got[:p2_page.D_E, :BLOCK * h * N] == 0xdeadbeef).all() and (got[G.D_LIVE:, :BLOCK * h * N] == 0xdeadbeef).all(), "a path column was written after the check pass refused"
    # and the good call right after them
    assert np.array_equal(call(13), oc.part(po2, zk, W, "2N+3", 13)[1])
    assert np.array_equal(data.to_vec().reshape(G.WD, n)[:, :n - zk], oc.part(po2, zk, W, "2N+3", 13)[0][:, :n - zk])
