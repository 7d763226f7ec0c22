"""P2-TREE on the GPU (zkh_page_tree_code / zkh_page_tree_witgen / zkh_page_tree_plan, csrc/page_tree.hip; SegmentProver.seal_page_out_tree,
prover.verify_page_tree_chain).  The device code group and witness against p2_tree's references word for word over
page_tree_cases.grid() and over every part, the blinding rows, `out`, and the witness with the library's accumulate against the
circuit's constraints on the device; the plan against p2_tree.parts; chains of seals and what their verifier refuses; the refusals of
the calls, by message, with the good call right after them; trees that do not belong together, which zkh_accumulate refuses and
check_bus names; and the same page-out's roots under P2-PAGE-ordered.

The yardstick applies the updates to a numpy image and reads every block from two plain trees built for the part; the device reads the
two trees of the WHOLE page-out and picks every source by its address alone.

Shapes, the smallest at which the new code can go wrong: (10, 500, 64) is a tree of 7 blocks; (12, 1994, 8 * 17 + 3) has a partial last
leaf; (10, 500, 512) with every word takes several parts, whose edge addresses fork from their neighbours at different layers;
(12, 1994, 2^14 + 3) has h = 12, ids and gaps with bit 11 set, and 40 random addresses in several parts; (12, 200, 2048) has 250 lanes
of the block kernel in workgroups of 64 and 3875 rows of the bookkeeping kernel in workgroups of 256, the last of each partial; `all`
at W = 512 and 2048 places more than 256 updates, so the placing kernel's scans carry."""
import ctypes as C
import re

import numpy as np
import pytest

import page_circuit_cases as cases
import page_tree_cases as tc
from args_gpu import image_buf
from zeth_amd import hal as zhal
from zeth_amd.circuits import p2_page, p2_page_ordered, p2_tree as G
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver, SegmentReceipt, verify_page_ordered_chain, verify_page_tree_chain

pytestmark = pytest.mark.gpu
P = tc.P
BLOCK = p2_page.BLOCK_ROWS


@pytest.fixture(scope="module")
def prover(hal):
    return SegmentProver(hal, G.p2_tree_circuit(), arguments=G.arguments())


_on_device = {}


def _device(hal, s, what):
    """the table on the device -> (proof buffer, proof words, nodes_before, nodes_after): the trees of the WHOLE page-out, once per table"""
    if (s, what) not in _on_device:
        t = tc.table(*s, what)
        before = hal.image_commit(image_buf(hal, t["image"]))
        after = hal.image_commit(image_buf(hal, t["image_after"]))
        proof = cases.host_proof(t["image"], t["addrs"], t["outs"], before.to_vec())
        assert int(proof[2]) == len(t["addrs"])
        _on_device[s, what] = (hal.copy_from("proof", proof), proof.size, before, after)
    return _on_device[s, what]


@pytest.mark.parametrize("g", tc.grid(), ids=tc.grid_id)
def test_the_generator_is_the_reference_word_for_word(hal, prover, g):
    (po2, zk, W), what, p = g
    t = tc.table(po2, zk, W, what)
    first, count = t["plan"][p]
    want_data, want_out, want_code = tc.part(po2, zk, W, what, p)
    n, A = 1 << po2, (1 << po2) - zk
    proof, words, before, after = _device(hal, (po2, zk, W), what)
    code = hal.page_tree_code(prover.circuit, po2, zk)
    bad = np.argwhere(code.to_vec().reshape(G.WC, n) != want_code)
    assert bad.size == 0, f"code: {len(bad)} cells differ, the first at (column, row) {tuple(bad[0])}"
    data = hal.alloc_elem("data", G.WD << po2)
    noise = tc.NOISE + p
    out = hal.page_tree_witgen(prover.circuit, po2, zk, code, proof, words, before, after, first, count, data, noise)
    got = data.to_vec().reshape(G.WD, n)
    bad = np.argwhere(got[:, :A] != want_data[:, :A])
    assert bad.size == 0, f"data: {len(bad)} cells differ, the first at (column, row) {tuple(bad[0])}"
    lib = zhal.load_library()
    kp = zhal.noise_key(noise).ctypes.data_as(C.POINTER(C.c_uint32))
    rows = sorted({A, A + 1, n - 1, *range(A, n, 97)})
    for col in (0, 95, G.D_ID, G.D_GACC):
        assert [int(got[col, r]) for r in rows] == [lib.zkh_noise_cell_host(kp, 2, col, r) for r in rows], f"blinding rows of column {col}"
    assert out.size == 18 and np.array_equal(out, want_out), "out is not the reference's 18 words"
    mix = np.random.default_rng(5).integers(0, P, G.MIX_WORDS, dtype=np.uint64).astype(np.uint32)
    accum = hal.alloc_elem("accum", G.WA << po2)
    hal.accumulate(prover.circuit, po2, zk, noise, code, data, mix, accum)
    r = hal.check_rows(prover.circuit, po2, accum, code, data, out, mix)
    assert r["row"] == -1 and r["failing_rows"] == 0, r


@pytest.mark.parametrize("s,what", tc.CASES, ids=lambda v: str(v))
def test_the_plan_is_p2_tree_parts(hal, s, what):
    po2, zk, W = s
    t = tc.table(po2, zk, W, what)
    assert hal.page_tree_plan(po2, zk, W, t["addrs"]) == t["plan"]


def _fmt(r):
    return " ".join(f"{int(w):08x}" for w in r)


@pytest.mark.parametrize("s,what", [(tc.H6, "all"), (tc.H12, "random"), (tc.H5, "random"), (tc.H3, 0)], ids=lambda v: str(v))
def test_the_chain_of_tree_seals(hal, prover, s, what):
    po2, zk, W = s
    t = tc.table(po2, zk, W, what)
    plan = t["plan"]
    proof, words, before, after = _device(hal, s, what)
    segs = [Segment(index=p, po2=po2, zk_cycles=zk, noise_seed=tc.NOISE + p) for p in range(len(plan))]
    recs = prover.seal_page_out_tree(segs, proof, words, before, after, check=True)
    assert [r.index for r in recs] == list(range(len(plan)))
    root = prover.code_root(hal.page_tree_code(prover.circuit, po2, zk), po2)
    for p, r in enumerate(recs):
        assert np.array_equal(r.output, tc.part(po2, zk, W, what, p)[1]) and np.array_equal(r.seal[:18], r.output) and np.array_equal(r.control_root, root)
    root_before, root_after = hal.image_root(before), hal.image_root(after)
    half = 1 << (t["h"] - 1)
    hi = half + (int(t["addrs"][-1]) >> 4) + 1 if len(t["addrs"]) else half
    for given in (root_before, None):
        got = verify_page_tree_chain(recs, root, t["h"], given)
        assert np.array_equal(got[0], root_before) and np.array_equal(got[1], root_after) and got[2] == hi
    with pytest.raises(HalError, match="verify_segment: "):                    # another control root: the seal's verifier refuses
        verify_page_tree_chain(recs, root_after, t["h"])
    bad = recs[0].seal.copy()
    bad[17] = (int(bad[17]) + tc.ONE) % P
    with pytest.raises(HalError, match="verify_segment: "):                    # a seal with `hi` altered
        verify_page_tree_chain([SegmentReceipt(seal=bad, index=0, po2=po2)] + recs[1:], root, t["h"])
    if len(recs) < 3:
        return
    # every seal is good, the chain is not: two parts swapped, a part dropped, another first root, another h
    with pytest.raises(HalError, match=re.escape(f"part 0 starts at lo {G.decode(recs[1].seal[16])}, not 2^{t['h'] - 1} = {half}")):
        verify_page_tree_chain([recs[1], recs[0]] + recs[2:], root, t["h"])
    with pytest.raises(HalError, match=re.escape(f"part 1 opens root {_fmt(recs[2].seal[:8])}, but part 0 left root {_fmt(recs[0].seal[8:16])}")):
        verify_page_tree_chain([recs[0]] + recs[2:], root, t["h"])
    with pytest.raises(HalError, match=re.escape(f"part 0 opens root {_fmt(root_before)}, not root_before {_fmt(root_after)}")):
        verify_page_tree_chain(recs, root, t["h"], root_after)
    with pytest.raises(HalError, match=re.escape(f"part 0 starts at lo {half}, not 2^{t['h']} = {2 * half}")):
        verify_page_tree_chain(recs, root, t["h"] + 1)
    with pytest.raises(HalError, match=re.escape(f"seal_page_out_tree: {len(plan) - 1} segments, but a table of {len(t['addrs'])} rows takes {len(plan)} parts")):
        prover.seal_page_out_tree(segs[:-1], proof, words, before, after)


def test_refusals(hal, prover):
    po2, zk, W = tc.H5
    t = tc.table(po2, zk, W, "one_pair")                                       # [3, 12, W - 1]: rows 0 and 1 share the pair of leaves 0
    h, B, n = t["h"], t["B"], 1 << po2
    proof, words, before, after = _device(hal, tc.H5, "one_pair")
    ordered = SegmentProver(hal, p2_page_ordered.p2_page_ordered_circuit())
    code = hal.page_tree_code(prover.circuit, po2, zk)
    data = hal.alloc_elem("data", G.WD * n)
    data.write(np.full(G.WD * n, 0xdeadbeef, dtype=np.uint32))
    call = lambda first, count, **kw: hal.page_tree_witgen(kw.get("circuit", prover.circuit), kw.get("po2", po2), kw.get("zk", zk), kw.get("code", code),
                                                           kw.get("proof", proof), kw.get("words", words), kw.get("before", before), kw.get("after", after),
                                                           first, count, kw.get("data", data), tc.NOISE)
    shape = "the circuit does not have P2-TREE's shape (kind 7, 41 / 106 / 24 columns, 18 outputs)"
    with pytest.raises(HalError, match=re.escape(f"page_tree_code: {shape}")):
        hal.page_tree_code(ordered.circuit, po2, zk, code=code)
    with pytest.raises(HalError, match=re.escape(f"page_tree_witgen: {shape}")):
        call(0, 3, circuit=ordered.circuit)
    with pytest.raises(HalError, match=re.escape("page_tree_witgen: buffer shape mismatch")):
        call(0, 3, data=hal.alloc_elem("data", p2_page.WD * n))
    with pytest.raises(HalError, match=re.escape("page_tree_witgen: the part [2, 4) of a table of 3 rows")):
        call(2, 2)
    with pytest.raises(HalError, match=re.escape("page_tree_witgen: the part [1, 1) of a table of 3 rows")):
        call(1, 0)
    # W <= 16 and B < h: from the shapes alone, for the plan as for the generator
    small = np.arange(1, 17, dtype=np.uint32)
    tree16 = hal.image_commit(image_buf(hal, small))
    proof16 = cases.host_proof(small, np.array([3]), np.array([5], dtype=np.uint32), tree16.to_vec())
    msg16 = "an image of 16 words has a single pair of leaves (W > 16"
    with pytest.raises(HalError, match=re.escape(f"page_tree_witgen: {msg16}")):
        call(0, 1, proof=hal.copy_from("proof", proof16), words=proof16.size, before=tree16, after=tree16)
    with pytest.raises(HalError, match=re.escape(f"page_tree_plan: {msg16}")):
        hal.page_tree_plan(po2, zk, 16, [3])
    t12 = tc.table(*tc.H12, 3)
    proof12, words12, before12, after12 = _device(hal, tc.H12, 3)
    room = "no room for the h 12 nodes of one path in 11 block slots (po2 10, 680 zk_cycles)"
    with pytest.raises(HalError, match=re.escape(f"page_tree_witgen: {room}")):
        call(0, 3, po2=10, zk=680, code=hal.page_tree_code(prover.circuit, 10, 680), proof=proof12, words=words12, before=before12, after=after12,
             data=hal.alloc_elem("data", G.WD << 10))
    with pytest.raises(HalError, match=re.escape(f"page_tree_plan: {room}")):
        hal.page_tree_plan(10, 680, tc.H12[2], t12["addrs"])
    assert bool((data.to_vec() == 0xdeadbeef).all()), "a refusal before any launch wrote into the data group"
    # the check pass: a part that splits a pair of leaves, and a part of more nodes than block slots
    with pytest.raises(HalError, match=re.escape("page_tree_witgen: the part [0, 1) splits a pair of leaves: rows 0 and 1 write the same 16 words")):
        call(0, 1)
    with pytest.raises(HalError, match=re.escape("page_tree_witgen: the part [1, 3) splits a pair of leaves: rows 0 and 1 write the same 16 words")):
        call(1, 2)
    all6 = tc.table(*tc.H6, "all")
    proof6, words6, before6, after6 = _device(hal, tc.H6, "all")
    with pytest.raises(HalError, match=re.escape("page_tree_witgen: the part [0, 512) has 63 dirty nodes, but po2 10 leaves 16 block slots")):
        call(0, 512, po2=10, zk=500, code=hal.page_tree_code(prover.circuit, 10, 500), proof=proof6, words=words6, before=before6, after=after6,
             data=hal.alloc_elem("data", G.WD << 10))
    assert len(all6["plan"]) > 1
    # a table out of order, and an address outside the image: k_page_check's messages
    host = proof.to_vec()
    t0 = 5 + h
    a0, a1 = int(host[t0]), int(host[t0 + 3])
    swapped = host.copy()
    swapped[t0], swapped[t0 + 3] = host[t0 + 3], host[t0]
    with pytest.raises(HalError, match=re.escape(f"page_tree_witgen: row 1: address {a0} does not follow a smaller one (row 0: address {a1})")):
        call(0, 3, proof=hal.copy_from("proof", swapped))
    outside = host.copy()
    outside[t0 + 6] = W
    with pytest.raises(HalError, match=re.escape(f"page_tree_witgen: row 2: address {W} outside the image of {W} words")):
        call(0, 3, proof=hal.copy_from("proof", outside))
    with pytest.raises(HalError, match=re.escape(f"page_tree_plan: row 1: address {a0} does not follow a smaller one")):
        hal.page_tree_plan(po2, zk, W, [a1, a0])
    got = data.to_vec().reshape(G.WD, n)
    assert (got[:, :BLOCK * B] == 0xdeadbeef).all(), "a block column was written after the check pass refused"
    # and the good call right after them
    assert np.array_equal(call(0, 3), tc.part(po2, zk, W, "one_pair")[1])
    assert np.array_equal(data.to_vec().reshape(G.WD, n)[:, :n - zk], tc.part(po2, zk, W, "one_pair")[0][:, :n - zk])


def test_trees_that_do_not_belong_to_the_table_give_no_seal(hal, prover):
    """the generator reads the table's addresses and the two trees; a digest of the tree after that is not the hash of its children (a
    tree that was not brought up to the table's page-out) reaches its parent block through the tree and the bus from its own block:
    the two do not cancel, zkh_accumulate refuses the witness, and with check=True the refusal names the key, the node's id"""
    po2, zk, W = tc.H5
    t = tc.table(po2, zk, W, "random")
    proof, words, before, after = _device(hal, tc.H5, "random")
    pairs = sorted({int(a) >> 4 for a in t["addrs"]})
    assert len(pairs) >= 3
    node = 16 + pairs[1]                                                      # a pair block that holds neither the first nor the last address
    stale = after.to_vec().copy()
    stale[8 * node] = (int(stale[8 * node]) + 1) % P
    after2 = hal.copy_from("nodes", stale)
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=tc.NOISE)
    with pytest.raises(HalError, match="does not balance") as refusal:
        prover.seal_page_out_tree([seg], proof, words, before, after2, check=True)
    assert re.search(rf"bus: key \(tag \d; {node}, ", str(refusal.value)), str(refusal.value)
    with pytest.raises(HalError, match="does not balance"):
        prover.seal_page_out_tree([seg], proof, words, before, after2)
    assert len(prover.seal_page_out_tree([seg], proof, words, before, after)) == 1


@pytest.mark.parametrize("what", [3, "one_pair", "random"], ids=str)
def test_the_ordered_seals_of_the_same_page_out_yield_the_same_roots(hal, prover, what):
    po2, zk, W = tc.H5
    t = tc.table(po2, zk, W, what)
    proof, words, before, after = _device(hal, tc.H5, what)
    ordered = SegmentProver(hal, p2_page_ordered.p2_page_ordered_circuit())
    plan = p2_page.parts(po2, zk, W, len(t["addrs"]))
    orecs = ordered.seal_page_out_ordered([Segment(index=p, po2=po2, zk_cycles=zk, noise_seed=tc.NOISE + p) for p in range(len(plan))], proof, words, before, after)
    oroot = ordered.code_root(hal.page_ordered_code(ordered.circuit, po2, zk, W), po2)
    want = verify_page_ordered_chain(orecs, oroot)
    recs = prover.seal_page_out_tree([Segment(index=p, po2=po2, zk_cycles=zk, noise_seed=tc.NOISE + p) for p in range(len(t["plan"]))], proof, words, before, after)
    got = verify_page_tree_chain(recs, prover.code_root(hal.page_tree_code(prover.circuit, po2, zk), po2), t["h"])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert len(recs) <= len(orecs)
