"""The dirty-node table on the GPU (zkh_image_proof_nodes, csrc/image.hip and hash.hip's k_hash_walk; csrc/zkn1.h) and the P2-TREE witness
from it (zkh_page_tree_witgen_nodes, csrc/page_tree.hip k_tree_find / k_tree_edges_nodes / k_tree_blocks_nodes), kinds 7 and 9.

1. the table is the numpy twin (logup.reference_page_out_nodes) word for word, the root is image_proof_verify's, the proof is only read;
2. the refusals are the walk's, message for message, `dirty` untouched, a good call right after; D = 0 has its own refusal;
3. the witness is the Python reference's (which knows nothing of the code under test) and the two-tree call's from dense trees, every
   data column, the blinding rows and out[18];
4. the table of another proof is refused by name, and no cell of a block is written.

Shapes, the smallest at which the new code can go wrong: page_tree_cases' H3 (lists of 1 and 2 items), H5 (a partial last leaf), H6 `all`
(parts whose edges meet at different layers), H8, H12, each with the address sets that leave a pair's second leaf clean (1, first_last,
adjacent) or dirty (one_pair, all); 600 rows over W = 8192, where the two lowest layers list more than 256 nodes, part 1's edge chain
starts in the middle of every list and the block kernel takes 17 workgroups; and, for the table alone, the walk's W = 2^17 + 5 with 6000
rows, lists of many workgroups of 256."""
import ctypes as C
import re

import numpy as np
import pytest

import page_nodes_cases as nc
import page_tree_cases as tc
import tied_cases
from args_gpu import image_buf
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, p2_tree as G, p2_tree_tied as TT
from zeth_amd.hal import HalError
from zeth_amd.prover import SegmentProver

pytestmark = pytest.mark.gpu
P = tc.P
NOISE = 0x0D17
POISON = 0xdeadbeef
SLACK = 40
BIG_W = (1 << 17) + 5                                                         # the walk's big shape: L = 2^15, h = 15


@pytest.fixture(scope="module")
def provers(hal):
    return {7: SegmentProver(hal, G.p2_tree_circuit(), arguments=G.arguments()), 9: SegmentProver(hal, TT.p2_tree_tied_circuit(), arguments=TT.arguments())}


_on_device = {}


def _device(hal, s, what):
    """one table on the device, once -> a dict: proof (the buffer), words, before / after (the dense trees), dirty (the table's buffer)"""
    if (s, what) not in _on_device:
        t, p = nc.table(*s, what), nc.proved(*s, what)
        d = {"proof": hal.copy_from("proof", p["proof"]), "words": p["proof"].size, "before": hal.image_commit(image_buf(hal, t["image"])),
             "after": hal.image_commit(image_buf(hal, t["image_after"]))}
        _, d["dirty"] = hal.image_proof_nodes(d["proof"], p["root_before"])
        _on_device[s, what] = d
    return _on_device[s, what]


def _nodes_call(hal, proof_buf, words, root, dirty):
    """the C call itself -> (None or the message, root_after as the call left it)"""
    lib, u32p = zhal.load_library(), C.POINTER(C.c_uint32)
    rb, after = np.ascontiguousarray(root, dtype=np.uint32), np.full(8, POISON, dtype=np.uint32)
    err = lib.zkh_image_proof_nodes(hal.ctx, proof_buf.h, words, rb.ctypes.data_as(u32p), after.ctypes.data_as(u32p), dirty.h)
    if not err:
        return None, after
    msg = C.cast(err, C.c_char_p).value.decode()
    lib.zkh_free_error(err)
    return msg, after


def _table_is_the_twin(hal, proof, root_before, want_nodes, want_root, W, D):
    whole = np.concatenate([proof, np.full(SLACK, POISON, dtype=np.uint32)])   # the proof in a longer buffer: only its own words are read
    buf = hal.copy_from("proof", whole)
    bound = hal.image_dirty_words(W, D)
    assert want_nodes.size <= bound
    dirty = hal.alloc("dirty", bound + SLACK)
    dirty.write(np.full(bound + SLACK, POISON, dtype=np.uint32))
    msg, root = _nodes_call(hal, buf, proof.size, root_before, dirty)
    assert msg is None, msg
    assert np.array_equal(root, want_root) and np.array_equal(root, zhal.image_proof_verify(proof, root_before))
    got = dirty.to_vec()
    bad = np.flatnonzero(got[:want_nodes.size] != want_nodes)
    assert bad.size == 0, f"{bad.size} words of the table differ from the twin's, the first at word {int(bad[0])}"
    assert (got[want_nodes.size:] == POISON).all(), "a word past the table's length was written"
    assert np.array_equal(buf.to_vec(), whole), "the call wrote into the proof's buffer"
    assert np.array_equal(hal.image_proof_walk(buf, root_before, words=proof.size), root)


# ---- 1. the table ----
@pytest.mark.parametrize("s,what", nc.TABLES, ids=[f"{s[0]}-{s[1]}-{s[2]}-{what}" for s, what in nc.TABLES])
def test_the_table_is_the_reference_word_for_word(hal, s, what):
    t, p = nc.table(*s, what), nc.proved(*s, what)
    _table_is_the_twin(hal, p["proof"], p["root_before"], p["nodes"], p["root_after"], t["W"], len(t["addrs"]))


def test_the_table_where_the_lists_span_many_workgroups(hal):
    rng = np.random.default_rng(BIG_W)
    image = rng.integers(0, P, BIG_W, dtype=np.uint64).astype(np.uint32)
    # 6000 random rows, and a run of one row per leaf over leaves 0 .. 299 with both sides of the seams at items 255 / 256 / 257
    addrs = np.unique(np.concatenate([rng.choice(BIG_W, 6000, replace=False), 8 * np.arange(300) + 3, [0, 7, 8 * 255 + 7, 8 * 256, 8 * 257, BIG_W - 1]])).astype(np.int64)
    outs = rng.integers(0, P, addrs.size, dtype=np.uint64).astype(np.uint32)
    tree = hal.image_commit(image_buf(hal, image)).to_vec()
    proof = nc.pcases.host_proof(image, addrs, outs, tree)
    assert int(proof[4]) == 15
    root_before = tree.reshape(-1, 8)[1]
    root_after, nodes = logup.reference_page_out_nodes(proof, root_before)
    _, _, _, layers, _ = nc.sections(nodes)
    assert len(layers[0][0]) > 4 * 256 and len(layers[3][0]) > 256
    _table_is_the_twin(hal, proof, root_before, nodes, root_after, BIG_W, addrs.size)


# ---- 2. the refusals ----
def _host_message(proof, root):
    with pytest.raises(HalError) as e:
        zhal.image_proof_verify(proof, root)
    assert str(e.value).startswith("image_proof_verify: ")
    return str(e.value)[len("image_proof_verify: "):]


def test_refusals_are_the_walks(hal):
    s, what = tc.H5, "random"
    t, p = nc.table(*s, what), nc.proved(*s, what)
    proof, root, h = p["proof"], p["root_before"], t["h"]
    bound = hal.image_dirty_words(t["W"], len(t["addrs"]))
    dirty = hal.alloc("dirty", bound)
    poison = np.full(bound, POISON, dtype=np.uint32)
    dirty.write(poison)
    good = hal.copy_from("proof", proof)
    wrong_root = root.copy()
    wrong_root[3] = (int(wrong_root[3]) + 1) % P
    count = proof.copy()
    k = next(k for k in range(h) if int(proof[5 + k]))
    count[5 + k] += 1
    count = np.concatenate([count, np.zeros(8, dtype=np.uint32)])             # the length the header now describes: the layer's count is what is refused
    differs = proof.copy()
    differs[5 + h + 3 * 7 + 1] = (int(differs[5 + h + 3 * 7 + 1]) + 1) % P
    for bad, bad_root, words in ((proof, wrong_root, "not root_before"), (count, root, f"layer {k}: "), (differs, root, "row 7: in ")):
        want = _host_message(bad, bad_root)
        assert words in want, want
        msg, after = _nodes_call(hal, hal.copy_from("proof", bad), bad.size, bad_root, dirty)
        assert msg == "image_proof_nodes: " + want
        assert (after == POISON).all(), "root_after written on a refusal"
        assert np.array_equal(dirty.to_vec(), poison), "dirty written on a refusal"
        with pytest.raises(HalError, match=re.escape("image_proof_walk: " + want)):
            hal.image_proof_walk(bad, bad_root)
        msg, after = _nodes_call(hal, good, proof.size, root, dirty)          # the good call right after
        assert msg is None and np.array_equal(after, p["root_after"]) and np.array_equal(dirty.to_vec()[:p["nodes"].size], p["nodes"])
        dirty.write(poison)
    # a buffer shorter than the bound, before any launch
    with pytest.raises(HalError, match=re.escape(f"image_proof_nodes: dirty nodes of {bound - 1} words; {len(t['addrs'])} rows over {t['W']} words may take {bound}")):
        hal.image_proof_nodes(good, root, dirty=hal.alloc("dirty", bound - 1))


def test_an_empty_table_is_refused_and_sent_to_the_tree(hal):
    image = np.arange(1, 65, dtype=np.uint32)
    tree = logup.reference_image_tree(image)
    proof = nc.pcases.host_proof(image, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint32), tree)
    assert proof.size == 5 + 3 and np.array_equal(hal.image_proof_walk(proof, tree[1]), tree[1])
    dirty = hal.alloc("dirty", 64)
    dirty.write(np.full(64, POISON, dtype=np.uint32))
    with pytest.raises(HalError, match=r"^image_proof_nodes: an empty table \(D = 0\) has no dirty nodes: its proof is the header alone and holds no node, not even "
                                       r"the root's children; such a page-out is sealed from the tree"):
        hal.image_proof_nodes(proof, tree[1], dirty=dirty)
    assert (dirty.to_vec() == POISON).all()


# ---- 3. the witness ----
@pytest.fixture(scope="module")
def reference():
    """(kind, shape, what, p) -> (the reference's data group over the active rows, its 18 out words), once per part"""
    cache = {}

    def get(kind, s, what, p):
        if (kind, s, what, p) not in cache:
            t = nc.table(*s, what)
            first, count = t["plan"][p]
            if kind == 7:
                active, out = G.reference_tree_part(*s, t["table"], t["image"], first, count)
            else:
                active, _accum, out = TT.reference_tree_tied_part(*s, t["table"], t["image"], first, count, tied_cases.CHALLENGE)
            cache[kind, s, what, p] = (active, np.asarray(out[:18], dtype=np.uint32))
        return cache[kind, s, what, p]
    return get


@pytest.mark.parametrize("kind", [7, 9])
@pytest.mark.parametrize("g", nc.grid(), ids=nc.grid_id)
def test_the_witness_is_the_two_tree_witness_and_the_reference(hal, provers, reference, g, kind):
    (po2, zk, W), what, p = g
    prover, wd = provers[kind], (G.WD if kind == 7 else TT.WD)
    t = nc.table(po2, zk, W, what)
    first, count = t["plan"][p]
    n, A = 1 << po2, (1 << po2) - zk
    d = _device(hal, (po2, zk, W), what)
    code = hal.page_tree_code(prover.circuit, po2, zk)
    noise = NOISE + p
    data = hal.alloc_elem("data", wd << po2)
    data.write(np.full(wd << po2, POISON, dtype=np.uint32))                    # every cell has a writer
    out = hal.page_tree_witgen_nodes(prover.circuit, po2, zk, code, d["proof"], d["words"], d["dirty"], first, count, data, noise)
    got = data.to_vec().reshape(wd, n)
    want_active, want_out = reference(kind, (po2, zk, W), what, p)
    bad = np.argwhere(got[:, :A] != want_active)
    assert bad.size == 0, f"data: {len(bad)} cells differ from the reference, the first at (column, row) {tuple(bad[0])}"
    assert out.size == 18 and np.array_equal(out, want_out), "out is not the reference's 18 words"
    two = hal.alloc_elem("data", wd << po2)
    out2 = hal.page_tree_witgen(prover.circuit, po2, zk, code, d["proof"], d["words"], d["before"], d["after"], first, count, two, noise)
    bad = np.argwhere(got != two.to_vec().reshape(wd, n))                      # all columns, the blinding rows too: the same noise key
    assert bad.size == 0, f"data: {len(bad)} cells differ from the two-tree witness, the first at (column, row) {tuple(bad[0])}"
    assert np.array_equal(out, out2)
    lib = zhal.load_library()
    kp = zhal.noise_key(noise).ctypes.data_as(C.POINTER(C.c_uint32))
    rows = sorted({A, A + 1, n - 1, *range(A, n, 97)})
    for col in (0, 95, G.D_ID, wd - 1):
        assert [int(got[col, r]) for r in rows] == [lib.zkh_noise_cell_host(kp, 2, col, r) for r in rows], f"blinding rows of column {col}"


# ---- 4. a table of another proof, and a table that does not fit ----
def test_the_dirty_nodes_of_another_proof_are_refused_by_name(hal, provers):
    s, what = tc.H5, 3
    po2, zk, W = s
    t, d = nc.table(*s, what), _device(hal, s, what)
    # the same image and the same number of rows at other addresses: same W and D, other nodes
    others = np.array([0, 64, 128], dtype=np.int64)
    assert not {int(a) >> 4 for a in others} & {int(a) >> 4 for a in t["addrs"]}
    tree = logup.reference_image_tree(t["image"])
    other_proof = nc.pcases.host_proof(t["image"], others, np.array([1, 2, 3], dtype=np.uint32), tree)
    _, other = hal.image_proof_nodes(other_proof, tree[1])
    assert [int(x) for x in other.slice(0, 4).to_vec()[1:]] == [W, 3, t["h"]]

    def ancestors(addrs):
        ids = set()
        for a in addrs:
            i = (1 << (t["h"] - 1)) + (int(a) >> 4)
            while i:
                ids.add(i)
                i >>= 1
        return ids
    missing = min(ancestors(t["addrs"]) - ancestors(others))                 # the lowest id of a block of the part that the other table lacks
    layer = t["h"] + 1 - missing.bit_length()
    n = 1 << po2
    for kind, wd in ((7, G.WD), (9, TT.WD)):
        prover = provers[kind]
        code = hal.page_tree_code(prover.circuit, po2, zk)
        data = hal.alloc_elem("data", wd * n)
        data.write(np.full(wd * n, POISON, dtype=np.uint32))
        with pytest.raises(HalError, match=re.escape(f"page_tree_witgen_nodes: node {missing} of layer {layer} is not in the dirty nodes")):
            hal.page_tree_witgen_nodes(prover.circuit, po2, zk, code, d["proof"], d["words"], other, 0, 3, data, NOISE)
        got = data.to_vec().reshape(wd, n)
        assert (got[:, :31 * t["B"]] == POISON).all(), "a cell of a block was written from a table of another proof"
        out = hal.page_tree_witgen_nodes(prover.circuit, po2, zk, code, d["proof"], d["words"], d["dirty"], 0, 3, data, NOISE)
        assert np.array_equal(out[:16], np.concatenate([nc.proved(*s, what)["root_before"], nc.proved(*s, what)["root_after"]]))


def test_a_table_that_does_not_fit_its_buffer_or_the_proof_is_refused_on_the_host(hal, provers):
    s, what = tc.H5, 3
    po2, zk, W = s
    t, d, p = nc.table(*s, what), _device(hal, s, what), nc.proved(*s, what)
    prover, n = provers[7], 1 << po2
    code = hal.page_tree_code(prover.circuit, po2, zk)
    data = hal.alloc_elem("data", G.WD * n)
    data.write(np.full(G.WD * n, POISON, dtype=np.uint32))
    call = lambda dirty, proof=d["proof"], words=d["words"]: hal.page_tree_witgen_nodes(prover.circuit, po2, zk, code, proof, words, dirty, 0, 3, data, NOISE)
    nodes, who = p["nodes"], "page_tree_witgen_nodes: "
    with pytest.raises(HalError, match=re.escape(who + "dirty nodes of 3 words: the header alone has 4")):
        call(hal.copy_from("dirty", nodes[:3]))
    magic = nodes.copy()
    magic[0] ^= 1
    with pytest.raises(HalError, match=re.escape(who + "dirty nodes: bad magic")):
        call(hal.copy_from("dirty", magic))
    with pytest.raises(HalError, match=re.escape(who + f"dirty nodes of {nodes.size - 1} words, but the header describes at least {nodes.size}")):
        call(hal.copy_from("dirty", nodes[:-1]))
    many = nodes.copy()
    many[4] = 4                                                               # four nodes on layer 1 from three rows
    with pytest.raises(HalError, match=re.escape(who + "dirty nodes: 4 nodes on layer 1, but 3 rows dirty at most 3 of its 16")):
        call(hal.copy_from("dirty", many))
    other = _device(hal, tc.H5, "random")                                     # the same image, 40 rows
    with pytest.raises(HalError, match=re.escape(who + f"dirty nodes of 40 rows over {W} words (h 5), but the proof has 3 rows over {W} words (h 5)")):
        call(other["dirty"])
    with pytest.raises(HalError, match=re.escape(who + "the part [2, 4) of a table of 3 rows")):
        hal.page_tree_witgen_nodes(prover.circuit, po2, zk, code, d["proof"], d["words"], d["dirty"], 2, 2, data, NOISE)
    assert (data.to_vec() == POISON).all(), "a refusal before any launch wrote into the data group"
    assert np.array_equal(call(d["dirty"])[:8], p["root_before"])
