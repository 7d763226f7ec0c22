"""The walk of a ZKU1 proof on the GPU (zkh_image_proof_walk; csrc/image.hip, the hashing lanes in csrc/hash.hip): for every (proof,
root_before) the device call and the host verifier zkh_image_proof_verify (hal.image_proof_verify, the yardstick) give the same root or
the same message after their prefixes, root_after is written only on success, the proof's buffer is only read, and no word past the
proof's length is looked at.  Proofs are built on the host (logup.reference_page_out_proof from a hand-made table), so the walk needs no
circuit on the device; one test takes the buffer zkh_page_out_proof wrote.  Where stated, a second route gives the root: p_out written
into the image, image_commit, image_root.

Shapes: W in {1, 7, 8, 9, 650, 1025} (L = 1: the leaf is the root; h = 1; partial and padding leaves), W = 1000 for the mutations, and
W = 2^17 + 5 (ceil(W / 8) = 2^14 + 1, so L = 2^15 and h = 15: lists of many workgroups).  Every layer takes the same four launches whatever its list holds, so the only
constant that switches a path is the workgroup size, 256: of the items of a list (flags, parents) and of the hashing lanes, two per
parent (128 parents).  Lists of 127 .. 129 and 255 .. 257 items that keep their count over many layers stand on both sides of each.
The seam tables of pages_cases (W = 4096) put a head decision of the row kernel, and of the flags of layer 0, on lane 0 of the second workgroup.

Mutants these cases are meant to catch: a carry dropped between scan workgroups (spread, twins, all at the big shape); the sibling on
the wrong side of an odd node, or taken when both children are dirty (twins, all, edges); old and new digests swapped or the new leaf
missing a row's out when several rows share a leaf (five, all, the mutation fixture); a section offset that ignores a layer with c_k = 0
(all, edges); a gate left open after a refusal (every mutation is followed by a good walk, and runs over two poisons)."""
import ctypes as C

import numpy as np
import pytest

import pages_cases as pc
from args_gpu import image_buf as _image, profiled, upload as _upload
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu
P = 2013265921
ONE = (1 << 32) % P
SLACK = 40
BIG_W = (1 << 17) + 5                                                        # 2^14 + 1 leaves hold words: L = 2^15, h = 15
BIG_H = 15
THREADS = 256                                                                # csrc/image.hip IMG_THREADS, the hashing kernel's workgroup
SCOPES = {"walk_check", "walk_leaves", "walk_layer", "walk_hash", "walk_top"}
u32p = C.POINTER(C.c_uint32)


def _words(rng, size, big=False):
    w = rng.integers(1, P, size, dtype=np.uint64).astype(np.uint32)
    if big:
        w[rng.random(size) < 0.33] += np.uint32(P)
    return w


@pytest.fixture(scope="module")
def args():
    return logup.Arguments.parse(pc.case("range5", 3, 8, 40)[1])


def _table(image, addrs, out, po2):
    data = np.zeros((pc.PAGED_W + 1, 1 << po2), dtype=np.uint32)
    D = len(addrs)
    data[pc.P_ON, :D], data[pc.P_ADDR, :D], data[pc.P_IN, :D], data[pc.P_OUT, :D] = ONE, pc.enc(addrs), image[addrs], out
    return data.reshape(-1)


def _po2(D):
    return max(int(D - 1).bit_length(), 3) if D > 1 else 3


def _host_proof(args, image, addrs, out, nodes):
    return logup.reference_page_out_proof(args, _po2(len(addrs)), 0, _table(image, addrs, out, _po2(len(addrs))), len(image), nodes)


def _raw(hal, buf, words, root, fill=0xdeadbeef):
    """the C call itself -> (None or the message, root_after as the call left it)"""
    lib = zhal.load_library()
    rb, after = np.ascontiguousarray(root, dtype=np.uint32), np.full(8, fill, dtype=np.uint32)
    err = lib.zkh_image_proof_walk(hal.ctx, buf.h, words, rb.ctypes.data_as(u32p), after.ctypes.data_as(u32p))
    if not err:
        return None, after
    msg = C.cast(err, C.c_char_p).value.decode()
    lib.zkh_free_error(err)
    return msg, after


def _host(proof, root):
    """the yardstick -> (None, root_after) or (the message after its prefix, None)"""
    try:
        return None, zhal.image_proof_verify(proof, root)
    except HalError as e:
        assert str(e).startswith("image_proof_verify: ")
        return str(e)[len("image_proof_verify: "):], None


def _agree(hal, proof, root, poisons=(0xdeadbeef,)):
    """walk `proof` on the device from a buffer SLACK words longer, once per poison of the slack: the buffer is only read, and the
    verdict, the message and the root are the host verifier's and the same for every poison -> (message, root_after)"""
    proof = np.ascontiguousarray(proof, dtype=np.uint32)
    want_msg, want_root = _host(proof, root)
    for poison in poisons:
        whole = np.concatenate([proof, np.full(SLACK, poison, dtype=np.uint32)])
        buf = hal.copy_from("proof", whole)
        msg, after = _raw(hal, buf, proof.size, root)
        assert np.array_equal(buf.to_vec(), whole), "the walk wrote into the proof's buffer"
        if want_msg is None:
            assert msg is None and np.array_equal(after, want_root), (msg, after, want_root)
        else:
            assert msg == "image_proof_walk: " + want_msg, (msg, want_msg)
            assert (after == 0xdeadbeef).all(), "root_after written on a refusal"
    return want_msg, want_root


def _refused(hal, proof, root, words, good=None, poisons=(0xdeadbeef,)):
    msg, _ = _agree(hal, proof, root, poisons)
    assert msg is not None and words in msg, msg
    if good is not None:                                                     # a good proof walked right afterwards gives the right root
        assert np.array_equal(hal.image_proof_walk(good[0], good[1]), good[2])
    return msg


# ---- 1. small images, every shape of the format ----
def _small_addresses(what, W, rng):
    if what == "none":
        return np.zeros(0, dtype=np.int64)
    if what == "one":
        return np.array([W // 2], dtype=np.int64)
    if what == "five":
        return np.sort(rng.choice(W, min(5, W), replace=False)).astype(np.int64)
    if what == "all":
        return np.arange(W, dtype=np.int64)
    if what == "edges":
        return np.unique(np.array([0, W - 1], dtype=np.int64))
    assert what == "twins"
    q = np.sort(rng.choice(max(W // 16, 1), min(3, max(W // 16, 1)), replace=False)).astype(np.int64)
    leaves = np.stack([2 * q, 2 * q + 1], axis=1).reshape(-1)
    a = np.stack([8 * leaves, 8 * leaves + 7], axis=1).reshape(-1)
    return a[a < W]


@pytest.mark.parametrize("W", [1, 7, 8, 9, 650, 1025])
@pytest.mark.parametrize("what", ["none", "one", "five", "all", "twins", "edges"])
def test_small_images(hal, args, W, what):
    rng = np.random.default_rng(1000 * W + 1)
    image = _words(rng, W)
    addrs = _small_addresses(what, W, rng)
    out = _words(rng, len(addrs))
    nodes = logup.reference_image_tree(image)
    proof = _host_proof(args, image, addrs, out, nodes)
    after = image.copy()
    after[addrs] = out
    msg, root = _agree(hal, proof, nodes[1])
    assert msg is None and np.array_equal(root, logup.reference_image_tree(after)[1])
    assert np.array_equal(hal.image_proof_walk(proof, nodes[1]), root)      # the wrapper, from an array


def test_raw_words_above_p_give_the_proof_of_their_residues(hal, args):
    W = 1000
    rng = np.random.default_rng(77)
    image = _words(rng, W, big=True)
    addrs = np.sort(rng.choice(W, 40, replace=False)).astype(np.int64)
    out = _words(rng, 40, big=True)
    assert (image >= P).sum() > 200 and (out >= P).any()
    proof = _host_proof(args, image, addrs, out, logup.reference_image_tree(image))
    assert (proof[5 + int(proof[4]):] < np.uint32(P)).all()
    after = image.copy()
    after[addrs] = out
    msg, root = _agree(hal, proof, logup.reference_image_root(image))
    assert msg is None and np.array_equal(root, logup.reference_image_root(after))


# ---- 2. the layered kernels: W = 2^17 + 5 ----
@pytest.fixture(scope="module")
def big(hal):
    """(image, nodes as the device commits them, read back once); a third of the words raw words >= P"""
    image = _words(np.random.default_rng(BIG_W), BIG_W, big=True)
    return image, hal.image_commit(_image(hal, image)).to_vec()


def _big_addresses(what, rng):
    W, L = BIG_W, 1 << BIG_H
    if what == "spread":
        return np.sort(rng.choice(W, 6000, replace=False)).astype(np.int64)
    if what == "twins":
        q = np.sort(rng.choice(W // 16 - 1, 1500, replace=False)).astype(np.int64)         # the leaves that hold words
        leaves = np.stack([2 * q, 2 * q + 1], axis=1).reshape(-1)
        return np.stack([8 * leaves, 8 * leaves + 7], axis=1).reshape(-1)
    if what == "edges":                                                      # both ends; both sides of a leaf boundary; items 255 / 256 / 257 of S_0
        run = 8 * np.arange(300, dtype=np.int64) + 3                         # leaves 0 .. 299, one row each: item j is leaf j
        extra = np.array([0, 7, 8, 8 * 255 + 7, 8 * 256, 8 * 256 + 7, 8 * 257, W - 1, W - 6, 8 * ((W - 1) // 8) - 1], dtype=np.int64)
        return np.unique(np.concatenate([run, extra]))
    if what == "all":
        return np.arange(W, dtype=np.int64)
    if what == "one":
        return np.array([W // 3], dtype=np.int64)
    count = int(what)                                                        # `count` leaves far apart: the lists keep their count for many layers
    step = 1 << ((W // 8 // count).bit_length() - 1)                         # a power of two: no two of the leaves are siblings on the way up
    return 8 * (np.arange(count, dtype=np.int64) * step + rng.integers(0, step, count)) + rng.integers(0, 8, count)


BIG_TABLES = ["spread", "twins", "edges", "all", "one"] + [str(c + d) for c in (THREADS // 2, THREADS) for d in (-1, 0, 1)]


@pytest.mark.parametrize("what", BIG_TABLES)
def test_layers_of_many_workgroups(hal, args, big, what):
    image, nodes = big
    rng = np.random.default_rng(len(what) + 17)
    addrs = _big_addresses(what, rng)
    assert (np.diff(addrs) > 0).all() and addrs[-1] < BIG_W
    out = _words(rng, len(addrs), big=True)
    proof = _host_proof(args, image, addrs, out, nodes)
    assert int(proof[4]) == BIG_H
    c = [int(x) for x in proof[5:5 + BIG_H]]
    if what == "all":                                                        # the last leaf with words is an even node: its sibling is padding, and clean
        assert int(proof[3]) == (BIG_W + 7) // 8 and c == [1] * (BIG_H - 1) + [0]
    if what.isdigit():                                                       # every leaf alone in its aligned block: the lists keep their count
        keeps = (BIG_W // 8 // int(what)).bit_length() - 1
        assert int(proof[3]) == int(what) and keeps >= 4 and c[:keeps] == [int(what)] * keeps, c
    msg, root = _agree(hal, proof, nodes[8:16])
    after = image.copy()
    after[addrs] = out
    assert msg is None and np.array_equal(root, hal.image_root(hal.image_commit(_image(hal, after))))


@pytest.mark.parametrize("D", pc.SEAM_ROWS)
@pytest.mark.parametrize("what", pc.SEAM_TABLES)
def test_a_head_on_the_seam_of_two_workgroups(hal, args, what, D):
    """rows 255 and 256 share a leaf, lie in sibling leaves, or lie under different parents (pages_cases.seam_table): the walk returns the
    host verifier's root_after, which is the root of the paged-out image"""
    W, po2, zk = 4096, 10, 40
    rng = np.random.default_rng(D + len(what))
    image = _words(rng, W, big=True)
    addrs = pc.seam_table(what, D, W, rng)
    out = _words(rng, D, big=True)
    nodes = logup.reference_image_tree(image)
    proof = logup.reference_page_out_proof(args, po2, zk, _table(image, addrs, out, po2), W, nodes)
    assert [int(x) for x in proof[1:3]] == [W, D] and int(proof[4]) == 9
    msg, root = _agree(hal, proof, nodes[1])
    image[addrs] = out
    assert msg is None and np.array_equal(root, logup.reference_image_root(image))


# ---- 3. a device-built proof, and the prover ----
def _paged(hal, po2, zk, W):
    desc, blob = syn_lookup.build_syn_lookup(syn_lookup.TINY, derive=True, limbs=True, link=True, reads=True, pages=True)
    image = np.random.default_rng(po2).integers(1, P, W, dtype=np.uint64).astype(np.uint32)
    code, _, _ = syn_lookup.witness(syn_lookup.TINY, po2, zk, seed=po2, addr_range=W, link=True, reads=True, pages=True, image=image)
    _, bare, _ = syn_lookup.witness(syn_lookup.TINY, po2, zk, seed=po2, addr_range=W, count=False, limbs=False, link=False, reads=True, pages=False, image=image)
    prover = SegmentProver(hal, desc, arguments=blob)

    def fresh(tree_of=None):
        dcode, ddata = _upload(hal, np.ascontiguousarray(code).reshape(-1), np.ascontiguousarray(bare).reshape(-1))
        dimage = _image(hal, image)
        tree = hal.image_commit(_image(hal, image if tree_of is None else tree_of))
        hal.derive_all_paged(prover.circuit, po2, zk, dcode, ddata, dimage)
        return ddata, dimage, tree
    return prover, Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=0x0C07), image, fresh


@pytest.mark.parametrize("po2,zk,W", [(8, 40, 64), (12, 1994, 1000)])
def test_a_device_built_proof_goes_straight_into_the_walk(hal, po2, zk, W):
    prover, seg, image, fresh = _paged(hal, po2, zk, W)
    ddata, dimage, tree = fresh()
    buf = hal.copy_from("proof", np.full(hal.image_proof_words(W, (1 << po2) - zk) + SLACK, 0xdeadbeef, dtype=np.uint32))
    words = hal.page_out_proof(prover.circuit, po2, zk, ddata, dimage, tree, proof=buf)
    root0 = hal.image_root(tree)
    assert int(words[2]) > 0 and words.size < buf.size()
    walked = hal.image_proof_walk(buf, root0, words=words.size)              # the buffer page_out_proof wrote, and the proof's own length
    hal.page_out_tree(prover.circuit, po2, zk, ddata, dimage, tree)
    assert np.array_equal(walked, hal.image_root(tree)) and not np.array_equal(walked, root0)
    assert np.array_equal(walked, zhal.image_proof_verify(words, root0))
    with pytest.raises(HalError, match=f"image_proof_walk: a proof of {buf.size()} words, but the header describes {words.size}"):
        hal.image_proof_walk(buf, root0)                                     # words defaults to the whole buffer
    # the prover: the same words with and without the walk
    ddata, dimage, tree = fresh()
    plain = prover.page_out(seg, ddata, dimage, tree=tree, proof=True)
    ddata, dimage, tree = fresh()
    checked = prover.page_out(seg, ddata, dimage, tree=tree, proof=True, walk=True)
    assert np.array_equal(plain, words) and np.array_equal(checked, words) and np.array_equal(hal.image_root(tree), walked)
    # a tree that is not the image's: the tree of an image that differs in a word the table does not page, inside a leaf it does
    paged = set(int(a) for a in words[5 + int(words[4]):5 + int(words[4]) + 3 * int(words[2]):3])
    near = [a for a in range(W) if a not in paged and any((a ^ b) < 8 for b in paged)]
    other = image.copy()
    other[near[0] if near else 0] ^= np.uint32(1)
    ddata, dimage, tree = fresh(tree_of=other)
    with pytest.raises(HalError) as e:
        prover.page_out(seg, ddata, dimage, tree=tree, proof=True, walk=True)
    if near:
        assert "page_out: the proof walks to root " in str(e.value) and ", but the tree's root after the page-out is " in str(e.value), str(e.value)


# ---- 5. refusals, message for message ----
@pytest.fixture(scope="module")
def good(args):
    """W = 1000 (h = 7), 5 spread rows plus two rows in one leaf: (proof, root_before, root_after, layout)"""
    rng = np.random.default_rng(1000)
    W = 1000
    image = _words(rng, W)
    addrs = np.array([3, 4, 100, 101 + 8, 333, 500, 999], dtype=np.int64)
    out = _words(rng, len(addrs))
    nodes = logup.reference_image_tree(image)
    proof = _host_proof(args, image, addrs, out, nodes)
    after = zhal.image_proof_verify(proof, nodes[1])
    image[addrs] = out
    assert np.array_equal(after, logup.reference_image_root(image))
    h, D, M = int(proof[4]), int(proof[2]), int(proof[3])
    t0 = 5 + h
    return proof, nodes[1].copy(), after, {"t0": t0, "l0": t0 + 3 * D, "s0": t0 + 3 * D + 8 * M, "D": D, "M": M, "h": h}


def _bump(word):
    return np.uint32((int(word) + 1) % P)


def _count_mutants(proof, h):
    """sibling counts +-1 with the length kept consistent, leaf count +-1: (the mutant, words of its message)"""
    c = [int(x) for x in proof[5:5 + h]]
    M = int(proof[3])
    k = next(k for k in range(h) if c[k] >= 1 and k >= 2)
    j = next(j for j in range(h) if j != k and c[j] >= 1)
    out = []
    for step in (1, -1):
        bad = proof.copy()
        bad[5 + k], bad[5 + j] = c[k] + step, c[j] - step
        first = min(k, j)
        moved = step if first == k else -step
        out.append((bad, f"layer {first}: {c[first] + moved} siblings, but the walk takes {c[first]}"))
        bad = proof.copy()
        bad[3], bad[5] = M + step, c[0] - step
        out.append((bad, f"M {M + step}, but the table's rows lie in {M} leaves"))
    return out


def test_refusals_message_for_message(hal, good):
    proof, root, after, at = good
    ok = (proof, root, after)
    t0, l0, s0 = at["t0"], at["l0"], at["s0"]
    cases = []

    def mutant(words, *edits, root_=None):
        bad = proof.copy()
        for off, v in edits:
            bad[off] = v
        cases.append((bad, root if root_ is None else root_, words))
    for off in (s0, s0 + 11, proof.size - 1):                                # a flipped sibling word
        mutant("not root_before", (off, _bump(proof[off])))
    mutant("not root_before", (l0 + 6, _bump(proof[l0 + 6])))                # a flipped unpaged leaf word
    mutant(f"row 2: in {int(_bump(proof[t0 + 7]))} at address 100, but its leaf holds {int(proof[t0 + 7])}", (t0 + 7, _bump(proof[t0 + 7])))
    mutant(f"row 1: in {int(_bump(proof[t0 + 4]))} at address 4, but", (t0 + 4, _bump(proof[t0 + 4])))     # the second row of a shared leaf
    swapped = proof.copy()
    r3, r4 = t0 + 9, t0 + 12
    swapped[r3:r3 + 3], swapped[r4:r4 + 3] = proof[r4:r4 + 3], proof[r3:r3 + 3]
    cases.append((swapped, root, "row 4: address 109 does not follow a smaller one (row 3: address 333)"))
    mutant("row 6: address 1000 outside the image of 1000 words", (t0 + 18, 1000))
    mutant("row 0: address 4000000000 outside the image", (t0, 4000000000))
    mutant("row 1: address 3 does not follow a smaller one (row 0: address 3)", (t0 + 3, 3))
    cases.extend((bad, root, words) for bad, words in _count_mutants(proof, at["h"]))
    cases.append((proof[:-1], root, f"a proof of {proof.size - 1} words, but the header describes {proof.size}"))
    cases.append((np.concatenate([proof, proof[-1:]]), root, f"a proof of {proof.size + 1} words, but the header describes {proof.size}"))
    cases.append((proof[:4], root, "a proof of 4 words: the header alone has 5"))
    cases.append((proof[:0], root, "a proof of 0 words: the header alone has 5"))
    cases.append((proof[:8], root, "a proof of 8 words, but the header describes at least 12"))
    for off in (t0 + 1, t0 + 5, l0 + 2, s0 + 9, proof.size - 1):             # a word + P in each section
        mutant(f"word {off} is {int(proof[off]) + P}, not below P", (off, proof[off] + np.uint32(P)))
    other = root.copy()
    other[5] = _bump(other[5])
    mutant("the proof opens root " + " ".join(f"{int(w):08x}" for w in root) + ", not root_before", root_=other)
    above = root.copy()
    above[7] += np.uint32(P)
    mutant("root_before is not 8 words below P", root_=above)
    mutant("bad magic 0x5a4b4131 (ZKU1 is 0x5a4b5531)", (0, 0x5A4B4131))
    mutant("h 6, but an image of 1000 words has h 7", (4, 6))
    mutant("h 7, but an image of 1025 words has h 8", (1, 1025))
    # two causes at once: the host verifier's order decides
    mutant(f"word {s0 + 9} is ", (s0 + 9, proof[s0 + 9] + np.uint32(P)), (t0 + 9, proof[t0 + 12]), (t0 + 12, proof[t0 + 9]))
    two = _count_mutants(proof, at["h"])[0][0]
    two[t0 + 7] = _bump(two[t0 + 7])
    cases.append((two, root, "row 2: in "))
    mutant("word ", (t0 + 5, proof[t0 + 5] + np.uint32(P)), root_=above)     # a word >= P comes before root_before
    for bad, rb, words in cases:
        _refused(hal, bad, rb, words, good=ok)
    with pytest.raises(HalError, match="image_proof_walk: a proof of 5000 words in a buffer of "):
        hal.image_proof_walk(hal.copy_from("proof", proof), root, words=5000)


def test_an_empty_table_with_a_leaf_count(hal):
    """D = 0 with M = 1, the length what the header describes; and D = 0 with a sibling count"""
    W = 1000
    h = 7
    root = _words(np.random.default_rng(3), 8)
    head = np.array([0x5A4B5531, W, 0, 1, h] + [0] * h, dtype=np.uint32)
    _refused(hal, np.concatenate([head, _words(np.random.default_rng(4), 8)]), root, "M 1, but the table's rows lie in 0 leaves")
    head[3], head[5 + 2] = 0, 1
    _refused(hal, np.concatenate([head, _words(np.random.default_rng(4), 8)]), root, "layer 2: 1 siblings, but the walk takes 0")
    head[5 + 2] = 0
    msg, after = _agree(hal, head, root)                                     # the header alone: root_after = root_before, nothing launched
    assert msg is None and np.array_equal(after, root)
    assert not SCOPES & set(profiled(hal, lambda: hal.image_proof_walk(head, root)))


@pytest.mark.parametrize("what", ["counts", "in"])
def test_refusals_where_the_layered_kernels_run(hal, args, big, what):
    """4. and 5. at the 2^17 + 5 shape: the sibling-count and wrong-`in` mutants, the slack poisoned twice"""
    image, nodes = big
    rng = np.random.default_rng(23)
    addrs = _big_addresses("spread", rng)
    out = _words(rng, len(addrs))
    proof = _host_proof(args, image, addrs, out, nodes)
    root = nodes[8:16]
    ok = (proof, root, zhal.image_proof_verify(proof, root))
    t0 = 5 + BIG_H
    if what == "counts":
        for bad, words in _count_mutants(proof, BIG_H):
            _refused(hal, bad, root, words, good=ok, poisons=(0xdeadbeef, 0x00000001))
        return
    for row in (5999, 4097, 300):                                            # the lowest wins, whatever the order of arrival
        proof[t0 + 3 * row + 1] = _bump(proof[t0 + 3 * row + 1])
        msg = _refused(hal, proof, root, f"row {row}: in ", poisons=(0xdeadbeef, 0x00000001))
    assert f"at address {int(addrs[300])}, but its leaf holds {int(image[addrs[300]] % P)}" in msg


def test_read_only_and_bounded(hal, good):
    """4.: two poisons of the slack give identical results, on the good proof and on the count mutants"""
    proof, root, after, at = good
    msg, got = _agree(hal, proof, root, poisons=(0xdeadbeef, 0x7fffffff, 0))
    assert msg is None and np.array_equal(got, after)
    for bad, words in _count_mutants(proof, at["h"]):
        _refused(hal, bad, root, words, poisons=(0xdeadbeef, 0x7fffffff, 0))


# ---- 6. a flipped out ----
def test_a_flipped_out_succeeds_with_another_root(hal, good):
    proof, root, after, at = good
    bad = proof.copy()
    bad[at["t0"] + 3 * 4 + 2] = _bump(bad[at["t0"] + 3 * 4 + 2])
    msg, other = _agree(hal, bad, root)
    assert msg is None and not np.array_equal(other, after)


# ---- 7. fuzz ----
def test_fuzz_against_the_host_verifier(hal, args):
    rng = np.random.default_rng(2024)
    verdicts = {"ok": 0, "refused": 0}
    for case in range(200):
        W = int(rng.integers(1, 301))
        image = _words(rng, W)
        D = int(rng.integers(0, W + 1)) if rng.random() < 0.5 else int(rng.integers(0, min(W, 6) + 1))
        addrs = np.sort(rng.choice(W, D, replace=False)).astype(np.int64)
        out = _words(rng, D)
        nodes = logup.reference_image_tree(image)
        proof = _host_proof(args, image, addrs, out, nodes)
        root = nodes[1].copy()
        if case % 2:
            proof[int(rng.integers(0, proof.size))] = np.uint32(rng.integers(0, 1 << 32))
        elif case % 8 == 0:
            root[int(rng.integers(0, 8))] = np.uint32(rng.integers(0, 1 << 32))
        msg, _ = _agree(hal, proof, root)
        verdicts["ok" if msg is None else "refused"] += 1
    assert verdicts["ok"] >= 60 and verdicts["refused"] >= 60, verdicts


# ---- 8. twice the same, 9. the profiler's scopes ----
def test_twice_the_same_and_the_scopes(hal, args, big):
    image, nodes = big
    rng = np.random.default_rng(31)
    addrs = _big_addresses("twins", rng)
    proof = _host_proof(args, image, addrs, _words(rng, len(addrs)), nodes)
    buf = hal.copy_from("proof", proof)
    got = []
    prof = profiled(hal, lambda: got.append(hal.image_proof_walk(buf, nodes[8:16])))
    assert SCOPES <= set(prof), set(prof)
    assert prof["walk_layer"]["calls"] == prof["walk_hash"]["calls"] == BIG_H and prof["walk_top"]["calls"] == 1
    got.append(hal.image_proof_walk(buf, nodes[8:16]))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], zhal.image_proof_verify(proof, nodes[8:16]))
    bad = proof.copy()
    bad[5 + BIG_H + 3 * 700 + 1] = _bump(bad[5 + BIG_H + 3 * 700 + 1])
    first, again = _raw(hal, hal.copy_from("proof", bad), bad.size, nodes[8:16]), _raw(hal, hal.copy_from("proof", bad), bad.size, nodes[8:16])
    assert first[0] == again[0] and "row 700: in " in first[0] and np.array_equal(first[1], again[1])
