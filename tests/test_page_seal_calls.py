"""The host layer that seals and verifies page-outs, WITHOUT a device: which calls every sealing entry point makes, with which operands
and in which order; the texts of its refusals; and which refusal a verifier gives when two causes hold at once.

The six sealing entry points (SegmentProver.seal_page_out, seal_page_out_parts, seal_page_out_ordered, seal_page_out_tree with
plan="host", prover.seal_tied and prover.seal_tied_tree) run over a recording stub: a SegmentProver that opens no context and a hal
whose page, alloc, copy_from, accumulate_open and table_fingerprint methods append (name, operands) to one log and hand back
placeholders; page_tree_plan and page_circuit_slots are the real host-only functions, and the challenge is hal.tie_challenge's.  The
whole log of each entry point is compared with the one recorded in tests/golden/page_seal_calls.json, which was written once from the
code as it stood when every entry point still drove the hal by hand.  seal_page_out alone is compared without its code_root call,
which is asserted to happen once: the call reads only the code group, and whether it comes before or after the witness is not pinned.

The proofs are real ZKU1 words made on the host: page_circuit_cases' h = 5 shape with the table of 2N + 3 rows (three parts) for the
circuits that lay out paths, and page_tree_cases' image of 64 words with every word paged at (po2 8, zk 40), 6 block slots and so two
parts, for those that lay out dirty nodes.

Last, page_seal.PAGE_KINDS, the one table of the kinds that seal a page-out, is held against the circuit modules it names."""
import json
import os
import re

import numpy as np
import pytest

import page_circuit_cases as cases
import page_ordered_cases as oc
import page_tree_cases as tc
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, p2_blocks, p2_page, p2_page_ordered, p2_page_tied, p2_tree, p2_tree_tied, syn_lookup as sl
from zeth_amd.hal import HalError
from zeth_amd.prover import (Segment, SegmentProver, SegmentReceipt, seal_tied, seal_tied_tree, verify_page_ordered_chain, verify_page_out_chain,
                             verify_page_tree_chain, verify_tied, verify_tied_tree)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "page_seal_calls.json")
PATHS = cases.SHAPES[1]                                                           # (12, 1994, 8 * 17 + 3): h = 5, 13 slots
TREES = (8, 40, 64)                                                               # h = 3, 6 block slots: the 7 nodes of a full image take two parts
NOISE = 0x5EA1


# ------------------------------------------------------------------------------------------------ the recording stub
class Buf(zhal.Buffer):
    """a device buffer that is only a name and a size; one made by copy_from also holds its words, which slice / to_vec read"""

    def __init__(self, name, n, words=None):
        self.hal, self.h, self.name, self.n, self.words = None, None, name, int(n), words

    def size(self):
        return self.n

    def slice(self, offset, size):
        assert offset + size <= self.n
        return Buf(self.name, size, self.words[offset:offset + size])

    def to_vec(self):
        return np.array(self.words, dtype=np.uint32)


def _enc(x):
    """an operand as the log holds it"""
    if isinstance(x, Buf):
        return f"{x.name}[{x.n}]"
    if isinstance(x, StubCircuit):
        return f"circuit {x.name}"
    if isinstance(x, np.ndarray):
        return [int(w) for w in x.reshape(-1)]
    if isinstance(x, (list, tuple)):
        return [_enc(y) for y in x]
    assert x is None or isinstance(x, (bool, int, str, np.integer)), type(x)
    return x if x is None or isinstance(x, (bool, str)) else int(x)


class StubCircuit:
    def __init__(self, name, desc, arguments, open_bus):
        self.name, self.desc, self._arguments, self._open_bus = name, np.asarray(desc, dtype=np.uint32), arguments, open_bus

    def has_arguments(self):
        return self._arguments

    def open_bus(self):
        return (logup.TIE_TAG, 4, 8, 12) if self._open_bus else None


class StubHal:
    """every call is logged as [name, operand, ...]; what a call returns is a placeholder of the right size"""

    def __init__(self, log):
        self.log, self.opens, self.total = log, 0, None

    def _call(self, name, *operands):
        self.log.append([name] + [_enc(x) for x in operands])

    def alloc(self, name, n_words, zero=False):
        self._call("alloc", name, n_words, zero)
        return Buf(name, n_words)

    def alloc_elem(self, name, size):
        self._call("alloc_elem", name, size)
        return Buf(name, size)

    def copy_from(self, name, host):
        words = np.ascontiguousarray(host, dtype=np.uint32).reshape(-1)
        self._call("copy_from", name, words.size)
        return Buf(name, words.size, words)

    def _code(self, name, circuit, po2, *shape):
        self._call(name, circuit, po2, *shape)
        return Buf("code", int(circuit.desc[4]) << po2)

    def page_circuit_code(self, circuit, po2, zk_cycles, image_words):
        return self._code("page_circuit_code", circuit, po2, zk_cycles, image_words)

    def page_ordered_code(self, circuit, po2, zk_cycles, image_words):
        return self._code("page_ordered_code", circuit, po2, zk_cycles, image_words)

    def page_tree_code(self, circuit, po2, zk_cycles):
        return self._code("page_tree_code", circuit, po2, zk_cycles)

    def _witgen(self, name, out_words, *operands):
        self._call(name, *operands)
        return np.arange(1000, 1000 + out_words, dtype=np.uint32)

    def page_circuit_witgen(self, circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, data, noise_seed):
        return self._witgen("page_circuit_witgen", 16, circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, data, noise_seed)

    def page_circuit_witgen_part(self, circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, first, data, noise_seed):
        return self._witgen("page_circuit_witgen_part", 16, circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, first, data, noise_seed)

    def page_ordered_witgen(self, circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, first, data, noise_seed):
        return self._witgen("page_ordered_witgen", 18, circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, first, data, noise_seed)

    def page_tree_witgen(self, circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, first, count, data, noise_seed):
        return self._witgen("page_tree_witgen", 18, circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, first, count, data, noise_seed)

    def page_circuit_slots(self, po2, zk_cycles, image_words):
        self._call("page_circuit_slots", po2, zk_cycles, image_words)
        zhal.load_library()
        return zhal.HipHal.page_circuit_slots(self, po2, zk_cycles, image_words)

    def page_tree_plan(self, po2, zk_cycles, image_words, addrs):
        self._call("page_tree_plan", po2, zk_cycles, image_words, np.asarray(addrs))
        return zhal.page_tree_plan(po2, zk_cycles, image_words, addrs)

    def accumulate_open(self, circuit, po2, zk_cycles, noise_seed, code, data, challenge, accum):
        self._call("accumulate_open", circuit, po2, zk_cycles, noise_seed, code, data, np.asarray(challenge), accum)
        self.opens += 1
        self.total = np.arange(4, dtype=np.uint32) + np.uint32(10 * self.opens)
        return self.total

    def table_fingerprint(self, table, table_at, rows, challenge):
        self._call("table_fingerprint", table, table_at, rows, np.asarray(challenge))
        return self.total.copy()


class StubProver(SegmentProver):
    """a SegmentProver of the circuit `desc` that opens no context: what reaches the device is logged instead"""

    def __init__(self, name, hal, desc, arguments=True, open_bus=True):
        self.name, self.hal, self.log, self.roots = name, hal, hal.log, 0
        self.circuit = StubCircuit(name, desc, arguments, open_bus)
        self._group_sizes = tuple(int(x) for x in self.circuit.desc[3:6])

    def code_root(self, code, po2):
        self.log.append(["code_root", self.name, _enc(code), po2])
        return np.arange(8, dtype=np.uint32) + np.uint32(500)

    def data_root(self, data, po2):
        self.log.append(["data_root", self.name, _enc(data), po2])
        self.roots += 1
        return np.full(8, len(self.name) + 100 * self.roots, dtype=np.uint32)

    def _accumulate(self, how, seg, *operands):
        self.log.append([how, self.name, seg.index] + [_enc(x) for x in operands])
        return lambda _mix: Buf(f"accum of {how}", self._group_sizes[0] << seg.po2)

    def syn_accumulate(self, seg, data):
        return self._accumulate("syn_accumulate", seg, data)

    def args_accumulate(self, seg, code, data, check=False):
        return self._accumulate("args_accumulate", seg, code, data, check)

    def seal_with_accum(self, seg, code, data, out_global, accumulate, check=False):
        out = np.ascontiguousarray(out_global, dtype=np.uint32)
        accum = accumulate(np.zeros(int(self.circuit.desc[8]), dtype=np.uint32))
        self.log.append(["seal_with_accum", self.name, seg.index, seg.po2, seg.zk_cycles, seg.noise_seed, _enc(code), _enc(data), _enc(out), _enc(accum), check])
        return SegmentReceipt(seal=out.copy(), index=seg.index, po2=seg.po2, output=out.copy())


def _segs(shape, parts, first=1):
    return [Segment(index=first + p, po2=shape[0], zk_cycles=shape[1], noise_seed=NOISE + first + p) for p in range(parts)]


def _proof(t):
    return cases.host_proof(t["image"], t["addrs"], t["outs"], logup.reference_image_tree(t["image"]).reshape(-1))


@pytest.fixture(scope="module")
def path_proof():
    t = oc.table(*PATHS, "2N+3")
    assert len(t["plan"]) == 3 and t["N"] == 13
    return _proof(t)


@pytest.fixture(scope="module")
def tree_proof():
    t = tc.table(*TREES, "all")
    assert t["plan"] == p2_tree.parts(*TREES, range(64)) and len(t["plan"]) == 2 and t["B"] == 6
    return _proof(t)


class Rig:
    """one log, one hal, and the operands every entry point takes"""

    def __init__(self):
        self.log = []
        self.hal = StubHal(self.log)
        self.before, self.after = Buf("nodes_before", 1), Buf("nodes_after", 1)

    def prover(self, desc, **kw):
        return StubProver("page", self.hal, desc, **kw)

    def segment(self, **kw):
        """the segment side of a tied group -> the operands seal_tied takes before the page-out's"""
        desc, _ = sl.syn_lookup_tiny_tied()
        prover = StubProver("segment", self.hal, desc, **kw)
        wa, wc, wd = prover.group_sizes()
        return prover, Segment(index=0, po2=8, zk_cycles=40, noise_seed=NOISE), Buf("segment code", wc << 8), Buf("segment data", wd << 8)


def _untied(rig, entry, desc, shape, parts, proof, check=False, **kw):
    prover = rig.prover(desc)
    return getattr(prover, entry)(_segs(shape, parts), proof, proof.size, rig.before, rig.after, check=check, **kw)


def _tied(rig, seal, desc, shape, parts, proof, prefix=4, seg_kw={}, page_kw={}, segs=None, **kw):
    seg_prover, seg, code, data = rig.segment(**seg_kw)
    return seal(seg_prover, seg, code, data, np.zeros(prefix, dtype=np.uint32), rig.prover(desc, **page_kw), _segs(shape, parts) if segs is None else segs,
                proof, proof.size, rig.before, rig.after, **kw)


def _run(entry, path_proof, tree_proof):
    """-> (the log, the receipts of the page-out's parts) of one entry point"""
    rig = Rig()
    if entry == "seal_page_out":
        receipts = [rig.prover(p2_page.p2_page_circuit()).seal_page_out(_segs(PATHS, 1)[0], path_proof, path_proof.size, rig.before, rig.after, check=True)]
    elif entry == "seal_page_out_parts":
        receipts = _untied(rig, entry, p2_page.p2_page_circuit(), PATHS, 3, path_proof)
    elif entry == "seal_page_out_ordered":
        receipts = _untied(rig, entry, p2_page_ordered.p2_page_ordered_circuit(), PATHS, 3, path_proof, check=True)
    elif entry == "seal_page_out_tree":
        receipts = _untied(rig, entry, p2_tree.p2_tree_circuit(), TREES, 2, tree_proof, check=True, plan="host")
    elif entry == "seal_tied":
        _, receipts = _tied(rig, seal_tied, p2_page_tied.p2_page_tied_circuit(), PATHS, 3, path_proof, check=True)
    else:
        _, receipts = _tied(rig, seal_tied_tree, p2_tree_tied.p2_tree_tied_circuit(), TREES, 2, tree_proof)
    return rig.log, receipts


ENTRY_POINTS = ["seal_page_out", "seal_page_out_parts", "seal_page_out_ordered", "seal_page_out_tree", "seal_tied", "seal_tied_tree"]


def _pinned(entry, log):
    """the part of an entry point's log that the golden file holds: all of it, but for seal_page_out's one code_root call"""
    if entry != "seal_page_out":
        return log
    roots = [c for c in log if c[0] == "code_root"]
    assert roots == [["code_root", "page", f"code[{p2_page.WC << PATHS[0]}]", PATHS[0]]]
    return [c for c in log if c[0] != "code_root"]


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_an_entry_point_makes_the_recorded_calls_in_the_recorded_order(entry, path_proof, tree_proof):
    log, receipts = _run(entry, path_proof, tree_proof)
    with open(GOLDEN) as fh:
        want = json.load(fh)[entry]
    got = _pinned(entry, log)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"call {i}"
    assert len(got) == len(want)
    assert len(receipts) == {"seal_page_out": 1, "seal_page_out_tree": 2, "seal_tied_tree": 2}.get(entry, 3)
    for r in receipts:                                                            # every part carries the one code group's root
        assert np.array_equal(r.control_root, np.arange(8) + 500)


# ------------------------------------------------------------------------------------------------ the refusals
def _refuses(text):
    return pytest.raises(HalError, match=f"^{re.escape(text)}$")


def test_the_refusals_of_the_untied_chains(path_proof, tree_proof):
    page, tree = p2_page_ordered.p2_page_ordered_circuit(), p2_tree.p2_tree_circuit()
    with _refuses("seal_page_out_parts: no segment"):
        _untied(Rig(), "seal_page_out_parts", p2_page.p2_page_circuit(), PATHS, 0, path_proof)
    with _refuses("seal_page_out_ordered: the parts share one code group: every segment must have the same (po2, zk_cycles)"):
        Rig().prover(page).seal_page_out_ordered(_segs(PATHS, 2) + _segs((12, 200), 1), path_proof, path_proof.size, None, None)
    with _refuses("seal_page_out_ordered: 2 segments, but a table of 29 rows takes 3 parts of 13 slots at po2 12"):
        _untied(Rig(), "seal_page_out_ordered", page, PATHS, 2, path_proof)
    with _refuses("seal_page_out_tree: 3 segments, but a table of 64 rows takes 2 parts of 6 block slots at po2 8"):
        _untied(Rig(), "seal_page_out_tree", tree, TREES, 3, tree_proof)
    with _refuses('seal_page_out_tree: plan="gpu" (the plan is made on the "host" or on the "device")'):
        _untied(Rig(), "seal_page_out_tree", tree, TREES, 0, tree_proof, plan="gpu")          # before the segments are looked at
    with _refuses("seal_page_out_tree: the prover was built without P2-TREE's arguments (arguments=p2_tree.arguments())"):
        Rig().prover(tree, arguments=False).seal_page_out_tree(_segs(TREES, 2), tree_proof, tree_proof.size, None, None)
    D = int(tree_proof[2])
    with _refuses(f"seal_page_out_tree: a proof of {5 + 3 + 3 * D - 1} words does not hold its header and a table of {D} rows"):
        Rig().prover(tree).seal_page_out_tree(_segs(TREES, 2), tree_proof, 5 + 3 + 3 * D - 1, None, None)


def test_the_refusals_of_the_tied_groups(path_proof, tree_proof):
    page, tree = p2_page_tied.p2_page_tied_circuit(), p2_tree_tied.p2_tree_tied_circuit()
    with _refuses("seal_tied: no segment for the page-out (a page-out of no rows still has one part)"):
        _tied(Rig(), seal_tied, page, PATHS, 0, path_proof)
    with _refuses("seal_tied_tree: the parts share one code group: every segment must have the same (po2, zk_cycles)"):
        _tied(Rig(), seal_tied_tree, tree, TREES, 0, tree_proof, segs=_segs(TREES, 1) + _segs((8, 41), 1))
    with _refuses("seal_tied: 2 segments, but a table of 29 rows takes 3 parts of 13 slots at po2 12"):
        _tied(Rig(), seal_tied, page, PATHS, 2, path_proof)
    with _refuses("seal_tied_tree: 1 segments, but a table of 64 rows takes 2 parts of 6 block slots at po2 8"):
        _tied(Rig(), seal_tied_tree, tree, TREES, 1, tree_proof)
    with _refuses("seal_tied: the segment prover's circuit has no open bus (its arguments hold no OPEN record)"):
        _tied(Rig(), seal_tied, page, PATHS, 3, path_proof, seg_kw={"open_bus": False}, page_kw={"open_bus": False})
    with _refuses("seal_tied: the page-out prover's circuit has no open bus (its arguments hold no OPEN record)"):
        _tied(Rig(), seal_tied, page, PATHS, 0, path_proof, page_kw={"open_bus": False})        # before the segments are looked at
    with _refuses('seal_tied_tree: plan="gpu" (the plan is made on the "host" or on the "device")'):
        _tied(Rig(), seal_tied_tree, tree, TREES, 2, tree_proof, seg_kw={"open_bus": False}, plan="gpu")      # before the buses are
    with _refuses("seal_tied_tree: the prover was built without P2-TREE's arguments (arguments=p2_tree.arguments())"):
        _tied(Rig(), seal_tied_tree, tree, TREES, 2, tree_proof, page_kw={"arguments": False})
    with _refuses("seal_tied_tree: a proof of 40 words does not hold its header and a table of 64 rows"):
        _tied(Rig(), seal_tied_tree, tree, TREES, 2, tree_proof[:40])                          # the upload is shorter than the table it states
    with _refuses("seal_tied: 17 out words (a prefix of 5, alpha, beta, the total), the circuit has 16"):
        _tied(Rig(), seal_tied, page, PATHS, 3, path_proof, prefix=5)
    rig = Rig()
    rig.hal.table_fingerprint = lambda *a: np.array([10, 11, 12, 14], dtype=np.uint32)
    with _refuses("seal_tied_tree: the proof's table is not the segment's page table: the segment's open total is 0000000a 0000000b 0000000c 0000000d, "
                  "the fingerprint of the proof's 64 rows is 0000000a 0000000b 0000000c 0000000e"):
        _tied(rig, seal_tied_tree, tree, TREES, 2, tree_proof)
    assert not [c for c in rig.log if c[0] == "seal_with_accum"]                                # no seal is spent on such a table


# ------------------------------------------------------------------------------------------------ which refusal a verifier gives
A, B, C_ = (np.full(8, v, dtype=np.uint32) for v in (1, 2, 3))
ROOT = np.zeros(8, dtype=np.uint32)
GOOD, BAD = 0x600D, 0xBAD
ABOVE = (1 << 29) + 1


def _receipt(out_words, opens, leaves, lo=None, hi=None, flag=GOOD):
    """a receipt whose seal is `out_words` out words and one word that says whether the stubbed verify_segment accepts it"""
    out = np.zeros(out_words, dtype=np.uint32)
    out[:8], out[8:16] = opens, leaves
    if lo is not None:
        out[16], out[17] = p2_blocks.enc(lo), p2_blocks.enc(hi)
    return SegmentReceipt(seal=np.concatenate([out, [flag]]).astype(np.uint32), index=0, po2=8)


@pytest.fixture()
def flagged(monkeypatch):
    """HostCircuit.verify_segment accepts exactly the seals that end on GOOD"""
    def verify_segment(self, seal, control_root, rc=None, diag=None):
        if int(seal[-1]) != GOOD:
            raise HalError("verify_segment: the seal is refused")
    monkeypatch.setattr(zhal.HostCircuit, "verify_segment", verify_segment)


def test_the_lazy_verifiers_bound_a_part_before_they_verify_the_next(flagged):
    """verify_page_out_chain, verify_page_ordered_chain and verify_tied: part 0 states a hi above 2^29, part 1 is no seal"""
    bound = f"part 0: hi {ABOVE} is above 2^29, the bound the order check is sound for"
    with _refuses(f"verify_page_ordered_chain: {bound}"):
        verify_page_ordered_chain([_receipt(18, A, B, 0, ABOVE), _receipt(18, B, C_, 0, 5, BAD)], ROOT)
    with pytest.raises(HalError, match="^verify_segment: "):                       # P2-PAGE's parts state no hi: every seal, then the links
        verify_page_out_chain([_receipt(16, A, B), _receipt(16, A, C_, flag=BAD)], ROOT)
    with _refuses(f"verify_page_out_chain: part 1 opens root {'00000001 ' * 7}00000001, but part 0 left root {'00000002 ' * 7}00000002"):
        verify_page_out_chain([_receipt(16, A, B), _receipt(16, A, C_)], ROOT)
    desc, _ = sl.syn_lookup_tiny_tied()
    seg = lambda flag: _receipt(16, A, A, flag=flag)
    with _refuses(f"verify_tied: {bound}"):
        verify_tied(seg(GOOD), desc, ROOT, [_receipt(30, A, B, 0, ABOVE), _receipt(30, B, C_, 0, 5, BAD)], ROOT)
    with pytest.raises(HalError, match="^verify_segment: "):                       # the segment's seal before any part
        verify_tied(seg(BAD), desc, ROOT, [_receipt(30, A, B, 0, ABOVE)], ROOT)


def test_the_tree_verifiers_verify_every_seal_before_they_look_at_h_or_link(flagged):
    """verify_page_tree_chain and verify_tied_tree: an empty list first, then every seal, then the range of h, then the links"""
    parts = lambda words: [_receipt(words, A, B, 4, ABOVE), _receipt(words, B, C_, 5, 8, BAD)]
    with pytest.raises(HalError, match="^verify_segment: "):
        verify_page_tree_chain(parts(18), ROOT, 3)
    with _refuses("verify_page_tree_chain: no receipt (a page-out of no rows still has one part)"):
        verify_page_tree_chain([], ROOT, 28)
    with _refuses("verify_page_tree_chain: h 28 (2 .. 27)"):
        verify_page_tree_chain([_receipt(18, A, B, 4, 8)], ROOT, 28)
    with _refuses(f"verify_page_tree_chain: part 0: hi {ABOVE} is above 2^29, the bound the order check is sound for"):
        verify_page_tree_chain(parts(18)[:1], ROOT, 3)
    desc, _ = sl.syn_lookup_tiny_tied()
    seg = lambda flag: _receipt(16, A, A, flag=flag)
    with pytest.raises(HalError, match="^verify_segment: "):                       # the segment's seal before the empty list is refused
        verify_tied_tree(seg(BAD), desc, ROOT, [], ROOT, 28)
    with _refuses("verify_tied_tree: no receipt (a page-out of no rows still has one part)"):
        verify_tied_tree(seg(GOOD), desc, ROOT, [], ROOT, 28)
    with pytest.raises(HalError, match="^verify_segment: "):
        verify_tied_tree(seg(GOOD), desc, ROOT, parts(31), ROOT, 3)
    with _refuses("verify_page_tree_chain: h 28 (2 .. 27)"):                       # the links of a tied tree group speak as P2-TREE's chain
        verify_tied_tree(seg(GOOD), desc, ROOT, [_receipt(31, A, B, 4, 8)], ROOT, 28)
    with _refuses("verify_page_tree_chain: part 0 starts at lo 5, not 2^2 = 4, the id of the first pair of leaves of a tree of height 3"):
        verify_tied_tree(seg(GOOD), desc, ROOT, [_receipt(31, A, B, 5, 8)], ROOT, 3)


# ------------------------------------------------------------------------------------------------ the table of kinds
def test_every_kind_of_the_table_is_its_circuit_modules():
    from zeth_amd.page_seal import PAGE_KINDS, TIE_WORDS
    modules = {5: p2_page, 6: p2_page_ordered, 7: p2_tree, 8: p2_page_tied, 9: p2_tree_tied}
    assert sorted(PAGE_KINDS) == sorted(modules)
    for kind, k in PAGE_KINDS.items():
        m, desc = modules[kind], k.desc()
        assert k.kind == kind and int(desc[13]) == kind and int(desc[7]) == k.out_words == m.OUT_WORDS
        assert k.prefix_words == getattr(m, "PREFIX_WORDS", m.OUT_WORDS)
        if k.accum == "open":                                                     # a tied kind: the prefix, kind 9's base, then alpha ‖ beta ‖ F
            assert k.prefix_words + (kind == 9) + TIE_WORDS == k.out_words
        else:
            assert k.prefix_words == k.out_words
        assert callable(getattr(zhal.HipHal, k.code)) and callable(getattr(zhal.HipHal, k.witgen))
