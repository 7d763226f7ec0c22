"""Held commitments WITHOUT a device (include/zkhal.h zkh_commit_data / zkh_prove_begin_held; page_seal.seal_tied_group's hold_bytes).

The header declares the five names, hal.py's table binds them and the built library exports them.  Then `seal_tied` and `seal_tied_tree`
run with `hold_bytes` set over a recording stub of this file's own, shaped like the one of tests/test_page_seal_calls.py and logging
in its format, so that the log of hold_bytes = 0 can be held against tests/golden/page_seal_calls.json entry for entry: a prover that
opens no context and whose data_root, commit_data, a commitment's release and seal_with_accum append to one log, over a hal whose page,
alloc, accumulate_open and table_fingerprint calls do.  A commitment of the stub reports the bytes page_seal.commitment_bytes states
for its shape, and its root is the root data_root would have given, so the challenge, and with it every `out` word, is the golden
log's whatever is held.

The proofs are the two of that test: page_ordered_cases' h = 5 table of 2N + 3 rows at (12, 1994), three parts of P2-PAGE-tied, and
page_tree_cases' image of 64 words with every word paged at (8, 40), two parts of P2-TREE-tied."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import page_circuit_cases as cases
import page_ordered_cases as oc
import page_tree_cases as tc
from zeth_amd import hal as zhal, page_seal
from zeth_amd.circuits import logup, p2_page_tied, p2_tree_tied, syn_lookup as sl
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver, SegmentReceipt, seal_tied, seal_tied_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "page_seal_calls.json")
NAMES = ("zkh_commit_data", "zkh_commitment_root", "zkh_commitment_bytes", "zkh_commitment_release", "zkh_prove_begin_held")
PATHS = cases.SHAPES[1]                                                           # (12, 1994, 8 * 17 + 3): three parts
TREES = (8, 40, 64)                                                               # two parts
NOISE = 0x5EA1
EVERYTHING = 1 << 40


# ------------------------------------------------------------------------------------------------ header, table, exports
def test_the_five_names_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "zkhal.h")).read(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+zkh_commitment\s+zkh_commitment\s*;", header)
    lib = zhal.load_library()
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "zeth_amd", "libzkhal_mi355x.so")], capture_output=True, text=True).stdout
    have = set(re.findall(r" T (zkh_\w+)", exported))
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared"
        assert name in zhal.ABI and hasattr(lib, name), f"{name} is not bound"
        assert name in have, f"{name} is not exported"
    assert zhal.ABI["zkh_commitment_bytes"][0] is C.c_size_t and zhal.ABI["zkh_commitment_release"][0] is None
    assert zhal.ABI["zkh_prove_begin_held"] == zhal.ABI["zkh_prove_begin"]        # the same operands, a commitment where the trace was
    lib.zkh_commitment_release(None)                                              # NULL is a no-op, on any machine
    assert lib.zkh_commitment_bytes(None) == 0


def test_the_bytes_of_a_commitment_by_the_formula():
    assert page_seal.commitment_bytes(138, 8) == 4 * 256 * (5 * 138 + 64)          # coefficients W n, evaluations 4 W n, nodes 64 n words
    assert page_seal.commitment_bytes(16, 20) == 4 * (1 << 20) * 144


# ------------------------------------------------------------------------------------------------ the recording stub
class Buf(zhal.Buffer):
    """a device buffer that is only a name and a size; one made by copy_from also holds its words; a release is logged by its serial"""

    def __init__(self, name, n, words=None, log=None, serial=None):
        self.hal, self.h, self.name, self.n, self.words, self.log, self.serial = None, None, name, int(n), words, log, serial

    def size(self):
        return self.n

    def slice(self, offset, size):
        assert offset + size <= self.n
        return Buf(self.name, size, self.words[offset:offset + size])

    def to_vec(self):
        return np.array(self.words, dtype=np.uint32)

    def release(self):
        if self.log is not None:
            self.log.append(["release", f"{self.name} #{self.serial}"])
            self.log = None

    def __del__(self):
        pass


def _enc(x):
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
    def __init__(self, name, desc):
        self.name, self.desc = name, np.asarray(desc, dtype=np.uint32)

    def has_arguments(self):
        return True

    def open_bus(self):
        return (logup.TIE_TAG, 4, 8, 12)


class StubHal:
    def __init__(self, log):
        self.log, self.opens, self.total, self.forge, self.refuse_open, self.allocs = log, 0, None, False, None, 0

    def _call(self, name, *operands):
        self.log.append([name] + [_enc(x) for x in operands])

    def alloc_elem(self, name, size):
        self._call("alloc_elem", name, size)
        self.allocs += 1
        return Buf(name, size, log=self.log if name == "data" else None, serial=self.allocs)

    def copy_from(self, name, host):
        words = np.ascontiguousarray(host, dtype=np.uint32).reshape(-1)
        self._call("copy_from", name, words.size)
        return Buf(name, words.size, words)

    def _code(self, name, circuit, po2, *shape):
        self._call(name, circuit, po2, *shape)
        return Buf("code", int(circuit.desc[4]) << po2)

    def page_ordered_code(self, circuit, po2, zk_cycles, image_words):
        return self._code("page_ordered_code", circuit, po2, zk_cycles, image_words)

    def page_tree_code(self, circuit, po2, zk_cycles):
        return self._code("page_tree_code", circuit, po2, zk_cycles)

    def _witgen(self, name, *operands):
        self._call(name, *operands)
        return np.arange(1000, 1018, dtype=np.uint32)

    def page_ordered_witgen(self, circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, first, data, noise_seed):
        return self._witgen("page_ordered_witgen", circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, first, data, noise_seed)

    def page_tree_witgen(self, circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, first, count, data, noise_seed):
        return self._witgen("page_tree_witgen", circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, first, count, data, noise_seed)

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
        if self.opens == self.refuse_open:
            raise HalError("accumulate_open: a denominator vanishes")
        self.total = np.arange(4, dtype=np.uint32) + np.uint32(10 * self.opens)
        return self.total

    def table_fingerprint(self, table, table_at, rows, challenge):
        self._call("table_fingerprint", table, table_at, rows, np.asarray(challenge))
        return self.total + np.uint32(self.forge)


class StubCommitment:
    def __init__(self, log, name, serial, root, nbytes):
        self.log, self.name, self.serial, self.root, self.bytes, self.h = log, name, serial, root, nbytes, serial

    def release(self):
        if self.h is not None:
            self.log.append(["release", f"commitment {self.name} #{self.serial}"])
            self.h = None


class StubProver(SegmentProver):
    def __init__(self, name, hal, desc):
        self.name, self.hal, self.log, self.roots, self.fail_check = name, hal, hal.log, 0, None
        self.circuit = StubCircuit(name, desc)
        self._group_sizes = tuple(int(x) for x in self.circuit.desc[3:6])

    def __del__(self):
        pass

    def code_root(self, code, po2):
        self.log.append(["code_root", self.name, _enc(code), po2])
        return np.arange(8, dtype=np.uint32) + np.uint32(500)

    def _root(self):
        self.roots += 1
        return np.full(8, len(self.name) + 100 * self.roots, dtype=np.uint32)

    def data_root(self, data, po2):
        self.log.append(["data_root", self.name, _enc(data), po2])
        return self._root()

    def commit_data(self, data, po2):
        self.log.append(["commit_data", self.name, _enc(data), po2])
        root = self._root()
        return StubCommitment(self.log, self.name, self.roots, root, page_seal.commitment_bytes(self._group_sizes[2], po2))

    def seal_with_accum(self, seg, code, data, out_global, accumulate, check=False, held=None):
        out = np.ascontiguousarray(out_global, dtype=np.uint32)
        accum = accumulate(np.zeros(int(self.circuit.desc[8]), dtype=np.uint32))
        if held is not None:
            assert held.h is not None, "a seal begins from a released commitment"
            self.log.append(["begin_held", self.name, seg.index, f"commitment {held.name} #{held.serial}"])
        self.log.append(["seal_with_accum", self.name, seg.index, seg.po2, seg.zk_cycles, seg.noise_seed, _enc(code), _enc(data), _enc(out), _enc(accum), check])
        if check and self.fail_check == seg.index:
            raise HalError("witness: row 3 fails constraint step 7")
        return SegmentReceipt(seal=out.copy(), index=seg.index, po2=seg.po2, output=out.copy())


def _proof(t):
    return cases.host_proof(t["image"], t["addrs"], t["outs"], logup.reference_image_tree(t["image"]).reshape(-1))


@pytest.fixture(scope="module")
def proofs():
    return {"seal_tied": _proof(oc.table(*PATHS, "2N+3")), "seal_tied_tree": _proof(tc.table(*TREES, "all"))}


ENTRIES = {"seal_tied": (seal_tied, p2_page_tied.p2_page_tied_circuit, PATHS, 3, True, "page_ordered_witgen"),
           "seal_tied_tree": (seal_tied_tree, p2_tree_tied.p2_tree_tied_circuit, TREES, 2, False, "page_tree_witgen")}


class Rig:
    def __init__(self, entry):
        self.entry, self.log = entry, []
        self.hal = StubHal(self.log)
        self.seal, desc, self.shape, self.parts, self.check, self.witgen = ENTRIES[entry]
        self.page = StubProver("page", self.hal, desc())
        self.segment = StubProver("segment", self.hal, sl.syn_lookup_tiny_tied()[0])

    def bytes_of(self, held_parts):
        """the budget that holds the segment and the first `held_parts` parts, from what the stub's commitments report"""
        part = page_seal.commitment_bytes(self.page.group_sizes()[2], self.shape[0]) + 4 * (self.page.group_sizes()[2] << self.shape[0])
        return page_seal.commitment_bytes(self.segment.group_sizes()[2], 8) + held_parts * part

    def run(self, proof, **kw):
        wa, wc, wd = self.segment.group_sizes()
        seg = Segment(index=0, po2=8, zk_cycles=40, noise_seed=NOISE)
        segs = [Segment(index=1 + p, po2=self.shape[0], zk_cycles=self.shape[1], noise_seed=NOISE + 1 + p) for p in range(self.parts)]
        kw.setdefault("check", self.check)
        return self.seal(self.segment, seg, Buf("segment code", wc << 8), Buf("segment data", wd << 8), np.zeros(4, dtype=np.uint32), self.page, segs, proof, proof.size,
                         Buf("nodes_before", 1), Buf("nodes_after", 1), **kw)


def _golden(entry):
    with open(GOLDEN) as fh:
        return json.load(fh)[entry]


def _of(log, *names):
    return [c for c in log if c[0] in names]


def _every_commitment_is_released_once(log):
    made = [f"commitment {c[1]} #{n}" for n, c in zip(_serials(log), _of(log, "commit_data"))]
    released = [c[1] for c in _of(log, "release") if c[1].startswith("commitment")]
    assert sorted(made) == sorted(released), (made, released)


def _serials(log):
    """the serial of each commit_data in the log: the number of the root its prover had handed out by then"""
    seen, out = {}, []
    for c in _of(log, "data_root", "commit_data"):
        seen[c[1]] = seen.get(c[1], 0) + 1
        if c[0] == "commit_data":
            out.append(seen[c[1]])
    return out


# ------------------------------------------------------------------------------------------------ the call order
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_hold_bytes_zero_makes_the_recorded_calls_entry_for_entry(entry, proofs):
    rig = Rig(entry)
    _, receipts = rig.run(proofs[entry], hold_bytes=0)
    assert rig.log == _golden(entry) and len(receipts) == rig.parts
    rig = Rig(entry)
    rig.run(proofs[entry])                                                        # and so does the call that does not name it
    assert rig.log == _golden(entry)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_a_budget_for_everything_commits_once_and_begins_every_seal_held(entry, proofs):
    rig, want = Rig(entry), _golden(entry)
    _, receipts = rig.run(proofs[entry], hold_bytes=EVERYTHING)
    log = rig.log
    assert not _of(log, "data_root") and len(receipts) == rig.parts
    # commit_data where data_root was, with its operands but for the parts' buffers, which are no longer one
    assert [c[1:] for c in _of(log, "commit_data")] == [c[1:] for c in _of(want, "data_root")]
    assert len(_of(log, rig.witgen)) == rig.parts and len(_of(want, rig.witgen)) == 2 * rig.parts          # one witness call per part
    assert _of(log, rig.witgen) == _of(want, rig.witgen)[:rig.parts]
    assert len(_of(log, "begin_held")) == len(_of(log, "seal_with_accum")) == 1 + rig.parts
    for i, c in enumerate(log):
        if c[0] == "seal_with_accum":
            assert log[i - 1][:3] == ["begin_held", c[1], c[2]]
    # the seals are the recorded ones, operand for operand: the same roots give the same challenge, the kept prefix the same `out`
    assert _of(log, "seal_with_accum", "accumulate_open", "table_fingerprint", "code_root") == _of(want, "seal_with_accum", "accumulate_open", "table_fingerprint", "code_root")
    # a held part keeps its trace: one buffer per part, each released after its seal, and none allocated after the last part
    data_allocs = [i for i, c in enumerate(log) if c[:2] == ["alloc_elem", "data"]]
    assert len(data_allocs) == rig.parts
    assert len([c for c in _of(log, "release") if c[1].startswith("data")]) == rig.parts
    _every_commitment_is_released_once(log)
    seals = [i for i, c in enumerate(log) if c[0] == "seal_with_accum"]
    for p, i in enumerate(seals):                                                 # each commitment goes right after its own seal
        assert log[i + 1][0] == "release" and log[i + 1][1].startswith("commitment"), (p, log[i + 1])


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_a_budget_for_the_segment_and_part_0_leaves_part_1_the_two_passes(entry, proofs):
    rig, want = Rig(entry), _golden(entry)
    rig.run(proofs[entry], hold_bytes=rig.bytes_of(1))
    log = rig.log
    pass_one = [c[:2] for c in _of(log, "commit_data", "data_root")]
    assert pass_one == [["commit_data", "segment"], ["commit_data", "page"]] + [["data_root", "page"]] * (rig.parts - 1)
    assert [c[2] for c in _of(log, "begin_held")] == [0, 1]
    # part 1 on: data_root, the witness again, the plain begin; part 0: one witness call
    starts = [c[-3 if entry == "seal_tied" else -4] for c in _of(log, rig.witgen)]
    firsts = [c[-3 if entry == "seal_tied" else -4] for c in _of(want, rig.witgen)][:rig.parts]
    assert starts == firsts + firsts[1:]
    sealed = [i for i, c in enumerate(log) if c[0] == "seal_with_accum"]
    assert log[sealed[2] - 1][0] == "accumulate_open" and log[sealed[2] - 3][0] == rig.witgen
    assert _of(log, "seal_with_accum", "accumulate_open", "table_fingerprint", "code_root") == _of(want, "seal_with_accum", "accumulate_open", "table_fingerprint", "code_root")
    assert len([c for c in log if c[:2] == ["alloc_elem", "data"]]) == 2           # part 0's own, and one that parts 1 .. share
    _every_commitment_is_released_once(log)
    # one byte less and part 0 is not held either; a budget below the segment's holds nothing, and then the log is the recorded one
    rig = Rig(entry)
    rig.run(proofs[entry], hold_bytes=rig.bytes_of(1) - 1)
    assert [c[:2] for c in _of(rig.log, "commit_data", "data_root")] == [["commit_data", "segment"]] + [["data_root", "page"]] * rig.parts
    rig = Rig(entry)
    rig.run(proofs[entry], hold_bytes=rig.bytes_of(0) - 1)
    assert rig.log == want


def test_the_held_seals_are_a_prefix_a_later_part_that_would_fit_is_not_held(proofs):
    """the segment does not fit, the parts would: nothing is held"""
    rig = Rig("seal_tied_tree")
    rig.segment._group_sizes = (rig.segment._group_sizes[0], rig.segment._group_sizes[1], 100000)
    rig.run(proofs["seal_tied_tree"], hold_bytes=10 * (rig.bytes_of(1) - rig.bytes_of(0)))
    assert not _of(rig.log, "commit_data", "begin_held")


# ------------------------------------------------------------------------------------------------ release on refusal
def _refused(entry, proofs, arm, text, **kw):
    rig = Rig(entry)
    arm(rig)
    with pytest.raises(HalError, match=text):
        rig.run(proofs[entry], hold_bytes=EVERYTHING, **kw)
    assert len(_of(rig.log, "commit_data")) == 1 + rig.parts
    _every_commitment_is_released_once(rig.log)
    assert len([c for c in _of(rig.log, "release") if c[1].startswith("data #")]) == rig.parts, "a held trace was not released"
    return rig.log


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_a_forged_fingerprint_releases_every_commitment_and_trace(entry, proofs):
    log = _refused(entry, proofs, lambda rig: setattr(rig.hal, "forge", True), r": the proof's table is not the segment's page table: ")
    assert not _of(log, "seal_with_accum", "begin_held")                          # no seal is spent on such a table


def test_a_failed_check_witness_and_a_refused_accumulate_release_them_too(proofs):
    log = _refused("seal_tied_tree", proofs, lambda rig: setattr(rig.page, "fail_check", 1), "^witness: row 3 fails", check=True)
    assert len(_of(log, "seal_with_accum")) == 2                                  # the segment's, and part 0's, which the check refused
    log = _refused("seal_tied", proofs, lambda rig: setattr(rig.hal, "refuse_open", 3), "^accumulate_open: a denominator vanishes$")
    assert len(_of(log, "seal_with_accum")) == 2                                  # the segment's and part 0's: part 1's accumulate refused
