"""Segment prover — the host-side mirror of what `default_prover().prove(env, elf)` runs per segment.

Reference call site: /root/reference/crates/host/src/lib.rs:137 (`BlockProcessor::prove`), which (through the
un-vendored risc0-zkvm 3.0.3 `ProverServer::prove_session` -> `prove_segment`, /root/reference/Cargo.lock:5418)
seals every 2^po2-cycle segment independently and returns `SegmentReceipt{seal, index, hashfn, claim}`.
Here `SegmentProver.prove_segment` does the same for one segment on one MI355X via `zkh_prove_segment`
(zeth_amd/csrc/prover.hip).  Because the rv32im circuit and the guest execution trace cannot be obtained
offline, a segment is described by a `Segment` (po2 + witness seeds for the SYN-AIR stand-in circuit).

Two ways a witness reaches the seal:
  * `prove_segment(seg)`            — SYN witness generated on the device (zkh_syn_witgen), then sealed;
  * `seal_host_witness(seg, ...)`   — code/data traces produced on the HOST (upstream's flow: CPU preflight + witgen),
                                      uploaded from pinned memory (zkh_host_alloc + zkh_write_async), sealed through
                                      zkh_prove_begin -> accum -> zkh_prove_finish, the two halves upstream's
                                      SegmentProver drives `Prover` in.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Tuple

import numpy as np

from . import hal as _hal, page_seal as _page_seal
from .circuits import syn_air
# what seals or verifies a page-out lives in page_seal.py; its public names stay importable from here
from .page_seal import (TIE_WORDS, PagedStep, link_page_parts, link_page_tree_chain, link_paged_run, link_tied_tree_chain,  # noqa: F401
                        preflight_paged_run, seal_paged_step, seal_tied, seal_tied_tree, seal_tied_tree_from_proof, verify_page_ordered_chain,
                        verify_page_out_chain, verify_page_tree_chain, verify_paged_run, verify_tied, verify_tied_tree)

DEFAULT_SEGMENT_PO2 = 20      # upstream default segment_limit_po2 (lib.rs:132-135 passes None -> 20)
_CONTROL_ROOTS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "circuits", "control_roots.json")


def fresh_noise_seed() -> int:
    """Seed of the zero-knowledge blinding rows: OS randomness, like upstream (which fills the last ZK_CYCLES rows of
    every trace column from an OS RNG).  Tests, benchmarks and golden fixtures pass an explicit seed instead."""
    return int.from_bytes(os.urandom(32), "little") | 1          # 256 bits: the ChaCha12 key of the blinding stream (csrc/noise.h); never 0


@dataclass(frozen=True)
class Segment:
    """One continuation segment: index within the session, size, and the synthetic witness seeds."""
    index: int
    po2: int = DEFAULT_SEGMENT_PO2
    seed: int = 0x5EED0000
    noise_seed: int = field(default_factory=fresh_noise_seed)
    zk_cycles: int = _hal.ZK_CYCLES
    pub: Tuple[int, ...] = ()        # public input words (Montgomery) for circuits with OUTPUT_SIZE > 4 (SYN-J joins)


def desc_key(desc) -> str:
    from .circuits.codegen import desc_hash64
    return f"{desc_hash64(np.asarray(desc, dtype=np.uint32)):016x}"


_shipped_roots: Optional[Dict[str, Dict[str, list]]] = None


def shipped_control_root(desc, po2: int) -> Optional[np.ndarray]:
    """Control root registered for (circuit, po2) at the protocol's ZK_CYCLES — the control-ID table upstream compiles
    into the verifier.  Generated on a GPU box by `python -m zeth_amd.prover` (this module's main)."""
    global _shipped_roots
    if _shipped_roots is None:
        try:
            with open(_CONTROL_ROOTS_JSON) as fh:
                _shipped_roots = json.load(fh)["roots"]
        except (OSError, ValueError, KeyError):
            _shipped_roots = {}
    words = _shipped_roots.get(desc_key(desc), {}).get(str(po2))
    return None if words is None else np.asarray(words, dtype=np.uint32)


@dataclass
class SegmentReceipt:
    """`risc0_zkvm::SegmentReceipt` analogue: seal words + the metadata upstream carries."""
    seal: np.ndarray
    index: int
    po2: int
    hashfn: str = "poseidon2"
    output: Optional[np.ndarray] = None      # `out` globals (the claim-bearing public outputs)
    control_root: Optional[np.ndarray] = None  # what the prover committed the code group to (informational; the
    #                                            verifier is given the EXPECTED root, it never trusts this field)

    def seal_bytes(self) -> bytes:
        return np.asarray(self.seal, dtype="<u4").tobytes()

    def to_words(self, circuit_desc, control_root) -> np.ndarray:
        """Receipt container (zkh_receipt_encode): what gets stored / shipped instead of upstream's bincode SegmentReceipt."""
        return _hal.HostCircuit(circuit_desc).receipt_encode(self.seal, self.index, control_root)

    @staticmethod
    def from_words(circuit_desc, blob) -> "SegmentReceipt":
        """Parse + integrity-check a container.  The control root inside is informational: `verify` takes the expected one."""
        hdr, seal = _hal.HostCircuit(circuit_desc).receipt_decode(blob)
        return SegmentReceipt(seal=seal, index=hdr["index"], po2=hdr["po2"], output=seal[:hdr["out_size"]].copy(),
                              control_root=hdr["control_root"])

    def verify(self, circuit_desc, control_root=None) -> None:
        """`Receipt::verify` for this segment (/root/reference/crates/host/src/bin/cli.rs:103): host-side, no GPU needed.
        `control_root`: the expected code commitment; None looks it up in the shipped table (zk_cycles = ZK_CYCLES).
        Raises `zeth_amd.hal.HalError` (the VerificationError analogue) if the seal is rejected."""
        desc = np.asarray(circuit_desc, dtype=np.uint32)
        if control_root is None:
            control_root = shipped_control_root(desc, self.po2)
            if control_root is None:
                raise _hal.HalError(f"verify_segment: no control root registered for circuit {desc_key(desc)} at po2 {self.po2}")
        hc = _hal.HostCircuit(desc)
        hc.verify_segment(self.seal, control_root)
        out_size = int(desc[7])
        if _hal.fp_decode(int(self.seal[out_size])) != self.po2:
            raise _hal.HalError("verify_segment: receipt metadata does not match the seal (po2)")
        if self.output is not None and not np.array_equal(np.asarray(self.output, dtype=np.uint32), self.seal[:out_size]):
            raise _hal.HalError("verify_segment: receipt output does not match the seal's output globals")


class Commitment:
    """A data group committed once and kept for its seal (zkh_commit_data): `root` is what data_root gives for the trace, `bytes` the
    device bytes of the three buffers held (coefficients, 4n evaluations, Merkle nodes; none aliases the trace).  `release()` gives
    them back; it is idempotent and runs on __del__.  The commitment may outlive the prover that made it, not the context."""

    def __init__(self, hal: "_hal.HipHal", handle, po2: int):
        self.hal, self.h, self.po2 = hal, handle, po2
        root = np.zeros(8, dtype=np.uint32)
        _hal._check(_hal._lib.zkh_commitment_root(handle, root.ctypes.data_as(C.POINTER(C.c_uint32))))
        self.root, self.bytes = root, int(_hal._lib.zkh_commitment_bytes(handle))

    def release(self) -> None:
        h, self.h = getattr(self, "h", None), None
        if h and _hal._lib is not None and getattr(self.hal, "ctx", None):     # like Buffer: only released into a live context
            _hal._lib.zkh_commitment_release(h)

    __del__ = release


class SegmentProver:
    """`SegmentProverImpl<H, C>` analogue bound to one HipHal (one GPU)."""

    def __init__(self, hal: "_hal.HipHal", circuit_desc=None, resident_code_group: bool = False, arguments=None):
        """resident_code_group: keep the committed code (control) group of each segment size in HBM instead of re-committing
        it for every segment (zkh_prover_cache_code): the group is a function of (circuit, po2, zk_cycles) alone.  Off by
        default — upstream's SegmentProver recomputes it, and so does the benchmark's headline number.
        arguments: the circuit's ZKA1 argument blob (circuits/logup.py), if its accum group is built by zkh_accumulate."""
        self.hal = hal
        self.circuit = hal.load_circuit(syn_air.syn_a() if circuit_desc is None else circuit_desc)
        if arguments is not None:
            self.circuit.set_arguments(arguments)
        h = C.c_void_p()
        _hal._check(_hal._lib.zkh_prover_create(hal.ctx, self.circuit.h, C.byref(h)))
        self.h = h
        self.resident_code_group = resident_code_group
        self._resident: Dict[int, int] = {}                 # po2 -> zk_cycles of the resident code group
        self._roots: Dict[Tuple[int, int], np.ndarray] = {}
        self._group_sizes = tuple(int(x) for x in self.circuit.desc[3:6])       # (accum, code, data): desc header words

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        # a prover may hold device buffers (the resident code group): like Buffer, it is only released into a live context
        if h and _hal._lib is not None and getattr(self.hal, "ctx", None):
            _hal._lib.zkh_prover_destroy(h)

    def group_sizes(self):
        return self._group_sizes

    def out_size(self) -> int:
        return int(self.circuit.desc[7])

    def control_root(self, po2: int, zk_cycles: int = _hal.ZK_CYCLES) -> np.ndarray:
        """Merkle root of the committed SYN code group for (po2, zk_cycles): computed on the GPU once and cached."""
        key = (po2, zk_cycles)
        if key not in self._roots:
            root = np.zeros(8, dtype=np.uint32)
            _hal._check(_hal._lib.zkh_syn_control_root(self.h, po2, zk_cycles, root.ctypes.data_as(C.POINTER(C.c_uint32))))
            self._roots[key] = root
        return self._roots[key]

    def code_root(self, code, po2: int) -> np.ndarray:
        root = np.zeros(8, dtype=np.uint32)
        _hal._check(_hal._lib.zkh_code_root(self.h, code.h, po2, root.ctypes.data_as(C.POINTER(C.c_uint32))))
        return root

    def data_root(self, data, po2: int) -> np.ndarray:
        """the root a seal of the data trace `data` will carry for its data group (zkh_data_root), before the seal is made"""
        root = np.zeros(8, dtype=np.uint32)
        _hal._check(_hal._lib.zkh_data_root(self.h, po2, data.h, root.ctypes.data_as(C.POINTER(C.c_uint32))))
        return root

    def commit_data(self, data, po2: int) -> Commitment:
        """commit the data trace `data` once and keep the commitment (zkh_commit_data): `.root` is data_root's, and
        seal_with_accum(held=...) begins the seal from it without committing again.  `data` is not aliased."""
        h = C.c_void_p()
        _hal._check(_hal._lib.zkh_commit_data(self.h, po2, data.h, C.byref(h)))
        return Commitment(self.hal, h, po2)

    def witgen(self, seg: Segment):
        """Witness generation (code + data traces resident in HBM) — reported separately from the seal."""
        wa, wc, wd = self.group_sizes()
        n = 1 << seg.po2
        # with this size's committed code group resident the trace is not needed again (kinds 1 / 2: the data generator does
        # not read it) -> code is None, and `seal` passes NULL
        held = self.resident_code_group and self._resident.get(seg.po2) == seg.zk_cycles and int(self.circuit.desc[13]) in (1, 2)
        code = None if held else self.hal.alloc_elem("code", wc * n)
        data = self.hal.alloc_elem("data", wd * n)
        out = self.hal.syn_witgen(self.circuit, seg.po2, seg.zk_cycles, seg.seed, seg.noise_seed, code, data,
                                  pub=np.asarray(seg.pub, dtype=np.uint32) if seg.pub else None)
        return code, data, out

    def chain_contribution(self, seg: Segment) -> int:
        """What a SYN-C segment adds to the running state: its post-state when started from state 0 (the witness generator run
        with pre = 0; the executor's pass of a chained session, outside any proving clock)."""
        seeds = (C.c_uint64 * 1)(seg.seed & (2**64 - 1))
        po2s, out = np.array([seg.po2], dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        _hal._check(_hal._lib.zkh_syn_chain_contributions(self.hal.ctx, self.circuit.h, seeds, po2s.ctypes.data_as(C.POINTER(C.c_uint32)), 1, seg.zk_cycles,
                                                          out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return int(out[0])

    def _take_seal(self, seal_p, n) -> np.ndarray:
        seal = np.ctypeslib.as_array(seal_p, shape=(n.value,)).copy()
        _hal._lib.zkh_free_seal(seal_p)
        return seal

    def _code_handle(self, seg: Segment, code):
        """The code operand of a seal: the trace, or NULL once this size's committed group is resident."""
        if not self.resident_code_group:
            return code.h
        if self._resident.get(seg.po2) != seg.zk_cycles:
            if code is None:
                raise _hal.HalError("seal: no code trace and no resident code group of this size")
            _hal._check(_hal._lib.zkh_prover_cache_code(self.h, seg.po2, code.h))
            self._resident[seg.po2] = seg.zk_cycles
        return None

    def seal(self, seg: Segment, code, data, out_global) -> SegmentReceipt:
        """Steps 3-7 of SURVEY.md §3.2 on traces already resident in HBM: the timed unit of work."""
        out = np.ascontiguousarray(out_global, dtype=np.uint32)
        seal_p = C.POINTER(C.c_uint32)()
        n = C.c_size_t()
        _k, kp = _hal._key_ptr(seg.noise_seed)
        _hal._check(_hal._lib.zkh_prove_segment(self.h, seg.po2, seg.zk_cycles, kp, self._code_handle(seg, code), data.h,
                                                out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(seal_p), C.byref(n)))
        return SegmentReceipt(seal=self._take_seal(seal_p, n), index=seg.index, po2=seg.po2, output=out.copy())

    def check_witness(self, seg: Segment, code, data, out_global, accum, mix_global) -> None:
        """Check the raw traces against the circuit's own constraints on every row (zkh_check_rows): raises HalError naming the lowest
        failing row, its lowest failing constraint step, the value that step wants zero, what it reads (circuits/check.py
        explain_step) and how many rows fail.  Costs one pass over the trace; a seal of a bad witness costs the whole seal and names
        neither row nor constraint."""
        from .circuits import check as _check_rows
        if code is None:
            raise _hal.HalError("check_witness: the constraints read the raw code trace; it is not held (resident code group)")
        r = self.hal.check_rows(self.circuit, seg.po2, accum, code, data, out_global, mix_global)
        if r["row"] < 0:
            return
        v = r["value"]
        value = str(v[0]) if not any(v[1:]) else "(" + ", ".join(str(x) for x in v) + ")"
        raise _hal.HalError(f"witness: row {r['row']} fails constraint step {r['step']} (value {value}; reads "
                            f"{_check_rows.describe_reads(self.circuit.desc, r['step'])}; {r['failing_rows']} rows fail)")

    def check_bus(self, seg: Segment, code, data) -> None:
        """Check the bus of a circuit with arguments key by key on the raw traces (zkh_check_bus; no mix, no accum, no seal): raises
        HalError with the one line of circuits/logup.py describe_bus — the key that does not balance, its net, and what every term of
        its tag holds of it — and returns quietly when every key balances."""
        from .circuits import logup as _logup
        if code is None:
            raise _hal.HalError("check_bus: the arguments read the raw code trace; it is not held (resident code group)")
        found = self.hal.check_bus(self.circuit, seg.po2, seg.zk_cycles, code, data, per_term=True)
        line = _logup.describe_bus(found, _logup.Arguments.parse(self.circuit._args))
        if line:
            raise _hal.HalError(line)

    def seal_with_accum(self, seg: Segment, code, data, out_global,
                        accumulate: Callable[[np.ndarray], "_hal.Buffer"], check: bool = False, held: Optional[Commitment] = None) -> SegmentReceipt:
        """The same seal through the circuit-agnostic halves: zkh_prove_begin (header, code, data -> mix challenges),
        `accumulate(mix_global) -> accum buffer` supplied by the caller (CircuitHal::accumulate), zkh_prove_finish.
        check: run check_witness between the accumulate and zkh_prove_finish; a witness that fails it raises, and no seal is made.
        held: the commitment of `data` (commit_data): the begin is zkh_prove_begin_held, which commits nothing, and the seal is the
        same byte for byte.  `data` is still passed: `accumulate` and check_witness read the raw trace.  The commitment is shared, not
        consumed: the caller releases it, before or after this call."""
        out = np.ascontiguousarray(out_global, dtype=np.uint32)
        wa = self.group_sizes()[0]
        job = C.c_void_p()
        mix = np.zeros(max(1, int(self.circuit.desc[8])), dtype=np.uint32)
        begin, operand = (_hal._lib.zkh_prove_begin, data.h) if held is None else (_hal._lib.zkh_prove_begin_held, held.h)
        _hal._check(begin(self.h, seg.po2, self._code_handle(seg, code), operand, out.ctypes.data_as(C.POINTER(C.c_uint32)),
                          C.byref(job), mix.ctypes.data_as(C.POINTER(C.c_uint32))))
        try:
            accum = accumulate(mix[: int(self.circuit.desc[8])])
            if accum.size() != wa << seg.po2:
                raise _hal.HalError("accumulate returned a buffer of the wrong shape")
            if check:
                self.check_witness(seg, code, data, out, accum, mix[: int(self.circuit.desc[8])])
        except BaseException:
            _hal._lib.zkh_prove_abort(job)
            raise
        seal_p = C.POINTER(C.c_uint32)()
        n = C.c_size_t()
        _hal._check(_hal._lib.zkh_prove_finish(job, accum.h, C.byref(seal_p), C.byref(n)))
        return SegmentReceipt(seal=self._take_seal(seal_p, n), index=seg.index, po2=seg.po2, output=out.copy())

    def syn_accumulate(self, seg: Segment, data):
        """`accumulate` callback for the SYN-AIR family (zkh_syn_accum)."""
        wa = self.group_sizes()[0]

        def acc(mix_global):
            accum = self.hal.alloc_elem("accum", wa << seg.po2)
            self.hal.syn_accum(self.circuit, seg.po2, seg.zk_cycles, seg.noise_seed, data, mix_global, accum)
            return accum
        return acc

    def args_accumulate(self, seg: Segment, code, data, check: bool = False):
        """`accumulate` callback for a circuit with arguments (zkh_accumulate over the raw code and data traces): refuses a witness
        whose denominators vanish or whose bus does not balance (HalError).  check: after a "does not balance" refusal run check_bus
        and raise the accumulate's message followed by the bus line; a witness that is accepted costs nothing more."""
        wa = self.group_sizes()[0]
        if code is None:
            raise _hal.HalError("args_accumulate: the arguments read the raw code trace; it is not held (resident code group)")

        def acc(mix_global):
            accum = self.hal.alloc_elem("accum", wa << seg.po2)
            try:
                self.hal.accumulate(self.circuit, seg.po2, seg.zk_cycles, seg.noise_seed, code, data, mix_global, accum)
            except _hal.HalError as refusal:
                if not check or "does not balance" not in str(refusal):
                    raise
                try:
                    self.check_bus(seg, code, data)
                except _hal.HalError as bus:
                    raise _hal.HalError(f"{refusal}; {bus}") from None
                raise
            return accum
        return acc

    def seal_host_witness(self, seg: Segment, host_code: np.ndarray, host_data: np.ndarray, out_global, check: bool = False,
                          image=None, page_out: bool = False, tree=None) -> SegmentReceipt:
        """Seal a segment whose code/data traces live in pinned HOST memory (hal.host_alloc views): enqueue both uploads
        on the context's stream (no host sync), then run the two-halves seal.  This is the PCIe-inclusive path.  A circuit whose
        arguments derive sorted copies, columns, linked accesses or lookup multiplicities gets them filled into the data trace first
        (zkh_derive_all); of those columns only the blinding rows are uploaded (zkh_upload_data_trace).  The traces may hold raw words
        >= P (a cell is read as its residue): after the derives both are reduced in place (zkh_reduce_elem), so the seal is a function
        of the residues.  The accum
        comes from the built-in generator of kinds 1..3, else from zkh_accumulate when the circuit carries arguments.
        check: check the finished witness row by row before the seal is spent on it (check_witness, seal_with_accum), and when
        zkh_accumulate refuses a bus that does not balance, name the key (check_bus, args_accumulate).
        image: the memory image (a device Buffer of raw Montgomery words) that a circuit whose arguments page memory starts from
        (zkh_derive_all_paged).  The derive only reads it.  page_out: after the seal has succeeded, write the segment's memory back
        into `image` (`page_out`), so that the next segment starts from it; a refused or failed seal leaves the image as it was.
        tree: the committed tree of `image` (hal.image_commit); the page-out then keeps it current (zkh_page_out_tree)."""
        code = self.hal.alloc_elem("code", host_code.size)
        data = self.hal.alloc_elem("data", host_data.size)
        self.hal.write_async(code, host_code)
        self.hal.upload_data_trace(self.circuit, seg.po2, seg.zk_cycles, data, host_data)
        self.hal.derive_all_paged(self.circuit, seg.po2, seg.zk_cycles, code, data, image)
        self.hal.reduce_elem(code)           # raw words >= P end here: the accumulate reads residues, the seal takes reduced words
        self.hal.reduce_elem(data)
        builtin =1 <= int(self.circuit.desc[13]) <= 3
        acc = self.args_accumulate(seg, code, data, check=check) if not builtin and self.circuit.has_arguments() else self.syn_accumulate(seg, data)
        receipt = self.seal_with_accum(seg, code, data, out_global, acc, check=check)
        if page_out:
            self.page_out(seg, data, image, tree=tree)
        return receipt

    def page_out(self, seg: Segment, data, image, tree=None, proof: bool = False, walk: bool = False, keep_before: bool = False, dirty: bool = False):
        """write the page table of the segment's derived data trace (a device Buffer) back into the memory image: image[p_addr] = p_out
        on the rows with p_on = 1 (zkh_page_out).  A call of its own, after the seal: a refused witness never touches the image.
        tree: the image's committed tree (hal.image_commit of the image as it is now), brought up to the new image in the same call
        (zkh_page_out_tree): its root is the commitment the next segment starts from.
        proof: with a tree, build the update's ZKU1 proof first (zkh_page_out_proof, from the tree as it is) and return its words:
        hal.image_proof_verify(proof, the old root) gives the new root without the image.  Otherwise None is returned.
        walk: with proof, the prover checks what it ships: the proof is walked on the device (zkh_image_proof_walk) from the tree's
        root as it is, and after the page-out the walked root must be the tree's; HalError, naming both roots, if it is not.
        keep_before: with proof, the tree is copied (zkh_eltwise_copy_elem) before the update and (words, the copy) is returned: the
        two trees and the proof are what a P2-PAGE prover's `seal_page_out` takes.
        dirty: with proof, (words, dirty) is returned, `dirty` the dirty-node table of the proof (hal.image_proof_nodes: the walk from
        the tree's root as it was, keeping what it recomputes), which with the proof is all that `seal_page_out_tree(dirty=...)` and
        `seal_tied_tree(dirty=...)` read on any rank.  No tree is copied.  As with walk, the root that comes back must be the updated
        tree's.  An empty page table is refused by image_proof_nodes (it is sealed from the tree)."""
        if dirty and not proof:
            raise _hal.HalError("page_out: dirty=True needs proof=True (the dirty nodes are read off the proof)")
        if dirty and keep_before:
            raise _hal.HalError("page_out: dirty=True with keep_before=True (the dirty nodes stand in place of the copied tree: ask for one)")
        if keep_before and not proof:
            raise _hal.HalError("page_out: keep_before=True needs proof=True (the copy goes with the proof)")
        if proof and tree is None:
            raise _hal.HalError("page_out: proof=True needs the image's committed tree (tree=hal.image_commit(image))")
        if walk and not proof:
            raise _hal.HalError("page_out: walk=True needs proof=True (the walk is of the proof)")
        if tree is None:
            self.hal.page_out(self.circuit, seg.po2, seg.zk_cycles, data, image)
            return None
        words = walked = table = None
        if proof and dirty:
            root_before = self.hal.image_root(tree)
            buf = self.hal.alloc("image_proof", self.hal.image_proof_words(image.size(), max(1, self.circuit.page_words()) * ((1 << seg.po2) - seg.zk_cycles)))
            words = self.hal.page_out_proof(self.circuit, seg.po2, seg.zk_cycles, data, image, tree, proof=buf)
        elif proof and walk:
            buf = self.hal.alloc("image_proof", self.hal.image_proof_words(image.size(), max(1, self.circuit.page_words()) * ((1 << seg.po2) - seg.zk_cycles)))
            words = self.hal.page_out_proof(self.circuit, seg.po2, seg.zk_cycles, data, image, tree, proof=buf)
            walked = self.hal.image_proof_walk(buf, self.hal.image_root(tree), words=words.size)
        elif proof:
            words = self.hal.page_out_proof(self.circuit, seg.po2, seg.zk_cycles, data, image, tree)
        before = None
        if keep_before:
            before = self.hal.alloc("image_nodes_before", tree.size())
            self.hal.eltwise_copy_elem(before, tree)
        self.hal.page_out_tree(self.circuit, seg.po2, seg.zk_cycles, data, image, tree)
        if dirty:
            walked, table = self.hal.image_proof_nodes(buf, root_before, words=words.size)
        if walked is not None:
            root = self.hal.image_root(tree)
            if not np.array_equal(walked, root):
                fmt = lambda r: " ".join(f"{int(w):08x}" for w in r)
                raise _hal.HalError(f"page_out: the proof walks to root {fmt(walked)}, but the tree's root after the page-out is {fmt(root)}")
        return (words, before) if keep_before else (words, table) if dirty else words

    def seal_page_out(self, seg: Segment, proof, proof_words: int, nodes_before, nodes_after, check: bool = False) -> SegmentReceipt:
        """Seal a page-out from root to root with P2-PAGE (this prover's circuit: circuits/p2_page.py): the code group for the image's
        tree height, the witness of the ZKU1 proof's table between the two trees (zkh_page_circuit_code / _witgen), P2-JOIN's accum
        and the two-halves seal.  proof: a device Buffer whose first `proof_words` words are the proof, or the proof's words (uploaded);
        nodes_before / nodes_after: the committed tree before and after the page-out (`page_out(..., proof=True, keep_before=True)`).
        The receipt's output is root_before ‖ root_after; `control_root` is the committed code group's root, which depends on the
        tree height as well as on po2.  check: check the witness row by row first (check_witness); a table that does not match
        the trees is named there."""
        return _page_seal.seal_chain("seal_page_out", self, 5, [seg], proof, proof_words, nodes_before, nodes_after, check, single=True)[0]

    def seal_page_out_parts(self, segs, proof, proof_words: int, nodes_before, nodes_after, check: bool = False) -> list:
        """Seal a page-out of ANY size with P2-PAGE as a chain of parts (circuits/p2_page.py `parts`): part p lays out the updates
        [first, first + count) of the ZKU1 proof's table (zkh_page_circuit_witgen_part), and its receipt's output is the root before
        update `first` ‖ the root after the part's last update, so part p + 1 opens the root part p left (`verify_page_out_chain`).
        segs: one Segment per part (page_seal.seal_chain); the other operands are seal_page_out's.  -> the receipts, in the order of the
        parts."""
        return _page_seal.seal_chain("seal_page_out_parts", self, 5, segs, proof, proof_words, nodes_before, nodes_after, check)

    def seal_page_out_ordered(self, segs, proof, proof_words: int, nodes_before, nodes_after, check: bool = False) -> list:
        """Seal a page-out of any size with P2-PAGE-ordered (this prover's circuit: circuits/p2_page_ordered.py) as a chain of parts:
        seal_page_out_parts with the order of the addresses constrained.  Part p's receipt's output is root_before ‖ root_after ‖ lo ‖
        hi of its run of updates (zkh_page_ordered_witgen), so part p + 1 opens the root and starts at the `hi` part p left
        (`verify_page_ordered_chain`).  The operands and the plan (p2_page.parts) are seal_page_out_parts'.  -> the receipts, in the
        order of the parts."""
        return _page_seal.seal_chain("seal_page_out_ordered", self, 6, segs, proof, proof_words, nodes_before, nodes_after, check)

    def seal_page_out_tree(self, segs, proof, proof_words: int, nodes_before, nodes_after, check: bool = False, plan: str = "host", dirty=None) -> list:
        """Seal a page-out of any size with P2-TREE (this prover's circuit: circuits/p2_tree.py, built with arguments=p2_tree.arguments())
        as a chain of parts: one block per DIRTY NODE of the tree instead of one path per word.  Part p's receipt's output is
        root_before ‖ root_after ‖ lo ‖ hi of its run of pairs of leaves (zkh_page_tree_witgen), so part p + 1 opens the root and
        starts at the `hi` part p left (`verify_page_tree_chain`).  The plan is zkh_page_tree_plan's over the table's addresses, read
        back once (D words).  The accum group is the circuit's bus (args_accumulate): a table that does not match the trees is refused
        there, and check=True names the key.  The other operands are seal_page_out_parts'; the control root does not depend on the
        image's size.  plan="device" plans where the table lies (zkh_page_tree_plan_device over (proof, 5 + h, D)): only the header is
        read back; the parts, and so the receipts, are the same.  dirty: the proof's dirty-node table (hal.image_proof_nodes, or
        `page_out(..., proof=True, dirty=True)`) in place of the two trees, which are then None (zkh_page_tree_witgen_nodes): the same
        receipts from (proof, dirty) alone.  -> the receipts, in the order of the parts."""
        return _page_seal.seal_chain("seal_page_out_tree", self, 7, segs, proof, proof_words, nodes_before, nodes_after, check, plan, dirty=dirty)

    def prove_segment(self, seg: Segment) -> SegmentReceipt:
        code, data, out = self.witgen(seg)
        return self.seal(seg, code, data, out)


def _generate_control_roots(po2s=range(13, 25)) -> None:
    """`python -m zeth_amd.prover` on a GPU box: (re)generate circuits/control_roots.json for the shipped circuits."""
    from .circuits import codegen
    hal = _hal.HipHal(0)
    roots: Dict[str, Dict[str, list]] = {}
    names = {}
    for name, desc in codegen.shipped().items():
        if int(np.asarray(desc)[13]) not in (1, 2, 3):     # only circuits with a built-in code generator have a per-size control root
            continue                                      # (a RECURSION program's control root belongs to the program: zkh_rec_program_info)
        prover = SegmentProver(hal, desc)
        key = desc_key(desc)
        names[key] = name
        roots[key] = {str(p): [int(x) for x in prover.control_root(p)] for p in po2s}
    with open(_CONTROL_ROOTS_JSON, "w") as fh:
        json.dump({"generator": "python -m zeth_amd.prover (zkh_syn_control_root on the GPU), zk_cycles = 1994",
                   "library": _hal.load_library().zkh_version().decode(), "names": names, "roots": roots}, fh, indent=1)
    print(f"wrote {_CONTROL_ROOTS_JSON}: {len(roots)} circuits x {len(list(po2s))} sizes")


if __name__ == "__main__":
    _generate_control_roots()
