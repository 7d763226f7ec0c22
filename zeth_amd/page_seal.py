"""Sealing and verifying a page-out: the host layer over the page-out circuits.  `PAGE_KINDS` states every circuit kind
that seals one, once.  `seal_chain` seals a page-out as a chain of parts (SegmentProver.seal_page_out, _parts, _ordered, _tree) and
`seal_tied_group` a paging segment and its page-out as one tied group (`seal_tied`, `seal_tied_tree`), both on `open_chain`;
`verify_chain` and `verify_tied_group` are their verifiers, HOST ONLY.  A PAGED RUN is many segments over one memory:
`preflight_paged_run` threads the image on the rank that holds it and ships one `PagedStep` per segment, `seal_paged_step`
(`seal_tied_tree_from_proof`) seals a step's whole group on any rank from the proof alone, and `verify_paged_run` (`link_paged_run`) takes
the groups from root_0 to root_S, HOST ONLY.  A prover reaches this module as an object (prover.py imports this
module, not the reverse), a receipt as what its `seal_with_accum` returns; the verifiers read only a receipt's `.seal`."""
from __future__ import annotations

import importlib
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import hal as _hal

TIE_WORDS = 12                                  # alpha (4) ‖ beta (4) ‖ F (4): the last words of `out` of every seal of a tied group


@dataclass(frozen=True)
class PageKind:
    """One circuit kind that seals a page-out.  module: zeth_amd/circuits/<module>.py, whose <module>_circuit() is the description and
    whose constants and `decode` are the kind's; code, witgen: the hal's code call and witness call, by method name.  family: "path" lays
    out one path per update (the plan is p2_page.parts, a part's operand is (first,), room is page_circuit_slots "slots"); "tree" lays out
    one block per dirty node (the plan is zkh_page_tree_plan's, made on the host or on the device, a part's operands are (first, count),
    room is "block slots").  ordered: the parts carry lo and hi; a path chain then starts at lo = 0, a tree chain is told h, checks its
    range and runs from 2^(h-1) to at most 2^h.  accum: "syn" (syn_accumulate), "args" (args_accumulate, with the chain's `check`) or
    "open": the kind is tied (the open accumulate); a tied tree part also states out_base(h) after its prefix, which its verifier checks."""
    kind: int
    module: str
    code: str
    witgen: str
    family: str
    ordered: bool
    accum: str
    mod = property(lambda self: importlib.import_module(f".circuits.{self.module}", __package__))
    out_words = property(lambda self: self.mod.OUT_WORDS)
    prefix_words = property(lambda self: getattr(self.mod, "PREFIX_WORDS", self.mod.OUT_WORDS))        # what the witness call returns
    desc = lambda self: getattr(self.mod, self.module + "_circuit")()

    def part(self, out) -> tuple:
        """link_page_parts' operands in a part's `out` words: root_before ‖ root_after and, ordered, lo ‖ hi, the last words of the prefix"""
        return (out[:8], out[8:16]) + (tuple(self.mod.decode(w) for w in out[self.prefix_words - 2:self.prefix_words]) if self.ordered else ())


PAGE_KINDS = {k.kind: k for k in (PageKind(5, "p2_page", "page_circuit_code", "page_circuit_witgen_part", "path", False, "syn"),
                                  PageKind(6, "p2_page_ordered", "page_ordered_code", "page_ordered_witgen", "path", True, "syn"),
                                  PageKind(7, "p2_tree", "page_tree_code", "page_tree_witgen", "tree", True, "args"),
                                  PageKind(8, "p2_page_tied", "page_ordered_code", "page_ordered_witgen", "path", True, "open"),
                                  PageKind(9, "p2_tree_tied", "page_tree_code", "page_tree_witgen", "tree", True, "open"))}


def _fmt_words(w) -> str:
    return " ".join(f"{int(x):08x}" for x in w)


def open_chain(who: str, prover, k: PageKind, segs: list, proof, proof_words: int, plan_where: str = "host", no_segment: str = "", buses=(), single: bool = False):
    """What a chain of parts and a tied group both open with -> (the proof on the device, po2, zk_cycles, the code group, the plan: per
    part the witness call's own operands).  segs: one Segment per part, all of one (po2, zk_cycles), each with its own noise seed;
    HalError if their number is not the plan's.  proof: a device Buffer whose first `proof_words` words are the proof, or the proof's
    words (uploaded).  plan_where: where a tree chain plans, refused before anything else unless "host" or "device"; buses: (name, prover)
    of the provers whose circuits must have an open bus, checked next; no_segment: the words after "no segment" for an empty `segs`.
    A path chain builds the code group (which refuses a shape without a path slot; P2-PAGE-ordered: and h > 26) and then plans; a tree
    chain plans (refusing W <= 16, B < h, addresses out of order), compares the plan with the segments and then builds the code group.
    single: P2-PAGE's one seal of a whole table (seal_page_out): one part, W from the header, no plan to compare with."""
    path = k.family == "path"
    if not path and plan_where not in ("host", "device"):
        raise _hal.HalError(f'{who}: plan="{plan_where}" (the plan is made on the "host" or on the "device")')
    for name, p in buses:
        if p.circuit.open_bus() is None:
            raise _hal.HalError(f"{who}: the {name} prover's circuit has no open bus (its arguments hold no OPEN record)")
    if not segs:
        raise _hal.HalError(f"{who}: no segment{no_segment}")
    hal, po2, zk = prover.hal, segs[0].po2, segs[0].zk_cycles
    if any((s.po2, s.zk_cycles) != (po2, zk) for s in segs):
        raise _hal.HalError(f"{who}: the parts share one code group: every segment must have the same (po2, zk_cycles)")
    if not isinstance(proof, _hal.Buffer):
        proof = hal.copy_from("image_proof", np.ascontiguousarray(proof, dtype=np.uint32).reshape(-1))
    if not path and not prover.circuit.has_arguments():
        raise _hal.HalError(f"{who}: the prover was built without P2-TREE's arguments (arguments=p2_tree.arguments())")
    header = [int(w) for w in proof.slice(0, min(5, proof.size())).to_vec()]
    code_call = lambda *shape: getattr(hal, k.code)(prover.circuit, po2, zk, *shape)
    if single:
        return proof, po2, zk, code_call(header[1] if len(header) > 1 else 0), [()]
    if path:
        from .circuits import p2_page
        W, D = header[1:3] if len(header) > 2 else (0, 0)
        code = code_call(W)
        plan, room = [(first,) for first, _count in p2_page.parts(po2, zk, W, D)], f"{hal.page_circuit_slots(po2, zk, W)} slots"
    else:
        W, D, h = (header[1], header[2], header[4]) if len(header) > 4 else (0, 0, 0)
        if 5 + h + 3 * D > min(proof_words, proof.size()):
            raise _hal.HalError(f"{who}: a proof of {proof_words} words does not hold its header and a table of {D} rows")
        if plan_where == "device":                                             # the table stays where zkh_page_out_proof left it
            plan = hal.page_tree_plan_device(po2, zk, W, proof, 5 + h, D)
        else:
            plan = hal.page_tree_plan(po2, zk, W, proof.slice(5 + h, 3 * D).to_vec()[::3] if D else np.zeros(0, dtype=np.uint32))
        room = f"{((1 << po2) - zk) // 31} block slots"
    if len(segs) != len(plan):
        raise _hal.HalError(f"{who}: {len(segs)} segments, but a table of {D} rows takes {len(plan)} parts of {room} at po2 {po2}")
    return proof, po2, zk, code if path else code_call(), plan


def part_witgen(who: str, prover, k: PageKind, nodes_before, nodes_after, dirty, single: bool = False):
    """The witness call of one part, by its source -> f(circuit, po2, zk_cycles, code, proof, proof_words, *part, data, noise_seed), a
    call of `prover`'s hal.  The two committed trees (nodes_before, nodes_after: the kind's own call), or `dirty`, the dirty-node table of
    the page-out's proof (HipHal.image_proof_nodes): then both trees must be None, the kind a tree kind, and the call is
    page_tree_witgen_nodes.  Only the keywords are looked at here: nothing of the prover is touched before the first witness."""
    if dirty is None:
        name = "page_circuit_witgen" if single else k.witgen
        return lambda circuit, po2, zk, code, proof, words, *rest: getattr(prover.hal, name)(circuit, po2, zk, code, proof, words, nodes_before, nodes_after, *rest)
    if k.family != "tree":
        raise _hal.HalError(f"{who}: dirty nodes seal the tree kinds (7, 9); kind {k.kind} lays out paths, which read the two trees")
    if nodes_before is not None or nodes_after is not None:
        raise _hal.HalError(f"{who}: dirty nodes stand in place of the two trees: nodes_before and nodes_after must be None")
    return lambda circuit, po2, zk, code, proof, words, *rest: prover.hal.page_tree_witgen_nodes(circuit, po2, zk, code, proof, words, dirty, *rest)


def seal_chain(who: str, prover, kind: int, segs, proof, proof_words: int, nodes_before, nodes_after, check: bool, plan_where: str = "host", single: bool = False,
               dirty=None) -> list:
    """Seal a page-out as a chain of parts of the untied kind `kind` -> the receipts, in the order of the parts.  segs, proof, single:
    open_chain's; nodes_before / nodes_after: the committed tree before and after the page-out.  Both trees are the WHOLE page-out's for
    every part, so the parts could be sealed in any order, or on several ranks; with `dirty` (part_witgen: the tree kinds) a rank needs
    neither tree, only the proof and its dirty-node table.  The code group and its control root are built once, before the first
    witness, and the data buffer is reused.  A single seal's witness call is page_circuit_witgen."""
    k, segs = PAGE_KINDS[kind], list(segs)
    witgen = part_witgen(who, prover, k, nodes_before, nodes_after, dirty, single)
    proof, po2, zk, code, plan = open_chain(who, prover, k, segs, proof, proof_words, plan_where, single=single)
    control_root = prover.code_root(code, po2)
    data = prover.hal.alloc_elem("data", prover.group_sizes()[2] << po2)
    receipts = []
    for seg, part in zip(segs, plan):
        out = witgen(prover.circuit, po2, zk, code, proof, proof_words, *part, data, seg.noise_seed)
        accum = prover.args_accumulate(seg, code, data, check=check) if k.accum == "args" else prover.syn_accumulate(seg, data)
        receipts.append(prover.seal_with_accum(seg, code, data, out, accum, check=check))
        receipts[-1].control_root = control_root.copy()
    return receipts


def commitment_bytes(columns: int, po2: int) -> int:
    """the device bytes a held commitment of `columns` columns at 2^po2 rows takes (zkh_commitment_bytes; include/zkhal.h): coefficients,
    4n evaluations, Merkle nodes.  Pass one of a tied group decides by it whether a seal fits before it commits."""
    return 4 * (5 * columns + 64) << po2


def _refuse_wide(who: str, seg_prover) -> None:
    """The tie puts one row (address, in, out) per word of the page-out's table on the open bus.  A memory of two value words per address has
    two such rows per page, (2 a + j, in_j, out_j), so its trace must carry the flat addresses: the PAGES record's flat-address columns
    (ZKA1 version 11; logup.py, FLAT).  A wide segment circuit with them goes through every tied entry point as a narrow one does: the
    proof's table is the flat one of 2 D rows, h the height of the flat image's tree, and the segment's open total the fingerprint of
    that table.  One without them is refused before anything is sealed."""
    ask = lambda name, default: getattr(seg_prover.circuit, name, lambda: default)()      # a circuit handle that cannot be asked pages what every circuit paged before
    words = ask("page_words", 1)
    if words > 1 and ask("page_flats", 0) == 0:
        raise _hal.HalError(f"{who}: the segment's memory holds {words} value words per address (ZKA1 version 10): the tie of a wide memory is not built without "
                            f"flat-address columns (ZKA1 version 11: derive_pages(..., flats=))")


def seal_tied_group(who: str, kind: int, seg_prover, seg, code, data, out_prefix, page_prover, page_segs, proof, proof_words: int, nodes_before, nodes_after,
                    check: bool, check_table: bool, plan_where: str = "host", dirty=None, hold_bytes: int = 0):
    """The two passes of `seal_tied` (kind 8) and `seal_tied_tree` (kind 9), on open_chain -> (the segment's receipt, [the parts'
    receipts]).  A part's `out` words before alpha are the kind's prefix of what the witness call returns and, for kind 9, out_base(h).
    dirty: part_witgen's (kind 9: the parts' witnesses from the dirty-node table, both trees None).
    hold_bytes: the device bytes pass one may keep for pass two (`seal_tied`); 0 holds nothing.  The held seals are a prefix of the
    group in its order, the segment first: `held` lists per held seal (its commitment, its trace if the trace is this call's, what its
    witness call returned).  Whatever ends the call, a refusal included, every held commitment and trace is released first."""
    _refuse_wide(who, seg_prover)
    k, hal, page_segs = PAGE_KINDS[kind], seg_prover.hal, list(page_segs)
    witgen = part_witgen(who, seg_prover, k, nodes_before, nodes_after, dirty)
    proof, po2, zk, page_code, plan = open_chain(who, page_prover, k, page_segs, proof, proof_words, plan_where,
                                                 " for the page-out (a page-out of no rows still has one part)", (("segment", seg_prover), ("page-out", page_prover)))
    head = proof.slice(0, 5).to_vec()
    rows, h, table_at = int(head[2]), int(head[4]), 5 + int(head[4])
    page_words = page_prover.group_sizes()[2] << po2
    page_data = hal.alloc_elem("data", page_words)
    held, room, holding = [], hold_bytes, hold_bytes > 0

    def part_witness(s, part, into):
        return witgen(page_prover.circuit, po2, zk, page_code, proof, proof_words, *part, into, s.noise_seed)

    def commit(prover, trace, trace_po2, own_trace, out):
        """pass one of one seal -> its data root.  The seal is held if every seal before it is and it fits in what is left of the budget:
        its commitment and, if the trace is this call's (a part's), the trace."""
        nonlocal room, holding
        trace_bytes = 4 * trace.size() if own_trace else 0
        holding = holding and commitment_bytes(prover.group_sizes()[2], trace_po2) + trace_bytes <= room
        if not holding:
            return prover.data_root(trace, trace_po2)
        com = prover.commit_data(trace, trace_po2)
        held.append((com, trace if own_trace else None, out))
        room -= com.bytes + trace_bytes
        if room < 0:                                                            # the allocator rounded a tiny buffer up: not held after all
            holding = False
            held.pop()[0].release()
        return com.root

    def open_seal(prover, s, code, data, prefix):
        accum = hal.alloc_elem("accum", prover.group_sizes()[0] << s.po2)
        total = hal.accumulate_open(prover.circuit, s.po2, s.zk_cycles, s.noise_seed, code, data, challenge, accum)
        out = np.concatenate([np.asarray(prefix, dtype=np.uint32).reshape(-1), challenge, total]).astype(np.uint32)
        if out.size != prover.out_size():
            raise _hal.HalError(f"{who}: {out.size} out words (a prefix of {out.size - TIE_WORDS}, alpha, beta, the total), the circuit has {prover.out_size()}")
        return accum, total, out

    try:
        # pass one: the data roots, the segment's first
        roots = [commit(seg_prover, data, seg.po2, False, None)]
        for s, part in zip(page_segs, plan):
            if page_data is None:                                               # a held part kept the buffer: it is not reused
                page_data = hal.alloc_elem("data", page_words)
            n_held, out = len(held), part_witness(s, part, page_data)
            roots.append(commit(page_prover, page_data, po2, True, out))
            if len(held) > n_held:
                page_data = None
        challenge = _hal.tie_challenge(np.concatenate(roots))

        seg_accum, seg_total, seg_out = open_seal(seg_prover, seg, code, data, out_prefix)
        if check_table:
            want = hal.table_fingerprint(proof, table_at, rows, challenge)
            if not np.array_equal(seg_total, want):
                raise _hal.HalError(f"{who}: the proof's table is not the segment's page table: the segment's open total is {_fmt_words(seg_total)}, "
                                    f"the fingerprint of the proof's {rows} rows is {_fmt_words(want)}")
        # pass two: the seals; a held seal begins from its commitment, which is then released with its trace
        begin = lambda p: {"held": held[p][0]} if p < len(held) else {}
        seg_receipt = seg_prover.seal_with_accum(seg, code, data, seg_out, lambda _mix: seg_accum, check=check, **begin(0))
        if held:
            _release(held[0])
        seg_receipt.control_root = seg_prover.code_root(code, seg.po2)
        del seg_accum
        page_root = page_prover.code_root(page_code, po2)
        receipts = []
        for p, (s, part) in enumerate(zip(page_segs, plan), 1):
            if p < len(held):
                _com, trace, out = held[p]
            else:
                if page_data is None:
                    page_data = hal.alloc_elem("data", page_words)
                trace, out = page_data, part_witness(s, part, page_data)
            prefix = np.concatenate([out[:k.prefix_words], [k.mod.out_base(h)] if k.family == "tree" else []])
            accum, _total, out = open_seal(page_prover, s, page_code, trace, prefix)
            receipts.append(page_prover.seal_with_accum(s, page_code, trace, out, lambda _mix, accum=accum: accum, check=check, **begin(p)))
            receipts[-1].control_root = page_root.copy()
            if p < len(held):
                _release(held[p])
        return seg_receipt, receipts
    finally:
        for seal in held:
            _release(seal)


def _release(held_seal) -> None:
    """give back what pass one kept of one seal: its commitment and, if it is the call's own, its trace (both releases are idempotent)"""
    com, trace, _out = held_seal
    com.release()
    if trace is not None:
        trace.release()


def seal_tied(seg_prover, seg, code, data, out_prefix, page_prover, page_segs, proof, proof_words: int,
              nodes_before, nodes_after, check: bool = False, check_table: bool = True, hold_bytes: int = 0):
    """Seal a paging segment and the page-out of its memory as ONE tied group (DESIGN.md §2 "THE TIE") -> (the segment's receipt, [the
    parts' receipts]): the seals share a bus under a challenge drawn from all their data roots, and `verify_tied` accepts them only
    together.  seg_prover: a prover of an open-bus paging circuit (SYN-LOOKUP-tied, built with its arguments); code, data: the segment's
    traces on the device, derived and reduced (what seal_host_witness hands its accumulate); out_prefix: the segment's `out` words before
    alpha.  page_prover: a prover of P2-PAGE-tied with p2_page_tied.arguments(); page_segs, proof, proof_words, nodes_before, nodes_after:
    seal_page_out_ordered's operands.  Two passes, so that one part's traces are held at a time:
      1. the roots: the segment's data root (zkh_data_root); per part the witness, its data root, and the buffer is reused; the
         challenge alpha ‖ beta = hal.tie_challenge(the roots, the segment's first).
      between, with check_table: the segment's open total must be hal.table_fingerprint of the proof's table under that challenge, else
         HalError "the proof's table is not the segment's page table": no part is sealed on a table that cannot cancel.
      2. the segment and then every part: the part's witness again (the same noise key gives the same trace, hence the same root),
         accumulate_open, out = prefix ‖ challenge ‖ total, zkh_prove_begin, with `check` check_witness, zkh_prove_finish.
    hold_bytes: device bytes pass one may keep for pass two, 0 (the default) none.  Pass one walks the seals in their order, the segment
    first, and holds a seal (commit_data instead of data_root) while the running sum stays within the budget: the commitment's bytes
    (page_seal.commitment_bytes) and, for a part, the bytes of its data trace, which is then not reused for the next part.  The held
    seals are a prefix: the first that does not fit and every one after it go the two passes above.  In pass two a held seal neither
    generates its witness nor commits again: accumulate_open on the kept trace, seal_with_accum(held=...) (zkh_prove_begin_held), then
    commitment and trace are released.  The seals are byte for byte those of hold_bytes = 0.  Whatever ends the call, the table
    refusal between the passes, a failed check_witness and a refused accumulate included, what is held is released first.
    Every receipt carries its code group's root as `control_root`."""
    return seal_tied_group("seal_tied", 8, seg_prover, seg, code, data, out_prefix, page_prover, page_segs, proof, proof_words, nodes_before, nodes_after, check, check_table,
                           hold_bytes=hold_bytes)


def seal_tied_tree(seg_prover, seg, code, data, out_prefix, page_prover, page_segs, proof, proof_words: int,
                   nodes_before, nodes_after, check: bool = False, check_table: bool = True, plan: str = "host", dirty=None, hold_bytes: int = 0):
    """`seal_tied` with P2-TREE-tied parts (circuits/p2_tree_tied.py): the page-out side of the group is one block per DIRTY NODE, not one
    path per word.  page_prover: a prover of P2-TREE-tied with p2_tree_tied.arguments(); the plan is seal_page_out_tree's, made on the
    "host" or on the "device" (`plan`); every other operand, both passes and the fingerprint check between them are seal_tied's.  A part's
    out = the witness call's 18 words ‖ p2_tree_tied.out_base(h) ‖ the challenge ‖ its open total.  dirty: the dirty-node table of the
    proof (HipHal.image_proof_nodes) in place of the two trees, which are then None: the same seals, byte for byte.  -> (the segment's
    receipt, [the parts' receipts]), for `verify_tied_tree`."""
    return seal_tied_group("seal_tied_tree", 9, seg_prover, seg, code, data, out_prefix, page_prover, page_segs, proof, proof_words, nodes_before, nodes_after, check, check_table, plan,
                           dirty, hold_bytes)


def _upload_traces(prover, seg, host_code, host_data, pinned: bool):
    """the segment's host traces on the device as seal_host_witness uploads them (of the derived columns only the blinding rows) -> (code,
    data).  pinned: both lie in hal.host_alloc blocks and the copies are enqueued; else any host memory, consumed before the return"""
    hal = prover.hal
    code, data = hal.alloc_elem("code", host_code.size), hal.alloc_elem("data", host_data.size)
    if pinned:
        hal.write_async(code, host_code)
    else:
        code.write(np.ascontiguousarray(host_code, dtype=np.uint32).reshape(-1))
        host_data = np.ascontiguousarray(host_data, dtype=np.uint32).reshape(-1)
    hal.upload_data_trace(prover.circuit, seg.po2, seg.zk_cycles, data, host_data, pinned_async=pinned)
    return code, data


def seal_tied_tree_from_proof(seg_prover, seg, host_code, host_data, out_prefix, page_prover, page_segs, proof, root_before, check: bool = False,
                              check_table: bool = True, plan: str = "device", hold_bytes: int = 0, pinned: bool = False):
    """Seal a whole tied group (`seal_tied_tree`) on a rank that holds NEITHER the image NOR its tree, from what the rank that does ships:
    the segment's underived host traces (host_code, host_data: what seal_host_witness is handed), the ZKU1 proof of its page-out and
    root_before -> (the segment's receipt, [the parts' receipts], root_after).  In order: hal.image_proof_nodes(proof, root_before), which
    refuses a proof that does not open root_before before anything is derived and leaves the dirty-node table; the upload; the derive
    stages with the proof's table where it lies in the image's place (derive_all_paged_table, table_at = 5 + h, W and D from the header);
    reduce_elem on both traces; seal_tied_group with both trees None.  With the same noise seeds the seals are byte for byte those of
    `seal_tied_tree` on the rank that holds the image.  proof: the proof's words, or a device Buffer that is the proof.  page_segs: a
    list, one Segment per part, or a callable p -> Segment asked once per part of the plan (made as `plan` says).  pinned: the host
    traces lie in hal.host_alloc blocks (the uploads are then enqueued, as seal_host_witness does).  The other operands are
    seal_tied_tree's."""
    who, hal = "seal_tied_tree_from_proof", seg_prover.hal
    _refuse_wide(who, seg_prover)
    if not isinstance(proof, _hal.Buffer):
        proof = hal.copy_from("image_proof", np.ascontiguousarray(proof, dtype=np.uint32).reshape(-1))
    words = proof.size()
    root_after, dirty = hal.image_proof_nodes(proof, root_before, words=words)
    head = proof.slice(0, 5).to_vec()                                        # image_proof_nodes has checked the header against the words
    W, D, h = int(head[1]), int(head[2]), int(head[4])
    if callable(page_segs):
        if plan not in ("host", "device"):
            raise _hal.HalError(f'{who}: plan="{plan}" (the plan is made on the "host" or on the "device")')
        first = page_segs(0)                                                 # every part has one (po2, zk_cycles): the first one's
        parts = (hal.page_tree_plan_device(first.po2, first.zk_cycles, W, proof, 5 + h, D) if plan == "device" else
                 hal.page_tree_plan(first.po2, first.zk_cycles, W, proof.slice(5 + h, 3 * D).to_vec()[::3]))
        page_segs = [first] + [page_segs(p) for p in range(1, len(parts))]
    code, data = _upload_traces(seg_prover, seg, host_code, host_data, pinned)
    hal.derive_all_paged_table(seg_prover.circuit, seg.po2, seg.zk_cycles, code, data, proof, W, table_at=5 + h, D=D)
    hal.reduce_elem(code)
    hal.reduce_elem(data)
    seg_receipt, receipts = seal_tied_group(who, 9, seg_prover, seg, code, data, out_prefix, page_prover, page_segs, proof, words, None, None, check, check_table,
                                            plan, dirty, hold_bytes)
    return seg_receipt, receipts, root_after


@dataclass(frozen=True)
class PagedStep:
    """What the rank that holds the image ships for one segment of a paged run (`preflight_paged_run`): the segment, its host traces as
    they were given (underived), the words of the ZKU1 proof of its page-out, and the roots the page-out leads between.  It holds no
    image, no tree and no derived trace: any rank seals the step's tied group from it (`seal_paged_step`)."""
    seg: object
    host_code: np.ndarray
    host_data: np.ndarray
    proof: np.ndarray
    root_before: np.ndarray
    root_after: np.ndarray


def preflight_paged_run(seg_prover, segs, witnesses, image, tree, pinned: bool = False) -> list:
    """Thread ONE memory image through the segments of a run, on the rank that holds it -> one PagedStep per segment.  segs: the
    Segments, in the run's order; witnesses: per segment (host_code, host_data), underived; image, tree: the image as a device Buffer
    and its committed tree (hal.image_commit), both the run's: they end as the last segment leaves them.  Per segment, in order: the
    upload; derive_all_paged from the image as it is now; reduce_elem; SegmentProver.page_out(..., proof=True, walk=True), which builds
    the proof from the tree as it is, writes the page table back, brings the tree up to date and checks that the proof walks to the new
    root.  No derived trace is kept.  A segment that pages no address (an empty table) is refused here: its group has no dirty node and
    is sealed from the tree (`seal_tied_tree`); its page-out has changed nothing."""
    _refuse_wide("preflight_paged_run", seg_prover)
    segs, witnesses, hal = list(segs), list(witnesses), seg_prover.hal
    if len(segs) != len(witnesses):
        raise _hal.HalError(f"preflight_paged_run: {len(segs)} segments, but {len(witnesses)} witnesses")
    steps = []
    for k, (seg, (host_code, host_data)) in enumerate(zip(segs, witnesses)):
        code, data = _upload_traces(seg_prover, seg, host_code, host_data, pinned)
        hal.derive_all_paged(seg_prover.circuit, seg.po2, seg.zk_cycles, code, data, image)
        hal.reduce_elem(data)
        root_before = hal.image_root(tree)
        proof = seg_prover.page_out(seg, data, image, tree=tree, proof=True, walk=True)
        if int(proof[2]) == 0:
            raise _hal.HalError(f"preflight_paged_run: segment {k} pages no address (an empty table has no dirty nodes): its group is sealed from the tree "
                                f"(seal_tied_tree)")
        steps.append(PagedStep(seg, host_code, host_data, proof, root_before, hal.image_root(tree)))
    return steps


def seal_paged_step(step: PagedStep, seg_prover, out_prefix, page_prover, page_segs, **kw):
    """`seal_tied_tree_from_proof` on one step of `preflight_paged_run` -> (the segment's receipt, [the parts' receipts]).  It is handed no
    image and no tree, and the steps of a run may be sealed in any order, on any rank.  HalError if the proof does not lead to the root
    the step states."""
    seg_receipt, receipts, root_after = seal_tied_tree_from_proof(seg_prover, step.seg, step.host_code, step.host_data, out_prefix, page_prover, page_segs, step.proof,
                                                                  step.root_before, **kw)
    if not np.array_equal(root_after, np.asarray(step.root_after, dtype=np.uint32)):
        raise _hal.HalError(f"seal_paged_step: the proof leads to root {_fmt_words(root_after)}, but the step states root_after {_fmt_words(step.root_after)}")
    return seg_receipt, receipts


def link_paged_run(roots, root_before=None) -> Tuple[np.ndarray, np.ndarray]:
    """The links of a paged run, HOST ONLY: what verify_paged_run checks once every group is verified -> (root_0, root_S).  roots: per
    group, in the run's order, (the root it opens, the root it leaves); an iterator is consumed group by group.  Group k + 1 must open
    the root group k left; with a `root_before`, group 0 must open it.  Raises HalError, one message per cause."""
    who = "verify_paged_run"
    chain = [(np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32)) for a, b in roots]
    if not chain:
        raise _hal.HalError(f"{who}: no group")
    if root_before is not None and not np.array_equal(chain[0][0], np.asarray(root_before, dtype=np.uint32)):
        raise _hal.HalError(f"{who}: group 0 opens root {_fmt_words(chain[0][0])}, not root_before {_fmt_words(root_before)}")
    for k in range(1, len(chain)):
        if not np.array_equal(chain[k][0], chain[k - 1][1]):
            raise _hal.HalError(f"{who}: group {k} opens root {_fmt_words(chain[k][0])}, but group {k - 1} left root {_fmt_words(chain[k - 1][1])}")
    return chain[0][0], chain[-1][1]


def verify_paged_run(groups, seg_circuit, seg_control_root, page_control_root, h: int, root_before=None) -> Tuple[np.ndarray, np.ndarray]:
    """Verify a paged run, HOST ONLY -> (root_0, root_S): the segments' page tables, applied in the run's order to the image under root_0,
    leave root_S.  groups: per segment (its receipt, [the parts' receipts]) of a tied group whose parts are P2-TREE-tied's
    (`seal_paged_step`, `seal_tied_tree`), in the run's order; one segment circuit, one control root each for the segments and for the
    parts, one tree height h.  Every group goes through `verify_tied_group` (kind 9) as verify_tied_tree runs it; then the groups must
    link (`link_paged_run`).  Raises HalError: a group's own message, or one line per cause on a run that does not link."""
    def verified():
        for seg_receipt, part_receipts in groups:
            yield verify_tied_group("verify_tied_tree", 9, seg_receipt, seg_circuit, seg_control_root, part_receipts, page_control_root, None, h)[:2]
    return link_paged_run(verified(), root_before)


def link_page_parts(who: str, parts, root_before=None, first_lo=None, last_hi=None) -> tuple:
    """The links of a chain of page-out seals, HOST ONLY: what verify_page_out_chain, verify_page_ordered_chain and
    link_page_tree_chain check once a seal is verified -> (root_before, root_after) of the whole page-out, and hi where the parts have
    one.  parts: per part (the root it opens, the root it leaves) or (…, lo, hi), lo and hi as integers; an iterator is consumed part
    by part, so a caller may verify each seal as it hands it over.  who: the prefix of every message.  Part p + 1 must open the root
    part p left; with a `root_before`, part 0 must open it.  Parts with lo and hi: every lo and hi must be at most 2^29 (what the
    circuits' 29-bit gaps are sound for); part p + 1 must start at the hi part p left; first_lo = (the lo part 0 must have, the words
    that say why); last_hi, if given = (the bound of the last hi, the words that say why).  Raises HalError, one message per cause."""
    from .circuits.p2_blocks import GAP_BITS
    chain = []
    for p, part in enumerate(parts):
        for name, v in zip(("lo", "hi"), part[2:]):
            if v > 1 << GAP_BITS:
                raise _hal.HalError(f"{who}: part {p}: {name} {v} is above 2^{GAP_BITS}, the bound the order check is sound for")
        chain.append((np.array(part[0], dtype=np.uint32), np.array(part[1], dtype=np.uint32)) + tuple(part[2:]))
    if not chain:
        raise _hal.HalError(f"{who}: no receipt (a page-out of no rows still has one part)")
    ordered = len(chain[0]) > 2
    if ordered and chain[0][2] != first_lo[0]:
        raise _hal.HalError(f"{who}: part 0 starts at lo {chain[0][2]}, not {first_lo[1]}")
    if root_before is not None and not np.array_equal(chain[0][0], np.asarray(root_before, dtype=np.uint32)):
        raise _hal.HalError(f"{who}: part 0 opens root {_fmt_words(chain[0][0])}, not root_before {_fmt_words(root_before)}")
    for p in range(len(chain) - 1):
        if not np.array_equal(chain[p + 1][0], chain[p][1]):
            raise _hal.HalError(f"{who}: part {p + 1} opens root {_fmt_words(chain[p + 1][0])}, but part {p} left root {_fmt_words(chain[p][1])}")
        if ordered and chain[p + 1][2] != chain[p][3]:
            raise _hal.HalError(f"{who}: part {p + 1} starts at lo {chain[p + 1][2]}, but part {p} left hi {chain[p][3]}")
    if ordered and last_hi is not None and chain[-1][3] > last_hi[0]:
        raise _hal.HalError(f"{who}: the last part leaves hi {chain[-1][3]}, above {last_hi[1]}")
    return (chain[0][0], chain[-1][1]) + chain[-1][3:]


def link_page_tree_chain(outs, h: int, root_before=None) -> Tuple[np.ndarray, np.ndarray, int]:
    """What verify_page_tree_chain checks of the parts' `out` words (18 each) once every seal is verified -> (root_before, root_after,
    hi).  Every lo and hi must decode to at most 2^29; part 0 must have lo = 2^(h-1), the id of the first pair of leaves; part p + 1
    must open the root part p left and start at the hi part p left; the last hi must be at most 2^h, so every pair block's id lies in
    [2^(h-1), 2^h): h - 1 levels below the root; with a `root_before`, part 0 must open it.  Raises HalError, one message per cause."""
    from .circuits import p2_tree as pt
    who = "verify_page_tree_chain"
    if not pt.MIN_H <= h <= pt.MAX_H:
        raise _hal.HalError(f"{who}: h {h} ({pt.MIN_H} .. {pt.MAX_H})")
    return link_page_parts(who, (PAGE_KINDS[7].part(out) for out in outs), root_before,
                           first_lo=(1 << (h - 1), f"2^{h - 1} = {1 << (h - 1)}, the id of the first pair of leaves of a tree of height {h}"),
                           last_hi=(1 << h, f"2^{h} = {1 << h}: a pair block outside a tree of height {h}"))


def link_tied_tree_chain(outs, h: int, root_before=None) -> Tuple[np.ndarray, np.ndarray, int]:
    """What verify_tied_tree checks of the parts' `out` words (31 each) besides the group's challenge and totals -> (root_before, root_after,
    hi): `link_page_tree_chain` on their first 18 words, then every part's out[18] must be p2_tree_tied.out_base(h), the word that turns a
    pair block's id into its addresses.  Raises HalError, one message per cause."""
    from .circuits import p2_tree_tied as tt
    outs = [np.asarray(out, dtype=np.uint32) for out in outs]
    linked = link_page_tree_chain([out[:tt.PREFIX_WORDS] for out in outs], h, root_before)
    for p, out in enumerate(outs):
        if int(out[tt.OUT_BASE]) != tt.out_base(h):
            raise _hal.HalError(f"verify_tied_tree: part {p}: base {tt.decode(out[tt.OUT_BASE])} is not {1 << (h + 3)} = 16 * 2^{h - 1}, sixteen times the id of "
                                f"the first pair of leaves of a tree of height {h}")
    return linked


def _verified_parts(receipts, k: PageKind, control_root):
    """per receipt, once its seal is verified against the kind's description and `control_root`: the operands of link_page_parts"""
    hc = None
    for r in receipts:
        hc = hc or _hal.HostCircuit(k.desc())
        hc.verify_segment(r.seal, control_root)
        yield k.part(r.seal)


def verify_chain(who: str, kind: int, receipts, control_root, root_before=None, h=None) -> tuple:
    """Verify the chain of seals of one page-out whose parts are of kind `kind`, HOST ONLY -> (root_before, root_after) and, where the
    parts have one, hi.  Every seal is verified against the kind's description and `control_root` (one for all parts), and the parts link
    by the kind's rule.  A path chain verifies part p and bounds its lo and hi before it verifies part p + 1.  A tree chain is told h: it
    refuses an empty list, verifies every seal, and only then looks at h and links (as verify_page_tree_chain, whoever asks)."""
    k, receipts = PAGE_KINDS[kind], list(receipts)
    parts = _verified_parts(receipts, k, control_root)
    if k.family == "path":
        return link_page_parts(who, parts, root_before, first_lo=(0, "0: addresses below it are not covered") if k.ordered else None)
    if not receipts:
        raise _hal.HalError(f"{who}: no receipt (a page-out of no rows still has one part)")
    list(parts)
    return (link_tied_tree_chain if k.accum == "open" else link_page_tree_chain)([r.seal[:k.out_words] for r in receipts], h, root_before)


def verify_tied_group(who: str, kind: int, seg_receipt, seg_circuit, seg_control_root, part_receipts, page_control_root, root_before=None, h=None) -> tuple:
    """Verify a tied group whose parts are of kind `kind`, HOST ONLY -> (root_before, root_after, hi): the segment's seal first, then
    the chain of parts as verify_chain does, then `_check_tied_totals` over all seals."""
    k, part_receipts = PAGE_KINDS[kind], list(part_receipts)
    desc = np.asarray(seg_circuit, dtype=np.uint32)
    seg_hc, seg_out_size = _hal.HostCircuit(desc), int(desc[7])
    if seg_out_size < TIE_WORDS:
        raise _hal.HalError(f"{who}: the segment circuit has {seg_out_size} out words: no room for alpha, beta and the total")
    seg_hc.verify_segment(seg_receipt.seal, seg_control_root)
    linked = verify_chain(who, kind, part_receipts, page_control_root, root_before, h)
    page_hc = _hal.HostCircuit(k.desc())
    _check_tied_totals(who, [("the segment", seg_hc, seg_receipt.seal, seg_out_size)] + [(f"part {p}", page_hc, r.seal, k.out_words) for p, r in enumerate(part_receipts)])
    return linked


def _check_tied_totals(who: str, seals) -> None:
    """The challenge and total checks of a tied group whose seals are verified.  seals: (name, HostCircuit, seal, out words) per seal, the
    segment's first.  Every seal must state the challenge `hal.tie_challenge` gives for the data roots read out of the seals in that
    order, and the totals F must add up to zero in Fp4.  Raises HalError, one line per cause."""
    want = _hal.tie_challenge(np.concatenate([hc.seal_data_root(seal) for _, hc, seal, _ in seals]))
    total = np.zeros(4, dtype=np.uint64)
    for name, _, seal, out_size in seals[1:] + seals[:1]:                     # a part that was swapped in is named before the segment
        stated = np.asarray(seal[out_size - TIE_WORDS:out_size - 4], dtype=np.uint32)
        if not np.array_equal(stated, want):
            raise _hal.HalError(f"{who}: {name}: its challenge {_fmt_words(stated)} is not the one the data roots give, {_fmt_words(want)}")
        total = (total + np.asarray(seal[out_size - 4:out_size], dtype=np.uint64)) % np.uint64(_hal.P)
    if total.any():
        raise _hal.HalError(f"{who}: the totals do not cancel: the segment's F plus the parts' is {_fmt_words(total)}, not zero: the parts' rows are not "
                            f"the segment's page table")


def verify_page_out_chain(receipts, control_root, root_before=None) -> Tuple[np.ndarray, np.ndarray]:
    """Verify the chain of P2-PAGE seals of one page-out (SegmentProver.seal_page_out_parts), HOST ONLY -> (root_before, root_after) of
    the whole page-out.  Every seal is verified against P2-PAGE's description and `control_root` (the code group's: one for all
    parts); part p + 1 must open the root part p left; with a `root_before`, part 0 must open it.  Raises HalError on a seal the
    verifier rejects, on a chain that does not link, on another first root, and on an empty list."""
    return verify_chain("verify_page_out_chain", 5, receipts, control_root, root_before)


def verify_page_ordered_chain(receipts, control_root, root_before=None) -> Tuple[np.ndarray, np.ndarray, int]:
    """Verify the chain of P2-PAGE-ordered seals of one page-out (SegmentProver.seal_page_out_ordered), HOST ONLY -> (root_before,
    root_after, hi) of the whole page-out: its live updates have strictly increasing addresses, the last of them hi - 1 (hi = 0: none).
    Every seal is verified against P2-PAGE-ordered's description and `control_root` (one for all parts); every lo and hi must decode
    to at most 2^29 (what the circuit's 29-bit gaps are sound for); part 0 must have lo = 0; part p + 1 must open the root part p left
    and start at the hi part p left; with a `root_before`, part 0 must open it.  Raises HalError, one message per cause."""
    return verify_chain("verify_page_ordered_chain", 6, receipts, control_root, root_before)


def verify_page_tree_chain(receipts, control_root, h: int, root_before=None) -> Tuple[np.ndarray, np.ndarray, int]:
    """Verify the chain of P2-TREE seals of one page-out (SegmentProver.seal_page_out_tree), HOST ONLY -> (root_before, root_after, hi)
    of the whole page-out.  Every seal is verified against P2-TREE's description and `control_root` (one per (po2, zk_cycles), for
    every image size); then the parts' outputs must link (`link_page_tree_chain`): the verifier is told h, the height of the image's
    tree.  Raises HalError on a seal the verifier rejects, and one message per cause on a chain that does not link."""
    return verify_chain("verify_page_tree_chain", 7, receipts, control_root, root_before, h)


def verify_tied(seg_receipt, seg_circuit, seg_control_root, part_receipts, page_control_root, root_before=None) -> Tuple[np.ndarray, np.ndarray, int]:
    """Verify a tied group (`seal_tied`), HOST ONLY -> (root_before, root_after, hi): the page table of the segment `seg_receipt` seals,
    applied in order to the image under root_before, leaves root_after, its last address hi - 1 (hi = 0: the segment touched no memory).
    seg_circuit: the segment circuit's description (its `out` ends on alpha ‖ beta ‖ F, as every tied circuit's does); the parts are
    P2-PAGE-tied's.  On top of the ordered chain (`link_page_parts`, as verify_page_ordered_chain) it makes the four checks of the design:
    every seal verifies against its control root; every seal states the challenge that `hal.tie_challenge` gives for the data roots read
    out of the seals themselves, the segment's first (one comparison per seal: they then all state the same one); the totals F of all
    seals add up to zero in Fp4.  Raises HalError, one line per cause, naming the seal and the two values that differ."""
    return verify_tied_group("verify_tied", 8, seg_receipt, seg_circuit, seg_control_root, part_receipts, page_control_root, root_before)


def verify_tied_tree(seg_receipt, seg_circuit, seg_control_root, part_receipts, page_control_root, h: int, root_before=None) -> Tuple[np.ndarray, np.ndarray, int]:
    """Verify a tied group whose page-out side is P2-TREE-tied's (`seal_tied_tree`), HOST ONLY -> (root_before, root_after, hi): the page
    table of the segment `seg_receipt` seals, applied to the image under root_before, leaves root_after; hi is one more than the id of
    the last pair of leaves it touches.  The verifier is told h, the height of the image's tree.  Every seal verifies against its
    control root; the parts link as P2-TREE's do and state base = 16 * 2^(h-1) (`link_tied_tree_chain`); then `verify_tied`'s checks of
    the challenge and of the totals.  Raises HalError, one line per cause."""
    return verify_tied_group("verify_tied_tree", 9, seg_receipt, seg_circuit, seg_control_root, part_receipts, page_control_root, root_before, h)
