#!/usr/bin/env python3
"""Per-op micro-benchmarks M1..M8 of SURVEY.md §8d (+ M9: the trace-driven witness, row f1; M10: the built-in accumulate of SYN-LOOKUP's
arguments and its share of that circuit's seal; M11 / M11w: derived lookup multiplicities of SYN-LOOKUP-derived / WIDE; M12: derived sorted copies of SYN-LOOKUP-sorted
against the host's lexsort + upload; M13: derived columns — the 64 limb columns of SYN-LOOKUP FULL — next to a plain copy of the same
bytes, and the host-witness seal with its upload; M14: linked accesses of SYN-LOOKUP-linked (zkh_derive_links) next to a plain copy of
the same bytes, to the host's sort + gather + upload, and the host-witness seal with the derive against the host-made columns; M14r: the read rule, zkh_derive_links on SYN-LOOKUP-reads
under its version-6 blob next to the same trace under the version-5 blob; M15: zkh_check_rows, the row-by-row constraint check of an honest
SYN-A / SYN-HEAVY witness, next to zkh_eval_check on the step interpreter for the same circuit in the same run, alternating; M16:
zkh_check_bus, the key-by-key bus check of the honest SYN-LOOKUP FULL witness, with and without its per-term pass, next to zkh_accumulate
and zkh_derive_multiplicities on the same trace in the same run, alternating; M17: paging, zkh_derive_links_paged on SYN-LOOKUP-paged
under its version-7 blob next to zkh_derive_links under the version-6 blob on the same trace, and zkh_page_out next to a copy of the
same bytes, alternating; M18: the committed image, zkh_page_out_tree (the page-out with the incremental update of the image's Merkle
tree) next to zkh_page_out followed by zkh_image_commit (the full rebuild), for the derive's own page table, a hand-made table of as many
pages spread over the whole image and a sparse one of 4096 pages, at two image sizes, alternating; M19: the update's proof,
zkh_page_out_proof next to zkh_page_out_tree on M18's tables and image sizes, alternating, with the proof's size; M20: the walk of
that proof on the device, zkh_image_proof_walk next to the host walk of the downloaded proof (zkh_image_proof_verify), the download and
zkh_page_out_tree, alternating, with the number of permutations; M21: P2-PAGE's witness, zkh_page_circuit_witgen with full slots at
h = 17 and h = 23 next to zkh_syn_witgen of P2-JOIN at the same po2, alternating, with both calls' stages; M22: P2-PAGE's parts,
zkh_page_circuit_witgen_part on a table of 4 N rows at first = 0, N, 2 N, 3 N next to zkh_page_circuit_witgen on its first N rows,
alternating, with every call's stages; M23: P2-PAGE-ordered, zkh_page_ordered_witgen next to zkh_page_circuit_witgen_part at first = 0 and
first = N of one table, and the seal of a part under both circuits, alternating, with every witness call's stages; M24: P2-TREE, the
parts of one page-out of 662 267 addresses under p2_tree's plan and under P2-PAGE's, zkh_page_tree_witgen next to
zkh_page_ordered_witgen and the seal of a part under both circuits, alternating, with every witness call's stages; M25: P2-TREE's plan
of M24's table by zkh_page_tree_plan_device next to the read-back of the table and zkh_page_tree_plan, alternating; M26: zkh_reduce_elem
at SYN-A's code and data widths next to zkh_eltwise_copy_elem over the same bytes, alternating; M27: the tie, zkh_data_root of a P2-PAGE-tied
part next to its seal, zkh_accumulate_open next to zkh_accumulate, zkh_table_fingerprint next to a copy of the same bytes, alternating;
M28: P2-TREE-tied, the witness and the seal of a kind-9 part next to the kind-7 part's, alternating, and the page-out side of a whole tied
group under P2-TREE-tied next to P2-PAGE-tied's on the same table; M29: P2-TREE from the proof alone, zkh_image_proof_nodes next to
zkh_image_proof_walk and part 0's witness from the dirty nodes next to part 0's witness from the two trees on M24's table, alternating, with
the words of the table, of the proof and of the two trees, and the copy of the tree that keep_before makes; M30: held commitments, a
whole tied group on M28's setup sealed in two passes next to the same group with hold_bytes for everything, alternating, and for one
part zkh_commit_data + zkh_prove_begin_held next to zkh_data_root + zkh_prove_begin, with the bytes held; M32: zkh_derive_links on three memory pairs as the PORTS of one memory (ZKA1 version 9) next to the version-6 blob of three separate
memories; M33: WIDE (ZKA1 version 10), zkh_derive_links_paged and zkh_page_out_tree on SYN-LOOKUP-paged-wide FULL (two value words per address)
next to SYN-LOOKUP-paged FULL on the same addresses and clocks, alternating; M34: FLAT (ZKA1 version 11), zkh_derive_links_paged on the
version-11 blob (flat-address columns) next to the version-10 blob on M33's addresses, and zkh_accumulate_open on SYN-LOOKUP-tied-wide next to
SYN-LOOKUP-tied, alternating; M31: paging in from a page
table, zkh_derive_links_paged_table next to zkh_derive_links_paged on the same SYN-LOOKUP-paged FULL trace at two image sizes, alternating,
with both calls' passes) on one MI355X, through the C ABI (HipHal).

Each line of output is one JSON object: the op, its shape, the average wall time of one call (stream drained on both
sides of `reps` back-to-back calls), its ALGORITHMIC bytes (SURVEY.md §8a "B_alg": inputs read once + outputs written
once) and what fraction of the 8.0 TB/s HBM3E peak (and of the 6.29 TB/s measured copy ceiling) that is.  The
Poseidon2 ops and the NTTs are integer-VALU-bound on gfx950, so they also carry `valu_frac`: modelled
issue cycles (DESIGN.md's per-permutation / per-butterfly counts, from tools/ubench_valu.hip) / (CUs*4 SIMDs*clock*t).

GPU only; inputs are random field elements generated on the host and uploaded before the clock starts.
    python tools/microbench.py [--po2 20] [--reps 5] [--only M3,M4]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zeth_amd.circuits import syn_air  # noqa: E402
from zeth_amd.circuits.desc import Circuit as Desc  # noqa: E402
from zeth_amd.hal import HipHal  # noqa: E402

P = 2013265921
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
SIMDS, CLOCK = 256 * 4, 2.4e9                 # 256 CUs x 4 SIMDs, peak engine clock
PERM_CYC = 8 * 1990 + 7 * 1259 + 711 + 480   # issue cycles of one wave64 over 64 Poseidon2 permutations
BFLY_CYC = 34                                 # mul_mod 18 + add_mod 8 + sub_mod 8


def rand_fp(rng, size):
    return rng.integers(0, P, size=size, dtype=np.uint64).astype(np.uint32)


def upload(hal, rng, name, words):
    """Random field elements, uploaded in 64M-word pieces (keeps the host staging small)."""
    buf = hal.alloc_elem(name, words)
    step = 1 << 26
    for off in range(0, words, step):
        buf.write(rand_fp(rng, min(step, words - off)), off)
    return buf


def timed(hal, fn, reps):
    fn()
    hal.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    hal.sync()
    return (time.perf_counter() - t0) / reps


def line(tag, op, shape, dt, alg_bytes, valu_cycles=None):
    rec = {"bench": tag, "op": op, "shape": shape, "ms": round(dt * 1e3, 4), "alg_GB": round(alg_bytes / 1e9, 4),
           "GB_per_s": round(alg_bytes / dt / 1e9, 1), "hbm_frac_8TBs": round(alg_bytes / dt / HBM_PEAK, 4),
           "hbm_frac_6.29TBs": round(alg_bytes / dt / HBM_COPY, 4)}
    if valu_cycles is not None:
        rec["valu_frac"] = round(valu_cycles / (SIMDS * CLOCK * dt), 4)
        rec["bound"] = "valu"
    else:
        rec["bound"] = "hbm"
    print(json.dumps(rec), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=208, help="columns of the group under test (SYN-A data group)")
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    want = lambda m: not only or m in only  # noqa: E731

    hal = HipHal(0)
    rng = np.random.default_rng(0xB0B)
    n, w = 1 << args.po2, args.width
    dom = 4 * n
    wave_perms = lambda perms: perms / 64 * PERM_CYC  # noqa: E731

    if want("M1") or want("M2"):
        io = upload(hal, rng, "m1", w * n)
        if want("M1"):
            dt = timed(hal, lambda: hal.batch_interpolate_ntt(io, w), args.reps)
            line("M1", "batch_interpolate_ntt", f"{w} x 2^{args.po2}", dt, 8 * w * n,
                 w * (n // 2) * args.po2 / 64 * BFLY_CYC)
            dt = timed(hal, lambda: hal.batch_interpolate_ntt_zk_shift(io, w), args.reps)
            line("M1b", "batch_interpolate_ntt+zk_shift (fused)", f"{w} x 2^{args.po2}", dt, 8 * w * n,
                 w * (n // 2) * args.po2 / 64 * BFLY_CYC)
        if want("M2"):
            ev = hal.alloc_elem("m2", w * dom)
            dt = timed(hal, lambda: hal.batch_expand_into_evaluate_ntt(ev, io, w, 2), args.reps)
            line("M2", "batch_expand_into_evaluate_ntt", f"{w} x 2^{args.po2} -> 2^{args.po2 + 2}", dt, 20 * w * n,
                 w * (dom // 2) * args.po2 / 64 * BFLY_CYC)
            del ev
        del io

    if want("M3") or want("M4"):
        nodes = hal.alloc_digest("nodes", 2 * dom)
        if want("M3"):
            mat = upload(hal, rng, "m3", w * dom)
            leaves = nodes.slice(8 * dom, 8 * dom)
            dt = timed(hal, lambda: hal.hash_rows(leaves, mat), args.reps)
            line("M3", "hash_rows", f"{w} cols x 2^{args.po2 + 2} rows", dt, 4 * w * dom + 32 * dom,
                 wave_perms(dom * -(-w // 16)))
            del mat, leaves
        if want("M4"):
            nodes.slice(8 * dom, 8 * dom).write(rand_fp(rng, 8 * dom))
            dt = timed(hal, lambda: hal.merkle_fold_all(nodes, dom), args.reps)
            line("M4", "hash_fold 2^%d -> 1 (merkle_fold_all)" % (args.po2 + 2), f"{dom} leaves", dt, 96 * dom,
                 wave_perms(dom - 1))
        del nodes

    if want("M5"):
        for m in (n, n >> 4, n >> 8):
            if m < 16:
                continue
            src = upload(hal, rng, "m5", 4 * m)
            dst = hal.alloc_elem("m5o", 4 * (m // 16))
            mix = rand_fp(rng, 4)
            dt = timed(hal, lambda: hal.fri_fold(dst, src, mix), args.reps)
            line("M5", "fri_fold", f"2^{m.bit_length() - 1} -> 2^{m.bit_length() - 5} ext", dt, 16 * m + m)
            del src, dst

    if want("M6") or want("M7"):
        coeffs = upload(hal, rng, "m6", w * n)
        if want("M6"):
            ncombo = 12
            # columns of one combo are adjacent, as a TapSet lays registers out (the accumulator is flushed on a change)
            combos = hal.copy_from("combos", (np.arange(w, dtype=np.uint32) * ncombo // w))
            out = hal.alloc_extelem("m6o", ncombo * n)
            ms, mx = rand_fp(rng, 4), rand_fp(rng, 4)
            dt = timed(hal, lambda: hal.mix_poly_coeffs(out, ms, mx, coeffs, combos, w, n), args.reps)
            line("M6", "mix_poly_coeffs", f"{w} x 2^{args.po2} -> {ncombo} combos", dt, 4 * w * n + 32 * ncombo * n)
            del out, combos
        if want("M7"):
            k = 256
            which = hal.copy_from("which", (np.arange(k, dtype=np.uint32) * 13) % w)
            xs = hal.copy_from("xs", rand_fp(rng, 4 * k))
            out = hal.alloc_extelem("m7o", k)
            dt = timed(hal, lambda: hal.batch_evaluate_any(coeffs, w, which, xs, out), args.reps)
            line("M7", "batch_evaluate_any", f"{k} taps over {w} x 2^{args.po2}", dt, 4 * k * n)
            del which, xs, out
            # a real tap set: every column at backs 0..4 (runs of 5 equal `which`): the column is streamed once per run
            k5 = 5 * w
            which = hal.copy_from("which", np.repeat(np.arange(w, dtype=np.uint32), 5))
            xs = hal.copy_from("xs", rand_fp(rng, 4 * k5))
            out = hal.alloc_extelem("m7o", k5)
            dt = timed(hal, lambda: hal.batch_evaluate_any(coeffs, w, which, xs, out), args.reps)
            line("M7t", "batch_evaluate_any, 5 taps per column", f"{k5} taps over {w} x 2^{args.po2}", dt, 4 * w * n)
            del which, xs, out
        del coeffs

    if want("M8"):
        desc = syn_air.syn_a()
        d = Desc.parse(desc)
        circ = hal.load_circuit(desc)
        groups = [upload(hal, rng, f"g{i}", gw * dom) for i, gw in enumerate(d.group_sizes)]
        globals_ = [hal.copy_from(f"gl{i}", rand_fp(rng, max(1, gs))) for i, gs in enumerate(d.global_sizes)]
        check = hal.alloc_elem("check", 4 * dom)
        mix = rand_fp(rng, 4)
        dt = timed(hal, lambda: circ.eval_check(check, groups, globals_, mix, args.po2), args.reps)
        line("M8", "eval_check (SYN-A, compiled kernel)" if circ.has_compiled_kernel() else "eval_check (interpreter)",
             f"{sum(d.group_sizes)} cols x 2^{args.po2 + 2} points", dt, 4 * sum(d.group_sizes) * dom + 16 * dom)
        dt = timed(hal, lambda: circ.eval_check(check, groups, globals_, mix, args.po2, use_interpreter=True), 1)
        line("M8i", "eval_check (SYN-A, step-list interpreter)", f"{sum(d.group_sizes)} cols x 2^{args.po2 + 2} points",
             dt, 4 * sum(d.group_sizes) * dom + 16 * dom)
        # the same evaluated groups under the heavy constraint system (same widths): VALU-bound generated kernels
        from zeth_amd.circuits import syn_heavy
        hdesc = syn_heavy.syn_heavy()
        hd = Desc.parse(hdesc)
        hcirc = hal.load_circuit(hdesc)
        dt = timed(hal, lambda: hcirc.eval_check(check, groups, globals_, mix, args.po2), args.reps)
        line("M8h", f"eval_check (SYN-HEAVY: {len(hd.steps)} steps, {len(hd.taps)} taps, {hcirc.compiled_parts()} generated kernels)",
             f"{sum(hd.group_sizes)} cols x 2^{args.po2 + 2} points", dt, 4 * sum(hd.group_sizes) * dom + 16 * dom)
        dt = timed(hal, lambda: hcirc.eval_check(check, groups, globals_, mix, args.po2, use_interpreter=True), 1)
        line("M8hi", "eval_check (SYN-HEAVY, step-list interpreter)", f"{sum(hd.group_sizes)} cols x 2^{args.po2 + 2} points",
             dt, 4 * sum(hd.group_sizes) * dom + 16 * dom)
    if want("M9"):
        # row f1: the trace-driven witness — host preflight (sequential, one core), then upload + row fill + scan + scatter on the GPU
        from zeth_amd import hal as H
        desc = syn_air.syn_a()
        d = Desc.parse(desc)
        circ = hal.load_circuit(desc)
        wa, wc, wd = d.group_sizes
        A = n - 1994
        pinned = hal.host_alloc(4 * A)
        t0 = time.perf_counter()
        _, ram, cpu_s = H.syn_preflight(0x5EED0000, args.po2, records=pinned)
        line("M9p", "syn_preflight (host, one core: the sequential producer)", f"2^{args.po2} cycles -> {16 * A / 1e6:.1f} MB of records",
             time.perf_counter() - t0, 16 * A)
        drec, data = hal.alloc("records", 4 * A), hal.alloc_elem("data", wd * n)

        def fill():
            hal.write_async(drec, pinned)
            hal.syn_witgen_trace(circ, args.po2, 1994, 0x2E80, drec, ram, None, data)
        dt = timed(hal, fill, args.reps)
        line("M9", "upload of the compact trace + k_syn_rowfill + running-sum scan + preload scatter", f"{wd} x 2^{args.po2} data group from 16-byte records",
             dt, 16 * A + 4 * wd * n)
        hal.sync()
        hal.host_free(pinned)
    if want("M10"):
        # the built-in accumulate (zkh_accumulate) of SYN-LOOKUP (67 terms in 23 accum columns), and the seal it is part of
        from zeth_amd.circuits import logup, syn_lookup
        from zeth_amd.prover import Segment, SegmentProver
        desc, blob = syn_lookup.syn_lookup()
        a = logup.Arguments.parse(blob)
        prover = SegmentProver(hal, desc, arguments=blob)
        code_h, data_h, out = syn_lookup.witness(syn_lookup.FULL, args.po2, 1994, seed=10)
        code, data = hal.alloc_elem("code", code_h.size), hal.alloc_elem("data", data_h.size)
        code.write(code_h)
        data.write(data_h)
        A = n - 1994
        seg = Segment(index=0, po2=args.po2, noise_seed=0x2E80)
        mix = rand_fp(rng, 8)
        accum = hal.alloc_elem("accum", 4 * a.k * n)
        acc = lambda: hal.accumulate(prover.circuit, args.po2, 1994, 0x2E80, code, data, mix, accum)
        dt_acc = timed(hal, acc, args.reps)
        cols = {c for t in a.terms for c in list(t.tuple_cols) + ([t.mult] if t.mult else []) + ([(1, t.sel)] if t.sel is not None else [])}
        line("M10", f"accumulate (SYN-LOOKUP: {len(a.terms)} terms in {a.k} accum columns)", f"{len(a.terms)} x {A} terms -> {4 * a.k} x 2^{args.po2}",
             dt_acc, 4 * len(cols) * A + 16 * a.k * n)
        seal = lambda: prover.seal_with_accum(seg, code, data, out, prover.args_accumulate(seg, code, data))
        dt_seal = timed(hal, seal, args.reps)
        line("M10s", "SYN-LOOKUP seal (prove_begin -> accumulate -> prove_finish, traces resident)", f"{sum(int(x) for x in desc[3:6])} cols x 2^{args.po2}",
             dt_seal, 4 * sum(int(x) for x in desc[3:6]) * n)
        print(json.dumps({"bench": "M10share", "accumulate_ms": round(dt_acc * 1e3, 3), "seal_ms": round(dt_seal * 1e3, 3),
                          "share": round(dt_acc / dt_seal, 4)}), flush=True)
    if want("M11"):
        # derived multiplicities (zkh_derive_multiplicities): SYN-LOOKUP-derived (64 byte-limb lookup columns into a 256-entry table, the
        # LDS count) and WIDE (M11w: a 2^16-entry table, the global count), against the host's bincount of the same limbs
        from zeth_amd.circuits import logup, syn_lookup
        from zeth_amd.prover import Segment, SegmentProver
        A = n - 1994
        for tag, shape in (("M11", syn_lookup.FULL), ("M11w", syn_lookup.WIDE)):
            desc, blob = syn_lookup.build_syn_lookup(shape, derive=True)
            a = logup.Arguments.parse(blob)
            circuit = hal.load_circuit(desc, jit=False)
            circuit.set_arguments(blob)
            code_h, data_h, _ = syn_lookup.witness(shape, args.po2, 1994, seed=11, count=False)
            code, data = hal.alloc_elem("code", code_h.size), hal.alloc_elem("data", data_h.size)
            code.write(code_h)
            data.write(data_h)
            dt = timed(hal, lambda: hal.derive_multiplicities(circuit, args.po2, 1994, code, data), args.reps)
            _words, limbs, _m, _mem, _perm = syn_lookup.layout(shape.n_words, shape.n_limbs, shape.n_mem)
            lk = [c for row in limbs for c in row]
            T = 1 << shape.limb_bits
            host = data_h.reshape(-1, n)
            vals = [logup._dec(host[c, :A]).astype(np.int64) for c in lk]
            t0 = time.perf_counter()
            counts = np.zeros(T, np.int64)
            for v in vals:
                counts += np.bincount(v, minlength=T)
            dt_host = time.perf_counter() - t0
            # lookup columns and the table's selector + values once, the m column written once
            line(tag, f"derive multiplicities ({len(lk)} lookup columns into a {T}-entry table)", f"{len(lk)} x {A} lookups -> 2^{args.po2}",
                 dt, 4 * len(lk) * A + 3 * 4 * A)
            rec = {"bench": tag + "host", "host_bincount_ms": round(dt_host * 1e3, 3), "device_ms": round(dt * 1e3, 4)}
            if tag == "M11":
                prover = SegmentProver(hal, desc, arguments=blob)
                seg = Segment(index=0, po2=args.po2, noise_seed=0x2E80)
                out = np.zeros(4, np.uint32)
                seal = lambda: prover.seal_with_accum(seg, code, data, out, prover.args_accumulate(seg, code, data))
                dt_seal = timed(hal, seal, args.reps)
                rec.update(seal_ms=round(dt_seal * 1e3, 3), share=round(dt / dt_seal, 4))
            print(json.dumps(rec), flush=True)
    if want("M12"):
        # derived sorted copies (zkh_derive_sorted) of SYN-LOOKUP-sorted: the (addr, val, time) tuple sorted by (addr, time) on the device,
        # per step (ProfScope events) and in total, next to the seal it precedes and to what it replaces on the host: np.lexsort over the
        # decoded keys, the gather of the three columns and their upload
        from zeth_amd.circuits import logup, syn_lookup
        from zeth_amd.prover import Segment, SegmentProver
        A = n - 1994
        shape = syn_lookup.FULL
        desc, blob = syn_lookup.build_syn_lookup(shape, sort=True)
        circuit = hal.load_circuit(desc, jit=False)
        circuit.set_arguments(blob)
        code_h, data_h, _ = syn_lookup.witness(shape, args.po2, 1994, seed=12, sort=False)
        code, data = hal.alloc_elem("code", code_h.size), hal.alloc_elem("data", data_h.size)
        code.write(code_h)
        data.write(data_h)
        derive = lambda: hal.derive_sorted(circuit, args.po2, 1994, code, data)
        dt = timed(hal, derive, args.reps)
        # key columns read twice (live bits, pack), 12 B of (key, row) per item, the three columns gathered and written
        line("M12", "derive sorted copies (SYN-LOOKUP-sorted: (addr, val, time) by (addr, time))", f"{shape.n_mem} x {A} rows -> 2^{args.po2}",
             dt, shape.n_mem * A * (4 * 2 * 2 + 12 + 4 * 2 * 3))
        hal.prof_enable(True)
        hal.prof_reset()
        for _ in range(args.reps):
            derive()
        hal.sync()
        steps = {r["name"]: round(r["total_ms"] / max(r["calls"], 1), 4) for r in hal.prof_get() if r["calls"] and r["name"].startswith("sort_")}
        hal.prof_enable(False)
        _words, _limbs, _m, mem, perm = syn_lookup.layout(shape.n_words, shape.n_limbs, shape.n_mem)
        host = data_h.reshape(-1, n)
        t0 = time.perf_counter()
        addr, tm = logup._dec(host[mem[0][0], :A]), logup._dec(host[mem[0][2], :A])
        order = np.lexsort((tm, addr))
        cols = np.ascontiguousarray(host[mem[0], :A][:, order])
        dt_sort = time.perf_counter() - t0
        up = hal.alloc_elem("perm", cols.size)
        dt_up = timed(hal, lambda: up.write(cols.reshape(-1)), args.reps)
        prover = SegmentProver(hal, desc, arguments=blob)
        seg = Segment(index=0, po2=args.po2, noise_seed=0x2E80)
        out = np.zeros(4, np.uint32)
        seal = lambda: prover.seal_with_accum(seg, code, data, out, prover.args_accumulate(seg, code, data))
        dt_seal = timed(hal, seal, args.reps)
        print(json.dumps({"bench": "M12share", "derive_sorted_ms": round(dt * 1e3, 4), "steps_ms": steps, "seal_ms": round(dt_seal * 1e3, 3),
                          "share": round(dt / dt_seal, 4), "host_lexsort_ms": round(dt_sort * 1e3, 2), "host_upload_ms": round(dt_up * 1e3, 3)}),
              flush=True)
    if want("M13"):
        # (a) derived columns (zkh_derive_columns) of SYN-LOOKUP FULL with limbs=True: 16 LIMBS records, 16 word columns read in the check
        # pass and again in the write pass, 64 limb columns written, next to zkh_eltwise_copy_elem moving the same bytes in the same run;
        # (b) the host-witness seal (SegmentProver.seal_host_witness from pinned memory; sort + multiplicities + limbs derived): bytes
        # uploaded and wall-clock per seal
        from zeth_amd.circuits import syn_lookup
        from zeth_amd.prover import Segment, SegmentProver
        zk = 1994
        A = n - zk
        shape = syn_lookup.FULL
        desc, blob = syn_lookup.build_syn_lookup(shape, limbs=True, sort=True, derive=True)
        circuit = hal.load_circuit(desc, jit=False)
        circuit.set_arguments(blob)
        code_h, data_h, out = syn_lookup.witness(shape, args.po2, zk, seed=13, sort=False, count=False, limbs=False)
        code, data = hal.alloc_elem("code", code_h.size), hal.alloc_elem("data", data_h.size)
        code.write(code_h)
        data.write(data_h)
        alg = 4 * A * shape.n_words * (2 + shape.n_limbs)
        derive = lambda: hal.derive_columns(circuit, args.po2, zk, code, data)
        dt = timed(hal, derive, args.reps)
        line("M13", "derive columns (SYN-LOOKUP FULL: 16 words -> 64 limbs; check + write pass)", f"{shape.n_words} records x {A} rows -> 2^{args.po2}", dt, alg)
        hal.prof_enable(True)
        hal.prof_reset()
        for _ in range(args.reps):
            derive()
        hal.sync()
        steps = {r["name"]: round(r["total_ms"] / max(r["calls"], 1), 4) for r in hal.prof_get() if r["calls"] and r["name"].startswith("columns_")}
        hal.prof_enable(False)
        src, dst = upload(hal, rng, "m13src", alg // 8), hal.alloc_elem("m13dst", alg // 8)
        dt_copy = timed(hal, lambda: hal.eltwise_copy_elem(dst, src), args.reps)
        line("M13copy", "eltwise_copy_elem of the same bytes (the streaming yardstick)", f"{alg // 8} words", dt_copy, alg)
        del src, dst
        prover = SegmentProver(hal, desc, arguments=blob)
        seg = Segment(index=0, po2=args.po2, noise_seed=0x2E80)
        hcode, hdata = hal.host_alloc(code_h.size), hal.host_alloc(data_h.size)
        hcode[:] = code_h
        hdata[:] = data_h
        before = hal.h2d_bytes()
        prover.seal_host_witness(seg, hcode, hdata, out)
        hal.sync()
        crossed = hal.h2d_bytes() - before
        dt_seal = timed(hal, lambda: prover.seal_host_witness(seg, hcode, hdata, out), args.reps)
        hal.host_free(hcode)
        hal.host_free(hdata)
        print(json.dumps({"bench": "M13seal", "derive_columns_ms": round(dt * 1e3, 4), "steps_ms": steps, "copy_ms": round(dt_copy * 1e3, 4),
                          "vs_copy": round(dt_copy / dt, 3), "host_witness_seal_ms": round(dt_seal * 1e3, 3), "h2d_bytes_per_seal": crossed,
                          "full_trace_bytes": 4 * (code_h.size + data_h.size), "derived_columns": len(circuit.derived_data_columns())}), flush=True)
    if want("M14"):
        # linked accesses (zkh_derive_links) of SYN-LOOKUP-linked FULL: the accesses sorted by address, then the check and the write pass
        # (7 destination columns), per step and in total, next to zkh_eltwise_copy_elem moving the same bytes and to the host's way:
        # reference_links' stable sort + gather over the decoded columns and the upload of the 7 columns; then the host-witness seal with
        # the derive against the same tree uploading the host-made columns (the flag-free blob)
        from zeth_amd.circuits import logup, syn_lookup
        from zeth_amd.prover import Segment, SegmentProver
        zk = 1994
        A = n - zk
        shape = syn_lookup.FULL
        desc, blob = syn_lookup.build_syn_lookup(shape, link=True)
        largs = logup.Arguments.parse(blob)
        circuit = hal.load_circuit(desc, jit=False)
        circuit.set_arguments(blob)
        code_h, full_h, out = syn_lookup.witness(shape, args.po2, zk, seed=14, link=True)
        bare_h = full_h.reshape(-1, n).copy()
        bare_h[circuit.derived_data_columns(), :A] = 0
        bare_h = bare_h.reshape(-1)
        code, data = hal.alloc_elem("code", code_h.size), hal.alloc_elem("data", bare_h.size)
        code.write(code_h)
        data.write(bare_h)
        derive = lambda: hal.derive_links(circuit, args.po2, zk, code, data)
        dt = timed(hal, derive, args.reps)
        assert np.array_equal(data.to_vec(), full_h)
        # the key read twice (live bits, pack) and 12 B of (key, row) per item and pass; per pass of k_links (key, row) 12 B, the clock at two
        # rows; the write pass also reads the carried value and writes 7 columns
        passes = 3
        alg = A * (4 * 2 + 12 + passes * 3 * 12 + 2 * (12 + 8) + 4 + 4 * 7)
        line("M14", "derive links (SYN-LOOKUP-linked: prev access by address; sort + check + write pass)", f"{A} accesses -> 2^{args.po2}", dt, alg)
        hal.prof_enable(True)
        hal.prof_reset()
        for _ in range(args.reps):
            derive()
        hal.sync()
        steps = {r["name"]: round(r["total_ms"] / max(r["calls"], 1), 4) for r in hal.prof_get()
                 if r["calls"] and r["name"].startswith(("sort_", "links_"))}
        hal.prof_enable(False)
        src, dst = upload(hal, rng, "m14src", alg // 8), hal.alloc_elem("m14dst", alg // 8)
        dt_copy = timed(hal, lambda: hal.eltwise_copy_elem(dst, src), args.reps)
        line("M14copy", "eltwise_copy_elem of the same bytes (the streaming yardstick)", f"{alg // 8} words", dt_copy, alg)
        del src, dst
        t0 = time.perf_counter()
        want_h = logup.reference_links(largs, args.po2, zk, code_h, bare_h)
        dt_host = time.perf_counter() - t0
        assert np.array_equal(want_h, full_h)
        cols = np.ascontiguousarray(want_h.reshape(-1, n)[circuit.derived_data_columns(), :A])
        up = hal.alloc_elem("links", cols.size)
        dt_up = timed(hal, lambda: up.write(cols.reshape(-1)), args.reps)
        seg = Segment(index=0, po2=args.po2, noise_seed=0x2E80)
        seals = {}
        for name, b, host in (("derive", blob, bare_h), ("host_made", largs.plain().blob(), full_h)):
            prover = SegmentProver(hal, desc, arguments=b)
            hcode, hdata = hal.host_alloc(code_h.size), hal.host_alloc(host.size)
            hcode[:] = code_h
            hdata[:] = host
            before = hal.h2d_bytes()
            prover.seal_host_witness(seg, hcode, hdata, out)
            hal.sync()
            crossed = hal.h2d_bytes() - before
            dt_seal = timed(hal, lambda: prover.seal_host_witness(seg, hcode, hdata, out), args.reps)
            hal.host_free(hcode)
            hal.host_free(hdata)
            seals[name] = {"seal_ms": round(dt_seal * 1e3, 3), "h2d_bytes_per_seal": crossed}
        sort_ms = sum(v for k, v in steps.items() if k.startswith("sort_"))
        print(json.dumps({"bench": "M14links", "derive_links_ms": round(dt * 1e3, 4), "steps_ms": steps, "sort_share": round(sort_ms / max(sum(steps.values()), 1e-9), 3),
                          "copy_ms": round(dt_copy * 1e3, 4), "vs_copy": round(dt_copy / dt, 3), "host_reference_links_ms": round(dt_host * 1e3, 2),
                          "host_upload_ms": round(dt_up * 1e3, 3), "host_witness_seal": seals}), flush=True)
    if want("M14r"):
        # the read rule (zkh_derive_links on SYN-LOOKUP-reads FULL, a ZKA1 version-6 blob) next to the same trace under the version-5 blob
        # of the same arguments (the LINK record without READS): the rule adds a flag read and up to two value reads per access to the
        # check pass, and nothing else; the check pass's share by its events
        from dataclasses import replace
        from zeth_amd.circuits import logup, syn_lookup
        zk = 1994
        A = n - zk
        shape = syn_lookup.FULL
        desc, blob = syn_lookup.build_syn_lookup(shape, link=True, reads=True)
        rargs = logup.Arguments.parse(blob)
        blob5 = logup.Arguments(rargs.k, rargs.alpha, rargs.beta, rargs.terms, [replace(r, write=None) for r in rargs.records]).blob()
        assert int(blob[1]) == 6 and int(blob5[1]) == 5
        code_h, full_h, _out = syn_lookup.witness(shape, args.po2, zk, seed=14, link=True, reads=True)
        res = {}
        for name, b in (("v6_reads", blob), ("v5", blob5)):
            circuit = hal.load_circuit(desc, jit=False)
            circuit.set_arguments(b)
            assert circuit.links_check_reads() == (1 if name == "v6_reads" else 0)
            bare_h = full_h.reshape(-1, n).copy()
            bare_h[circuit.derived_data_columns(), :A] = 0
            code, data = hal.alloc_elem("code", code_h.size), hal.alloc_elem("data", bare_h.size)
            code.write(code_h)
            data.write(bare_h.reshape(-1))
            derive = lambda: hal.derive_links(circuit, args.po2, zk, code, data)
            dt = timed(hal, derive, args.reps)
            assert np.array_equal(data.to_vec(), full_h)
            hal.prof_enable(True)
            hal.prof_reset()
            for _ in range(args.reps):
                derive()
            hal.sync()
            steps = {r["name"]: round(r["total_ms"] / max(r["calls"], 1), 4) for r in hal.prof_get()
                     if r["calls"] and r["name"].startswith(("sort_", "links_"))}
            hal.prof_enable(False)
            res[name] = {"derive_links_ms": round(dt * 1e3, 4), "steps_ms": steps,
                         "check_share": round(steps.get("links_check", 0) / max(sum(steps.values()), 1e-9), 3)}
            del code, data
        print(json.dumps({"bench": "M14reads", **res, "reads_vs_v5": round(res["v6_reads"]["derive_links_ms"] / res["v5"]["derive_links_ms"], 3),
                          "check_vs_v5": round(res["v6_reads"]["steps_ms"].get("links_check", 0) / max(res["v5"]["steps_ms"].get("links_check", 0), 1e-9), 3)}),
              flush=True)
    if want("M15"):
        # the row-by-row constraint check (zkh_check_rows: the interpreter's program on the n rows of the trace domain, no mix arithmetic)
        # of an honest witness of the built-in generator, next to its yardstick in the same run: zkh_eval_check on the step interpreter
        # (use_interpreter = 1), the same program over the 4n points of the evaluation domain with Fp4 mix arithmetic.  The two are
        # timed in alternation, `runs` windows of `reps` calls each; median and spread (min, max) of the windows.  check_rows is a
        # whole call: its globals' upload, the pass, the read-back of the result.
        from zeth_amd.circuits import syn_heavy
        from zeth_amd.prover import Segment, SegmentProver
        runs = 7
        # (SYN-HUGE only when asked for: --only M15,M15huge)
        circuits = [("SYN-A", syn_air.syn_a()), ("SYN-HEAVY", syn_heavy.syn_heavy())] + ([("SYN-HUGE", syn_heavy.syn_huge())] if "M15huge" in only else [])
        for name, desc in circuits:
            d = Desc.parse(desc)
            prover = SegmentProver(hal, desc)
            seg = Segment(index=0, po2=args.po2, noise_seed=0x2E80)
            code, data, out = prover.witgen(seg)
            mix = rand_fp(rng, d.global_sizes[1])
            accum = prover.syn_accumulate(seg, data)(mix)
            found = hal.check_rows(prover.circuit, args.po2, accum, code, data, out, mix)
            assert found["row"] == -1, found                     # an honest witness: the pass alone, no second launch
            groups = [upload(hal, rng, "m15g", wg * dom) for wg in d.group_sizes]
            globals_ = [hal.copy_from("m15o", out), hal.copy_from("m15m", mix)]
            check = hal.alloc_elem("m15c", 4 * dom)
            poly_mix = rand_fp(rng, 4)
            rows_fn = lambda: hal.check_rows(prover.circuit, args.po2, accum, code, data, out, mix)      # noqa: E731
            eval_fn = lambda: prover.circuit.eval_check(check, groups, globals_, poly_mix, args.po2, use_interpreter=True)   # noqa: E731
            t_rows, t_eval = [], []
            for _ in range(runs):
                t_rows.append(timed(hal, rows_fn, args.reps))
                t_eval.append(timed(hal, eval_fn, args.reps))
            spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
            total_w = sum(d.group_sizes)
            print(json.dumps({"bench": "M15", "circuit": name, "po2": args.po2, "steps": len(d.steps), "columns": total_w, "runs": runs, "reps": args.reps,
                              "check_rows": spread(t_rows), "eval_check_interp": spread(t_eval),
                              "check_rows_trace_GB": round(4 * total_w * n / 1e9, 4), "eval_check_domain_GB": round(4 * total_w * dom / 1e9, 4),
                              "check_rows_vs_eval_check_interp": round(float(np.median(t_rows)) / float(np.median(t_eval)), 4)}), flush=True)
            del groups, globals_, check, accum, code, data, prover
    if want("M16"):
        # the key-by-key bus check (zkh_check_bus) of the honest SYN-LOOKUP FULL witness under its derived blob, next to its yardsticks on
        # the same trace in the same run: zkh_accumulate (the call whose refusal it explains) and zkh_derive_multiplicities (the other
        # keyed table over the trace).  The per-term pass runs only on an unbalanced bus: it is forced by a second data trace in which
        # one table multiplicity is raised by one (one cell: the build and the scan cost what they cost on the honest trace).  The four
        # are timed in alternation, `runs` windows of `reps` calls each; median and spread (min, max) of the windows.  check_bus is a
        # whole call: its terms' upload, the table's clearing, build, scan and the read-backs.
        from zeth_amd.circuits import logup, syn_lookup
        runs, zk = 7, 1994
        A = n - zk
        shape = syn_lookup.FULL
        desc, blob = syn_lookup.build_syn_lookup(shape, derive=True)
        a = logup.Arguments.parse(blob)
        circuit = hal.load_circuit(desc, jit=False)
        circuit.set_arguments(blob)
        code_h, data_h, _out = syn_lookup.witness(shape, args.po2, zk, seed=16)
        m_col = syn_lookup.layout(shape.n_words, shape.n_limbs, shape.n_mem)[2]
        forged_h = data_h.copy()
        forged_h[m_col * n + 7] = (int(forged_h[m_col * n + 7]) + (1 << 32) % P) % P
        code, data, forged = (hal.alloc_elem(nm, h.size) for nm, h in (("code", code_h), ("data", data_h), ("forged", forged_h)))
        for b, h in ((code, code_h), (data, data_h), (forged, forged_h)):
            b.write(h)
        mix = rand_fp(rng, 8)
        accum = hal.alloc_elem("accum", 4 * a.k * n)
        bus_fn = lambda: hal.check_bus(circuit, args.po2, zk, code, data)                                   # noqa: E731
        per_fn = lambda: hal.check_bus(circuit, args.po2, zk, code, forged, per_term=True)                  # noqa: E731
        acc_fn = lambda: hal.accumulate(circuit, args.po2, zk, 0x2E80, code, data, mix, accum)              # noqa: E731
        der_fn = lambda: hal.derive_multiplicities(circuit, args.po2, zk, code, data)                       # noqa: E731  (rewrites what is there)
        found, named = bus_fn(), per_fn()
        assert found["row"] == -1 and found["unbalanced_keys"] == 0, found
        assert named["unbalanced_keys"] == 1 and named["key"] == (7, 0, 0, 0) and named["net"] == P - 1, named
        start = logup.bus_slots(A, 0)
        t = {"check_bus": [], "check_bus_per_term": [], "accumulate": [], "derive_multiplicities": []}
        for _ in range(runs):
            for name, fn in (("check_bus", bus_fn), ("accumulate", acc_fn), ("check_bus_per_term", per_fn), ("derive_multiplicities", der_fn)):
                t[name].append(timed(hal, fn, args.reps))
        assert np.array_equal(data.to_vec(), data_h)
        hal.prof_enable(True)
        hal.prof_reset()
        for _ in range(args.reps):
            per_fn()
        hal.sync()
        steps = {r["name"]: round(r["total_ms"] / max(r["calls"], 1), 4) for r in hal.prof_get() if r["calls"] and r["name"].startswith("bus_")}
        hal.prof_enable(False)
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps({"bench": "M16", "circuit": "SYN-LOOKUP FULL (derived blob)", "library": os.path.basename(os.environ.get("ZKH_LIBRARY", "") or "libzkhal_mi355x.so"),
                          "po2": args.po2, "terms": len(a.terms), "entries": len(a.terms) * A - (A - (1 << shape.limb_bits)),
                          "runs": runs, "reps": args.reps, **{k: spread(v) for k, v in t.items()}, "kernels_ms_per_term_call": steps,
                          "distinct_keys": found["distinct_keys"], "slots": found["slots"], "start_slots": start,
                          "growths": int(np.log2(found["slots"] // start)), "table_bytes": 24 * found["slots"],
                          "check_bus_vs_accumulate": round(med["check_bus"] / med["accumulate"], 3),
                          "check_bus_vs_derive_multiplicities": round(med["check_bus"] / med["derive_multiplicities"], 3),
                          "per_term_vs_check_bus": round(med["check_bus_per_term"] / med["check_bus"], 3)}), flush=True)
        del code, data, forged, accum
    if want("M17"):
        # paging (zkh_derive_links_paged on SYN-LOOKUP-paged FULL, a ZKA1 version-7 blob) next to its yardstick in the same run:
        # zkh_derive_links under the version-6 blob of the same arguments (the PAGES record dropped) on the same trace, code this path
        # does not share beyond the sort.  The image is all zeros, so that the trace's first loads return 0 and the version-6 read rule
        # accepts them too.  zkh_page_out next to zkh_eltwise_copy_elem over the bytes it moves (p_on, p_addr and p_out read, one word
        # per page written).  Timed in alternation, `runs` windows of `reps` calls; median and spread (min, max) of the windows; then
        # the passes by their events.
        from zeth_amd.circuits import logup, syn_lookup
        runs, zk = 7, 1994
        A = n - zk
        shape = syn_lookup.FULL
        desc, blob = syn_lookup.build_syn_lookup(shape, link=True, reads=True, pages=True)
        pargs = logup.Arguments.parse(blob)
        blob6 = logup.Arguments(pargs.k, pargs.alpha, pargs.beta, pargs.terms, [r for r in pargs.records if not isinstance(r, logup.Pages)]).blob()
        assert int(blob[1]) == 7 and int(blob6[1]) == 6
        W = 1 << 20
        image_h = np.zeros(W, dtype=np.uint32)
        code_h, full_h, _out = syn_lookup.witness(shape, args.po2, zk, seed=17, link=True, reads=True, pages=True, image=image_h)
        paged, plain = hal.load_circuit(desc, jit=False), hal.load_circuit(desc, jit=False)
        paged.set_arguments(blob)
        plain.set_arguments(blob6)
        assert paged.pages() and not plain.pages()
        bare_h = full_h.reshape(-1, n).copy()
        bare_h[paged.derived_data_columns(), :A] = 0
        code, data, data6, image = (hal.alloc_elem(nm, sz) for nm, sz in (("code", code_h.size), ("data", bare_h.size), ("data6", bare_h.size), ("image", W)))
        code.write(code_h)
        data.write(bare_h.reshape(-1))
        data6.write(bare_h.reshape(-1))
        image.write(image_h)
        paged_fn = lambda: hal.derive_links_paged(paged, args.po2, zk, code, data, image)                   # noqa: E731
        plain_fn = lambda: hal.derive_links(plain, args.po2, zk, code, data6)                               # noqa: E731
        out_fn = lambda: hal.page_out(paged, args.po2, zk, data, image)                                     # noqa: E731  (after the first call it rewrites what is there)
        pages = int((full_h.reshape(-1, n)[pargs.pages.p_on, :A] != 0).sum())
        moved = 3 * A + pages                                                # words: three table columns read, one image word per page written
        src, dst = upload(hal, rng, "m17s", moved // 2), hal.alloc_elem("m17d", moved // 2)
        copy_fn = lambda: hal.eltwise_copy_elem(dst, src)                                                   # noqa: E731
        paged_fn()
        assert np.array_equal(data.to_vec(), full_h)
        out_fn()
        assert np.array_equal(image.to_vec(), logup.reference_page_out(pargs, args.po2, zk, full_h, image_h))
        image.write(image_h)
        t = {"derive_links_paged": [], "derive_links_v6": [], "page_out": [], "copy_same_bytes": []}
        for _ in range(runs):
            for name, fn in (("derive_links_paged", paged_fn), ("derive_links_v6", plain_fn), ("page_out", out_fn), ("copy_same_bytes", copy_fn)):
                t[name].append(timed(hal, fn, args.reps))
                if name == "page_out":                                       # the next window's derive starts from the first image again
                    image.write(image_h)
        steps = {}
        for name, fn in (("paged", paged_fn), ("v6", plain_fn), ("page_out", out_fn)):
            hal.prof_enable(True)
            hal.prof_reset()
            for _ in range(args.reps):
                fn()
            hal.sync()
            steps[name] = {r["name"]: round(r["total_ms"] / max(r["calls"], 1), 4) for r in hal.prof_get()
                           if r["calls"] and r["name"].startswith(("sort_", "links_", "pages_", "page_out_"))}
            hal.prof_enable(False)
            image.write(image_h)
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps({"bench": "M17", "circuit": "SYN-LOOKUP-paged FULL", "po2": args.po2, "accesses": A, "pages": pages, "image_words": W, "runs": runs,
                          "reps": args.reps, **{k: spread(v) for k, v in t.items()}, "steps_ms": steps, "page_out_words": moved,
                          "paged_vs_v6": round(med["derive_links_paged"] / med["derive_links_v6"], 3),
                          "page_out_vs_copy": round(med["page_out"] / med["copy_same_bytes"], 3)}), flush=True)
        del code, data, data6, image, src, dst
    if want("M18"):
        # the committed image: zkh_page_out_tree (page-out + the incremental update of the tree: only the paths of the paged words are
        # hashed again) next to its yardstick in the same run, zkh_page_out followed by zkh_image_commit (the rebuild with the fold
        # kernels the library already had), each into its own image and nodes.  SYN-LOOKUP-paged FULL at M17's image size (2^20 words)
        # and at 2^26 words.  Tables: `derive`, the page table that zkh_derive_links_paged leaves (its addresses lie below 2^20 at
        # either image size); `spread`, a hand-made table of as many pages at random addresses over the whole image (zkh_page_out
        # reads p_on, p_addr and p_out alone); `sparse`, a hand-made one of 4096 pages.  Timed in alternation, `runs` windows of `reps`
        # calls; median and spread (min, max) of the windows; then the stages by their events.  After the first call a page-out
        # rewrites what is there and the update hashes the same paths again: every call does the same work.
        from zeth_amd.circuits import logup, syn_lookup
        runs, zk = 7, 1994
        A = n - zk
        shape = syn_lookup.FULL
        desc, blob = syn_lookup.build_syn_lookup(shape, link=True, reads=True, pages=True)
        pargs = logup.Arguments.parse(blob)
        pg = pargs.pages
        code_h, full_h, _out = syn_lookup.witness(shape, args.po2, zk, seed=17, link=True, reads=True, pages=True, image=np.zeros(1 << 20, dtype=np.uint32))
        paged = hal.load_circuit(desc, jit=False)
        paged.set_arguments(blob)
        full = full_h.reshape(-1, n)
        pages = int((full[pg.p_on, :A] != 0).sum())
        one = np.uint32((1 << 32) % P)
        enc = lambda x: (np.asarray(x, dtype=np.uint64) * np.uint64(one) % np.uint64(P)).astype(np.uint32)   # noqa: E731
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        data = hal.alloc_elem("m18d", full_h.size)
        for W in (1 << 20, 1 << 26):
            for table in ("derive", "spread", "sparse"):
                if table == "derive":
                    D = pages
                    data.write(full_h)
                else:
                    D = pages if table == "spread" else 4096
                    hand = np.zeros_like(full)
                    hand[pg.p_on, :D], hand[pg.p_out, :D] = one, rand_fp(rng, D)
                    if W <= 1 << 22:
                        addrs = rng.choice(W, D, replace=False)
                    else:                                                    # (no permutation of 2^26 words: distinct draws, D of them at random)
                        addrs = np.unique(rng.integers(0, W, D + D // 8))
                        addrs = addrs[rng.choice(addrs.size, D, replace=False)]
                    hand[pg.p_addr, :D] = enc(np.sort(addrs))
                    data.write(hand.reshape(-1))
                    del hand
                image_h = rand_fp(rng, W)
                images = [hal.alloc_elem("m18i", W) for _ in range(2)]
                for im in images:
                    im.write(image_h)
                nodes = [hal.image_commit(im) for im in images]
                tree_fn = lambda: hal.page_out_tree(paged, args.po2, zk, data, images[0], nodes[0])            # noqa: E731
                yard_fn = lambda: (hal.page_out(paged, args.po2, zk, data, images[1]), hal.image_commit(images[1], nodes[1]))   # noqa: E731
                tree_fn()
                yard_fn()
                assert np.array_equal(images[0].to_vec(), images[1].to_vec()) and not np.array_equal(images[0].to_vec(), image_h)
                assert np.array_equal(nodes[0].to_vec(), nodes[1].to_vec())
                t = {"page_out_tree": [], "page_out_then_commit": []}
                for _ in range(runs):
                    for name, fn in (("page_out_tree", tree_fn), ("page_out_then_commit", yard_fn)):
                        t[name].append(timed(hal, fn, args.reps))
                steps = {}
                for name, fn in (("page_out_tree", tree_fn), ("page_out_then_commit", yard_fn)):
                    hal.prof_enable(True)
                    hal.prof_reset()
                    for _ in range(args.reps):
                        fn()
                    hal.sync()
                    steps[name] = {r["name"]: {"calls_per_call": r["calls"] // args.reps, "ms_per_call": round(r["total_ms"] / args.reps, 4)} for r in hal.prof_get()
                                   if r["calls"] and r["name"].startswith(("page_out_", "image_", "hash_fold"))}
                    hal.prof_enable(False)
                assert np.array_equal(nodes[0].to_vec(), nodes[1].to_vec())
                med = {k: float(np.median(v)) for k, v in t.items()}
                print(json.dumps({"bench": "M18", "circuit": "SYN-LOOKUP-paged FULL", "library": os.path.basename(os.environ.get("ZKH_LIBRARY", "") or "libzkhal_mi355x.so"),
                                  "po2": args.po2, "table": table, "pages": D, "image_words": W, "leaves": logup.image_tree_leaves(W), "runs": runs,
                                  "reps": args.reps, **{k: spread(v) for k, v in t.items()}, "steps": steps,
                                  "tree_vs_rebuild": round(med["page_out_tree"] / med["page_out_then_commit"], 3)}), flush=True)
                del images, nodes
        del data
    if want("M19"):
        # the update's proof: zkh_page_out_proof (the ZKU1 proof of a page-out, built from the tree as it is: the table, the old leaves,
        # the clean siblings of every layer; it hashes nothing) next to its yardstick in the same run, zkh_page_out_tree (the page-out
        # and the incremental update: unchanged code), each on its own image and nodes.  M18's setup: SYN-LOOKUP-paged FULL, the tables
        # `derive`, `spread` and `sparse`, 2^20 and 2^26 image words; p_in is set to the image's word, which the proof's check pass
        # demands.  The proof's call goes through the C ABI directly: HipHal.page_out_proof would read the proof back.  Timed in
        # alternation, `runs` windows of `reps` calls; median and spread (min, max) of the windows; then the stages by their events.
        # The sparse table's proof is walked on the host (zkh_image_proof_verify) to the root the update leaves.
        from zeth_amd import hal as zhal
        from zeth_amd.circuits import logup, syn_lookup
        runs, zk = 7, 1994
        A = n - zk
        shape = syn_lookup.FULL
        desc, blob = syn_lookup.build_syn_lookup(shape, link=True, reads=True, pages=True)
        pargs = logup.Arguments.parse(blob)
        pg = pargs.pages
        code_h, full_h, _out = syn_lookup.witness(shape, args.po2, zk, seed=17, link=True, reads=True, pages=True, image=np.zeros(1 << 20, dtype=np.uint32))
        paged = hal.load_circuit(desc, jit=False)
        paged.set_arguments(blob)
        full = full_h.reshape(-1, n)
        pages = int((full[pg.p_on, :A] != 0).sum())
        one = np.uint32((1 << 32) % P)
        rinv = pow(int(one), -1, P)
        enc = lambda x: (np.asarray(x, dtype=np.uint64) * np.uint64(one) % np.uint64(P)).astype(np.uint32)   # noqa: E731
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        data = hal.alloc_elem("m19d", full_h.size)
        for W in (1 << 20, 1 << 26):
            for table in ("derive", "spread", "sparse"):
                image_h = rand_fp(rng, W)
                hand = full.copy() if table == "derive" else np.zeros_like(full)
                if table == "derive":
                    D = pages
                    addrs = (hand[pg.p_addr, :D].astype(np.uint64) * np.uint64(rinv) % np.uint64(P)).astype(np.int64)
                else:
                    D = pages if table == "spread" else 4096
                    hand[pg.p_on, :D], hand[pg.p_out, :D] = one, rand_fp(rng, D)
                    if W <= 1 << 22:
                        addrs = rng.choice(W, D, replace=False)
                    else:                                                    # (no permutation of 2^26 words: distinct draws, D of them at random)
                        addrs = np.unique(rng.integers(0, W, D + D // 8))
                        addrs = addrs[rng.choice(addrs.size, D, replace=False)]
                    addrs = np.sort(addrs).astype(np.int64)
                    hand[pg.p_addr, :D] = enc(addrs)
                hand[pg.p_in, :D] = image_h[addrs]
                data.write(hand.reshape(-1))
                del hand
                images = [hal.alloc_elem("m19i", W) for _ in range(2)]
                for im in images:
                    im.write(image_h)
                nodes = [hal.image_commit(im) for im in images]
                root0 = hal.image_root(nodes[0])
                buf = hal.alloc("m19p", hal.image_proof_words(W, A))
                proof_fn = lambda: zhal._check(zhal._lib.zkh_page_out_proof(hal.ctx, paged.h, args.po2, zk, data.h, images[0].h, nodes[0].h, buf.h))   # noqa: E731
                tree_fn = lambda: hal.page_out_tree(paged, args.po2, zk, data, images[1], nodes[1])            # noqa: E731
                words = hal.page_out_proof(paged, args.po2, zk, data, images[0], nodes[0], proof=buf)
                tree_fn()
                assert int(words[2]) == D and np.array_equal(nodes[0].to_vec()[8:16], root0)
                walked = None
                if table == "sparse":
                    walked = bool(np.array_equal(zhal.image_proof_verify(words, root0), hal.image_root(nodes[1])))
                    assert walked
                t = {"page_out_proof": [], "page_out_tree": []}
                for _ in range(runs):
                    for name, fn in (("page_out_proof", proof_fn), ("page_out_tree", tree_fn)):
                        t[name].append(timed(hal, fn, args.reps))
                steps = {}
                for name, fn in (("page_out_proof", proof_fn), ("page_out_tree", tree_fn)):
                    hal.prof_enable(True)
                    hal.prof_reset()
                    for _ in range(args.reps):
                        fn()
                    hal.sync()
                    steps[name] = {r["name"]: {"calls_per_call": r["calls"] // args.reps, "ms_per_call": round(r["total_ms"] / args.reps, 4)} for r in hal.prof_get()
                                   if r["calls"] and r["name"].startswith(("page_out_", "proof_", "image_", "hash_fold"))}
                    hal.prof_enable(False)
                assert np.array_equal(buf.slice(0, words.size).to_vec(), words)
                h = int(words[4])
                med = {k: float(np.median(v)) for k, v in t.items()}
                print(json.dumps({"bench": "M19", "circuit": "SYN-LOOKUP-paged FULL", "library": os.path.basename(os.environ.get("ZKH_LIBRARY", "") or "libzkhal_mi355x.so"),
                                  "po2": args.po2, "table": table, "pages": D, "image_words": W, "leaves": logup.image_tree_leaves(W), "dirty_leaves": int(words[3]),
                                  "clean_siblings": [int(x) for x in words[5:5 + h]], "proof_bytes": 4 * int(words.size),
                                  "bound_bytes": 4 * hal.image_proof_words(W, D), "walked_on_the_host": walked, "runs": runs, "reps": args.reps,
                                  **{k: spread(v) for k, v in t.items()}, "steps": steps,
                                  "proof_vs_tree": round(med["page_out_proof"] / med["page_out_tree"], 3)}), flush=True)
                del images, nodes, buf
        del data
    if want("M20"):
        # the walk of the update's proof on the device: zkh_image_proof_walk on the buffer zkh_page_out_proof wrote (through the C ABI,
        # the proof's own length) next to its yardstick, zkh_image_proof_verify on the downloaded proof (the parent's host walk), the
        # download timed on its own, and next to zkh_page_out_tree (the update of the same paths: one permutation per dirty node where
        # the walk runs two).  M18 / M19's setup: SYN-LOOKUP-paged FULL, the tables `derive`, `spread` and `sparse`, 2^20 and 2^26 image
        # words.  Timed in alternation, `runs` windows of `reps` calls of the device calls and ONE host walk per window; median and
        # spread (min, max) of the windows; then the walk's stages by their events.  Every layer of the walk is its own four launches
        # (the narrow-layer variant that was built); permutations = 2 sum |S_{k+1}|, from the proof's counts.
        from zeth_amd import hal as zhal
        from zeth_amd.circuits import logup, syn_lookup
        runs, zk = 7, 1994
        A = n - zk
        shape = syn_lookup.FULL
        desc, blob = syn_lookup.build_syn_lookup(shape, link=True, reads=True, pages=True)
        pargs = logup.Arguments.parse(blob)
        pg = pargs.pages
        code_h, full_h, _out = syn_lookup.witness(shape, args.po2, zk, seed=17, link=True, reads=True, pages=True, image=np.zeros(1 << 20, dtype=np.uint32))
        paged = hal.load_circuit(desc, jit=False)
        paged.set_arguments(blob)
        full = full_h.reshape(-1, n)
        pages = int((full[pg.p_on, :A] != 0).sum())
        one = np.uint32((1 << 32) % P)
        rinv = pow(int(one), -1, P)
        enc = lambda x: (np.asarray(x, dtype=np.uint64) * np.uint64(one) % np.uint64(P)).astype(np.uint32)   # noqa: E731
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        data = hal.alloc_elem("m20d", full_h.size)
        u32p = zhal._u32p
        for W in (1 << 20, 1 << 26):
            for table in ("derive", "spread", "sparse"):
                image_h = rand_fp(rng, W)
                hand = full.copy() if table == "derive" else np.zeros_like(full)
                if table == "derive":
                    D = pages
                    addrs = (hand[pg.p_addr, :D].astype(np.uint64) * np.uint64(rinv) % np.uint64(P)).astype(np.int64)
                else:
                    D = pages if table == "spread" else 4096
                    hand[pg.p_on, :D], hand[pg.p_out, :D] = one, rand_fp(rng, D)
                    if W <= 1 << 22:
                        addrs = rng.choice(W, D, replace=False)
                    else:
                        addrs = np.unique(rng.integers(0, W, D + D // 8))
                        addrs = addrs[rng.choice(addrs.size, D, replace=False)]
                    addrs = np.sort(addrs).astype(np.int64)
                    hand[pg.p_addr, :D] = enc(addrs)
                hand[pg.p_in, :D] = image_h[addrs]
                data.write(hand.reshape(-1))
                del hand
                images = [hal.alloc_elem("m20i", W) for _ in range(2)]
                for im in images:
                    im.write(image_h)
                nodes = [hal.image_commit(im) for im in images]
                root0 = hal.image_root(nodes[0])
                buf = hal.alloc("m20p", hal.image_proof_words(W, A))
                words = hal.page_out_proof(paged, args.po2, zk, data, images[0], nodes[0], proof=buf)
                tree_fn = lambda: hal.page_out_tree(paged, args.po2, zk, data, images[1], nodes[1])            # noqa: E731
                tree_fn()
                root1 = hal.image_root(nodes[1])
                after = np.empty(8, dtype=np.uint32)
                walk_fn = lambda: zhal._check(zhal._lib.zkh_image_proof_walk(hal.ctx, buf.h, words.size, root0.ctypes.data_as(u32p), after.ctypes.data_as(u32p)))   # noqa: E731
                walk_fn()
                assert np.array_equal(after, root1), "the walk does not reach the root the update leaves"
                host = np.empty(words.size, dtype=np.uint32)
                down_fn = lambda: zhal._check(zhal._lib.zkh_read(hal.ctx, buf.h, host.ctypes.data_as(u32p), 0, host.size))      # noqa: E731
                t = {"image_proof_walk": [], "page_out_tree": [], "download": [], "image_proof_verify": []}
                for _ in range(runs):
                    for name, fn in (("image_proof_walk", walk_fn), ("page_out_tree", tree_fn), ("download", down_fn)):
                        t[name].append(timed(hal, fn, args.reps))
                    t0 = time.perf_counter()
                    assert np.array_equal(zhal.image_proof_verify(host, root0), root1)
                    t["image_proof_verify"].append(time.perf_counter() - t0)
                hal.prof_enable(True)
                hal.prof_reset()
                for _ in range(args.reps):
                    walk_fn()
                hal.sync()
                steps = {r["name"]: {"calls_per_call": r["calls"] // args.reps, "ms_per_call": round(r["total_ms"] / args.reps, 4)} for r in hal.prof_get()
                         if r["calls"] and r["name"].startswith("walk_")}
                hal.prof_enable(False)
                assert np.array_equal(buf.slice(0, words.size).to_vec(), words)
                h = int(words[4])
                items, perms = int(words[3]), 0
                for k in range(h):                                           # |S_{k+1}| = c_k + (|S_k| - c_k) / 2
                    items = int(words[5 + k]) + (items - int(words[5 + k])) // 2
                    perms += 2 * items
                med = {k: float(np.median(v)) for k, v in t.items()}
                print(json.dumps({"bench": "M20", "circuit": "SYN-LOOKUP-paged FULL", "library": os.path.basename(os.environ.get("ZKH_LIBRARY", "") or "libzkhal_mi355x.so"),
                                  "po2": args.po2, "table": table, "pages": D, "image_words": W, "leaves": logup.image_tree_leaves(W), "layers": h,
                                  "dirty_leaves": int(words[3]), "proof_bytes": 4 * int(words.size), "permutations": perms, "narrow_layers": "one launch set per layer",
                                  "runs": runs, "reps": args.reps, **{k: spread(v) for k, v in t.items()}, "steps": steps,
                                  "walk_vs_download_and_host_walk": round(med["image_proof_walk"] / (med["download"] + med["image_proof_verify"]), 5),
                                  "walk_vs_tree": round(med["image_proof_walk"] / med["page_out_tree"], 3)}), flush=True)
                del images, nodes, buf
        del data
    if want("M21"):
        # P2-PAGE's witness: zkh_page_circuit_witgen (csrc/page_circuit.hip: two permutations per row, one lane per (path, old / new)
        # walking its h blocks in turn) with every path slot full, at h = 17 (2^20 image words) and h = 23 (2^26), next to its yardstick
        # in the same run, zkh_syn_witgen of P2-JOIN at the same po2 (one permutation per row at half the width, one lane per block;
        # that call also writes its code group, so the kernels' own events are reported too).  Timed in alternation, `runs` windows of
        # `reps` calls; median and spread (min, max) of the windows; then both calls' stages by their events.  The generator reads the
        # proof's header and table only, so the proof here is exactly that: a ZKU1 header that describes no leaves and no siblings, and
        # the table.  per_block_ratio = (page_paths per block of two permutations) / (p2join_blocks per block of one).
        from zeth_amd import hal as zhal
        from zeth_amd.circuits import p2_join, p2_page
        runs, zk = 7, 1994
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        join, page = hal.load_circuit(p2_join.p2_join_circuit()), hal.load_circuit(p2_page.p2_page_circuit())
        K = (n - zk) // 31
        jcode, jdata = hal.alloc_elem("m21jc", p2_join.WC * n), hal.alloc_elem("m21jd", p2_join.WD * n)
        kids = rand_fp(rng, 16)
        join_fn = lambda: hal.syn_witgen(join, args.po2, zk, 0, 0x2E80, jcode, jdata, pub=kids)               # noqa: E731
        pdata = hal.alloc_elem("m21pd", p2_page.WD * n)
        u32p = zhal._u32p
        key = zhal.noise_key(0x2E80)
        for W in (1 << 20, 1 << 26):
            h = p2_page.tree_height(W)
            N = p2_page.slots(args.po2, zk, h)
            image_h = rand_fp(rng, W)
            addrs = np.unique(rng.integers(0, W, N + N // 8))
            addrs = np.sort(addrs[rng.choice(addrs.size, N, replace=False)]).astype(np.int64)
            outs = rand_fp(rng, N)
            table = np.stack([addrs.astype(np.uint32), image_h[addrs], outs], axis=1).reshape(-1)
            proof_h = np.concatenate([np.array([0x5A4B5531, W, N, 0, h] + [0] * h, dtype=np.uint32), table])
            image = hal.alloc_elem("m21i", W)
            image.write(image_h)
            before = hal.image_commit(image)
            image_h[addrs] = outs
            image.write(image_h)
            after = hal.image_commit(image)
            del image
            proof = hal.copy_from("m21p", proof_h)
            pcode = hal.page_circuit_code(page, args.po2, zk, W)
            roots = np.zeros(16, dtype=np.uint32)
            page_fn = lambda: zhal._check(zhal._lib.zkh_page_circuit_witgen(hal.ctx, page.h, args.po2, zk, pcode.h, proof.h, proof_h.size, before.h, after.h, pdata.h,   # noqa: E731
                                                                            roots.ctypes.data_as(u32p), key.ctypes.data_as(u32p)))
            page_fn()
            assert np.array_equal(roots[:8], hal.image_root(before)) and np.array_equal(roots[8:], hal.image_root(after))
            top = 31 * h * N - 1                                             # the last path's output row holds root_after on its new side
            got = np.array([pdata.get_at((p2_page.D_SN + j) * n + top) for j in range(8)], dtype=np.uint32)
            assert np.array_equal(got, roots[8:]), "the last path does not end on the root of the tree after the page-out"
            t = {"page_circuit_witgen": [], "p2join_syn_witgen": []}
            for _ in range(runs):
                for name, fn in (("page_circuit_witgen", page_fn), ("p2join_syn_witgen", join_fn)):
                    t[name].append(timed(hal, fn, args.reps))
            steps = {}
            for fn in (page_fn, join_fn):
                hal.prof_enable(True)
                hal.prof_reset()
                for _ in range(args.reps):
                    fn()
                hal.sync()
                steps.update({r["name"]: {"calls_per_call": r["calls"] // args.reps, "ms_per_call": round(r["total_ms"] / args.reps, 4)} for r in hal.prof_get()
                              if r["calls"] and r["name"].startswith(("page_", "p2join_"))})
                hal.prof_enable(False)
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(json.dumps({"bench": "M21", "library": os.path.basename(os.environ.get("ZKH_LIBRARY", "") or "libzkhal_mi355x.so"), "po2": args.po2,
                              "image_words": W, "layers": h, "slots": N, "page_blocks": h * N, "join_blocks": K, "lanes": 2 * N, "runs": runs, "reps": args.reps,
                              **{k: spread(v) for k, v in t.items()}, "steps": steps,
                              "call_ratio": round(med["page_circuit_witgen"] / med["p2join_syn_witgen"], 3),
                              "per_block_ratio": round((steps["page_paths"]["ms_per_call"] / (h * N)) / (steps["p2join_blocks"]["ms_per_call"] / K), 3)}), flush=True)
            del before, after, proof, pcode
        del jcode, jdata, pdata
    if want("M22"):
        # P2-PAGE's parts: zkh_page_circuit_witgen_part on a table of 4 N rows at first = 0, N, 2 N, 3 N (every slot full; the parts after
        # the first walk the root before them, k_page_root: h hash_pairs in one lane after the paths; the parts before the last copy the
        # root they leave out of the rows), next to zkh_page_circuit_witgen on the table's first N rows between the trees of THAT
        # page-out.  M21's setup and windows: `runs` alternating windows of `reps` calls, median and spread, then every call's stages by
        # their events.  The parts' roots must chain from the tree before to the tree after, and part 0 must leave the root of the N-row
        # page-out's tree.
        from zeth_amd import hal as zhal
        from zeth_amd.circuits import p2_page
        runs, zk = 7, 1994
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        page = hal.load_circuit(p2_page.p2_page_circuit())
        pdata = hal.alloc_elem("m22pd", p2_page.WD * n)
        u32p = zhal._u32p
        key = zhal.noise_key(0x2E80)
        for W in (1 << 20, 1 << 26):
            h = p2_page.tree_height(W)
            N = p2_page.slots(args.po2, zk, h)
            assert int(zhal._lib.zkh_page_circuit_slots(args.po2, zk, W)) == N
            D = 4 * N
            image_h = rand_fp(rng, W)
            addrs = np.unique(rng.integers(0, W, D + D // 8))
            addrs = np.sort(addrs[rng.choice(addrs.size, D, replace=False)]).astype(np.int64)
            outs = rand_fp(rng, D)
            table = np.stack([addrs.astype(np.uint32), image_h[addrs], outs], axis=1).reshape(-1)
            head = lambda rows: np.array([0x5A4B5531, W, rows, 0, h] + [0] * h, dtype=np.uint32)   # noqa: E731
            proof_h, proof1_h = np.concatenate([head(D), table]), np.concatenate([head(N), table[:3 * N]])
            image = hal.alloc_elem("m22i", W)
            image.write(image_h)
            before = hal.image_commit(image)
            image_h[addrs[:N]] = outs[:N]
            image.write(image_h)
            after1 = hal.image_commit(image)
            image_h[addrs] = outs
            image.write(image_h)
            after = hal.image_commit(image)
            del image
            proof, proof1 = hal.copy_from("m22p", proof_h), hal.copy_from("m22p1", proof1_h)
            pcode = hal.page_circuit_code(page, args.po2, zk, W)
            roots = np.zeros(16, dtype=np.uint32)
            whole_fn = lambda: zhal._check(zhal._lib.zkh_page_circuit_witgen(hal.ctx, page.h, args.po2, zk, pcode.h, proof1.h, proof1_h.size, before.h, after1.h, pdata.h,   # noqa: E731
                                                                             roots.ctypes.data_as(u32p), key.ctypes.data_as(u32p)))
            part_fn = lambda first: lambda: zhal._check(zhal._lib.zkh_page_circuit_witgen_part(hal.ctx, page.h, args.po2, zk, pcode.h, proof.h, proof_h.size, before.h,   # noqa: E731
                                                                                               after.h, first, pdata.h, roots.ctypes.data_as(u32p), key.ctypes.data_as(u32p)))
            fns = [("page_circuit_witgen", whole_fn)] + [(f"part_first_{p}N", part_fn(p * N)) for p in range(4)]
            chain = []
            for name, fn in fns:
                fn()
                chain.append(roots.copy())
            assert np.array_equal(chain[0][:8], hal.image_root(before)) and np.array_equal(chain[0][8:], hal.image_root(after1))
            assert np.array_equal(chain[1], chain[0]), "part 0 of the long table does not leave the root of the N-row page-out"
            assert all(np.array_equal(chain[p][8:], chain[p + 1][:8]) for p in range(1, 4)) and np.array_equal(chain[4][8:], hal.image_root(after))
            t = {name: [] for name, _ in fns}
            for _ in range(runs):
                for name, fn in fns:
                    t[name].append(timed(hal, fn, args.reps))
            steps = {}
            for name, fn in fns:
                hal.prof_enable(True)
                hal.prof_reset()
                for _ in range(args.reps):
                    fn()
                hal.sync()
                steps[name] = {r["name"]: {"calls_per_call": r["calls"] // args.reps, "ms_per_call": round(r["total_ms"] / args.reps, 4)} for r in hal.prof_get()
                               if r["calls"] and r["name"].startswith("page_")}
                hal.prof_enable(False)
            print(json.dumps({"bench": "M22", "library": os.path.basename(os.environ.get("ZKH_LIBRARY", "") or "libzkhal_mi355x.so"), "po2": args.po2,
                              "image_words": W, "layers": h, "slots": N, "table_rows": D, "runs": runs, "reps": args.reps,
                              **{k: spread(v) for k, v in t.items()}, "steps": steps}), flush=True)
            del before, after, after1, proof, proof1, pcode
        del pdata
    if want("M23"):
        # P2-PAGE-ordered: zkh_page_ordered_witgen next to zkh_page_circuit_witgen_part on one table of 2 N rows (every slot full) at
        # first = 0 and first = N, and the seal of the part at 0 under both circuits (zkh_prove_begin / zkh_syn_accum /
        # zkh_prove_finish: 42 + 129 = 171 code and data columns against 39 + 125 = 164, 4 accum columns under both).  M21's windows: `runs`
        # alternating windows of `reps` calls, median and spread, then every witness call's stages by their events; page_order is the
        # one stage the ordered call adds.  Both calls must give the same roots, and the ordered parts' lo / hi must chain.
        from zeth_amd import hal as zhal
        from zeth_amd.circuits import p2_page, p2_page_ordered
        from zeth_amd.prover import Segment, SegmentProver
        runs, zk = 7, 1994
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        provers = {"page": SegmentProver(hal, p2_page.p2_page_circuit()), "ordered": SegmentProver(hal, p2_page_ordered.p2_page_ordered_circuit())}
        datas = {"page": hal.alloc_elem("m23pd", p2_page.WD * n), "ordered": hal.alloc_elem("m23od", p2_page_ordered.WD * n)}
        u32p = zhal._u32p
        key = zhal.noise_key(0x2E80)
        for W in (1 << 20, 1 << 26):
            h = p2_page.tree_height(W)
            N = p2_page.slots(args.po2, zk, h)
            D = 2 * N
            image_h = rand_fp(rng, W)
            addrs = np.unique(rng.integers(0, W, D + D // 8))
            addrs = np.sort(addrs[rng.choice(addrs.size, D, replace=False)]).astype(np.int64)
            outs = rand_fp(rng, D)
            table = np.stack([addrs.astype(np.uint32), image_h[addrs], outs], axis=1).reshape(-1)
            proof_h = np.concatenate([np.array([0x5A4B5531, W, D, 0, h] + [0] * h, dtype=np.uint32), table])
            image = hal.alloc_elem("m23i", W)
            image.write(image_h)
            before = hal.image_commit(image)
            image_h[addrs] = outs
            image.write(image_h)
            after = hal.image_commit(image)
            del image
            proof = hal.copy_from("m23p", proof_h)
            codes = {"page": hal.page_circuit_code(provers["page"].circuit, args.po2, zk, W), "ordered": hal.page_ordered_code(provers["ordered"].circuit, args.po2, zk, W)}
            outs16, outs18 = np.zeros(16, dtype=np.uint32), np.zeros(18, dtype=np.uint32)
            page_fn = lambda first: lambda: zhal._check(zhal._lib.zkh_page_circuit_witgen_part(hal.ctx, provers["page"].circuit.h, args.po2, zk, codes["page"].h, proof.h,   # noqa: E731
                                                                                               proof_h.size, before.h, after.h, first, datas["page"].h,
                                                                                               outs16.ctypes.data_as(u32p), key.ctypes.data_as(u32p)))
            ordered_fn = lambda first: lambda: zhal._check(zhal._lib.zkh_page_ordered_witgen(hal.ctx, provers["ordered"].circuit.h, args.po2, zk, codes["ordered"].h, proof.h,   # noqa: E731
                                                                                             proof_h.size, before.h, after.h, first, datas["ordered"].h,
                                                                                             outs18.ctypes.data_as(u32p), key.ctypes.data_as(u32p)))
            fns = [(f"{name}_first_{p}N", mk(p * N)) for p in range(2) for name, mk in (("page_circuit_witgen_part", page_fn), ("page_ordered_witgen", ordered_fn))]
            bounds = []
            for p in (1, 0):                                                 # the part at 0 last: its witness is the one sealed below
                page_fn(p * N)()
                ordered_fn(p * N)()
                assert np.array_equal(outs18[:16], outs16), "the ordered call's roots are not P2-PAGE's"
                bounds.append((p2_page_ordered.decode(outs18[16]), p2_page_ordered.decode(outs18[17])))
            assert bounds[1] == (0, int(addrs[N - 1]) + 1) and bounds[0] == (bounds[1][1], int(addrs[D - 1]) + 1)
            seg = Segment(index=0, po2=args.po2, zk_cycles=zk, noise_seed=0x2E80)
            seal_fn = lambda name, out: lambda: provers[name].seal_with_accum(seg, codes[name], datas[name], out, provers[name].syn_accumulate(seg, datas[name]))   # noqa: E731
            seals = [("seal_page", seal_fn("page", outs16.copy())), ("seal_ordered", seal_fn("ordered", outs18.copy()))]
            t = {name: [] for name, _ in fns + seals}
            for _ in range(runs):
                for name, fn in fns:
                    t[name].append(timed(hal, fn, args.reps))
            steps = {}
            for name, fn in fns:
                hal.prof_enable(True)
                hal.prof_reset()
                for _ in range(args.reps):
                    fn()
                hal.sync()
                steps[name] = {r["name"]: {"calls_per_call": r["calls"] // args.reps, "ms_per_call": round(r["total_ms"] / args.reps, 4)} for r in hal.prof_get()
                               if r["calls"] and r["name"].startswith("page_")}
                hal.prof_enable(False)
            page_fn(0)()                                                     # the witnesses of the part at 0 again, for the seals
            ordered_fn(0)()
            for _ in range(runs):
                for name, fn in seals:
                    t[name].append(timed(hal, fn, args.reps))
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(json.dumps({"bench": "M23", "library": os.path.basename(os.environ.get("ZKH_LIBRARY", "") or "libzkhal_mi355x.so"), "po2": args.po2,
                              "image_words": W, "layers": h, "slots": N, "table_rows": D, "runs": runs, "reps": args.reps,
                              **{k: spread(v) for k, v in t.items()}, "steps": steps,
                              "ordered_minus_page_ms": {f"first_{p}N": round((med[f"page_ordered_witgen_first_{p}N"] - med[f"page_circuit_witgen_part_first_{p}N"]) * 1e3, 4)
                                                        for p in range(2)},
                              "seal_ratio": round(med["seal_ordered"] / med["seal_page"], 4), "code_and_data_columns": {"page": 39 + 125, "ordered": 42 + 129}}),
                  flush=True)
            del before, after, proof, codes
        del datas
    if want("M24"):
        # P2-TREE: one page-out of 662 267 random addresses (the paging segment's own table at po2 20) planned and sealed by dirty nodes
        # next to P2-PAGE-ordered's paths: the parts under both plans, zkh_page_tree_witgen (part 0 and the middle part) next to
        # zkh_page_ordered_witgen (first = 0) in M23's windows with every call's stages by their events, and the seal of part 0 under both
        # circuits (41 + 106 code and data columns and 24 accum columns through zkh_accumulate against 42 + 129 and 4 through zkh_syn_accum).
        # Both chains must start from the same root; no threshold on any time.
        from zeth_amd import hal as zhal
        from zeth_amd.circuits import p2_page, p2_page_ordered, p2_tree
        from zeth_amd.prover import Segment, SegmentProver
        runs, zk, D = 7, 1994, 662267
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        provers = {"tree": SegmentProver(hal, p2_tree.p2_tree_circuit(), arguments=p2_tree.arguments()),
                   "ordered": SegmentProver(hal, p2_page_ordered.p2_page_ordered_circuit())}
        datas = {"tree": hal.alloc_elem("m24td", p2_tree.WD * n), "ordered": hal.alloc_elem("m24od", p2_page_ordered.WD * n)}
        u32p = zhal._u32p
        key = zhal.noise_key(0x2E80)
        for W in (1 << 20, 1 << 26):
            h = p2_page.tree_height(W)
            image_h = rand_fp(rng, W)
            addrs = np.sort(rng.choice(W, D, replace=False)).astype(np.int64)
            outs = rand_fp(rng, D)
            table = np.stack([addrs.astype(np.uint32), image_h[addrs], outs], axis=1).reshape(-1)
            proof_h = np.concatenate([np.array([0x5A4B5531, W, D, 0, h] + [0] * h, dtype=np.uint32), table])
            image = hal.alloc_elem("m24i", W)
            image.write(image_h)
            before = hal.image_commit(image)
            image_h[addrs] = outs
            image.write(image_h)
            after = hal.image_commit(image)
            del image
            proof = hal.copy_from("m24p", proof_h)
            t0 = time.perf_counter()
            plan = hal.page_tree_plan(args.po2, zk, W, addrs)
            plan_ms = (time.perf_counter() - t0) * 1e3
            ordered_plan = p2_page.parts(args.po2, zk, W, D)
            codes = {"tree": hal.page_tree_code(provers["tree"].circuit, args.po2, zk), "ordered": hal.page_ordered_code(provers["ordered"].circuit, args.po2, zk, W)}
            out_t, out_o = np.zeros(18, dtype=np.uint32), np.zeros(18, dtype=np.uint32)
            tree_fn = lambda part: lambda: zhal._check(zhal._lib.zkh_page_tree_witgen(hal.ctx, provers["tree"].circuit.h, args.po2, zk, codes["tree"].h, proof.h,   # noqa: E731
                                                                                      proof_h.size, before.h, after.h, part[0], part[1], datas["tree"].h,
                                                                                      out_t.ctypes.data_as(u32p), key.ctypes.data_as(u32p)))
            ordered_fn = lambda first: lambda: zhal._check(zhal._lib.zkh_page_ordered_witgen(hal.ctx, provers["ordered"].circuit.h, args.po2, zk, codes["ordered"].h, proof.h,   # noqa: E731
                                                                                             proof_h.size, before.h, after.h, first, datas["ordered"].h,
                                                                                             out_o.ctypes.data_as(u32p), key.ctypes.data_as(u32p)))
            mid = len(plan) // 2
            fns = [("page_tree_witgen_part_0", tree_fn(plan[0])), ("page_ordered_witgen_first_0", ordered_fn(0)), (f"page_tree_witgen_part_{mid}", tree_fn(plan[mid]))]
            tree_fn(plan[0])()
            ordered_fn(0)()
            assert np.array_equal(out_t[:8], out_o[:8]), "the two chains do not start from the same root"
            assert p2_tree.decode(out_t[16]) == 1 << (h - 1) and p2_tree.decode(out_t[17]) == (1 << (h - 1)) + (int(addrs[plan[0][1] - 1]) >> 4) + 1
            seg = Segment(index=0, po2=args.po2, zk_cycles=zk, noise_seed=0x2E80)
            seals = [("seal_tree", lambda: provers["tree"].seal_with_accum(seg, codes["tree"], datas["tree"], out_t.copy(),
                                                                           provers["tree"].args_accumulate(seg, codes["tree"], datas["tree"]))),
                     ("seal_ordered", lambda: provers["ordered"].seal_with_accum(seg, codes["ordered"], datas["ordered"], out_o.copy(),
                                                                                 provers["ordered"].syn_accumulate(seg, datas["ordered"])))]
            t = {name: [] for name, _ in fns + seals}
            for _ in range(runs):
                for name, fn in fns:
                    t[name].append(timed(hal, fn, args.reps))
            steps = {}
            for name, fn in fns:
                hal.prof_enable(True)
                hal.prof_reset()
                for _ in range(args.reps):
                    fn()
                hal.sync()
                steps[name] = {r["name"]: {"calls_per_call": r["calls"] // args.reps, "ms_per_call": round(r["total_ms"] / args.reps, 4)} for r in hal.prof_get()
                               if r["calls"] and r["name"].startswith(("page_", "tree_"))}
                hal.prof_enable(False)
            tree_fn(plan[0])()                                               # the witnesses of part 0 again, for the seals
            ordered_fn(0)()
            for _ in range(runs):
                for name, fn in seals:
                    t[name].append(timed(hal, fn, args.reps))
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(json.dumps({"bench": "M24", "library": os.path.basename(os.environ.get("ZKH_LIBRARY", "") or "libzkhal_mi355x.so"), "po2": args.po2,
                              "image_words": W, "layers": h, "table_rows": D, "block_slots": p2_tree.block_slots(args.po2, zk),
                              "path_slots": p2_page.slots(args.po2, zk, h), "parts": {"tree": len(plan), "ordered": len(ordered_plan)},
                              "tree_part_rows": {"min": min(c for _, c in plan), "max": max(c for _, c in plan)}, "plan_host_ms": round(plan_ms, 3),
                              "runs": runs, "reps": args.reps, **{k: spread(v) for k, v in t.items()}, "steps": steps,
                              "seal_ratio_tree_over_ordered": round(med["seal_tree"] / med["seal_ordered"], 4),
                              "columns": {"tree": {"code": p2_tree.WC, "data": p2_tree.WD, "accum": p2_tree.WA},
                                          "ordered": {"code": p2_page_ordered.WC, "data": p2_page_ordered.WD, "accum": p2_page_ordered.WA}}}),
                  flush=True)
            del before, after, proof, codes
        del datas
    if want("M25"):
        # P2-TREE's plan where the table lies: M24's table (the same draws in the same order, so `--only M25` plans the addresses `--only
        # M24` seals) planned by the parent's path, the read-back of the table and zkh_page_tree_plan over every third word, and by
        # zkh_page_tree_plan_device, in one run, alternating, M24's windows; the device call's three stages by their events.  The
        # yardstick is the parent's path in this run.  Both plans must be the same; no threshold on any time.
        import ctypes as C
        from zeth_amd import hal as zhal
        from zeth_amd.circuits import p2_page, p2_tree
        runs, zk, D, cap = 7, 1994, 662267, 4096
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        for W in (1 << 20, 1 << 26):
            h = p2_page.tree_height(W)
            image_h = rand_fp(rng, W)
            addrs = np.sort(rng.choice(W, D, replace=False)).astype(np.int64)
            outs = rand_fp(rng, D)
            table = np.stack([addrs.astype(np.uint32), image_h[addrs], outs], axis=1).reshape(-1)
            del image_h
            proof = hal.copy_from("m25p", np.concatenate([np.array([0x5A4B5531, W, D, 0, h] + [0] * h, dtype=np.uint32), table]))
            parts = {k: (C.c_size_t * (2 * cap))() for k in ("host", "device")}
            count = {k: C.c_size_t() for k in parts}
            got = {}
            read_back = lambda: got.__setitem__("addrs", np.ascontiguousarray(proof.slice(5 + h, 3 * D).to_vec()[::3]))   # noqa: E731
            host_plan = lambda: zhal._check(zhal._lib.zkh_page_tree_plan(args.po2, zk, W, zhal._ptr(got["addrs"]), D, parts["host"], cap,   # noqa: E731
                                                                         C.byref(count["host"])))
            parent = lambda: got.__setitem__("plan", hal.page_tree_plan(args.po2, zk, W, proof.slice(5 + h, 3 * D).to_vec()[::3]))   # noqa: E731
            device = lambda: zhal._check(zhal._lib.zkh_page_tree_plan_device(hal.ctx, args.po2, zk, W, proof.h, 5 + h, D, parts["device"], cap,   # noqa: E731
                                                                             C.byref(count["device"]), None))
            wrapper = lambda: got.__setitem__("device_plan", hal.page_tree_plan_device(args.po2, zk, W, proof, 5 + h, D))   # noqa: E731
            fns = [("parent_path_read_back_and_plan", parent), ("plan_device_call", device), ("read_back_alone", read_back), ("host_plan_alone", host_plan),
                   ("plan_device_python_wrapper", wrapper)]
            t = {name: [] for name, _ in fns}
            for _ in range(runs):
                for name, fn in fns:
                    t[name].append(timed(hal, fn, args.reps))
            assert got["plan"] == got["device_plan"] == p2_tree.parts_by_scan(args.po2, zk, W, addrs), "the device plan is not the host plan"
            assert count["host"].value == count["device"].value == len(got["plan"]) and list(parts["host"]) == list(parts["device"])
            hal.prof_enable(True)
            hal.prof_reset()
            for _ in range(args.reps):
                device()
            hal.sync()
            stages = {r["name"]: {"calls_per_call": r["calls"] // args.reps, "ms_per_call": round(r["total_ms"] / args.reps, 4)} for r in hal.prof_get()
                      if r["calls"] and r["name"].startswith("tree_plan_")}
            hal.prof_enable(False)
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(json.dumps({"bench": "M25", "library": os.path.basename(os.environ.get("ZKH_LIBRARY", "") or "libzkhal_mi355x.so"), "po2": args.po2,
                              "image_words": W, "layers": h, "table_rows": D, "block_slots": p2_tree.block_slots(args.po2, zk), "parts": len(got["plan"]),
                              "workgroups": -(-D // 256), "runs": runs, "reps": args.reps, **{k: spread(v) for k, v in t.items()}, "stages": stages,
                              "device_over_parent": round(med["plan_device_call"] / med["parent_path_read_back_and_plan"], 4)}),
                  flush=True)
            del proof
    if want("M26"):
        # zkh_reduce_elem (w := w % P in place; the caller-trace seal paths run it on code and data between zkh_derive_all and the
        # accumulate) at SYN-A's widths next to zkh_eltwise_copy_elem moving the same bytes (one read and one write per word), in one
        # run, alternating windows.  About 30 % of the words are >= P; the kernel's time does not depend on it, the result is checked.
        from zeth_amd.circuits import syn_air
        runs = 7
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        desc = syn_air.syn_a()
        for group, width in (("code", int(desc[4])), ("data", int(desc[5]))):
            words = width * n
            src = upload(hal, rng, "m26s", words)
            head = src.slice(0, 1 << 20).to_vec()
            raised = np.where((rng.random(head.size) < 0.3) & (head < (1 << 32) - P), head + np.uint32(P), head).astype(np.uint32)
            src.write(raised, 0)
            dst = hal.alloc_elem("m26d", words)
            t = {"reduce_elem": [], "eltwise_copy_elem": []}
            for _ in range(runs):
                t["reduce_elem"].append(timed(hal, lambda: hal.reduce_elem(src), args.reps))
                t["eltwise_copy_elem"].append(timed(hal, lambda: hal.eltwise_copy_elem(dst, src), args.reps))
            assert np.array_equal(src.slice(0, 1 << 20).to_vec(), head), "reduce_elem did not give w % P"
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(json.dumps({"bench": "M26", "library": os.path.basename(os.environ.get("ZKH_LIBRARY", "") or "libzkhal_mi355x.so"), "po2": args.po2,
                              "group": group, "columns": width, "alg_GB": round(8 * words / 1e9, 4), "runs": runs, "reps": args.reps,
                              **{k: spread(v) for k, v in t.items()}, "reduce_GB_per_s": round(8 * words / med["reduce_elem"] / 1e9, 1),
                              "copy_GB_per_s": round(8 * words / med["eltwise_copy_elem"] / 1e9, 1),
                              "reduce_over_copy": round(med["reduce_elem"] / med["eltwise_copy_elem"], 4)}), flush=True)
            del src, dst
    if want("M27"):
        # THE TIE: what a tied group costs beside what its seals cost anyway, on M24's table (662 267 random addresses over an
        # image of 2^20 words), in one run, alternating windows, median and spread.  zkh_data_root of a P2-PAGE-tied part (pass one commits
        # every part's data group once more) next to the seal of that part; zkh_accumulate_open on SYN-LOOKUP-tied FULL next to
        # zkh_accumulate on SYN-LOOKUP-paged's blob over the same traces (the parent's yardstick: one term more, and the total returned);
        # zkh_table_fingerprint over the table next to zkh_eltwise_copy_elem over the same bytes.  No threshold on any time.
        from zeth_amd import hal as zhal
        from zeth_amd.circuits import logup, p2_page, p2_page_tied, syn_lookup
        from zeth_amd.prover import Segment, SegmentProver
        runs, zk, D, W = 7, 1994, 662267, 1 << 20
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        h = p2_page.tree_height(W)
        image_h = rand_fp(rng, W)
        addrs = np.sort(rng.choice(W, D, replace=False)).astype(np.int64)
        outs = rand_fp(rng, D)
        table = np.stack([addrs.astype(np.uint32), image_h[addrs], outs], axis=1).reshape(-1)
        proof_h = np.concatenate([np.array([0x5A4B5531, W, D, 0, h] + [0] * h, dtype=np.uint32), table])
        image = hal.alloc_elem("m27i", W)
        image.write(image_h)
        before = hal.image_commit(image)
        image_h[addrs] = outs
        image.write(image_h)
        after = hal.image_commit(image)
        del image
        proof = hal.copy_from("m27p", proof_h)
        challenge = zhal.tie_challenge(rand_fp(rng, 16))
        t, got = {}, {}
        # (a) the data root of a part next to its seal
        page = SegmentProver(hal, p2_page_tied.p2_page_tied_circuit(), arguments=p2_page_tied.arguments())
        seg = Segment(index=0, po2=args.po2, zk_cycles=zk, noise_seed=0x2E80)
        code = hal.page_ordered_code(page.circuit, args.po2, zk, W)
        data = hal.alloc_elem("m27d", p2_page_tied.WD * n)
        prefix = hal.page_ordered_witgen(page.circuit, args.po2, zk, code, proof, proof_h.size, before, after, 0, data, seg.noise_seed)
        accum = hal.alloc_elem("m27a", p2_page_tied.WA * n)

        def seal_part():
            total = got["part_total"] = hal.accumulate_open(page.circuit, args.po2, zk, seg.noise_seed, code, data, challenge, accum)
            return page.seal_with_accum(seg, code, data, np.concatenate([prefix, challenge, total]), lambda _mix: accum)
        fns = [("data_root_part", lambda: page.data_root(data, args.po2)), ("seal_part", seal_part)]
        # (c) the fingerprint next to a copy of the same bytes
        rows = hal.copy_from("m27t", table)
        rows_copy = hal.alloc_elem("m27c", table.size)
        fns += [("table_fingerprint", lambda: got.__setitem__("f", hal.table_fingerprint(proof, 5 + h, D, challenge))),
                ("eltwise_copy_elem_same_bytes", lambda: hal.eltwise_copy_elem(rows_copy, rows))]
        for name, _ in fns:
            t[name] = []
        for _ in range(runs):
            for name, fn in fns:
                t[name].append(timed(hal, fn, args.reps))
        slots = p2_page.slots(args.po2, zk, h)
        part_rows = hal.table_fingerprint(proof, 5 + h, min(slots, D), challenge).astype(np.uint64)
        assert not ((part_rows + got["part_total"]) % np.uint64(P)).any(), "part 0's open total is not minus the fingerprint of its rows"
        del code, data, accum, rows, rows_copy, before, after, proof
        # (b) the open accumulate next to the closed one, SYN-LOOKUP FULL over one pair of traces
        shape = syn_lookup.FULL
        code_h, full_h, _out = syn_lookup.witness(shape, args.po2, zk, seed=17, link=True, reads=True, pages=True, image=np.zeros(1 << 20, dtype=np.uint32))
        circuits = {}
        for name, tied in (("paged", False), ("tied", True)):
            desc, blob = syn_lookup.build_syn_lookup(shape, link=True, reads=True, pages=True, tied=tied)
            circuits[name] = hal.load_circuit(desc, jit=False)
            circuits[name].set_arguments(blob)
        k = {name: len(logup.Arguments.parse(c._args).by_column()) for name, c in circuits.items()}
        dcode, ddata = hal.copy_from("m27sc", code_h), hal.copy_from("m27sd", full_h)
        accums = {name: hal.alloc_elem("m27sa", 4 * k[name] * n) for name in circuits}
        mix = rand_fp(rng, 8)
        acc = [("accumulate_paged", lambda: hal.accumulate(circuits["paged"], args.po2, zk, 0x2E80, dcode, ddata, mix, accums["paged"])),
               ("accumulate_open_tied", lambda: got.__setitem__("total", hal.accumulate_open(circuits["tied"], args.po2, zk, 0x2E80, dcode, ddata, challenge, accums["tied"])))]
        for name, _ in acc:
            t[name] = []
        for _ in range(runs):
            for name, fn in acc:
                t[name].append(timed(hal, fn, args.reps))
        assert got["total"].any(), "the tied segment's open total is zero"
        med = {name: float(np.median(v)) for name, v in t.items()}
        print(json.dumps({"bench": "M27", "library": os.path.basename(os.environ.get("ZKH_LIBRARY", "") or "libzkhal_mi355x.so"), "po2": args.po2,
                          "image_words": W, "layers": h, "table_rows": D, "path_slots": slots, "runs": runs, "reps": args.reps,
                          **{name: spread(v) for name, v in t.items()}, "accum_columns": k,
                          "data_root_over_seal": round(med["data_root_part"] / med["seal_part"], 4),
                          "open_over_closed": round(med["accumulate_open_tied"] / med["accumulate_paged"], 4),
                          "fingerprint_over_copy": round(med["table_fingerprint"] / med["eltwise_copy_elem_same_bytes"], 4),
                          "fingerprint_rows_per_us": round(D / med["table_fingerprint"] / 1e6, 1)}), flush=True)
    if want("M28"):
        # P2-TREE-tied (DESIGN.md §2 "THE TIE"): what tying P2-TREE costs, on M24's table (662 267 random addresses over an image of 2^20
        # words), in one run, alternating windows, median and spread.  The witness of a kind-9 part next to the kind-7 part's (the same
        # part of the same plan: 32 more columns by one more kernel, and a wider tail); a tied part's seal (zkh_accumulate_open over 12
        # Fp4 columns, 138 data columns) next to the P2-TREE part's seal (zkh_accumulate over 6, 106); and the page-out side of a whole
        # tied group, both passes of every part (witness, data root; witness, open accumulate, seal), timed once each, P2-TREE-tied's
        # parts next to P2-PAGE-tied's.  The yardsticks are the parent's kind-7 and P2-PAGE-tied paths in this run.  No threshold.
        from zeth_amd import hal as zhal
        from zeth_amd.circuits import p2_page, p2_page_tied, p2_tree, p2_tree_tied
        from zeth_amd.prover import Segment, SegmentProver
        runs, zk, D, W = 7, 1994, 662267, 1 << 20
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        h = p2_page.tree_height(W)
        image_h = rand_fp(rng, W)
        addrs = np.sort(rng.choice(W, D, replace=False)).astype(np.int64)
        outs = rand_fp(rng, D)
        table = np.stack([addrs.astype(np.uint32), image_h[addrs], outs], axis=1).reshape(-1)
        proof_h = np.concatenate([np.array([0x5A4B5531, W, D, 0, h] + [0] * h, dtype=np.uint32), table])
        image = hal.alloc_elem("m28i", W)
        image.write(image_h)
        before = hal.image_commit(image)
        image_h[addrs] = outs
        image.write(image_h)
        after = hal.image_commit(image)
        del image
        proof = hal.copy_from("m28p", proof_h)
        challenge = zhal.tie_challenge(rand_fp(rng, 16))
        seg = Segment(index=0, po2=args.po2, zk_cycles=zk, noise_seed=0x2E80)
        plan = hal.page_tree_plan(args.po2, zk, W, addrs)
        mods = {"tree": p2_tree, "tree_tied": p2_tree_tied}
        provers = {"tree": SegmentProver(hal, p2_tree.p2_tree_circuit(), arguments=p2_tree.arguments()),
                   "tree_tied": SegmentProver(hal, p2_tree_tied.p2_tree_tied_circuit(), arguments=p2_tree_tied.arguments())}
        code = hal.page_tree_code(provers["tree"].circuit, args.po2, zk)         # one code group serves both kinds
        datas = {k: hal.alloc_elem("m28d", m.WD * n) for k, m in mods.items()}
        accum = hal.alloc_elem("m28a", p2_tree_tied.WA * n)
        prefix = {}
        witness = lambda k, part: lambda: prefix.__setitem__(k, hal.page_tree_witgen(provers[k].circuit, args.po2, zk, code, proof, proof_h.size, before, after,   # noqa: E731
                                                                                      part[0], part[1], datas[k], seg.noise_seed))

        def tied_out(total):
            return np.concatenate([prefix["tree_tied"], [p2_tree_tied.out_base(h)], challenge, total]).astype(np.uint32)

        def seal_tied_part():
            total = hal.accumulate_open(provers["tree_tied"].circuit, args.po2, zk, seg.noise_seed, code, datas["tree_tied"], challenge, accum)
            return provers["tree_tied"].seal_with_accum(seg, code, datas["tree_tied"], tied_out(total), lambda _mix: accum)
        seal_tree_part = lambda: provers["tree"].seal_with_accum(seg, code, datas["tree"], prefix["tree"].copy(),   # noqa: E731
                                                                 provers["tree"].args_accumulate(seg, code, datas["tree"]))
        fns = [("witness_tree_part_0", witness("tree", plan[0])), ("witness_tree_tied_part_0", witness("tree_tied", plan[0]))]
        seals = [("seal_tree_part", seal_tree_part), ("seal_tree_tied_part", seal_tied_part)]
        t = {name: [] for name, _ in fns + seals}
        for _ in range(runs):
            for name, fn in fns:
                t[name].append(timed(hal, fn, args.reps))
        assert np.array_equal(prefix["tree"], prefix["tree_tied"]), "the two kinds do not state the same 18 words"
        steps = {}
        for name, fn in fns:
            hal.prof_enable(True)
            hal.prof_reset()
            for _ in range(args.reps):
                fn()
            hal.sync()
            steps[name] = {r["name"]: {"calls_per_call": r["calls"] // args.reps, "ms_per_call": round(r["total_ms"] / args.reps, 4)} for r in hal.prof_get()
                           if r["calls"] and r["name"].startswith(("page_", "tree_"))}
            hal.prof_enable(False)
        for _ in range(runs):
            for name, fn in seals:
                t[name].append(timed(hal, fn, args.reps))
        # the page-out side of a whole group, once: pass one (witness, data root) and pass two (witness, accumulate, seal) of every part
        totals = np.zeros(4, dtype=np.uint64)

        def tree_group():
            totals[:] = 0
            for part in plan:
                witness("tree_tied", part)()
                provers["tree_tied"].data_root(datas["tree_tied"], args.po2)
            for part in plan:
                witness("tree_tied", part)()
                total = hal.accumulate_open(provers["tree_tied"].circuit, args.po2, zk, seg.noise_seed, code, datas["tree_tied"], challenge, accum)
                totals[:] = (totals + total) % np.uint64(P)
                provers["tree_tied"].seal_with_accum(seg, code, datas["tree_tied"], tied_out(total), lambda _mix: accum)
        group = {"tree_tied": {"parts": len(plan), "total_ms": round(timed(hal, tree_group, 1) * 1e3, 2)}}
        want_total = hal.table_fingerprint(proof, 5 + h, D, challenge).astype(np.uint64)
        assert not ((totals + want_total) % np.uint64(P)).any(), "the parts' open totals are not minus the fingerprint of the table"
        del datas, accum
        page = SegmentProver(hal, p2_page_tied.p2_page_tied_circuit(), arguments=p2_page_tied.arguments())
        page_code = hal.page_ordered_code(page.circuit, args.po2, zk, W)
        page_data = hal.alloc_elem("m28pd", p2_page_tied.WD * n)
        page_accum = hal.alloc_elem("m28pa", p2_page_tied.WA * n)
        page_plan = p2_page.parts(args.po2, zk, W, D)
        page_witness = lambda first: hal.page_ordered_witgen(page.circuit, args.po2, zk, page_code, proof, proof_h.size, before, after, first, page_data, seg.noise_seed)   # noqa: E731

        def page_group():
            for first, _count in page_plan:
                page_witness(first)
                page.data_root(page_data, args.po2)
            for first, _count in page_plan:
                words = page_witness(first)
                total = hal.accumulate_open(page.circuit, args.po2, zk, seg.noise_seed, page_code, page_data, challenge, page_accum)
                page.seal_with_accum(seg, page_code, page_data, np.concatenate([words[:p2_page_tied.PREFIX_WORDS], challenge, total]), lambda _mix: page_accum)
        group["page_tied"] = {"parts": len(page_plan), "total_ms": round(timed(hal, page_group, 1) * 1e3, 2)}
        med = {name: float(np.median(v)) for name, v in t.items()}
        print(json.dumps({"bench": "M28", "library": os.path.basename(os.environ.get("ZKH_LIBRARY", "") or "libzkhal_mi355x.so"), "po2": args.po2,
                          "image_words": W, "layers": h, "table_rows": D, "block_slots": p2_tree.block_slots(args.po2, zk), "runs": runs, "reps": args.reps,
                          **{name: spread(v) for name, v in t.items()}, "steps": steps, "group_page_out_side": group,
                          "columns": {k: {"code": m.WC, "data": m.WD, "accum": m.WA} for k, m in mods.items()},
                          "witness_tied_over_tree": round(med["witness_tree_tied_part_0"] / med["witness_tree_part_0"], 4),
                          "seal_tied_over_tree": round(med["seal_tree_tied_part"] / med["seal_tree_part"], 4),
                          "group_tree_tied_over_page_tied": round(group["tree_tied"]["total_ms"] / group["page_tied"]["total_ms"], 4)}), flush=True)
    if want("M29"):
        # P2-TREE from the proof alone: on M24's table (662 267 random addresses, po2 20, W = 2^20 and 2^26), zkh_image_proof_nodes (the walk
        # that keeps the dirty-node table) next to zkh_image_proof_walk, the yardstick, and part 0's witness from the dirty nodes
        # (zkh_page_tree_witgen_nodes) next to part 0's witness from the two trees (zkh_page_tree_witgen, the parent's path), and the copy
        # of the tree that page_out(keep_before=True) makes, in one run, alternating, M24's windows; every call's stages by their events;
        # the words of the table, of its bound, of the proof and of the two trees it replaces.  The proof is built on the host from the
        # device's tree, read back once.  Both witnesses must be the same buffer; no threshold on any time.
        from zeth_amd import hal as zhal
        from zeth_amd.circuits import p2_page, p2_tree
        from zeth_amd.prover import SegmentProver
        runs, zk, D = 7, 1994, 662267
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        prover = SegmentProver(hal, p2_tree.p2_tree_circuit(), arguments=p2_tree.arguments())
        code = hal.page_tree_code(prover.circuit, args.po2, zk)
        datas = {k: hal.alloc_elem("m29d", p2_tree.WD * n) for k in ("nodes", "trees")}
        u32p = zhal._u32p
        key = zhal.noise_key(0x2E80)
        for W in (1 << 20, 1 << 26):
            h = p2_page.tree_height(W)
            L = 1 << h
            image_h = rand_fp(rng, W)
            addrs = np.sort(rng.choice(W, D, replace=False)).astype(np.int64)
            outs = rand_fp(rng, D)
            table = np.stack([addrs.astype(np.uint32), image_h[addrs], outs], axis=1).reshape(-1)
            image = hal.alloc_elem("m29i", W)
            image.write(image_h)
            before = hal.image_commit(image)
            tree_h = before.to_vec().reshape(-1, 8)
            S = np.unique(addrs >> 3)                                        # the ZKU1 proof: logup.reference_page_out_proof's sections
            counts, sections = [], [tree_h[L + S].reshape(-1)]
            for k in range(h):
                clean = (S ^ 1)[~np.isin(S ^ 1, S)]
                counts.append(clean.size)
                sections.append(tree_h[(L >> k) + clean].reshape(-1))
                S = np.unique(S >> 1)
            proof_h = np.concatenate([np.array([0x5A4B5531, W, D, sections[0].size // 8, h] + counts, dtype=np.uint32), table] + sections).astype(np.uint32)
            root_before = tree_h[1].copy()
            del tree_h, sections
            image_h[addrs] = outs
            image.write(image_h)
            after = hal.image_commit(image)
            del image
            proof = hal.copy_from("m29p", proof_h)
            plan = hal.page_tree_plan(args.po2, zk, W, addrs)
            bound = hal.image_dirty_words(W, D)
            dirty = hal.alloc("m29n", bound)
            copy = hal.alloc("m29c", before.size())
            root = {k: np.zeros(8, dtype=np.uint32) for k in ("walk", "nodes")}
            outw = {k: np.zeros(18, dtype=np.uint32) for k in datas}
            rb = root_before.ctypes.data_as(u32p)
            walk_fn = lambda: zhal._check(zhal._lib.zkh_image_proof_walk(hal.ctx, proof.h, proof_h.size, rb, root["walk"].ctypes.data_as(u32p)))   # noqa: E731
            nodes_fn = lambda: zhal._check(zhal._lib.zkh_image_proof_nodes(hal.ctx, proof.h, proof_h.size, rb, root["nodes"].ctypes.data_as(u32p), dirty.h))   # noqa: E731
            wit_nodes = lambda: zhal._check(zhal._lib.zkh_page_tree_witgen_nodes(hal.ctx, prover.circuit.h, args.po2, zk, code.h, proof.h, proof_h.size, dirty.h,   # noqa: E731
                                                                                 plan[0][0], plan[0][1], datas["nodes"].h, outw["nodes"].ctypes.data_as(u32p),
                                                                                 key.ctypes.data_as(u32p)))
            wit_trees = lambda: zhal._check(zhal._lib.zkh_page_tree_witgen(hal.ctx, prover.circuit.h, args.po2, zk, code.h, proof.h, proof_h.size, before.h, after.h,   # noqa: E731
                                                                           plan[0][0], plan[0][1], datas["trees"].h, outw["trees"].ctypes.data_as(u32p),
                                                                           key.ctypes.data_as(u32p)))
            copy_fn = lambda: hal.eltwise_copy_elem(copy, before)             # noqa: E731
            fns = [("image_proof_walk", walk_fn), ("image_proof_nodes", nodes_fn), ("witness_part_0_from_trees", wit_trees), ("witness_part_0_from_dirty_nodes", wit_nodes),
                   ("keep_before_tree_copy", copy_fn)]
            for _name, fn in fns:
                fn()
            hal.sync()
            assert np.array_equal(root["walk"], root["nodes"]) and np.array_equal(root["nodes"], hal.image_root(after)), "the walks do not reach the tree's root"
            assert np.array_equal(outw["nodes"], outw["trees"]) and np.array_equal(datas["nodes"].to_vec(), datas["trees"].to_vec()), "the two witnesses differ"
            head = dirty.slice(0, 4 + h).to_vec()
            dirty_words = 4 + h + 33 * int(head[4:].astype(np.uint64).sum())
            t = {name: [] for name, _ in fns}
            for _ in range(runs):
                for name, fn in fns:
                    t[name].append(timed(hal, fn, args.reps))
            steps = {}
            for name, fn in fns[:4]:
                hal.prof_enable(True)
                for _ in range(2):                                           # the first pass creates the scopes' events: only the second is kept
                    hal.prof_reset()
                    for _ in range(args.reps):
                        fn()
                    hal.sync()
                steps[name] = {r["name"]: {"calls_per_call": r["calls"] // args.reps, "ms_per_call": round(r["total_ms"] / args.reps, 4)} for r in hal.prof_get()
                               if r["calls"] and r["name"].startswith(("walk_", "tree_", "page_"))}
                hal.prof_enable(False)
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(json.dumps({"bench": "M29", "library": os.path.basename(os.environ.get("ZKH_LIBRARY", "") or "libzkhal_mi355x.so"), "po2": args.po2,
                              "image_words": W, "layers": h, "table_rows": D, "block_slots": p2_tree.block_slots(args.po2, zk), "parts": len(plan),
                              "part_0_rows": plan[0][1], "dirty_nodes_per_layer": [int(x) for x in head[4:]],
                              "words": {"dirty": dirty_words, "dirty_bound": bound, "proof": int(proof_h.size), "two_trees": 2 * before.size()},
                              "runs": runs, "reps": args.reps, **{k: spread(v) for k, v in t.items()}, "steps": steps,
                              "nodes_over_walk": round(med["image_proof_nodes"] / med["image_proof_walk"], 4),
                              "witness_nodes_over_trees": round(med["witness_part_0_from_dirty_nodes"] / med["witness_part_0_from_trees"], 4)}), flush=True)
            del before, after, proof, dirty, copy
        del datas
    if want("M30"):
        # Held commitments (DESIGN.md §2 "THE TIE"): a whole tied group sealed in two passes (hold_bytes = 0, the parent's path: every data
        # group committed twice, every part's witness generated twice) next to the same group with a budget that holds everything
        # (zkh_commit_data in pass one, zkh_prove_begin_held in pass two), on M28's setup: po2 20, M24's table of 662 267 addresses over
        # 2^20 words, kind 9, 4 parts; the segment is SYN-LOOKUP-tied FULL over M27's traces, whose page table is not this table, so the
        # group is sealed with check_table=False: every seal is made, at the cost it has in a group that cancels.  Beside it, for one
        # part, zkh_commit_data + zkh_prove_begin_held next to zkh_data_root + zkh_prove_begin (the job is dropped: no finish).  One
        # run, alternating windows, median and spread; the bytes a part's commitment holds and the live high-water mark after each arm's
        # first group (meaningful with --only M30: the mark is the context's).  The seals of the two arms must be the same.  No threshold.
        import ctypes as C
        from zeth_amd import hal as zhal, page_seal
        from zeth_amd.circuits import p2_page, p2_tree, p2_tree_tied, syn_lookup
        from zeth_amd.prover import Segment, SegmentProver
        runs, zk, D, W = 7, 1994, 662267, 1 << 20
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        h = p2_page.tree_height(W)
        image_h = rand_fp(rng, W)
        addrs = np.sort(rng.choice(W, D, replace=False)).astype(np.int64)
        outs = rand_fp(rng, D)
        table = np.stack([addrs.astype(np.uint32), image_h[addrs], outs], axis=1).reshape(-1)
        proof_h = np.concatenate([np.array([0x5A4B5531, W, D, 0, h] + [0] * h, dtype=np.uint32), table])
        image = hal.alloc_elem("m30i", W)
        image.write(image_h)
        before = hal.image_commit(image)
        image_h[addrs] = outs
        image.write(image_h)
        after = hal.image_commit(image)
        del image
        proof = hal.copy_from("m30p", proof_h)
        page = SegmentProver(hal, p2_tree_tied.p2_tree_tied_circuit(), arguments=p2_tree_tied.arguments())
        plan = hal.page_tree_plan(args.po2, zk, W, addrs)
        desc, blob = syn_lookup.build_syn_lookup(syn_lookup.FULL, link=True, reads=True, pages=True, tied=True)
        segp = SegmentProver(hal, desc, arguments=blob)
        code_h, data_h, _out = syn_lookup.witness(syn_lookup.FULL, args.po2, zk, seed=17, link=True, reads=True, pages=True, image=np.zeros(1 << 20, dtype=np.uint32))
        scode, sdata = hal.copy_from("m30sc", code_h), hal.copy_from("m30sd", data_h)
        del code_h, data_h
        seg = Segment(index=0, po2=args.po2, zk_cycles=zk, noise_seed=0x2E80)
        parts = [Segment(index=1 + p, po2=args.po2, zk_cycles=zk, noise_seed=0x2E81 + p) for p in range(len(plan))]
        prefix = np.zeros(segp.out_size() - page_seal.TIE_WORDS, dtype=np.uint32)
        sealed = {}

        def group(name, hold):
            def fn():
                sealed[name] = page_seal.seal_tied_tree(segp, seg, scode, sdata, prefix, page, parts, proof, proof_h.size, before, after, check_table=False, hold_bytes=hold)
            return fn
        arms = [("group_two_passes", group("two_passes", 0)), ("group_held", group("held", 1 << 50))]
        live0, peaks = hal.memory()["live"], {}
        for name, fn in arms:                                                # the first group of each arm: the mark it leaves, and the seals
            fn()
            peaks[name] = hal.memory()["peak"] - live0
        (seg_a, parts_a), (seg_b, parts_b) = sealed["two_passes"], sealed["held"]
        assert np.array_equal(seg_a.seal, seg_b.seal) and all(np.array_equal(a.seal, b.seal) for a, b in zip(parts_a, parts_b)), "the held group's seals differ"
        # one part: the commit and the begin, the job dropped
        code = hal.page_tree_code(page.circuit, args.po2, zk)
        data = hal.alloc_elem("m30d", p2_tree_tied.WD * n)
        hal.page_tree_witgen(page.circuit, args.po2, zk, code, proof, proof_h.size, before, after, plan[0][0], plan[0][1], data, seg.noise_seed)
        out = np.zeros(page.out_size(), dtype=np.uint32)
        mix = np.zeros(max(1, int(page.circuit.desc[8])), dtype=np.uint32)
        job, u32p = C.c_void_p(), zhal._u32p
        part_bytes = {}

        def part_two_passes():
            page.data_root(data, args.po2)
            zhal._check(zhal._lib.zkh_prove_begin(page.h, args.po2, code.h, data.h, out.ctypes.data_as(u32p), C.byref(job), mix.ctypes.data_as(u32p)))
            zhal._lib.zkh_prove_abort(job)

        def part_held():
            com = page.commit_data(data, args.po2)
            part_bytes["commitment"] = com.bytes
            zhal._check(zhal._lib.zkh_prove_begin_held(page.h, args.po2, code.h, com.h, out.ctypes.data_as(u32p), C.byref(job), mix.ctypes.data_as(u32p)))
            zhal._lib.zkh_prove_abort(job)
            com.release()
        fns = arms + [("part_data_root_then_prove_begin", part_two_passes), ("part_commit_data_then_prove_begin_held", part_held)]
        t = {name: [] for name, _ in fns}
        for _ in range(runs):
            for name, fn in fns:
                t[name].append(timed(hal, fn, args.reps))
        med = {name: float(np.median(v)) for name, v in t.items()}
        print(json.dumps({"bench": "M30", "library": os.path.basename(os.environ.get("ZKH_LIBRARY", "") or "libzkhal_mi355x.so"), "po2": args.po2,
                          "image_words": W, "layers": h, "table_rows": D, "block_slots": p2_tree.block_slots(args.po2, zk), "parts": len(plan),
                          "runs": runs, "reps": args.reps, **{name: spread(v) for name, v in t.items()},
                          "columns": {"segment_data": segp.group_sizes()[2], "part_data": p2_tree_tied.WD},
                          "bytes": {"part_commitment": part_bytes["commitment"], "part_trace": 4 * p2_tree_tied.WD * n,
                                    "segment_commitment": page_seal.commitment_bytes(segp.group_sizes()[2], args.po2),
                                    "peak_live_over_start": peaks},
                          "group_held_over_two_passes": round(med["group_held"] / med["group_two_passes"], 4),
                          "part_held_over_two_passes": round(med["part_commit_data_then_prove_begin_held"] / med["part_data_root_then_prove_begin"], 4)}), flush=True)
        del scode, sdata, code, data, before, after, proof
    if want("M31"):
        # Paging in from a page table (zkh_derive_links_paged_table: the rows (a_i, in_i, out_i) of the proof's table in the image's
        # place) next to its yardstick in the same run, zkh_derive_links_paged on the same trace with the image itself, for an image of
        # 2^20 and of 2^26 words with the addresses drawn over the whole image.  SYN-LOOKUP-paged FULL; the table is read off the image
        # variant's own output and lies where a proof would hold it (after 5 + h header words).  Timed in alternation, `runs` windows of
        # `reps` calls; median and spread (min, max) of the windows; then the passes by their events.  No threshold.
        from zeth_amd.circuits import logup, p2_page, syn_lookup
        runs, zk = 7, 1994
        A = n - zk
        shape = syn_lookup.FULL
        desc, blob = syn_lookup.build_syn_lookup(shape, link=True, reads=True, pages=True)
        pargs = logup.Arguments.parse(blob)
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        for W in (1 << 20, 1 << 26):
            image_h = np.random.default_rng(31).integers(1, P, W, dtype=np.uint64).astype(np.uint32)
            code_h, full_h, _out = syn_lookup.witness(shape, args.po2, zk, seed=17, addr_range=W, link=True, reads=True, pages=True, image=image_h)
            paged = hal.load_circuit(desc, jit=False)
            paged.set_arguments(blob)
            full = full_h.reshape(-1, n)
            on = full[pargs.pages.p_on, :A] != 0
            D, at = int(on.sum()), 5 + p2_page.tree_height(W)
            rows = np.stack([logup._dec(full[pargs.pages.p_addr, :A][on]).astype(np.uint32), full[pargs.pages.p_in, :A][on] % P, full[pargs.pages.p_out, :A][on] % P], axis=1)
            bare_h = full.copy()
            bare_h[paged.derived_data_columns(), :A] = 0
            code, data_i, data_t, image = (hal.alloc_elem(nm, sz) for nm, sz in (("code", code_h.size), ("data_i", bare_h.size), ("data_t", bare_h.size), ("image", W)))
            table = hal.copy_from("m31t", np.concatenate([np.zeros(at, dtype=np.uint32), rows.reshape(-1).astype(np.uint32)]))
            code.write(code_h)
            data_i.write(bare_h.reshape(-1))
            data_t.write(bare_h.reshape(-1))
            image.write(image_h)
            image_fn = lambda: hal.derive_links_paged(paged, args.po2, zk, code, data_i, image)                              # noqa: E731
            table_fn = lambda: hal.derive_links_paged_table(paged, args.po2, zk, code, data_t, table, W, table_at=at, D=D)    # noqa: E731
            image_fn()
            table_fn()
            assert np.array_equal(data_i.to_vec(), full_h) and np.array_equal(data_t.to_vec() % P, full_h % P), "the table variant's trace differs"
            fns = (("derive_links_paged", image_fn), ("derive_links_paged_table", table_fn))
            t = {name: [] for name, _ in fns}
            for _ in range(runs):
                for name, fn in fns:
                    t[name].append(timed(hal, fn, args.reps))
            steps = {}
            for name, fn in fns:
                hal.prof_enable(True)
                hal.prof_reset()
                for _ in range(args.reps):
                    fn()
                hal.sync()
                steps[name] = {r["name"]: round(r["total_ms"] / max(r["calls"], 1), 4) for r in hal.prof_get()
                               if r["calls"] and r["name"].startswith(("sort_", "links_", "pages_"))}
                hal.prof_enable(False)
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(json.dumps({"bench": "M31", "circuit": "SYN-LOOKUP-paged FULL", "po2": args.po2, "accesses": A, "pages": D, "image_words": W, "table_words": 3 * D,
                              "runs": runs, "reps": args.reps, **{k: spread(v) for k, v in t.items()}, "steps_ms": steps,
                              "table_vs_image": round(med["derive_links_paged_table"] / med["derive_links_paged"], 3)}), flush=True)
            del code, data_i, data_t, image, table, image_h, code_h, full_h, bare_h
    if want("M32"):
        # PORTS (ZKA1 version 9): zkh_derive_links on FULL widened to 3 memory pairs as the PORTS of one memory, next to its yardstick in the
        # same run, the same library on the version-6 blob of three SEPARATE memories over the same columns.  Their clocks differ (one
        # memory counts 3 row + port, three memories count rows), so each has its own valid witness over the same addresses' range.  One sort
        # run of 3 A items against three runs of A.  Timed in alternation, `runs` windows of `reps` calls; median and spread (min, max) of the
        # windows; then the passes by their events.  No threshold.
        from zeth_amd.circuits import logup, syn_lookup
        runs, zk = 7, 1994
        A = n - zk
        shape = syn_lookup.Shape(16, 4, 8, 3)
        assert 3 * A < 1 << (syn_lookup.ORDER_LIMBS * shape.limb_bits), "the ported clocks must fit the link limbs"
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        arms, fns, keep = {}, [], []
        for name, ported in (("ports_v9", True), ("separate_v6", False)):
            desc, blob = syn_lookup.build_syn_lookup(shape, link=True, reads=True, ports=ported)
            assert int(blob[1]) == (9 if ported else 6)
            code_h, full_h, _out = syn_lookup.witness(shape, args.po2, zk, seed=32, link=True, reads=True, ports=ported)
            circuit = hal.load_circuit(desc, jit=False)
            circuit.set_arguments(blob)
            bare_h = full_h.reshape(-1, n).copy()
            bare_h[circuit.derived_data_columns(), :A] = 0
            code, data = hal.alloc_elem("code", code_h.size), hal.alloc_elem("data", bare_h.size)
            code.write(code_h)
            data.write(bare_h.reshape(-1))
            fn = lambda circuit=circuit, code=code, data=data: hal.derive_links(circuit, args.po2, zk, code, data)      # noqa: E731
            fn()
            got, lk = data.to_vec().reshape(-1, n), [c for r in logup.Arguments.parse(blob).records if isinstance(r, logup.Link) for c in r.dsts]
            assert np.array_equal(got[lk], full_h.reshape(-1, n)[lk]), f"{name}: the derived link columns differ from the host-made ones"
            fns.append((name, fn))
            keep.append((circuit, code, data))
            del code_h, full_h, bare_h, got
        t = {name: [] for name, _ in fns}
        for _ in range(runs):
            for name, fn in fns:
                t[name].append(timed(hal, fn, args.reps))
        for name, fn in fns:
            hal.prof_enable(True)
            hal.prof_reset()
            for _ in range(args.reps):
                fn()
            hal.sync()
            steps = {r["name"]: round(r["total_ms"] / max(r["calls"], 1), 4) for r in hal.prof_get() if r["calls"] and r["name"].startswith(("sort_", "links_"))}
            hal.prof_enable(False)
            sort_ms = sum(v for k, v in steps.items() if k.startswith("sort_"))
            arms[name] = {**spread(t[name]), "steps_ms": steps, "sort_ms": round(sort_ms, 4), "check_ms": steps.get("links_check", 0), "write_ms": steps.get("links_write", 0)}
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps({"bench": "M32", "circuit": "SYN-LOOKUP-reads FULL widened to 3 memory pairs", "po2": args.po2, "accesses": 3 * A, "addresses_below": 1 << 20,
                          "runs": runs, "reps": args.reps, **arms, "ports_vs_separate": round(med["ports_v9"] / med["separate_v6"], 3)}), flush=True)
        del keep
    if want("M33"):
        # WIDE (ZKA1 version 10): what the second value word costs.  SYN-LOOKUP-paged-wide FULL (two value words per address, the image 2 W
        # words) next to SYN-LOOKUP-paged FULL in the same run, the same library, on the same addresses, write flags and clocks (the witnesses
        # of one seed): zkh_derive_links_paged, and zkh_page_out_tree into a committed image (the wide one lays out the flat table of 2 D rows
        # first and its tree has twice the leaves).  Timed in alternation, `runs` windows of `reps` calls; median and spread (min, max) of
        # the windows; then the passes by their events.  No threshold.
        from zeth_amd.circuits import logup, syn_lookup
        runs, zk = 7, 1994
        A = n - zk
        shape, W = syn_lookup.FULL, 1 << 20
        image_w = rand_fp(np.random.default_rng(33), 2 * W)
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        arms, fns, keep, pages = {}, [], [], {}
        for name, wide in (("wide_v10", True), ("narrow_v7", False)):
            desc, blob = syn_lookup.build_syn_lookup(shape, link=True, reads=True, pages=True, wide=wide)
            pargs = logup.Arguments.parse(blob)
            assert int(blob[1]) == (10 if wide else 7)
            image_h = image_w if wide else image_w[:W].copy()
            code_h, full_h, _out = syn_lookup.witness(shape, args.po2, zk, seed=33, link=True, reads=True, pages=True, image=image_h, wide=wide)
            circuit = hal.load_circuit(desc, jit=False)
            circuit.set_arguments(blob)
            assert circuit.page_words() == (2 if wide else 1)
            bare_h = full_h.reshape(-1, n).copy()
            bare_h[circuit.derived_data_columns(), :A] = 0
            code, data, image = hal.alloc_elem("code", code_h.size), hal.alloc_elem("data", bare_h.size), hal.alloc_elem("image", image_h.size)
            paged = hal.alloc_elem("image_out", image_h.size)                # the page-out's own image and tree: the derive pages in from the first image every time
            code.write(code_h)
            data.write(bare_h.reshape(-1))
            image.write(image_h)
            paged.write(image_h)
            nodes = hal.image_commit(paged)
            derive = lambda circuit=circuit, code=code, data=data, image=image: hal.derive_links_paged(circuit, args.po2, zk, code, data, image)      # noqa: E731
            out = lambda circuit=circuit, data=data, image=paged, nodes=nodes: hal.page_out_tree(circuit, args.po2, zk, data, image, nodes)         # noqa: E731  (after the first call it rewrites what is there)
            derive()
            lk = [c for r in pargs.records if isinstance(r, (logup.Link, logup.Pages)) for c in r.dsts]
            assert np.array_equal(data.to_vec().reshape(-1, n)[lk], full_h.reshape(-1, n)[lk]), f"{name}: the derived columns differ from the host-made ones"
            out()
            assert np.array_equal(paged.to_vec(), logup.reference_page_out(pargs, args.po2, zk, full_h, image_h)), f"{name}: the image differs from the twin's"
            assert np.array_equal(nodes.to_vec(), hal.image_commit(paged).to_vec()), f"{name}: the updated tree is not the fresh commit's"
            pages[name] = int((full_h.reshape(-1, n)[pargs.pages.p_on, :A] != 0).sum())
            fns += [(name + ".derive_links_paged", derive), (name + ".page_out_tree", out)]
            keep.append((circuit, code, data, image, paged, nodes))
            del code_h, full_h, bare_h
        assert pages["wide_v10"] == pages["narrow_v7"], "the two witnesses page the same addresses"
        t = {name: [] for name, _ in fns}
        for _ in range(runs):
            for name, fn in fns:
                t[name].append(timed(hal, fn, args.reps))
        for name, fn in fns:
            hal.prof_enable(True)
            hal.prof_reset()
            for _ in range(args.reps):
                fn()
            hal.sync()
            steps = {r["name"]: round(r["total_ms"] / max(r["calls"], 1), 4) for r in hal.prof_get()
                     if r["calls"] and r["name"].startswith(("sort_", "links_", "pages_", "page_out_", "image_"))}
            hal.prof_enable(False)
            arms[name] = {**spread(t[name]), "steps_ms": steps}
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps({"bench": "M33", "circuit": "SYN-LOOKUP-paged-wide FULL next to SYN-LOOKUP-paged FULL", "po2": args.po2, "accesses": A, "pages": pages["wide_v10"],
                          "image_addresses": W, "runs": runs, "reps": args.reps, **arms,
                          "derive_wide_vs_narrow": round(med["wide_v10.derive_links_paged"] / med["narrow_v7.derive_links_paged"], 3),
                          "page_out_tree_wide_vs_narrow": round(med["wide_v10.page_out_tree"] / med["narrow_v7.page_out_tree"], 3)}), flush=True)
        del keep
    if want("M34"):
        # FLAT (ZKA1 version 11): what the two flat-address columns cost.  (a) zkh_derive_links_paged on the version-11 blob (SYN-LOOKUP-paged-wide
        # with flats) next to the version-10 blob (SYN-LOOKUP-paged-wide) in the same run, on M33's addresses, write flags, clocks and values: the
        # version-10 arm's data group is the version-11 arm's without its last two columns.  Two more scattered 4-byte stores per page and two
        # more coalesced ones per row below the table, in the write pass.  (b) zkh_accumulate_open on SYN-LOOKUP-tied-wide (two tie terms of
        # width 3 and the wide memory's terms) next to SYN-LOOKUP-tied.  Timed in alternation, `runs` windows of `reps` calls; median and
        # spread (min, max) of the windows; then the passes by their events.  No threshold.
        from zeth_amd.circuits import logup, syn_lookup
        runs, zk = 7, 1994
        A = n - zk
        shape, W = syn_lookup.FULL, 1 << 20
        image_w = rand_fp(np.random.default_rng(33), 2 * W)                  # M33's image
        spread = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}   # noqa: E731
        kw = dict(link=True, reads=True, pages=True)
        code_h, flat_h, _out = syn_lookup.witness(shape, args.po2, zk, seed=33, image=image_w, wide=True, flat=True, **kw)
        _code, narrow_h, _out = syn_lookup.witness(shape, args.po2, zk, seed=33, image=image_w[:W].copy(), **kw)
        assert np.array_equal(_code, code_h)
        challenge = rand_fp(np.random.default_rng(34), 8)
        arms, fns, keep, pages = {}, [], [], {}
        for name, build, full_h, image_h in (("flat_v11", dict(wide=True, flat=True), flat_h, image_w),
                                             ("wide_v10", dict(wide=True), flat_h.reshape(-1, n)[:-2].reshape(-1), image_w),
                                             ("tied_wide_v11", dict(wide=True, flat=True, tied=True), flat_h, image_w),
                                             ("tied_v8", dict(tied=True), narrow_h, image_w[:W].copy())):
            desc, blob = syn_lookup.build_syn_lookup(shape, **kw, **build)
            pargs = logup.Arguments.parse(blob)
            assert int(blob[1]) == (11 if build.get("flat") else 10 if build.get("wide") else 8)
            circuit = hal.load_circuit(desc, jit=False)
            circuit.set_arguments(blob)
            assert circuit.page_flats() == (2 if build.get("flat") else 0)
            bare_h = full_h.reshape(-1, n).copy()
            bare_h[circuit.derived_data_columns(), :A] = 0
            code, data, image = hal.alloc_elem("code", code_h.size), hal.alloc_elem("data", bare_h.size), hal.alloc_elem("image", image_h.size)
            code.write(code_h)
            data.write(bare_h.reshape(-1))
            image.write(image_h)
            derive = lambda circuit=circuit, code=code, data=data, image=image: hal.derive_links_paged(circuit, args.po2, zk, code, data, image)      # noqa: E731
            derive()
            lk = [c for r in pargs.records if isinstance(r, (logup.Link, logup.Pages)) for c in r.dsts] + list(pargs.pages.flats)
            assert np.array_equal(data.to_vec().reshape(-1, n)[lk], full_h.reshape(-1, n)[lk]), f"{name}: the derived columns differ from the host-made ones"
            pages[name] = int((full_h.reshape(-1, n)[pargs.pages.p_on, :A] != 0).sum())
            if build.get("tied"):
                data.write(np.ascontiguousarray(full_h).reshape(-1))
                hal.reduce_elem(code)
                hal.reduce_elem(data)
                accum = hal.alloc_elem("accum", (4 * pargs.k) << args.po2)
                fn = lambda circuit=circuit, code=code, data=data, accum=accum: hal.accumulate_open(circuit, args.po2, zk, 0x34, code, data, challenge, accum)      # noqa: E731
                total = fn()
                rows = pages[name] * (2 if build.get("wide") else 1)
                d = full_h.reshape(-1, n)
                cols = ([(pargs.pages.flats[j], pargs.pages.p_ins[j], pargs.pages.p_outs[j]) for j in range(2)] if build.get("wide") else
                        [(pargs.pages.p_addr, pargs.pages.p_in, pargs.pages.p_out)])
                table = np.stack([np.stack([d[c, :pages[name]] for c in trio], axis=1) for trio in cols], axis=1).reshape(-1, 3)
                table[:, 0] = logup._dec(table[:, 0]).astype(np.uint32)       # ZKU1 rows hold the address as an integer
                want_total = hal.table_fingerprint(hal.copy_from("table", table.reshape(-1)), 0, rows, challenge)
                assert np.array_equal(total, want_total), f"{name}: the open total is not the fingerprint of the (flat) table"
                fns.append((name + ".accumulate_open", fn))
                keep.append((circuit, code, data, image, accum))
            else:
                fns.append((name + ".derive_links_paged", derive))
                keep.append((circuit, code, data, image))
            del bare_h
        assert pages["flat_v11"] == pages["wide_v10"] == pages["tied_wide_v11"] == pages["tied_v8"], "the witnesses page the same addresses"
        t = {name: [] for name, _ in fns}
        for _ in range(runs):
            for name, fn in fns:
                t[name].append(timed(hal, fn, args.reps))
        for name, fn in fns:
            hal.prof_enable(True)
            hal.prof_reset()
            for _ in range(args.reps):
                fn()
            hal.sync()
            steps = {r["name"]: round(r["total_ms"] / max(r["calls"], 1), 4) for r in hal.prof_get() if r["calls"]}
            hal.prof_enable(False)
            arms[name] = {**spread(t[name]), "steps_ms": steps}
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps({"bench": "M34", "circuit": "SYN-LOOKUP-paged-wide FULL with flat-address columns next to without; SYN-LOOKUP-tied-wide next to SYN-LOOKUP-tied",
                          "po2": args.po2, "accesses": A, "pages": pages["flat_v11"], "image_addresses": W, "runs": runs, "reps": args.reps, **arms,
                          "derive_flat_vs_wide": round(med["flat_v11.derive_links_paged"] / med["wide_v10.derive_links_paged"], 3),
                          "links_write_flat_vs_wide_ms": [arms["flat_v11.derive_links_paged"]["steps_ms"].get("links_write"),
                                                          arms["wide_v10.derive_links_paged"]["steps_ms"].get("links_write")],
                          "accumulate_open_tied_wide_vs_tied": round(med["tied_wide_v11.accumulate_open"] / med["tied_v8.accumulate_open"], 3)}), flush=True)
        del keep
    hal.close()


if __name__ == "__main__":
    main()
