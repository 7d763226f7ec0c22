"""Python mirror of `risc0_zkp::hal::{Hal, CircuitHal, Buffer}` over libzkhal_mi355x.so (ctypes, no torch types).

Method names and argument meaning follow the upstream trait (risc0-zkp 3.0.2 src/hal/mod.rs, un-vendored:
/root/reference/Cargo.lock:5393) so that tests read like upstream's cpu-vs-gpu HAL parity tests.  The product
path is the HIP library ONLY: importing this module without the built .so, or creating a HipHal without a
GPU, raises — there is no CPU fallback here (the CPU oracle lives in oracle/ and is test-only).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZKH_LIBRARY") or os.path.join(_HERE, "libzkhal_mi355x.so")   # override: another build of the same ABI

INV_RATE, QUERIES, FRI_FOLD, FRI_MIN_DEGREE, ZK_CYCLES, CHECK_SIZE, EXT_SIZE, DIGEST_WORDS = 4, 50, 16, 256, 1994, 16, 4, 8
P = 2013265921                      # BabyBear
_RINV = pow(1 << 32, -1, P)


def fp_decode(word: int) -> int:
    """Montgomery word -> canonical residue (seal words are raw Montgomery `Elem`s, like upstream's)."""
    return (int(word) * _RINV) % P


def noise_key(noise_seed) -> Optional[np.ndarray]:
    """The 8-word blinding key of include/zkhal.h (BLINDING ROWS) from the `noise_seed` this package's API takes: an integer below
    2^256 (little-endian words; 0x2E80 -> (0x2E80, 0, ..)), 32 bytes, or 8 words; None / 0 -> None = NULL at the ABI = a fresh 256-bit
    key from the OS for that call (the product default)."""
    if noise_seed is None:
        return None
    if isinstance(noise_seed, (bytes, bytearray)):
        noise_seed = int.from_bytes(noise_seed, "little")
    if isinstance(noise_seed, (int, np.integer)):
        v = int(noise_seed)
        if v == 0:
            return None
        if not 0 < v < (1 << 256):
            raise ValueError("noise seed out of range (256 bits)")
        return np.array([(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)], dtype=np.uint32)
    k = np.ascontiguousarray(noise_seed, dtype=np.uint32)
    if k.shape != (8,):
        raise ValueError("a noise key is 8 words")
    return k if k.any() else None


def _key_ptr(noise_seed):
    """-> (keep-alive array or None, ctypes pointer or None)"""
    k = noise_key(noise_seed)
    return k, (None if k is None else k.ctypes.data_as(C.POINTER(C.c_uint32)))


def fp_encode(x: int) -> int:
    return ((int(x) % P) << 32) % P

class SegmentSpec(C.Structure):
    """`zkh_segment` (include/zkhal.h): one segment of a session."""
    _fields_ = [("po2", C.c_uint32), ("seed", C.c_uint64), ("noise_key", C.c_uint32 * 8), ("pub", C.POINTER(C.c_uint32)), ("n_pub", C.c_size_t),
                ("host_code", C.POINTER(C.c_uint32)), ("host_data", C.POINTER(C.c_uint32)), ("out_global", C.POINTER(C.c_uint32))]


class ProveInfo(C.Structure):
    """`zkh_prove_info`: what zkh_session_prove returns."""
    _fields_ = [("n_segments", C.c_size_t), ("seals", C.POINTER(C.POINTER(C.c_uint32))), ("seal_words", C.POINTER(C.c_size_t)),
                ("root_seal", C.POINTER(C.c_uint32)), ("root_seal_words", C.c_size_t), ("n_joins", C.c_size_t),
                ("wall_s", C.c_double), ("leaves_s", C.c_double), ("join_s", C.c_double), ("witgen_s_sum", C.c_double), ("seal_s_sum", C.c_double),
                ("n_lifts", C.c_size_t), ("root_program", C.c_size_t), ("lift_s", C.c_double),
                ("n_retries", C.c_size_t), ("fold_tail_s", C.c_double), ("fold_busy_s_sum", C.c_double), ("streamed", C.c_int),
                ("preflight_cpu_s_sum", C.c_double), ("trace_bytes", C.c_double),
                ("root_core", C.c_uint32 * 8), ("root_pre", C.c_uint32), ("root_post", C.c_uint32)]


# every symbol include/zkhal.h declares: (restype, argtypes)
_sz, _u32, _u64, _vp, _i = C.c_size_t, C.c_uint32, C.c_uint64, C.c_void_p, C.c_int
_u32p = C.POINTER(C.c_uint32)
_err = C.c_void_p    # heap error string (freed with zkh_free_error)


class ProfRec(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("calls", C.c_uint64), ("total_ms", C.c_double), ("alg_bytes", C.c_double)]


class CheckRowsResult(C.Structure):
    """`zkh_check_rows_result`: what zkh_check_rows found (row -1: no row of the window fails)."""
    _fields_ = [("row", C.c_int64), ("step", C.c_uint32), ("failing_rows", C.c_uint32), ("value", C.c_uint32 * 4)]


class CheckBusResult(C.Structure):
    """`zkh_check_bus_result`: what zkh_check_bus found (term, row -1: every key balances)."""
    _fields_ = [("row", C.c_int64), ("term", C.c_int32), ("tag", C.c_uint32), ("key", C.c_uint32 * 4), ("net", C.c_uint32),
                ("unbalanced_keys", C.c_uint32), ("distinct_keys", C.c_uint32), ("slots", C.c_uint32)]


class BusTerm(C.Structure):
    """`zkh_bus_term`: what one term holds of the key zkh_check_bus reports (count 0: nothing; the rows are then 0xffffffff)."""
    _fields_ = [("count", C.c_uint32), ("first_row", C.c_uint32), ("last_row", C.c_uint32), ("weight", C.c_uint32)]


ABI = {
    "zkh_free_error": (None, [_vp]),
    "zkh_version": (C.c_char_p, []),
    "zkh_ctx_create": (_err, [_i, C.c_char_p, C.POINTER(_vp)]),
    "zkh_ctx_destroy": (None, [_vp]),
    "zkh_sync": (_err, [_vp]),
    "zkh_ctx_memory": (None, [_vp, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz)]),
    "zkh_ctx_trim": (_err, [_vp]),
    "zkh_ctx_stream": (_vp, [_vp]),
    "zkh_poseidon2_set_constants": (_err, [_vp, _u32p, _u32p]),
    "zkh_alloc": (_err, [_vp, C.c_char_p, _sz, _i, C.POINTER(_vp)]),
    "zkh_copy_from": (_err, [_vp, C.c_char_p, _u32p, _sz, C.POINTER(_vp)]),
    "zkh_wrap": (_err, [_vp, _vp, _sz, C.POINTER(_vp)]),
    "zkh_slice": (_err, [_vp, _sz, _sz, C.POINTER(_vp)]),
    "zkh_retain": (None, [_vp]),
    "zkh_release": (None, [_vp]),
    "zkh_size": (_sz, [_vp]),
    "zkh_device_ptr": (_vp, [_vp]),
    "zkh_read": (_err, [_vp, _vp, _u32p, _sz, _sz]),
    "zkh_write": (_err, [_vp, _vp, _u32p, _sz, _sz]),
    "zkh_host_alloc": (_err, [_vp, _sz, C.POINTER(_u32p)]),
    "zkh_host_free": (None, [_vp, _u32p]),
    "zkh_write_async": (_err, [_vp, _vp, _u32p, _sz, _sz]),
    "zkh_batch_interpolate_ntt": (_err, [_vp, _vp, _sz]),
    "zkh_batch_expand_into_evaluate_ntt": (_err, [_vp, _vp, _vp, _sz, _sz]),
    "zkh_batch_bit_reverse": (_err, [_vp, _vp, _sz]),
    "zkh_zk_shift": (_err, [_vp, _vp, _sz]),
    "zkh_batch_interpolate_ntt_zk_shift": (_err, [_vp, _vp, _sz]),
    "zkh_batch_interpolate_ntt_from": (_err, [_vp, _vp, _vp, _sz, _i]),
    "zkh_hash_rows": (_err, [_vp, _vp, _vp]),
    "zkh_hash_fold": (_err, [_vp, _vp, _sz, _sz]),
    "zkh_merkle_fold_all": (_err, [_vp, _vp, _sz]),
    "zkh_merkle_build": (_err, [_vp, _vp, _vp, _sz]),
    "zkh_batch_evaluate_any": (_err, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "zkh_batch_evaluate_any_bitrev": (_err, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "zkh_batch_bit_reverse_extelem": (_err, [_vp, _vp, _sz]),
    "zkh_mix_poly_coeffs": (_err, [_vp, _vp, _u32p, _u32p, _vp, _vp, _sz, _sz]),
    "zkh_combos_prepare": (_err, [_vp, _vp, _u32p, _u32p, _sz]),
    "zkh_combos_prepare_regs": (_err, [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp, _u32p]),
    "zkh_combos_divide": (_err, [_vp, _vp, _sz, _sz, _u32p, _sz, _vp]),
    "zkh_combos_divide_all": (_err, [_vp, _vp, _sz, _sz, _u32p, _u32p, _vp]),
    "zkh_eltwise_add_elem": (_err, [_vp, _vp, _vp, _vp]),
    "zkh_eltwise_copy_elem": (_err, [_vp, _vp, _vp]),
    "zkh_eltwise_zeroize_elem": (_err, [_vp, _vp]),
    "zkh_reduce_elem": (_err, [_vp, _vp]),
    "zkh_eltwise_sum_extelem": (_err, [_vp, _vp, _vp]),
    "zkh_fri_fold": (_err, [_vp, _vp, _vp, _u32p]),
    "zkh_gather_sample": (_err, [_vp, _vp, _vp, _sz, _sz, _sz]),
    "zkh_scatter": (_err, [_vp, _vp, _u32p, _u32p, _u32p, _sz, _sz]),
    "zkh_prefix_products": (_err, [_vp, _vp]),
    "zkh_merkle_open": (_err, [_vp, _vp, _vp, _sz, _sz, _u32p, _sz, _vp]),
    "zkh_circuit_load": (_err, [_vp, _u32p, _sz, C.POINTER(_vp)]),
    "zkh_circuit_destroy": (None, [_vp]),
    "zkh_circuit_has_compiled_kernel": (_i, [_vp]),
    "zkh_circuit_attach_code_object": (_err, [_vp, C.c_char_p, _sz, C.c_char_p]),
    "zkh_circuit_attach_code_object_part": (_err, [_vp, C.c_char_p, _sz, C.c_char_p, _sz, _sz]),
    "zkh_circuit_compiled_parts": (_sz, [_vp]),
    "zkh_eval_check": (_err, [_vp, _vp, _vp, C.POINTER(_vp), _sz, C.POINTER(_vp), _sz, _u32p, _sz, _sz, _i]),
    "zkh_check_rows": (_err, [_vp, _vp, _sz, C.POINTER(_vp), _sz, _u32p, _u32p, _sz, _sz, _vp, C.POINTER(CheckRowsResult)]),
    "zkh_check_bus": (_err, [_vp, _vp, _sz, _sz, _vp, _vp, C.POINTER(BusTerm), _sz, C.POINTER(CheckBusResult)]),
    "zkh_syn_code": (_err, [_vp, _vp, _sz, _sz, _vp]),
    "zkh_sha256": (None, [C.c_char_p, _sz, C.POINTER(C.c_uint8)]),
    "zkh_session_check_termination": (_err, [_vp, C.POINTER(_u32p), C.POINTER(_sz), _sz, C.c_char_p, _sz]),
    "zkh_session_check_output": (_err, [_vp, C.POINTER(_u32p), C.POINTER(_sz), _sz, C.c_char_p, _sz, _u32p]),
    "zkh_assumptions_digest": (None, [_u32p, _u32p, _sz, _u32p]),
    "zkh_noise_cell_host": (_u32, [_u32p, _u32, _u32, _u32]),
    "zkh_chacha_block_host": (None, [_u32p, _u32p, _i, _u32p]),
    "zkh_syn_witgen": (_err, [_vp, _vp, _sz, _sz, _u64, _u32p, _u32p, _vp, _vp, _u32p]),
    "zkh_syn_accum": (_err, [_vp, _vp, _sz, _sz, _u32p, _vp, _u32p, _vp]),
    "zkh_circuit_set_arguments": (_err, [_vp, _u32p, _sz]),
    "zkh_circuit_has_arguments": (_i, [_vp]),
    "zkh_accumulate": (_err, [_vp, _vp, _sz, _sz, _u32p, _vp, _vp, _u32p, _vp]),
    "zkh_circuit_open_bus": (_i, [_vp, _u32p]),
    "zkh_accumulate_open": (_err, [_vp, _vp, _sz, _sz, _u32p, _vp, _vp, _u32p, _vp, _u32p]),
    "zkh_table_fingerprint": (_err, [_vp, _vp, _sz, _sz, _u32p, _u32p]),
    "zkh_circuit_derives_multiplicities": (_i, [_vp]),
    "zkh_derive_multiplicities": (_err, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "zkh_circuit_derives_sorted": (_i, [_vp]),
    "zkh_derive_sorted": (_err, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "zkh_circuit_derives_columns": (_i, [_vp]),
    "zkh_derive_columns": (_err, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "zkh_circuit_derives_links": (_i, [_vp]),
    "zkh_circuit_links_check_reads": (_i, [_vp]),
    "zkh_derive_links": (_err, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "zkh_derive_all": (_err, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "zkh_circuit_pages": (_i, [_vp]),
    "zkh_circuit_page_words": (_i, [_vp]),
    "zkh_circuit_page_flats": (_i, [_vp]),
    "zkh_derive_links_paged": (_err, [_vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "zkh_derive_all_paged": (_err, [_vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "zkh_derive_links_paged_table": (_err, [_vp, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _sz, _sz]),
    "zkh_derive_all_paged_table": (_err, [_vp, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _sz, _sz]),
    "zkh_page_out": (_err, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "zkh_image_tree_words": (_sz, [_sz]),
    "zkh_image_commit": (_err, [_vp, _vp, _vp]),
    "zkh_page_out_tree": (_err, [_vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "zkh_image_proof_words": (_sz, [_sz, _sz]),
    "zkh_page_out_proof": (_err, [_vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
    "zkh_image_proof_verify": (_err, [_u32p, _sz, _u32p, _u32p]),
    "zkh_image_proof_walk": (_err, [_vp, _vp, _sz, _u32p, _u32p]),
    "zkh_image_dirty_words": (_sz, [_sz, _sz]),
    "zkh_image_proof_nodes": (_err, [_vp, _vp, _sz, _u32p, _u32p, _vp]),
    "zkh_page_circuit_code": (_err, [_vp, _vp, _sz, _sz, _sz, _vp]),
    "zkh_page_circuit_witgen": (_err, [_vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _u32p, _u32p]),
    "zkh_page_circuit_witgen_part": (_err, [_vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _u32p, _u32p]),
    "zkh_page_circuit_slots": (_sz, [_sz, _sz, _sz]),
    "zkh_page_ordered_code": (_err, [_vp, _vp, _sz, _sz, _sz, _vp]),
    "zkh_page_ordered_witgen": (_err, [_vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _u32p, _u32p]),
    "zkh_page_tree_code": (_err, [_vp, _vp, _sz, _sz, _vp]),
    "zkh_page_tree_plan": (_err, [_sz, _sz, _sz, _u32p, _sz, C.POINTER(C.c_size_t), _sz, C.POINTER(C.c_size_t)]),
    "zkh_page_tree_plan_device": (_err, [_vp, _sz, _sz, _sz, _vp, _sz, _sz, C.POINTER(C.c_size_t), _sz, C.POINTER(C.c_size_t), _u32p]),
    "zkh_page_tree_witgen": (_err, [_vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _vp, _sz, _sz, _vp, _u32p, _u32p]),
    "zkh_page_tree_witgen_nodes": (_err, [_vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _sz, _sz, _vp, _u32p, _u32p]),
    "zkh_circuit_derived_data_columns": (_err, [_vp, _u32p, _sz, C.POINTER(_sz)]),
    "zkh_upload_data_trace": (_err, [_vp, _vp, _sz, _sz, _vp, _u32p, _i]),
    "zkh_ctx_h2d_bytes": (_sz, [_vp]),
    "zkh_syn_chain_contributions": (_err, [_vp, _vp, C.POINTER(_u64), _u32p, _sz, _sz, _u32p]),
    "zkh_syn_preflight_ram_words": (_sz, []),
    "zkh_syn_preflight": (_err, [_u64, _sz, _sz, _u32p, _u32p, C.POINTER(C.c_double)]),
    "zkh_syn_witgen_trace": (_err, [_vp, _vp, _sz, _sz, _u32p, _vp, _u32p, _vp, _vp, _u32p]),
    "zkh_poseidon2_mix": (_err, [_vp, _vp, _sz]),
    "zkh_poseidon2_mix_host": (_err, [_u32p, _u32p, _u32p, _sz]),
    "zkh_prover_create": (_err, [_vp, _vp, C.POINTER(_vp)]),
    "zkh_prover_destroy": (None, [_vp]),
    "zkh_prover_cache_code": (_err, [_vp, _sz, _vp]),
    "zkh_prover_drop_code_cache": (None, [_vp]),
    "zkh_prover_cached_code_root": (_err, [_vp, _sz, _u32p]),
    "zkh_prove_segment": (_err, [_vp, _sz, _sz, _u32p, _vp, _vp, _u32p, C.POINTER(_u32p), C.POINTER(_sz)]),
    "zkh_free_seal": (None, [_u32p]),
    "zkh_prove_begin": (_err, [_vp, _sz, _vp, _vp, _u32p, C.POINTER(_vp), _u32p]),
    "zkh_prove_finish": (_err, [_vp, _vp, C.POINTER(_u32p), C.POINTER(_sz)]),
    "zkh_prove_abort": (None, [_vp]),
    "zkh_code_root": (_err, [_vp, _vp, _sz, _u32p]),
    "zkh_data_root": (_err, [_vp, _sz, _vp, _u32p]),
    "zkh_commit_data": (_err, [_vp, _sz, _vp, C.POINTER(_vp)]),
    "zkh_commitment_root": (_err, [_vp, _u32p]),
    "zkh_commitment_bytes": (_sz, [_vp]),
    "zkh_commitment_release": (None, [_vp]),
    "zkh_prove_begin_held": (_err, [_vp, _sz, _vp, _vp, _u32p, C.POINTER(_vp), _u32p]),
    "zkh_syn_control_root": (_err, [_vp, _sz, _sz, _u32p]),
    "zkh_seal_data_root": (_err, [_vp, _u32p, _sz, _u32p]),
    "zkh_tie_challenge": (_err, [_u32p, _sz, _u32p]),
    "zkh_verify_segment": (_err, [_vp, _u32p, _sz, _u32p, _u32p, _u32p]),
    "zkh_receipt_claim": (_err, [_vp, _u32p, _sz, _u32p, _u32p, _u32p, _u32p]),
    "zkh_receipt_encode": (_err, [_vp, _u32p, _sz, _u32, _u32p, C.POINTER(_u32p), C.POINTER(_sz)]),
    "zkh_receipt_decode": (_err, [_vp, _u32p, _sz, _u32p, C.POINTER(_sz)]),
    "zkh_shipped_circuit_count": (_sz, []),
    "zkh_shipped_circuit_name": (C.c_char_p, [_sz]),
    "zkh_shipped_circuit_desc": (_err, [C.c_char_p, C.POINTER(_u32p), C.POINTER(_sz)]),
    "zkh_rec_build_program": (_err, [_u32, _u32p, _sz, _u32p, _u32p, _u32, C.POINTER(_u32p), C.POINTER(_sz)]),
    "zkh_rec_program_load": (_err, [_vp, _vp, _u32p, _sz, C.POINTER(_vp)]),
    "zkh_rec_program_destroy": (None, [_vp]),
    "zkh_rec_program_info": (_err, [_vp, _u32p, _u32p]),
    "zkh_rec_program_has_graph": (_i, [_vp]),
    "zkh_rec_code": (_err, [_vp, _vp]),
    "zkh_rec_witgen": (_err, [_vp, _u32p, _sz, _u32p, _vp, _u32p]),
    "zkh_rec_accum": (_err, [_vp, _u32p, _vp, _u32p, _vp]),
    "zkh_rec_prove": (_err, [_vp, _u32p, _sz, _u32p, _u32p, C.POINTER(_u32p), C.POINTER(_sz)]),
    "zkh_session_create": (_err, [C.POINTER(_i), _sz, _sz, _u32p, _sz, _u32p, _sz, C.POINTER(_vp)]),
    "zkh_session_destroy": (None, [_vp]),
    "zkh_session_lanes": (_sz, [_vp]),
    "zkh_session_circuit": (_vp, [_vp, _sz, _i]),
    "zkh_session_set_accumulate": (None, [_vp, _vp, _vp]),
    "zkh_session_set_resident_code": (None, [_vp, _i]),
    "zkh_session_set_streamed_fold": (None, [_vp, _i]),
    "zkh_session_set_witness_source": (_err, [_vp, _i, _sz]),
    "zkh_session_set_chained": (_err, [_vp, _i, _u32]),
    "zkh_session_set_journal": (_err, [_vp, C.c_char_p, _sz]),
    "zkh_session_set_recursion": (_err, [_vp, _u32p, _sz, C.POINTER(_u32p), C.POINTER(_sz), _u32p, _sz]),
    "zkh_succinct_verify": (_err, [_u32p, _sz, _u32p, _sz, _sz, _u32p, _sz, _sz]),
    "zkh_succinct_verify_resolved": (_err, [_u32p, _sz, _u32p, _sz, _sz, _u32p, _sz, _sz, _u32p, _sz]),
    "zkh_session_build_recursion": (_err, [_vp, _u32p, _sz, _i]),
    "zkh_session_set_assumptions": (_err, [_vp, _u32p, _sz, C.POINTER(_u32p), C.POINTER(_sz), _u32p, _u32p, _sz]),
    "zkh_session_prove": (_err, [_vp, C.POINTER(SegmentSpec), _sz, _i, _sz, _u32p, C.POINTER(ProveInfo)]),
    "zkh_prove_info_free": (None, [C.POINTER(ProveInfo)]),
    "zkh_session_verify": (_err, [_vp, C.POINTER(SegmentSpec), C.POINTER(ProveInfo), _sz]),
    "zkh_parse_cpulist": (_err, [C.c_char_p, C.POINTER(_i), _sz, C.POINTER(_sz)]),
    "zkh_pci_numa_cpus": (_err, [C.c_char_p, C.c_char_p, C.POINTER(_i), C.POINTER(_i), _sz, C.POINTER(_sz)]),
    "zkh_device_numa_node": (_err, [_i, C.POINTER(_i), C.c_char_p]),
    "zkh_device_identity": (_err, [_i, C.c_char_p, C.c_char_p, C.POINTER(_i), C.c_char_p, C.POINTER(_i)]),
    "zkh_bind_thread_to_device": (_err, [_i, _sz, _sz, C.POINTER(_i), C.POINTER(_sz)]),
    "zkh_prof_enable": (_err, [_vp, _i]),
    "zkh_prof_get": (_err, [_vp, C.POINTER(ProfRec), _sz, C.POINTER(_sz)]),
    "zkh_prof_reset": (_err, [_vp]),
}

_lib = None


class HalError(RuntimeError):
    pass


def load_library():
    """dlopen libzkhal_mi355x.so and bind every symbol of include/zkhal.h (fails loudly if anything is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HalError(f"{LIB_PATH} is missing: run `python -m zeth_amd.build` (no CPU fallback exists)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in ABI.items():
        fn = getattr(lib, name)      # AttributeError if the library does not export it
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _check(err):
    if err:
        lib = load_library()
        msg = C.cast(err, C.c_char_p).value.decode(errors="replace")
        lib.zkh_free_error(err)
        raise HalError(msg)


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint32)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(_u32p)


def image_proof_verify(proof, root_before) -> np.ndarray:
    """root_after from a ZKU1 proof (HipHal.page_out_proof) and root_before, on the host alone: no HipHal, no GPU
    (zkh_image_proof_verify; include/zkhal.h "THE UPDATE'S PROOF"; the numpy twin is logup.check_page_out_proof).  Raises HalError with
    one message per cause; nothing is returned then"""
    lib = load_library()
    words, before, after = _u32(proof).reshape(-1), _u32(root_before).reshape(-1), np.empty(DIGEST_WORDS, dtype=np.uint32)
    if before.size != DIGEST_WORDS:
        raise HalError(f"image_proof_verify: root_before of {before.size} words")
    _check(lib.zkh_image_proof_verify(_ptr(words), words.size, _ptr(before), _ptr(after)))
    return after


def tie_challenge(roots) -> np.ndarray:
    """alpha ‖ beta (8 Montgomery words) of a tied group from its data roots in order, the segment's first and then the parts', on the host
    alone (zkh_tie_challenge): the one function the prover and the verifier of a tied group both call"""
    lib = load_library()
    r, out = _u32(roots).reshape(-1), np.zeros(8, dtype=np.uint32)
    if not r.size or r.size % DIGEST_WORDS:
        raise HalError(f"tie_challenge: roots of {r.size} words (one or more digests of {DIGEST_WORDS})")
    _check(lib.zkh_tie_challenge(_ptr(r), r.size // DIGEST_WORDS, _ptr(out)))
    return out


class Buffer:
    """`hal::Buffer<T>`: size / slice / to_vec (view) / get_at."""

    def __init__(self, hal: "HipHal", handle):
        self.hal, self.h = hal, handle

    def release(self) -> None:
        """give the handle back now instead of when the object is collected; idempotent (the buffer is unusable afterwards)"""
        h, self.h = getattr(self, "h", None), None
        if h and _lib is not None and getattr(self.hal, "ctx", None):
            _lib.zkh_release(h)      # (a context that is already closed has freed its pool)

    __del__ = release

    def size(self) -> int:
        return _lib.zkh_size(self.h)

    def slice(self, offset: int, size: int) -> "Buffer":
        out = _vp()
        _check(_lib.zkh_slice(self.h, offset, size, C.byref(out)))
        return Buffer(self.hal, out)

    def to_vec(self) -> np.ndarray:
        out = np.empty(self.size(), dtype=np.uint32)
        _check(_lib.zkh_read(self.hal.ctx, self.h, _ptr(out), 0, out.size))
        return out

    def get_at(self, idx: int) -> int:
        out = np.empty(1, dtype=np.uint32)
        _check(_lib.zkh_read(self.hal.ctx, self.h, _ptr(out), idx, 1))
        return int(out[0])

    def write(self, host, offset: int = 0) -> None:
        a = _u32(host)
        _check(_lib.zkh_write(self.hal.ctx, self.h, _ptr(a), offset, a.size))

    def device_ptr(self) -> int:
        return _lib.zkh_device_ptr(self.h)


class Circuit:
    """A loaded circuit description (TapSet + PolyExtStep list) — the `CircuitHal` side."""

    def __init__(self, hal: "HipHal", desc):
        self.hal = hal
        self.desc = _u32(desc)
        h = _vp()
        _check(_lib.zkh_circuit_load(hal.ctx, _ptr(self.desc), self.desc.size, C.byref(h)))
        self.h = h

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h and _lib is not None:
            _lib.zkh_circuit_destroy(h)

    def has_compiled_kernel(self) -> bool:
        return bool(_lib.zkh_circuit_has_compiled_kernel(self.h))

    def kernel_kind(self) -> str:
        """'attached' (code object compiled at load time), 'builtin' (generated at build time) or 'interpreter'."""
        return ("interpreter", "builtin", "attached")[_lib.zkh_circuit_has_compiled_kernel(self.h)]

    def attach_code_object(self, image: bytes, kernel_name: str, part: int = 0, n_parts: int = 1) -> None:
        _check(_lib.zkh_circuit_attach_code_object_part(self.h, image, len(image), kernel_name.encode(), part, n_parts))

    def compiled_parts(self) -> int:
        return int(_lib.zkh_circuit_compiled_parts(self.h))

    def set_arguments(self, blob) -> None:
        """attach a ZKA1 argument blob (circuits/logup.py): zkh_accumulate then builds this circuit's accum group; None removes it"""
        self._args = _u32(blob) if blob is not None else np.zeros(0, np.uint32)
        _check(_lib.zkh_circuit_set_arguments(self.h, _ptr(self._args) if self._args.size else None, self._args.size))

    def has_arguments(self) -> bool:
        return bool(_lib.zkh_circuit_has_arguments(self.h))

    def derives_multiplicities(self) -> bool:
        """the arguments (ZKA1 version 2) have a term whose multiplicity the library derives (zkh_derive_multiplicities)"""
        return bool(_lib.zkh_circuit_derives_multiplicities(self.h))

    def derives_sorted(self) -> bool:
        """the arguments (ZKA1 version 3) have a term that is a sorted copy the library derives (zkh_derive_sorted)"""
        return bool(_lib.zkh_circuit_derives_sorted(self.h))

    def derives_columns(self) -> bool:
        """the arguments (ZKA1 version 4) hold derived-column records the library fills (zkh_derive_columns)"""
        return bool(_lib.zkh_circuit_derives_columns(self.h))

    def derives_links(self) -> bool:
        """the arguments (ZKA1 version 5) hold LINK records the library fills (zkh_derive_links)"""
        return bool(_lib.zkh_circuit_derives_links(self.h))

    def links_check_reads(self) -> int:
        """the LINK records with READS (ZKA1 version 6): zkh_derive_links refuses a load that does not return the last store"""
        return int(_lib.zkh_circuit_links_check_reads(self.h))

    def pages(self) -> bool:
        """the arguments (ZKA1 version 7) hold a PAGES record: the memory of its LINK starts from an image (derive_links_paged,
        derive_all_paged) and page_out writes it back; derive_links and derive_all refuse such a circuit"""
        return bool(_lib.zkh_circuit_pages(self.h))

    def page_words(self) -> int:
        """V, the value words per address of the paged memory (zkh_circuit_page_words): 0 without a PAGES record, else 1 or (ZKA1 version
        10, a LINK that carries two values) 2.  The image is then V W words, word j of address a at V a + j, and the page-out's table
        is the flat one of V D rows"""
        return int(_lib.zkh_circuit_page_words(self.h))

    def page_flats(self) -> int:
        """F, the flat-address destinations of the PAGES record (zkh_circuit_page_flats): 2 when the links stage writes p_flat_j = 2 a_i + j
        beside a wide page table (ZKA1 version 11), which is what the tie of a wide memory needs; else 0"""
        return int(_lib.zkh_circuit_page_flats(self.h))

    def open_bus(self) -> Optional[Tuple[int, int, int, int]]:
        """(the open tag, the `out` offsets of alpha, beta and the total) of arguments that are an OPEN bus (ZKA1 version 8), else None"""
        where = np.zeros(4, dtype=np.uint32)
        return tuple(int(x) for x in where) if _lib.zkh_circuit_open_bus(self.h, _ptr(where)) else None

    def derived_data_columns(self) -> List[int]:
        """the data columns the library's derives (sorted, columns, links, multiplicities) write on the active rows, ascending"""
        cols = np.zeros(max(1, int(self.desc[5])), dtype=np.uint32)
        n = C.c_size_t()
        _check(_lib.zkh_circuit_derived_data_columns(self.h, _ptr(cols), cols.size, C.byref(n)))
        return [int(x) for x in cols[: n.value]]

    def jit(self, use_cache: bool = True) -> None:
        """Generate + compile (hipcc --genco per part, in parallel, disk-cached) + attach the straight-line eval_check
        kernels for this desc."""
        from .circuits import jit as _jit
        objs = _jit.compile_code_objects(self.desc, use_cache=use_cache)
        for i, (image, name) in enumerate(objs):
            self.attach_code_object(image, name, i, len(objs))

    def eval_check(self, check: Buffer, groups: Sequence[Buffer], globals_: Sequence[Buffer], poly_mix, po2: int,
                   use_interpreter: bool = False) -> None:
        g = (_vp * len(groups))(*[b.h for b in groups])
        gl = (_vp * len(globals_))(*[b.h for b in globals_])
        pm = _u32(poly_mix)
        _check(_lib.zkh_eval_check(self.hal.ctx, self.h, check.h, g, len(groups), gl, len(globals_), _ptr(pm), po2,
                                   1 << po2, int(use_interpreter)))


class HostCircuit:
    """A circuit description loaded WITHOUT a GPU context: enough for `verify_segment` (upstream verifies on the CPU)."""

    def __init__(self, desc):
        load_library()
        self.desc = _u32(desc)
        h = _vp()
        _check(_lib.zkh_circuit_load(None, _ptr(self.desc), self.desc.size, C.byref(h)))
        self.h = h

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h and _lib is not None:
            _lib.zkh_circuit_destroy(h)

    def verify_segment(self, seal, control_root, rc=None, diag=None) -> None:
        """`Receipt::verify` for one segment seal: raises HalError (VerificationError analogue) if rejected.
        `control_root` (8 words) is the expected code commitment for (circuit, po2): required, like upstream's control ID."""
        s = _u32(seal)
        cr = _u32(control_root) if control_root is not None else None
        if cr is not None and cr.size != 8:
            raise HalError("verify_segment: control root must be 8 words")
        r = _ptr(_u32(rc)) if rc is not None else None
        d = _ptr(_u32(diag)) if diag is not None else None
        _check(_lib.zkh_verify_segment(self.h, _ptr(s), s.size, _ptr(cr) if cr is not None else None, r, d))


    def receipt_encode(self, seal, segment_index: int, control_root) -> np.ndarray:
        """Seal -> receipt container words (zkh_receipt_encode)."""
        s, cr = _u32(seal), _u32(control_root)
        if cr.size != 8:
            raise HalError("receipt_encode: control root must be 8 words")
        blob, n = _u32p(), _sz()
        _check(_lib.zkh_receipt_encode(self.h, _ptr(s), s.size, segment_index, _ptr(cr), C.byref(blob), C.byref(n)))
        out = np.ctypeslib.as_array(blob, shape=(n.value,)).copy()
        _lib.zkh_free_seal(blob)
        return out

    def receipt_decode(self, blob):
        """Container words -> (header dict, seal words); raises HalError on any integrity failure."""
        b = _u32(blob)
        info = np.zeros(26, dtype=np.uint32)
        off = _sz()
        _check(_lib.zkh_receipt_decode(self.h, _ptr(b), b.size, _ptr(info), C.byref(off)))
        hdr = {"version": int(info[1]), "circuit_hash": int(info[2]) | (int(info[3]) << 32), "po2": int(info[4]),
               "hashfn": "poseidon2", "placeholder_tables": bool(info[6] & 1),
               "tables": "placeholder" if info[6] & 1 else "derived" if info[6] & 2 else "upstream", "index": int(info[7]), "out_size": int(info[8]),
               "control_root": info[10:18].copy(), "claim": info[18:26].copy()}
        return hdr, b[off.value: off.value + int(info[9])].copy()

    def receipt_claim(self, seal, control_root, rc=None, diag=None) -> np.ndarray:
        """Claim digest (8 words) of a sealed segment: Poseidon2(out globals, po2, control root)."""
        s, cr = _u32(seal), _u32(control_root)
        if cr.size != 8:
            raise HalError("receipt_claim: control root must be 8 words")
        out = np.zeros(8, dtype=np.uint32)
        r = _ptr(_u32(rc)) if rc is not None else None
        d = _ptr(_u32(diag)) if diag is not None else None
        _check(_lib.zkh_receipt_claim(self.h, _ptr(s), s.size, _ptr(cr), r, d, _ptr(out)))
        return out

    def seal_data_root(self, seal) -> np.ndarray:
        """the root (8 words) of the data group a seal of this circuit commits to, folded from the top layer the seal carries as the
        verifier folds it (zkh_seal_data_root).  It proves nothing about a seal that has not been verified."""
        s, out = _u32(seal), np.zeros(8, dtype=np.uint32)
        _check(_lib.zkh_seal_data_root(self.h, _ptr(s), s.size, _ptr(out)))
        return out


class RecProgram:
    """A loaded RECURSION program (lift / join): zkh_rec_program_*.  `circuit` = the RECURSION description on the same HAL."""

    def __init__(self, hal: "HipHal", circuit: Circuit, blob):
        self.hal, self.circuit = hal, circuit
        b = _u32(blob)
        h = _vp()
        _check(_lib.zkh_rec_program_load(hal.ctx, circuit.h, _ptr(b), b.size, C.byref(h)))
        self.h = h
        root, info = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
        _check(_lib.zkh_rec_program_info(h, _ptr(root), _ptr(info)))
        self.root = root
        self.po2, self.zk_cycles, self.n_inputs, self.n_p2, self.n_gates, self.n_ops, self.n_levels, self.n_vars = (int(x) for x in info)
        self.graph_steps = int(_lib.zkh_rec_program_has_graph(h))       # > 0: the witness schedule is a hipGraph of that many plan steps

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        # a program holds device buffers and a prover (the resident code group): only released into a live context
        if h and _lib is not None and getattr(self.hal, "ctx", None):
            _lib.zkh_rec_program_destroy(h)

    def code(self, code: Buffer) -> None:
        _check(_lib.zkh_rec_code(self.h, code.h))

    def witgen(self, inputs, data: Buffer, noise_seed: int = 0x2E80) -> np.ndarray:
        i = _u32(inputs)
        out = np.zeros(16, np.uint32)
        _k, kp = _key_ptr(noise_seed)
        _check(_lib.zkh_rec_witgen(self.h, _ptr(i), i.size, kp, data.h, _ptr(out)))
        return out

    def accum(self, data: Buffer, mix_global, accum: Buffer, noise_seed: int = 0x2E80) -> None:
        m = _u32(mix_global)
        assert m.size == 20
        _k, kp = _key_ptr(noise_seed)
        _check(_lib.zkh_rec_accum(self.h, kp, data.h, _ptr(m), accum.h))

    def prove(self, inputs, noise_seed: int = 0x2E80):
        """-> (seal words, out globals): the witness exists only if the program's in-circuit verifier accepts `inputs`"""
        i = _u32(inputs)
        out = np.zeros(16, np.uint32)
        seal, n = _u32p(), _sz()
        _k, kp = _key_ptr(noise_seed)
        _check(_lib.zkh_rec_prove(self.h, _ptr(i), i.size, kp, _ptr(out), C.byref(seal), C.byref(n)))
        words = np.ctypeslib.as_array(seal, shape=(n.value,)).copy()
        _lib.zkh_free_seal(seal)
        return words, out


def syn_preflight(seed: int, po2: int, zk_cycles: int = ZK_CYCLES, records: Optional[np.ndarray] = None):
    """The sequential host machine (csrc/preflight.hip): -> (records: 4 words per active cycle, RAM image, CPU seconds).
    `records` may be a pinned view from HipHal.host_alloc (filled in place)."""
    load_library()
    A = (1 << po2) - zk_cycles
    rec = records if records is not None else np.empty(4 * A, dtype=np.uint32)
    assert rec.size == 4 * A and rec.dtype == np.uint32
    ram = np.empty(int(_lib.zkh_syn_preflight_ram_words()), dtype=np.uint32)
    secs = C.c_double(0.0)
    _check(_lib.zkh_syn_preflight(seed & (2**64 - 1), po2, zk_cycles, _ptr(rec), _ptr(ram), C.byref(secs)))
    return rec, ram, secs.value


# ---- host placement (csrc/topology.hip) ----
def parse_cpulist(text: str) -> List[int]:
    load_library()
    n = _sz()
    _check(_lib.zkh_parse_cpulist(text.encode(), None, 0, C.byref(n)))
    cpus = (_i * max(1, n.value))()
    _check(_lib.zkh_parse_cpulist(text.encode(), cpus, n.value, C.byref(n)))
    return list(cpus[: n.value])


def pci_numa_cpus(bdf: str, sysfs_root: str = "/sys"):
    """-> (NUMA node of the PCI function or -1, the node's CPU ids)"""
    load_library()
    node, n = _i(-1), _sz()
    cpus = (_i * 4096)()
    _check(_lib.zkh_pci_numa_cpus(sysfs_root.encode(), bdf.encode(), C.byref(node), cpus, 4096, C.byref(n)))
    return node.value, list(cpus[: min(n.value, 4096)])


def device_numa_node(device: int):
    """-> (NUMA node of the HIP device or -1, its PCI bus id)"""
    load_library()
    node = _i(-1)
    bdf = C.create_string_buffer(32)
    _check(_lib.zkh_device_numa_node(device, C.byref(node), bdf))
    return node.value, bdf.value.decode()


def device_identity(device: int) -> dict:
    """-> {"pci_bus_id", "uuid", "numa_node", "name", "visible_devices"} of a HIP device: what tells one GPU from another across
    processes (bench.py gathers it from every rank)"""
    load_library()
    bdf, uuid, name = C.create_string_buffer(32), C.create_string_buffer(40), C.create_string_buffer(64)
    node, count = _i(-1), _i(0)
    _check(_lib.zkh_device_identity(device, bdf, uuid, C.byref(node), name, C.byref(count)))
    return {"pci_bus_id": bdf.value.decode(), "uuid": uuid.value.decode(), "numa_node": node.value, "name": name.value.decode(),
            "visible_devices": count.value}


def bind_to_device(device: int, slot: int = 0, share: int = 1) -> dict:
    """Bind the calling thread (threads created afterwards inherit it) to the cores next to `device`: slice `slot` of `share`
    slices of its NUMA node when several ranks share the node.  -> {"numa_node": n or -1, "cpus": count}"""
    load_library()
    node, n = _i(-1), _sz()
    _check(_lib.zkh_bind_thread_to_device(device, slot, share, C.byref(node), C.byref(n)))
    return {"numa_node": node.value, "cpus": n.value}


def placement_slot(device: int, devices: Sequence[int]):
    """Which slice of its NUMA node the rank driving `device` takes when the ranks of `devices` share the host:
    -> (slot, share) = (index of `device` among the devices on the same node, their number); (0, 1) if the node is unknown."""
    mine = device_numa_node(device)[0]
    if mine < 0:
        return 0, 1
    same = [d for d in devices if device_numa_node(d)[0] == mine]
    return same.index(device), len(same)


def page_tree_plan(po2: int, zk_cycles: int, image_words: int, addrs) -> list:
    """the parts [(first, count), ...] of a page-out with the addresses `addrs` (host words, strictly increasing) as P2-TREE traces
    (zkh_page_tree_plan: host only, no GPU; the Python twin is circuits/p2_tree.py `parts`).  Raises HalError on W <= 16, on B < h and
    on addresses that do not increase below `image_words`"""
    load_library()
    addrs = np.ascontiguousarray(addrs, dtype=np.uint32).reshape(-1)
    cap = max(1, addrs.size)
    parts = (C.c_size_t * (2 * cap))()
    n = C.c_size_t()
    _check(_lib.zkh_page_tree_plan(po2, zk_cycles, image_words, _ptr(addrs), addrs.size, parts, cap, C.byref(n)))
    return [(int(parts[2 * p]), int(parts[2 * p + 1])) for p in range(n.value)]


def image_dirty_words(image_words: int, pages: int) -> int:
    """the bound on the words of the dirty-node table of a page-out of `pages` rows over an image of `image_words` words
    (zkh_image_dirty_words: host only, no GPU; the Python twin is logup.image_dirty_words): 4 + h + 33 sum_k min(D, L >> k)"""
    load_library()
    return int(_lib.zkh_image_dirty_words(image_words, pages))


class HipHal:
    """`impl Hal for HipHal` — one MI355X, one HIP stream, one driving thread."""

    def __init__(self, device: int = 0, hash_suite: str = "poseidon2"):
        load_library()
        ctx = _vp()
        _check(_lib.zkh_ctx_create(device, hash_suite.encode(), C.byref(ctx)))
        self.ctx = ctx
        self.device = device

    @staticmethod
    def version() -> str:
        return load_library().zkh_version().decode()

    def close(self):
        ctx, self.ctx = getattr(self, "ctx", None), None
        if ctx and _lib is not None:
            _lib.zkh_ctx_destroy(ctx)

    def __del__(self):
        # buffers hold a reference to the hal, so the context outlives them
        self.close()

    def memory(self) -> dict:
        """Bytes of device memory: held by live buffers, cached by the free list, live high-water mark."""
        live, cached, peak = _sz(), _sz(), _sz()
        _lib.zkh_ctx_memory(self.ctx, C.byref(live), C.byref(cached), C.byref(peak))
        return {"live": live.value, "cached": cached.value, "peak": peak.value}

    def trim(self) -> None:
        """Drain the stream and hand the cached blocks back to the driver."""
        _check(_lib.zkh_ctx_trim(self.ctx))

    def sync(self) -> None:
        _check(_lib.zkh_sync(self.ctx))

    # ---- allocation (alloc_elem / alloc_extelem / alloc_digest / alloc_u32 / copy_from_*) ----
    def alloc(self, name: str, n_words: int, zero: bool = False) -> Buffer:
        out = _vp()
        _check(_lib.zkh_alloc(self.ctx, name.encode(), n_words, int(zero), C.byref(out)))
        return Buffer(self, out)

    def alloc_elem(self, name: str, size: int) -> Buffer:
        return self.alloc(name, size)

    def alloc_extelem(self, name: str, size: int) -> Buffer:
        return self.alloc(name, size * EXT_SIZE)

    def alloc_digest(self, name: str, size: int) -> Buffer:
        return self.alloc(name, size * DIGEST_WORDS)

    def copy_from(self, name: str, host) -> Buffer:
        a = _u32(host).reshape(-1)
        out = _vp()
        _check(_lib.zkh_copy_from(self.ctx, name.encode(), _ptr(a), a.size, C.byref(out)))
        return Buffer(self, out)

    copy_from_elem = copy_from_extelem = copy_from_u32 = copy_from_digest = copy_from

    def host_alloc(self, n_words: int) -> np.ndarray:
        """Pinned host memory (a numpy view) for witnesses produced on the CPU; release with host_free."""
        p = _u32p()
        _check(_lib.zkh_host_alloc(self.ctx, n_words, C.byref(p)))
        return np.ctypeslib.as_array(p, shape=(n_words,))

    def host_free(self, arr: np.ndarray) -> None:
        _lib.zkh_host_free(self.ctx, arr.ctypes.data_as(_u32p))

    def write_async(self, buf: Buffer, pinned: np.ndarray, offset: int = 0) -> None:
        """Enqueue H2D from a host_alloc block on the context's stream (no host sync)."""
        _check(_lib.zkh_write_async(self.ctx, buf.h, pinned.ctypes.data_as(_u32p), offset, pinned.size))

    def wrap(self, device_ptr: int, n_words: int) -> Buffer:
        out = _vp()
        _check(_lib.zkh_wrap(self.ctx, device_ptr, n_words, C.byref(out)))
        return Buffer(self, out)

    # ---- trait Hal ----
    def batch_interpolate_ntt(self, io: Buffer, count: int) -> None:
        _check(_lib.zkh_batch_interpolate_ntt(self.ctx, io.h, count))

    def batch_expand_into_evaluate_ntt(self, out: Buffer, inp: Buffer, count: int, expand_bits: int) -> None:
        _check(_lib.zkh_batch_expand_into_evaluate_ntt(self.ctx, out.h, inp.h, count, expand_bits))

    def batch_bit_reverse(self, io: Buffer, count: int) -> None:
        _check(_lib.zkh_batch_bit_reverse(self.ctx, io.h, count))

    def zk_shift(self, io: Buffer, count: int) -> None:
        _check(_lib.zkh_zk_shift(self.ctx, io.h, count))

    def batch_interpolate_ntt_zk_shift(self, io: Buffer, count: int) -> None:
        _check(_lib.zkh_batch_interpolate_ntt_zk_shift(self.ctx, io.h, count))

    def batch_interpolate_ntt_from(self, out: Buffer, inp: Buffer, count: int, zk_shift: bool) -> None:
        _check(_lib.zkh_batch_interpolate_ntt_from(self.ctx, out.h, inp.h, count, int(zk_shift)))

    def hash_rows(self, output: Buffer, matrix: Buffer) -> None:
        _check(_lib.zkh_hash_rows(self.ctx, output.h, matrix.h))

    def hash_fold(self, io: Buffer, input_size: int, output_size: int) -> None:
        _check(_lib.zkh_hash_fold(self.ctx, io.h, input_size, output_size))

    def merkle_fold_all(self, nodes: Buffer, rows: int) -> None:
        _check(_lib.zkh_merkle_fold_all(self.ctx, nodes.h, rows))

    def merkle_build(self, nodes: Buffer, matrix: Buffer, rows: int) -> None:
        """`MerkleTreeProver::new`: leaves = hash_rows(matrix) at nodes[rows..2 rows), then every layer above."""
        _check(_lib.zkh_merkle_build(self.ctx, nodes.h, matrix.h, rows))

    def batch_evaluate_any(self, coeffs: Buffer, poly_count: int, which: Buffer, xs: Buffer, out: Buffer) -> None:
        _check(_lib.zkh_batch_evaluate_any(self.ctx, coeffs.h, poly_count, which.h, xs.h, out.h))

    def batch_evaluate_any_bitrev(self, coeffs: Buffer, poly_count: int, which: Buffer, xs: Buffer, out: Buffer) -> None:
        _check(_lib.zkh_batch_evaluate_any_bitrev(self.ctx, coeffs.h, poly_count, which.h, xs.h, out.h))

    def batch_bit_reverse_extelem(self, io: Buffer, count: int) -> None:
        _check(_lib.zkh_batch_bit_reverse_extelem(self.ctx, io.h, count))

    def mix_poly_coeffs(self, output: Buffer, mix_start, mix, inp: Buffer, combos: Buffer, input_size: int, count: int) -> None:
        ms, m = _u32(mix_start), _u32(mix)
        _check(_lib.zkh_mix_poly_coeffs(self.ctx, output.h, _ptr(ms), _ptr(m), inp.h, combos.h, input_size, count))

    def combos_prepare(self, combos: Buffer, pos, vals_ext) -> None:
        p, v = _u32(pos), _u32(vals_ext).reshape(-1)
        _check(_lib.zkh_combos_prepare(self.ctx, combos.h, _ptr(p), _ptr(v), p.size))

    def combos_prepare_regs(self, combos: Buffer, coeff_u: Buffer, combo_count: int, cycles: int, reg_sizes: Buffer,
                            reg_combo_ids: Buffer, mix) -> None:
        """`Hal::combos_prepare` with upstream's literal argument list (all operands on the device)."""
        m = _u32(mix)
        _check(_lib.zkh_combos_prepare_regs(self.ctx, combos.h, coeff_u.h, combo_count, cycles, reg_sizes.size(), reg_sizes.h,
                                            reg_combo_ids.h, _ptr(m)))

    def combos_divide(self, combos: Buffer, combo: int, cycles: int, pts_ext, rem_out: Buffer) -> None:
        p = _u32(pts_ext).reshape(-1)
        _check(_lib.zkh_combos_divide(self.ctx, combos.h, combo, cycles, _ptr(p), p.size // 4, rem_out.h))

    def combos_divide_all(self, combos: Buffer, cycles: int, pts_ext, pts_begin, rem_out: Buffer) -> None:
        p, b = _u32(pts_ext).reshape(-1), _u32(pts_begin)
        _check(_lib.zkh_combos_divide_all(self.ctx, combos.h, cycles, b.size - 1, _ptr(p), _ptr(b), rem_out.h))

    def eltwise_add_elem(self, out: Buffer, a: Buffer, b: Buffer) -> None:
        _check(_lib.zkh_eltwise_add_elem(self.ctx, out.h, a.h, b.h))

    def eltwise_copy_elem(self, out: Buffer, inp: Buffer) -> None:
        _check(_lib.zkh_eltwise_copy_elem(self.ctx, out.h, inp.h))

    def eltwise_zeroize_elem(self, io: Buffer) -> None:
        _check(_lib.zkh_eltwise_zeroize_elem(self.ctx, io.h))

    def reduce_elem(self, io: Buffer) -> None:
        """io[i] %= P in place (zkh_reduce_elem): a caller's trace of raw words becomes the reduced words that prove_begin takes"""
        _check(_lib.zkh_reduce_elem(self.ctx, io.h))

    def eltwise_sum_extelem(self, out: Buffer, inp: Buffer) -> None:
        _check(_lib.zkh_eltwise_sum_extelem(self.ctx, out.h, inp.h))

    def fri_fold(self, out: Buffer, inp: Buffer, mix) -> None:
        m = _u32(mix)
        _check(_lib.zkh_fri_fold(self.ctx, out.h, inp.h, _ptr(m)))

    def gather_sample(self, dst: Buffer, src: Buffer, idx: int, size: int, stride: int) -> None:
        _check(_lib.zkh_gather_sample(self.ctx, dst.h, src.h, idx, size, stride))

    def scatter(self, into: Buffer, index, offsets, values) -> None:
        i, o, v = _u32(index), _u32(offsets), _u32(values)
        _check(_lib.zkh_scatter(self.ctx, into.h, _ptr(i), _ptr(o), _ptr(v), o.size - 1, v.size))

    def prefix_products(self, io: Buffer) -> None:
        _check(_lib.zkh_prefix_products(self.ctx, io.h))

    def merkle_open(self, matrix: Buffer, nodes: Buffer, rows: int, cols: int, idx, out: Buffer) -> None:
        i = _u32(idx)
        _check(_lib.zkh_merkle_open(self.ctx, matrix.h, nodes.h, rows, cols, _ptr(i), i.size, out.h))

    def poseidon2_mix(self, states: "Buffer") -> None:
        """The bare permutation on `states.size() // 24` states (24 Montgomery words each), in place."""
        _check(_lib.zkh_poseidon2_mix(self.ctx, states.h, states.size() // 24))

    def poseidon2_set_constants(self, rc, diag) -> None:
        r, d = _u32(rc), _u32(diag)
        assert r.size == 24 * 29 and d.size == 24
        _check(_lib.zkh_poseidon2_set_constants(self.ctx, _ptr(r), _ptr(d)))

    # ---- circuit + SYN witness ----
    def load_circuit(self, desc, jit: Optional[bool] = None) -> Circuit:
        """CircuitHal for a description blob.  jit=None (default): a desc without a built-in eval_check kernel gets one
        compiled at load time when hipcc is on the machine, and runs on the step interpreter otherwise; jit=True:
        always compile (raises if that is impossible); jit=False: never."""
        c = Circuit(self, desc)
        if jit or (jit is None and not c.has_compiled_kernel()):
            from .circuits import jit as _jit
            if jit or _jit.hipcc_path() is not None:
                c.jit()
        return c

    def syn_code(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer) -> None:
        _check(_lib.zkh_syn_code(self.ctx, circuit.h, po2, zk_cycles, code.h))

    def syn_witgen(self, circuit: Circuit, po2: int, zk_cycles: int, seed: int, noise_seed: int, code: Buffer, data: Buffer,
                   pub=None) -> np.ndarray:
        """-> out globals.  `code` may be None for kinds 1 / 2 (the code group of this size is already held, e.g. resident).
        SYN-AIR (kind 1): OUTPUT_SIZE words s, 0, 0, 0, then the public input words `pub`.
        KECCAK-F (kind 2): `pub` = optional input state of the LAST permutation (25 lanes = 50 words, low word first);
        out = that permutation's output state as 100 16-bit limbs."""
        out_size = int(circuit.desc[7])
        out = np.zeros(out_size, dtype=np.uint32)
        p = _u32(pub) if pub is not None else np.zeros(0, np.uint32)
        if int(circuit.desc[13]) == 2:
            if p.size not in (0, 50):
                raise HalError(f"syn_witgen: KECCAK-F takes an optional 50-word input state, got {p.size} words")
        elif int(circuit.desc[13]) == 3:
            if p.size != 16:
                raise HalError(f"syn_witgen: P2-JOIN takes the two child claims (16 words), got {p.size}")
        elif p.size != out_size - 4:
            raise HalError(f"syn_witgen: circuit takes {out_size - 4} public input words, got {p.size}")
        _k, kp = _key_ptr(noise_seed)
        _check(_lib.zkh_syn_witgen(self.ctx, circuit.h, po2, zk_cycles, seed & (2**64 - 1), kp,
                                   _ptr(p) if p.size else None, code.h if code is not None else None, data.h, _ptr(out)))
        return out

    def syn_witgen_trace(self, circuit: Circuit, po2: int, zk_cycles: int, noise_seed: int, records: Buffer, ram_image, code: Optional[Buffer],
                         data: Buffer) -> np.ndarray:
        """records (device, 4 words per active cycle) + the RAM image -> code (None: already held), data; returns the out globals"""
        out = np.zeros(int(circuit.desc[7]), dtype=np.uint32)
        ram = _u32(ram_image) if ram_image is not None else None
        _k, kp = _key_ptr(noise_seed)
        _check(_lib.zkh_syn_witgen_trace(self.ctx, circuit.h, po2, zk_cycles, kp, records.h, _ptr(ram) if ram is not None else None,
                                         code.h if code is not None else None, data.h, _ptr(out)))
        return out

    def syn_accum(self, circuit: Circuit, po2: int, zk_cycles: int, noise_seed: int, data: Buffer, mix_global, accum: Buffer) -> None:
        m = _u32(mix_global)
        _k, kp = _key_ptr(noise_seed)
        _check(_lib.zkh_syn_accum(self.ctx, circuit.h, po2, zk_cycles, kp, data.h, _ptr(m), accum.h))

    def accumulate(self, circuit: Circuit, po2: int, zk_cycles: int, noise_seed: int, code: Buffer, data: Buffer, mix_global,
                   accum: Buffer) -> None:
        """CircuitHal::accumulate for a circuit with arguments (zkh_accumulate): raises HalError if a denominator vanishes or the bus
        does not balance (the accum is then left zeroed)"""
        m = _u32(mix_global)
        _k, kp = _key_ptr(noise_seed)
        _check(_lib.zkh_accumulate(self.ctx, circuit.h, po2, zk_cycles, kp, code.h, data.h, _ptr(m), accum.h))

    def accumulate_open(self, circuit: Circuit, po2: int, zk_cycles: int, noise_seed: int, code: Buffer, data: Buffer, challenge,
                        accum: Buffer) -> np.ndarray:
        """accumulate for a circuit whose arguments are an OPEN bus (zkh_accumulate_open; ZKA1 version 8): challenge = alpha ‖ beta (8
        reduced Montgomery words) where the mix globals were -> the bus total, 4 Montgomery words, which the seal states in `out`.
        Raises HalError if a denominator vanishes (the accum is then left zeroed), or on a closed blob"""
        ch, total = _u32(challenge), np.zeros(4, dtype=np.uint32)
        if ch.size != 8:
            raise HalError(f"accumulate_open: a challenge of {ch.size} words (alpha and beta: 8)")
        _k, kp = _key_ptr(noise_seed)
        _check(_lib.zkh_accumulate_open(self.ctx, circuit.h, po2, zk_cycles, kp, code.h, data.h, _ptr(ch), accum.h, _ptr(total)))
        return total

    def table_fingerprint(self, table: Buffer, table_at: int, rows: int, challenge) -> np.ndarray:
        """the fingerprint (4 Montgomery words) of the `rows` table rows (address, in, out) at word `table_at` of `table`, where
        zkh_page_out_proof left them (word 5 + h of the proof), under challenge = alpha ‖ beta (zkh_table_fingerprint; host twin:
        circuits/logup.py table_fingerprint): what a tied segment's open total must be.  Raises HalError, naming the lowest row, if a
        denominator vanishes"""
        ch, total = _u32(challenge), np.zeros(4, dtype=np.uint32)
        if ch.size != 8:
            raise HalError(f"table_fingerprint: a challenge of {ch.size} words (alpha and beta: 8)")
        _check(_lib.zkh_table_fingerprint(self.ctx, table.h, table_at, rows, _ptr(ch), _ptr(total)))
        return total

    def derive_all(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, data: Buffer) -> None:
        """fill everything the circuit's arguments derive into `data`, the stages in their order (zkh_derive_all); nothing to derive:
        nothing done.  Raises the HalError of the first stage that refuses; the stages before it have written their columns"""
        _check(_lib.zkh_derive_all(self.ctx, circuit.h, po2, zk_cycles, code.h, data.h))

    def derive_all_paged(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, data: Buffer, image: Optional[Buffer]) -> None:
        """derive_all with the memory image (a Buffer of W raw Montgomery words, or None) that the links stage of a paging circuit reads
        (zkh_derive_all_paged); a paging circuit without an image is refused before any stage writes"""
        _check(_lib.zkh_derive_all_paged(self.ctx, circuit.h, po2, zk_cycles, code.h, data.h, None if image is None else image.h))

    def derive_links_paged(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, data: Buffer, image: Optional[Buffer]) -> None:
        """derive_links from a memory image (zkh_derive_links_paged): an unlinked access of the paged LINK record (with ZKA1 version 9: of any
        port of the paged memory) takes image[address] as
        its previous access, and the PAGES record's page table is written.  Raises HalError as derive_links does, and on an address
        outside the image, a clock 0 and an unlinked load that does not return the image's word (`data` is then unchanged).  Without a
        PAGES record the image is ignored"""
        _check(_lib.zkh_derive_links_paged(self.ctx, circuit.h, po2, zk_cycles, code.h, data.h, None if image is None else image.h))

    def _page_table(self, who: str, table, table_at: int, D: Optional[int], image_words: int):
        """the page-table operands of the `_table` derives -> (Buffer or None, table_at, D): a Buffer with `table_at` and `D`, or a (D, 3) array
        of rows (address, in, out), which is uploaded; None (a circuit without a PAGES record ignores the table) passes NULL"""
        if table is None:
            return None, 0, 0
        if not isinstance(table, Buffer):
            rows = _u32(table)
            if rows.ndim != 2 or rows.shape[1] != 3:
                raise HalError(f"{who}: a page table of shape {rows.shape} (rows of 3 words: address, in, out)")
            if D is not None and D != rows.shape[0] or table_at:
                raise HalError(f"{who}: a page table given as rows is uploaded whole: table_at {table_at} and D {D} go with a Buffer")
            table, D = self.copy_from("page_table", rows) if rows.size else self.alloc("page_table", 1), rows.shape[0]
        if D is None:
            raise HalError(f"{who}: a page table in a Buffer needs its rows (D)")
        if min(table_at, D, image_words) < 0:
            raise HalError(f"{who}: negative argument (table_at {table_at}, D {D}, image_words {image_words})")
        return table, table_at, D

    def derive_links_paged_table(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, data: Buffer, table, image_words: int,
                                 table_at: int = 0, D: Optional[int] = None) -> None:
        """derive_links_paged from the page table of a ZKU1 proof in place of the image (zkh_derive_links_paged_table): row i of the table
        is (a_i, in_i, out_i), and in_i stands for image[a_i].  table: a Buffer that holds D rows of 3 words from word `table_at` (a
        proof: table_at = 5 + h), or a (D, 3) array, which is uploaded; image_words: W.  The result is derive_links_paged's on the image
        the table was made from, cell for cell as residues.  Raises HalError as derive_links_paged does, and when the table's rows are
        not the trace's pages (`data` is then unchanged).  Without a PAGES record the table is ignored.  A circuit whose page_words() is
        2 takes the FLAT table: two rows (2 a + j, in_j, out_j) per page, D its flat rows, image_words the flat image's words"""
        buf, at, rows = self._page_table("derive_links_paged_table", table, table_at, D, image_words)
        _check(_lib.zkh_derive_links_paged_table(self.ctx, circuit.h, po2, zk_cycles, code.h, data.h, None if buf is None else buf.h, at, rows, image_words))

    def derive_all_paged_table(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, data: Buffer, table, image_words: int,
                               table_at: int = 0, D: Optional[int] = None) -> None:
        """derive_all_paged with the page table of a ZKU1 proof where the links stage gets the image (zkh_derive_all_paged_table); the
        operands are derive_links_paged_table's"""
        buf, at, rows = self._page_table("derive_all_paged_table", table, table_at, D, image_words)
        _check(_lib.zkh_derive_all_paged_table(self.ctx, circuit.h, po2, zk_cycles, code.h, data.h, None if buf is None else buf.h, at, rows, image_words))

    def page_out(self, circuit: Circuit, po2: int, zk_cycles: int, data: Buffer, image: Buffer) -> None:
        """write the page table of `data` back into `image`: image[p_addr] = p_out on every active row with p_on = 1 (zkh_page_out).
        Raises HalError, with the image unchanged, on a p_on other than 0 / 1, an address outside the image, or page addresses that
        do not strictly increase over a prefix of rows"""
        _check(_lib.zkh_page_out(self.ctx, circuit.h, po2, zk_cycles, data.h, image.h))

    def image_tree_words(self, image_words: int) -> int:
        """the words of the committed tree of an image of `image_words` words: 16 L, L the smallest power of two >= ceil(W / 8); 0 for 0
        (zkh_image_tree_words; the commitment: `logup.reference_image_tree`)"""
        return int(_lib.zkh_image_tree_words(image_words))

    def image_commit(self, image: Buffer, nodes: Optional[Buffer] = None) -> Buffer:
        """the committed tree of `image` (a Buffer of W raw Montgomery words), built on the device (zkh_image_commit): 2 L digests in heap
        order, the leaves the image's residues eight at a time, zero-padded, every node above hash_pair of its two children; the root is
        digest 1 (`image_root`).  nodes: a Buffer of image_tree_words(W) words to build it in (default: a new one).  Raises HalError on
        an empty image and on a `nodes` of another size"""
        if nodes is None:
            nodes = self.alloc("image_nodes", self.image_tree_words(image.size()) or 16)
        _check(_lib.zkh_image_commit(self.ctx, image.h, nodes.h))
        return nodes

    def page_out_tree(self, circuit: Circuit, po2: int, zk_cycles: int, data: Buffer, image: Buffer, nodes: Buffer) -> None:
        """page_out, and `nodes` (the committed tree of `image` before the call) brought up to the new image by hashing only the paths
        of the paged words again (zkh_page_out_tree): afterwards `nodes` is, word for word, what image_commit gives for the new image.
        Raises HalError as page_out does, and on a `nodes` that is not image_tree_words(W) words; image and nodes are then unchanged"""
        _check(_lib.zkh_page_out_tree(self.ctx, circuit.h, po2, zk_cycles, data.h, image.h, nodes.h))

    def image_proof_words(self, image_words: int, pages: int) -> int:
        """the bound on the words of a ZKU1 proof of `pages` pages over an image of `image_words` words (zkh_image_proof_words)"""
        return int(_lib.zkh_image_proof_words(image_words, pages))

    def page_out_proof(self, circuit: Circuit, po2: int, zk_cycles: int, data: Buffer, image: Buffer, nodes: Buffer, proof: Optional[Buffer] = None) -> np.ndarray:
        """the ZKU1 proof of the page-out of `data`'s page table (zkh_page_out_proof; include/zkhal.h "THE UPDATE'S PROOF"): what takes a
        holder of the root of `nodes` to the root after the page-out (`image_proof_verify`).  Only reads data, image and nodes, `nodes`
        the committed tree of `image` as it is: call it before page_out_tree.  proof: a Buffer to build it in (default: a new one of
        image_proof_words(W, the active rows) words).  Returns exactly the proof's words.  Raises HalError as page_out does, when a
        p_in is not the word the tree holds, and on a `nodes` or `proof` of the wrong size"""
        if proof is None:
            proof = self.alloc("image_proof", self.image_proof_words(image.size(), max(1, circuit.page_words()) * ((1 << po2) - zk_cycles)))
        _check(_lib.zkh_page_out_proof(self.ctx, circuit.h, po2, zk_cycles, data.h, image.h, nodes.h, proof.h))
        h = proof.get_at(4)
        header = proof.slice(0, 5 + h).to_vec()
        words = 5 + h + 3 * int(header[2]) + 8 * int(header[3]) + 8 * int(header[5:].astype(np.uint64).sum())
        return proof.slice(0, words).to_vec()

    def image_proof_walk(self, proof, root_before, words: Optional[int] = None) -> np.ndarray:
        """root_after from a ZKU1 proof and root_before, walked on the device (zkh_image_proof_walk): the same verdict, root and message
        (after "image_proof_walk: ") as `image_proof_verify` gives on the host.  proof: a Buffer whose first `words` words are the proof
        (default: all of it; the buffer page_out_proof built in goes in with the proof's own length), or an array, which is uploaded.
        The buffer is only read.  Raises HalError with one message per cause; nothing is returned then"""
        before, after = _u32(root_before).reshape(-1), np.empty(DIGEST_WORDS, dtype=np.uint32)
        if before.size != DIGEST_WORDS:
            raise HalError(f"image_proof_walk: root_before of {before.size} words")
        if not isinstance(proof, Buffer):
            host = _u32(proof).reshape(-1)
            proof = self.alloc("image_proof", max(host.size, 1))
            if host.size:
                _check(_lib.zkh_write(self.ctx, proof.h, _ptr(host), 0, host.size))
            if words is None:
                words = host.size
        if words is None:
            words = proof.size()
        _check(_lib.zkh_image_proof_walk(self.ctx, proof.h, words, _ptr(before), _ptr(after)))
        return after

    def image_dirty_words(self, image_words: int, pages: int) -> int:
        """the module's image_dirty_words (host only: it needs no context)"""
        return image_dirty_words(image_words, pages)

    def image_proof_nodes(self, proof, root_before, words: Optional[int] = None, dirty: Optional[Buffer] = None):
        """image_proof_walk that keeps what it recomputes (zkh_image_proof_nodes) -> (root_after, dirty): `dirty` is a Buffer that
        starts with the DIRTY-NODE TABLE of the page-out (include/zkhal.h "THE UPDATE'S PROOF"; the numpy twin:
        logup.reference_page_out_nodes), what page_tree_witgen_nodes reads in place of the two trees.  proof, root_before, words:
        image_proof_walk's.  dirty: a Buffer of at least image_dirty_words(W, D) words to write (default: a new one of that size); it
        is written only on success.  Raises HalError with the walk's message per cause after "image_proof_nodes: ", and on D = 0"""
        before, after = _u32(root_before).reshape(-1), np.empty(DIGEST_WORDS, dtype=np.uint32)
        if before.size != DIGEST_WORDS:
            raise HalError(f"image_proof_nodes: root_before of {before.size} words")
        if not isinstance(proof, Buffer):
            proof = self.copy_from("image_proof", _u32(proof).reshape(-1))
        if words is None:
            words = proof.size()
        if dirty is None:
            head = proof.slice(0, 3).to_vec() if min(words, proof.size()) >= 3 else np.zeros(3, dtype=np.uint32)
            bound = image_dirty_words(int(head[1]), int(head[2]))
            dirty = self.alloc("image_dirty", bound if 0 < bound < 1 << 32 else 1)   # a bound past 32 bits, or a header that lies: the call refuses
        _check(_lib.zkh_image_proof_nodes(self.ctx, proof.h, words, _ptr(before), _ptr(after), dirty.h))
        return after, dirty

    def image_root(self, nodes: Buffer) -> np.ndarray:
        """the root of a committed tree: digest 1 of `nodes`, 8 words"""
        out = np.empty(DIGEST_WORDS, dtype=np.uint32)
        _check(_lib.zkh_read(self.ctx, nodes.h, _ptr(out), DIGEST_WORDS, DIGEST_WORDS))
        return out

    def _page_code(self, fn, circuit: Circuit, po2: int, code: Optional[Buffer], *shape) -> Buffer:
        """a page-out circuit's code call `fn` over (po2, *shape) into `code`, or into a new buffer of the circuit's code columns"""
        if code is None:
            code = self.alloc_elem("code", int(circuit.desc[4]) << po2)
        _check(fn(self.ctx, circuit.h, po2, *shape, code.h))
        return code

    def _page_witgen(self, fn, out_words: int, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, proof: Buffer, proof_words: int, nodes_before: Buffer,
                     nodes_after: Buffer, part: tuple, data: Buffer, noise_seed: int) -> np.ndarray:
        """a page-out circuit's witness call `fn` for the part `part` (the call's own operands: none, first, or first and count) -> its
        `out_words` out globals"""
        out = np.zeros(out_words, dtype=np.uint32)
        _k, kp = _key_ptr(noise_seed)
        _check(fn(self.ctx, circuit.h, po2, zk_cycles, code.h, proof.h, proof_words, nodes_before.h, nodes_after.h, *part, data.h, _ptr(out), kp))
        return out

    def page_circuit_code(self, circuit: Circuit, po2: int, zk_cycles: int, image_words: int, code: Optional[Buffer] = None) -> Buffer:
        """the code group of P2-PAGE (circuits/p2_page.py) for (po2, zk_cycles, the tree height of an image of `image_words` words)
        (zkh_page_circuit_code; the host twin: p2_page.reference_page_code).  code: a Buffer of 39 x 2^po2 words to write (default: a
        new one).  Raises HalError on a circuit of another shape, W <= 8, h > 27 and a trace without room for one path"""
        return self._page_code(_lib.zkh_page_circuit_code, circuit, po2, code, zk_cycles, image_words)

    def page_circuit_witgen(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, proof: Buffer, proof_words: int, nodes_before: Buffer,
                            nodes_after: Buffer, data: Buffer, noise_seed: int) -> np.ndarray:
        """the data group of P2-PAGE for the page-out a ZKU1 proof describes (zkh_page_circuit_witgen; the host twin:
        p2_page.reference_page_trace) -> the out globals, root_before ‖ root_after (16 words).  proof: a Buffer whose first
        `proof_words` words are the proof (only its header and table are read); nodes_before / nodes_after: the committed tree before
        and after page_out_tree; code: page_circuit_code of the same (po2, zk_cycles, image size).  Raises HalError with one message
        per cause (include/zkhal.h "P2-PAGE"); `data` is unspecified then"""
        return self._page_witgen(_lib.zkh_page_circuit_witgen, 2 * DIGEST_WORDS, circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, (), data, noise_seed)

    def page_circuit_slots(self, po2: int, zk_cycles: int, image_words: int) -> int:
        """N, the path slots of a P2-PAGE trace of 2^po2 rows over an image of `image_words` words, 0 where page_circuit_code refuses the
        shape (zkh_page_circuit_slots: host only; the Python twin is p2_page.slots, the plan of the parts p2_page.parts)"""
        return int(_lib.zkh_page_circuit_slots(po2, zk_cycles, image_words))

    def page_circuit_witgen_part(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, proof: Buffer, proof_words: int, nodes_before: Buffer,
                                 nodes_after: Buffer, first: int, data: Buffer, noise_seed: int) -> np.ndarray:
        """the data group of P2-PAGE for ONE PART of the page-out a ZKU1 proof describes: the updates [first, first + min(N, D - first)) of
        its table (zkh_page_circuit_witgen_part; the host twin: p2_page.reference_page_part) -> the out globals, the root before
        update `first` ‖ the root after the part's last update (16 words).  Every other operand is page_circuit_witgen's, and both trees
        are the whole page-out's whichever part is laid out.  A table of any size is refused only for first >= D (first = D = 0 is
        the empty table's one part); the other refusals are page_circuit_witgen's after "page_circuit_witgen_part: " """
        return self._page_witgen(_lib.zkh_page_circuit_witgen_part, 2 * DIGEST_WORDS, circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, (first,), data, noise_seed)

    def page_ordered_code(self, circuit: Circuit, po2: int, zk_cycles: int, image_words: int, code: Optional[Buffer] = None) -> Buffer:
        """the code group of P2-PAGE-ordered (circuits/p2_page_ordered.py) for (po2, zk_cycles, the tree height of an image of
        `image_words` words) (zkh_page_ordered_code; the host twin: p2_page_ordered.reference_ordered_code).  code: a Buffer of 42 x
        2^po2 words to write (default: a new one).  Raises HalError as page_circuit_code does, and on h > 26"""
        return self._page_code(_lib.zkh_page_ordered_code, circuit, po2, code, zk_cycles, image_words)

    def page_ordered_witgen(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, proof: Buffer, proof_words: int, nodes_before: Buffer,
                            nodes_after: Buffer, first: int, data: Buffer, noise_seed: int) -> np.ndarray:
        """the data group of P2-PAGE-ordered for the part at `first` of the page-out a ZKU1 proof describes (zkh_page_ordered_witgen;
        the host twin: p2_page_ordered.reference_ordered_part) -> the out globals, root_before ‖ root_after ‖ lo ‖ hi (18 words: lo
        and hi as the trace holds them, p2_page_ordered.decode).  The operands are page_circuit_witgen_part's, `data` of 129 x 2^po2
        words; first = 0 with D <= N is the single-seal case.  Raises HalError with one message per cause (include/zkhal.h
        "P2-PAGE-ordered"); `data` is unspecified then"""
        return self._page_witgen(_lib.zkh_page_ordered_witgen, 2 * DIGEST_WORDS + 2, circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, (first,), data, noise_seed)

    def page_tree_code(self, circuit: Circuit, po2: int, zk_cycles: int, code: Optional[Buffer] = None) -> Buffer:
        """the code group of P2-TREE (circuits/p2_tree.py) and of P2-TREE-tied (circuits/p2_tree_tied.py: the same words) for (po2,
        zk_cycles): it does not depend on the image (zkh_page_tree_code; the host twin: p2_tree.reference_tree_code).  code: a Buffer of
        41 x 2^po2 words to write (default: a new one)"""
        return self._page_code(_lib.zkh_page_tree_code, circuit, po2, code, zk_cycles)

    def page_tree_plan(self, po2: int, zk_cycles: int, image_words: int, addrs) -> list:
        """the module's page_tree_plan (host only: it needs no context)"""
        return page_tree_plan(po2, zk_cycles, image_words, addrs)

    def page_tree_plan_device(self, po2: int, zk_cycles: int, image_words: int, table: Buffer, table_at: int, D: int, nodes: bool = False):
        """page_tree_plan over a table that lies on the device (zkh_page_tree_plan_device; the numpy twin is p2_tree.parts_by_scan): the
        words of `table` from `table_at` on are D rows of a ZKU1 table (stride 3, the address first; for a proof table_at = 5 + h).
        -> the parts [(first, count), ...]; with nodes=True (plan, the dirty nodes of every part: p2_tree.part_nodes).  Nothing per row
        comes back to the host.  Raises HalError as page_tree_plan does on the shape, on rows that do not fit the buffer, and with the
        witness generator's message for the lowest row whose address does not follow a smaller one below `image_words`"""
        who = "page_tree_plan_device"
        if not isinstance(table, Buffer):
            raise HalError(f"{who}: the table is a {type(table).__name__}, not a device Buffer (a host array is page_tree_plan's)")
        if min(po2, zk_cycles, image_words, table_at, D) < 0:
            raise HalError(f"{who}: negative argument (po2 {po2}, zk_cycles {zk_cycles}, image_words {image_words}, table_at {table_at}, D {D})")
        cap = max(1, D)
        parts, n, counts = (C.c_size_t * (2 * cap))(), C.c_size_t(), np.zeros(cap if nodes else 0, dtype=np.uint32)
        _check(_lib.zkh_page_tree_plan_device(self.ctx, po2, zk_cycles, image_words, table.h, table_at, D, parts, cap, C.byref(n), _ptr(counts) if nodes else None))
        plan = [(int(parts[2 * p]), int(parts[2 * p + 1])) for p in range(n.value)]
        return (plan, [int(c) for c in counts[:n.value]]) if nodes else plan

    def page_tree_witgen(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, proof: Buffer, proof_words: int, nodes_before: Buffer,
                         nodes_after: Buffer, first: int, count: int, data: Buffer, noise_seed: int) -> np.ndarray:
        """the data group of P2-TREE for the part [first, first + count) of the page-out a ZKU1 proof describes (zkh_page_tree_witgen; the
        host twin: p2_tree.reference_tree_part) -> the out globals, root_before ‖ root_after ‖ lo ‖ hi (18 words: lo and hi bound the
        heap ids of the part's pair blocks, p2_tree.decode).  The other operands are page_ordered_witgen's, `data` of 106 x 2^po2
        words, both trees the whole page-out's; the part is one of page_tree_plan's.  A P2-TREE-tied circuit (kind 9) gets its 138
        columns (the host twin: p2_tree_tied.reference_tree_tied_part) and the same 18 words.  Raises HalError with one message per cause
        (include/zkhal.h "P2-TREE"); `data` is unspecified then"""
        return self._page_witgen(_lib.zkh_page_tree_witgen, 2 * DIGEST_WORDS + 2, circuit, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, (first, count), data, noise_seed)

    def page_tree_witgen_nodes(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, proof: Buffer, proof_words: int, dirty: Buffer, first: int, count: int,
                               data: Buffer, noise_seed: int) -> np.ndarray:
        """page_tree_witgen from (proof, dirty) alone (zkh_page_tree_witgen_nodes): `dirty`, the table image_proof_nodes left, stands
        in place of the two trees; the same cells and the same 18 words, for kinds 7 and 9.  Raises HalError as page_tree_witgen does,
        on a table whose header does not fit its buffer or the proof, and with "node N of layer K is not in the dirty nodes" on a table
        of another proof (include/zkhal.h "P2-TREE")"""
        out = np.zeros(2 * DIGEST_WORDS + 2, dtype=np.uint32)
        _k, kp = _key_ptr(noise_seed)
        _check(_lib.zkh_page_tree_witgen_nodes(self.ctx, circuit.h, po2, zk_cycles, code.h, proof.h, proof_words, dirty.h, first, count, data.h, _ptr(out), kp))
        return out

    def derive_multiplicities(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, data: Buffer) -> None:
        """fill the derived multiplicity columns of `data` on the active rows (zkh_derive_multiplicities): raises HalError on a table
        selector other than 0 / 1 or a lookup without a table entry (`data` is then unchanged)"""
        _check(_lib.zkh_derive_multiplicities(self.ctx, circuit.h, po2, zk_cycles, code.h, data.h))

    def derive_columns(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, data: Buffer) -> None:
        """fill the destination columns of the derived-column records of `data` on the active rows (zkh_derive_columns): raises
        HalError on a value that does not fit its limbs or on keys that are not in order, naming the lowest (record, row) (`data` is
        then unchanged)"""
        _check(_lib.zkh_derive_columns(self.ctx, circuit.h, po2, zk_cycles, code.h, data.h))

    def derive_links(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, data: Buffer) -> None:
        """fill the destination columns of the LINK records of `data` on the active rows (zkh_derive_links): every access gets the
        previous access to its own address.  Raises HalError on a selector
        other than 0 / 1, on a clock that does not increase or on a difference that does not fit its limbs, naming the lowest
        (record, row) (`data` is then unchanged)"""
        _check(_lib.zkh_derive_links(self.ctx, circuit.h, po2, zk_cycles, code.h, data.h))

    def check_rows(self, circuit: Circuit, po2: int, accum: Buffer, code: Buffer, data: Buffer, out_global, mix_global,
                   row_lo: int = 0, row_hi: Optional[int] = None, per_row: bool = False) -> dict:
        """the circuit's constraints evaluated exactly on every row of the window [row_lo, row_hi) of the RAW traces (zkh_check_rows;
        the definition: circuits/check.py reference_check_rows).  -> {"row": lowest failing row or -1, "step": its lowest failing
        and_eqz step (an index into the ZKC1 step list; explain with circuits.check.explain_step), "failing_rows", "value": the four
        canonical words of the value that step wants zero, "per_row": None, or with per_row=True the 2^po2 words F(ret) of every
        row, NONE = 0xffffffff outside the window and where nothing fails}.  A failing row is an answer, not an error."""
        o, m = _u32(out_global), _u32(mix_global)
        g = (_vp * 3)(accum.h, code.h, data.h)
        rows = self.copy_from("check_rows_per_row", np.full(1 << po2, 0xFFFFFFFF, dtype=np.uint32)) if per_row else None
        res = CheckRowsResult()
        _check(_lib.zkh_check_rows(self.ctx, circuit.h, po2, g, 3, _ptr(o) if o.size else None, _ptr(m) if m.size else None, row_lo,
                                   (1 << po2) if row_hi is None else row_hi, rows.h if rows is not None else None, C.byref(res)))
        return {"row": int(res.row), "step": int(res.step), "failing_rows": int(res.failing_rows), "value": tuple(int(x) for x in res.value),
                "per_row": rows.to_vec() if rows is not None else None}

    def check_bus(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, data: Buffer, per_term: bool = False) -> dict:
        """the bus of a circuit with arguments checked key by key on the RAW traces (zkh_check_bus; the definition: circuits/logup.py
        reference_bus, which returns the same dict).  -> {"term", "row": the representative of the reported unbalanced key, or -1, -1,
        "tag", "key": its four canonical tuple words, "net", "unbalanced_keys", "distinct_keys", "slots", "per_term": None, or with
        per_term=True an (n_terms, 4) int64 array of (count, first_row, last_row, weight) of the reported key's entries per blob term,
        (0, -1, -1, 0) for a term without one}.  An unbalanced bus is an answer, not an error (circuits.logup.describe_bus words it)."""
        n_terms = int(circuit._args[5]) if getattr(circuit, "_args", None) is not None and circuit._args.size > 5 else 0
        terms = (BusTerm * max(1, n_terms))() if per_term else None
        res = CheckBusResult()
        _check(_lib.zkh_check_bus(self.ctx, circuit.h, po2, zk_cycles, code.h if code is not None else None, data.h, terms, n_terms,
                                  C.byref(res)))
        table = None
        if per_term:
            table = np.array([[t.count, t.first_row if t.count else -1, t.last_row if t.count else -1, t.weight] for t in terms[:n_terms]],
                             dtype=np.int64).reshape(n_terms, 4)
        return {"term": int(res.term), "row": int(res.row), "tag": int(res.tag), "key": tuple(int(x) for x in res.key), "net": int(res.net),
                "unbalanced_keys": int(res.unbalanced_keys), "distinct_keys": int(res.distinct_keys), "slots": int(res.slots),
                "per_term": table}

    def upload_data_trace(self, circuit: Circuit, po2: int, zk_cycles: int, data: Buffer, host: np.ndarray, pinned_async: bool = True) -> None:
        """upload a caller's data trace without what the library derives (zkh_upload_data_trace): the other columns whole, the derived
        ones on their blinding rows only.  pinned_async: `host` is a host_alloc view and the copies are enqueued without a host sync"""
        if host.dtype != np.uint32 or not host.flags["C_CONTIGUOUS"]:
            raise HalError("upload_data_trace: the host trace must be a C-contiguous uint32 array")
        if host.size != data.size():
            raise HalError(f"upload_data_trace: a host trace of {host.size} words for a buffer of {data.size()}")
        _check(_lib.zkh_upload_data_trace(self.ctx, circuit.h, po2, zk_cycles, data.h, host.ctypes.data_as(_u32p), int(pinned_async)))

    def h2d_bytes(self) -> int:
        """bytes this context has copied host to device so far (zkh_ctx_h2d_bytes)"""
        return int(_lib.zkh_ctx_h2d_bytes(self.ctx))

    def derive_sorted(self, circuit: Circuit, po2: int, zk_cycles: int, code: Buffer, data: Buffer) -> None:
        """fill the tuple columns of the derived sorted copies of `data` on the active rows (zkh_derive_sorted): raises HalError on a
        selector other than 0 / 1 (`data` is then unchanged)"""
        _check(_lib.zkh_derive_sorted(self.ctx, circuit.h, po2, zk_cycles, code.h, data.h))

    # ---- profiling ----
    def prof_enable(self, on: bool = True) -> None:
        _check(_lib.zkh_prof_enable(self.ctx, int(on)))

    def prof_reset(self) -> None:
        _check(_lib.zkh_prof_reset(self.ctx))

    def prof_get(self) -> List[dict]:
        recs = (ProfRec * 128)()
        n = _sz()
        _check(_lib.zkh_prof_get(self.ctx, recs, 128, C.byref(n)))
        return [{"name": recs[i].name.decode(), "calls": int(recs[i].calls), "total_ms": float(recs[i].total_ms),
                 "alg_bytes": float(recs[i].alg_bytes)} for i in range(n.value)]
