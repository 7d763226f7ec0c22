/*
 * zkhal.h — C ABI of libzkhal_mi355x.so: an MI355X (gfx950) implementation of the operator set behind
 * risc0_zkp::hal::{Hal, CircuitHal, Buffer}, plus the per-segment prover that drives it.
 *
 * What this replaces.  risc0/zeth reaches the prover through exactly one call,
 *     default_prover().prove(env, elf)            /root/reference/crates/host/src/lib.rs:137
 * (imports at lib.rs:26; segment size chosen at lib.rs:132-135; result checked by receipt.verify at
 * /root/reference/crates/host/src/bin/cli.rs:103-107).  Below that call sits the un-vendored
 * risc0-zkp 3.0.2 (/root/reference/Cargo.lock:5393): `prove::Prover<H: Hal>` issues every op declared
 * here through `hal::Hal` (src/hal/mod.rs) — upstream backends: CpuHal (src/hal/cpu.rs), CudaHal
 * (src/hal/cuda.rs + risc0-sys kernels).  Each entry point below names the trait method it stands in for.
 * A Rust `impl Hal for HipHal` binds these 1:1 (INTEGRATION.md shows the extern block).
 *
 * Conventions (same as upstream's risc0-sys C exports):
 *   - every function returns `const char*`: NULL on success, otherwise a heap error string that the
 *     caller releases with zkh_free_error();
 *   - element words are raw Montgomery-form BabyBear u32 exactly as upstream stores `Elem` in memory and in
 *     seals; Elem = 1 word, ExtElem = 4 words (AoS), Digest = 8 words.  Every op expects REDUCED words (< P) and
 *     produces reduced words; upstream's Elem::INVALID marker (0xffffffff) is not an input (upstream asserts on it);
 *   - matrices are column-major like upstream Buffer<T>: element (row r, column c) at c*rows + r;
 *   - a zkh_ctx is one GPU + one HIP stream, driven by one host thread at a time (upstream HALs are driven
 *     by a single prover thread).  Ops are enqueued in order on the ctx stream and are asynchronous;
 *     zkh_read / zkh_sync are the only host-visible sync points;
 *   - zkh_buf handles are reference counted views {allocation, word offset, word length}; slices share the
 *     allocation.  Host pointers are borrowed for the duration of the call only.
 *   - There is NO CPU fallback in this library: without a HIP device every call fails.
 */
#ifndef ZKHAL_H
#define ZKHAL_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zkh_ctx zkh_ctx;
typedef struct zkh_buf zkh_buf;
typedef struct zkh_circuit zkh_circuit;
typedef struct zkh_prover zkh_prover;

/* protocol constants — risc0-zkp 3.0.2 src/lib.rs */
#define ZKH_INV_RATE 4
#define ZKH_QUERIES 50
#define ZKH_FRI_FOLD 16
#define ZKH_FRI_MIN_DEGREE 256
#define ZKH_ZK_CYCLES 1994
#define ZKH_CHECK_SIZE 16
#define ZKH_EXT_SIZE 4
#define ZKH_DIGEST_WORDS 8

void zkh_free_error(const char* err);
/* library/ABI version, the gfx arch the kernels were compiled for ("gfx950"), and where the shipped Poseidon2 tables come
 * from: "poseidon2_consts=derived" (output of the published parameter-generation procedure, tools/gen_poseidon2_consts.py,
 * which reproduces every value of the published instance on record; not yet compared with upstream's consts.rs itself),
 * "=upstream" once that comparison has been made, "=placeholder" for filler tables (digests cannot match upstream's) */
const char* zkh_version(void);

/* ---- context: CudaHal::new / HalPair (hal/cuda.rs) ---- */
/* hash_suite must be "poseidon2" (the suite zeth's default ProverOpts selects). */
const char* zkh_ctx_create(int device_ordinal, const char* hash_suite, zkh_ctx** out);
void zkh_ctx_destroy(zkh_ctx*);
const char* zkh_sync(zkh_ctx*);
/* Device memory of this context: bytes held by live buffers, bytes cached by the stream-ordered free list (blocks are
 * recycled by exact size, so a host that proves many segment sizes accumulates cache), and the live high-water mark.
 * zkh_ctx_trim drains the stream and returns the cached blocks to the driver; allocation does the same on its own
 * before reporting out-of-memory. */
void zkh_ctx_memory(const zkh_ctx*, size_t* live_bytes, size_t* cached_bytes, size_t* peak_live_bytes);
const char* zkh_ctx_trim(zkh_ctx*);
/* raw hipStream_t of the context (for callers that interleave their own work) */
void* zkh_ctx_stream(zkh_ctx*);
/* Replace the Poseidon2 tables (canonical residues): rc[24*29], diag[24] — consts.rs as data. */
const char* zkh_poseidon2_set_constants(zkh_ctx*, const uint32_t* rc, const uint32_t* diag);

/* ---- Buffer<T>: alloc_* / copy_from_* / slice / view / get_at (hal/mod.rs trait Buffer) ---- */
const char* zkh_alloc(zkh_ctx*, const char* name, size_t n_words, int zero, zkh_buf** out);
const char* zkh_copy_from(zkh_ctx*, const char* name, const uint32_t* host, size_t n_words, zkh_buf** out);
/* wrap device memory owned by the caller (e.g. a torch tensor's data_ptr); never freed by the library */
const char* zkh_wrap(zkh_ctx*, void* device_ptr, size_t n_words, zkh_buf** out);
const char* zkh_slice(zkh_buf*, size_t off_words, size_t n_words, zkh_buf** out);
void zkh_retain(zkh_buf*);
void zkh_release(zkh_buf*);
size_t zkh_size(const zkh_buf*);
void* zkh_device_ptr(const zkh_buf*);
/* view(): synchronises the stream, then D2H */
const char* zkh_read(zkh_ctx*, const zkh_buf*, uint32_t* host, size_t off_words, size_t n_words);
/* view_mut()/copy: H2D ordered on the stream */
const char* zkh_write(zkh_ctx*, zkh_buf*, const uint32_t* host, size_t off_words, size_t n_words);
/* Witness ingress for hosts that run preflight + witgen on the CPU (upstream: SegmentProver steps 1-2 before
 * Prover::commit_group; 0.94 GB of code + data per po2-20 SYN-A segment): pinned host memory the caller fills in place,
 * and an upload that is only ENQUEUED on the context's stream (no host sync; the block must not be rewritten before the
 * next zkh_sync / zkh_read of this context).  The DMA overlaps kernels of other contexts on the same GPU. */
const char* zkh_host_alloc(zkh_ctx*, size_t n_words, uint32_t** host);
void zkh_host_free(zkh_ctx*, uint32_t* host);
const char* zkh_write_async(zkh_ctx*, zkh_buf*, const uint32_t* pinned_host, size_t off_words, size_t n_words);

/* ---- trait Hal ops (hal/mod.rs); semantics = CpuHal (hal/cpu.rs) ---- */
/* Hal::batch_interpolate_ntt(io, count): per column inverse NTT, natural in -> bit-reversed coeffs, * n^-1 */
const char* zkh_batch_interpolate_ntt(zkh_ctx*, zkh_buf* io, size_t count);
/* Hal::batch_expand_into_evaluate_ntt(out, in, count, expand_bits): per column, bit-reversed coeffs in -> evaluations on the
 * domain 2^expand_bits times larger.  Accepted: expand_bits in 0 .. log2(out column), with out column == in column << expand_bits;
 * expand_bits == log2(out column) (one coefficient per column) replicates it.  Anything else is refused, `out` untouched. */
const char* zkh_batch_expand_into_evaluate_ntt(zkh_ctx*, zkh_buf* out, const zkh_buf* in, size_t count,
                                               size_t expand_bits);
/* Hal::batch_bit_reverse(io, count) */
const char* zkh_batch_bit_reverse(zkh_ctx*, zkh_buf* io, size_t count);
/* Hal::zk_shift(io, count): io[c][i] *= 3^bitrev(i) */
const char* zkh_zk_shift(zkh_ctx*, zkh_buf* io, size_t count);
/* Fused Prover::commit_group prefix: interpolate_ntt + zk_shift in one pass over HBM (same result as the
 * two calls above in sequence). */
const char* zkh_batch_interpolate_ntt_zk_shift(zkh_ctx*, zkh_buf* io, size_t count);
/* Out-of-place variant that also absorbs commit_group's eltwise_copy_elem: out = iNTT(in) [* 3^bitrev(i)];
 * `in` (the witness) is left untouched. */
const char* zkh_batch_interpolate_ntt_from(zkh_ctx*, zkh_buf* out, const zkh_buf* in, size_t count, int zk_shift);
/* Hal::hash_rows(output, matrix): rows = output digests; leaf r = Poseidon2 sponge over matrix[c*rows + r] */
const char* zkh_hash_rows(zkh_ctx*, zkh_buf* out_digests, const zkh_buf* matrix);
/* Hal::hash_fold(io, input_size, output_size): io[out+i] = H(io[in+2i], io[in+2i+1]) */
const char* zkh_hash_fold(zkh_ctx*, zkh_buf* io_digests, size_t input_size, size_t output_size);
/* Fused MerkleTreeProver::new tail: every hash_fold layer from `rows` leaves down to the root.
 * nodes has 2*rows digests, leaves already at [rows, 2*rows). */
const char* zkh_merkle_fold_all(zkh_ctx*, zkh_buf* nodes, size_t rows);
/* MerkleTreeProver::new as one call: nodes[rows .. 2 rows) = hash_rows(matrix), then every layer above down to the root at nodes[1];
 * digests are identical to zkh_hash_rows + zkh_merkle_fold_all. */
const char* zkh_merkle_build(zkh_ctx*, zkh_buf* nodes, const zkh_buf* matrix, size_t rows);
/* The bare permutation (risc0_zkp::core::hash::poseidon2::poseidon2_mix): `count` states of 24 Montgomery words each,
 * in place — on the device with the context's tables, or on the host (rc / diag canonical residues, NULL = the shipped
 * tables).  What the published known-answer vector of the instance is checked against (tests/golden/poseidon2_kat.json). */
const char* zkh_poseidon2_mix(zkh_ctx*, zkh_buf* states, size_t count);
const char* zkh_poseidon2_mix_host(const uint32_t* rc, const uint32_t* diag, uint32_t* states, size_t count);
/* Hal::batch_evaluate_any(coeffs, poly_count, which, xs, out): out[k] = sum_j coeffs[which[k]][j] xs[k]^j */
const char* zkh_batch_evaluate_any(zkh_ctx*, const zkh_buf* coeffs, size_t poly_count, const zkh_buf* which,
                                   const zkh_buf* xs, zkh_buf* out);
/* Same, for coefficient columns still in the bit-reversed order batch_interpolate_ntt produced (position p holds
 * coefficient bitrev(p)); column length a power of two >= 2^14.  Lets PolyGroup::new skip its W x n batch_bit_reverse. */
const char* zkh_batch_evaluate_any_bitrev(zkh_ctx*, const zkh_buf* coeffs, size_t poly_count, const zkh_buf* which,
                                          const zkh_buf* xs, zkh_buf* out);
/* batch_bit_reverse for ExtElem (AoS) columns: used on the few combo polynomials instead of on every coefficient column */
const char* zkh_batch_bit_reverse_extelem(zkh_ctx*, zkh_buf* io_ext, size_t count);
/* Hal::mix_poly_coeffs(output, mix_start, mix, input, combos, input_size, count) */
const char* zkh_mix_poly_coeffs(zkh_ctx*, zkh_buf* out, const uint32_t mix_start[4], const uint32_t mix[4],
                                const zkh_buf* in, const zkh_buf* combos, size_t input_size, size_t count);
/* Hal::combos_prepare: combos[combo_of_reg*cycles + i] -= mix^reg * coeff_u[...]  (flattened on the host into
 * (position, value) pairs: combos[pos[k]] -= val[k]) */
const char* zkh_combos_prepare(zkh_ctx*, zkh_buf* combos, const uint32_t* pos, const uint32_t* vals_ext,
                               size_t n_entries);
/* Hal::combos_prepare with upstream's own argument list (combos, coeff_u, combo_count, cycles, regs_count, reg_sizes,
 * reg_combo_ids, mix), all operands device buffers as in `impl Hal`:
 *   cur = 1; for r < regs_count: combos[cycles*reg_combo_ids[r] + i] -= cur * coeff_u[pos + i] (i < reg_sizes[r]); cur *= mix; pos += reg_sizes[r];
 *   then ZKH_CHECK_SIZE times: combos[cycles*combo_count] -= cur * coeff_u[pos]; pos += 1; cur *= mix.
 * combos: (combo_count + 1) x cycles ExtElems; registers of any size 1 .. cycles.  Nothing is read back: the register list is
 * VALIDATED ON THE DEVICE before it is used (sizes, combo ids, and that coeff_u holds sum(sizes) + ZKH_CHECK_SIZE coefficients); an
 * inconsistent list leaves combos untouched — never an out-of-bounds read — and is REPORTED BY THE NEXT zkh_sync / zkh_read of the
 * context (the error names the register).  (zkh_combos_prepare above is the host-flattened form the in-library prover uses.) */
const char* zkh_combos_prepare_regs(zkh_ctx*, zkh_buf* combos, const zkh_buf* coeff_u, size_t combo_count, size_t cycles,
                                    size_t regs_count, const zkh_buf* reg_sizes, const zkh_buf* reg_combo_ids,
                                    const uint32_t mix[4]);
/* Hal::combos_divide: synthetic division of combo polynomial `combo` (cycles ExtElems at combos[combo*cycles..])
 * by (x - pt) for every pt in pts; remainders (must be 0) are written to rem_out (n_pts ExtElems, device). */
const char* zkh_combos_divide(zkh_ctx*, zkh_buf* combos, size_t combo, size_t cycles, const uint32_t* pts_ext,
                              size_t n_pts, zkh_buf* rem_out);
/* The same for every combo of the buffer in one call: combo i (i < n_combos) is divided by (x - pt) for each of its points
 * pts_ext[4*pts_begin[i] .. 4*pts_begin[i+1]); remainders go to rem_out in point order.  The r-th divisions of all
 * combos share their kernel launches (they are independent; only the divisions of one combo are sequential). */
const char* zkh_combos_divide_all(zkh_ctx*, zkh_buf* combos, size_t cycles, size_t n_combos, const uint32_t* pts_ext,
                                  const uint32_t* pts_begin, zkh_buf* rem_out);
/* Hal::eltwise_add_elem / eltwise_copy_elem / eltwise_zeroize_elem / eltwise_sum_extelem */
const char* zkh_eltwise_add_elem(zkh_ctx*, zkh_buf* out, const zkh_buf* a, const zkh_buf* b);
const char* zkh_eltwise_copy_elem(zkh_ctx*, zkh_buf* out, const zkh_buf* in);
const char* zkh_eltwise_zeroize_elem(zkh_ctx*, zkh_buf* io);   /* INVALID (0xffffffff) -> 0 */
/* io[i] = io[i] % P in place, for any 32-bit words: where a caller's trace, whose raw words >= P are legal for the entry points that
 * take arguments as data (zkh_derive_*, zkh_check_rows, zkh_check_bus, zkh_accumulate, the image calls), becomes the reduced words
 * that every Hal-level op and zkh_prove_begin expect (below).  No upstream counterpart: upstream's Elem is reduced by construction. */
const char* zkh_reduce_elem(zkh_ctx*, zkh_buf* io);
const char* zkh_eltwise_sum_extelem(zkh_ctx*, zkh_buf* out_elem, const zkh_buf* in_ext);
/* Hal::fri_fold(output, input, mix) */
const char* zkh_fri_fold(zkh_ctx*, zkh_buf* out, const zkh_buf* in, const uint32_t mix[4]);
/* Hal::gather_sample(dst, src, idx, size, stride): dst[g] = src[g*stride + idx] */
const char* zkh_gather_sample(zkh_ctx*, zkh_buf* dst, const zkh_buf* src, size_t idx, size_t size, size_t stride);
/* Hal::scatter(into, index, offsets, values) */
const char* zkh_scatter(zkh_ctx*, zkh_buf* into, const uint32_t* index, const uint32_t* offsets,
                        const uint32_t* values, size_t n_idx, size_t n_val);
/* Hal::prefix_products(io): io[i] *= io[i-1] over ExtElems */
const char* zkh_prefix_products(zkh_ctx*, zkh_buf* io_ext);
/* batched MerkleTreeProver::prove for many indices at once (query phase): for each idx writes
 * (cols column words, then the path digests down to the top layer) consecutively into `out` (device).
 * words per query = cols + 8*(log2(rows) - top_layer). */
const char* zkh_merkle_open(zkh_ctx*, const zkh_buf* matrix, const zkh_buf* nodes, size_t rows, size_t cols,
                            const uint32_t* idx, size_t n_idx, zkh_buf* out);

/* ---- CircuitHal (risc0-circuit-rv32im 4.0.2 src/prove/hal/; circuit is data: zeth_amd/circuits/desc.py) ---- */
const char* zkh_circuit_load(zkh_ctx*, const uint32_t* desc, size_t n_words, zkh_circuit** out);
void zkh_circuit_destroy(zkh_circuit*);
/* 2 if a code object was attached at run time (below), 1 if a build-time generated straight-line eval_check
 * kernel matches this desc, 0 if the on-device step interpreter will be used. */
int zkh_circuit_has_compiled_kernel(const zkh_circuit*);
/* Attach a gfx950 code object (ELF or clang offload bundle, borrowed for the call) that holds
 *   extern "C" __global__ void <kernel_name>(zkh::EvalCheckArgs)        -- csrc/circuit.h
 * generated for this circuit's PolyExtStep list; zkh_eval_check then launches it instead of the interpreter.
 * Replaces upstream's per-circuit machine-generated eval_check kernel (risc0-circuit-rv32im-sys 4.0.2
 * kernels/…/eval_check.cu, un-vendored: /root/reference/Cargo.lock:5320) for circuits that arrive as data.
 * Not thread-safe against a concurrent zkh_eval_check on the same circuit. */
const char* zkh_circuit_attach_code_object(zkh_circuit*, const void* image, size_t len, const char* kernel_name);
/* A constraint system of realistic size is generated as n_parts kernels over disjoint constraint ranges (upstream splits
 * its generated eval_check over many translation units for the same reason); each part arrives as its own code object.
 * zkh_eval_check uses them once all n_parts are attached: part 0 writes `check`, the others add their share.
 * A code object may export `<kernel_name>_exps` (device data: {count, e_0, e_1, ...}): the kernel then reads slot k of
 * EvalCheckArgs::mix_pows as poly_mix^e_k — its powers gathered into the order its code touches them — and zkh_eval_check
 * builds that table per call (all parts of a circuit export it, or none: zkh_eval_check refuses a mixed set). */
const char* zkh_circuit_attach_code_object_part(zkh_circuit*, const void* image, size_t len, const char* kernel_name,
                                                size_t part, size_t n_parts);
/* number of kernels zkh_eval_check will launch for this circuit (0: step interpreter) */
size_t zkh_circuit_compiled_parts(const zkh_circuit*);
/* CircuitHal::eval_check(check, groups, globals, poly_mix, po2, steps).  groups = evaluated accum, code, data
 * (each W x 4n; n_groups must be 3); globals = out, mix (n_globals must be 2); steps = 2^po2 like upstream.
 * use_interpreter != 0 forces the generic interpreter kernel. */
const char* zkh_eval_check(zkh_ctx*, const zkh_circuit*, zkh_buf* check, const zkh_buf* const* groups, size_t n_groups,
                           const zkh_buf* const* globals, size_t n_globals, const uint32_t poly_mix[4], size_t po2,
                           size_t steps, int use_interpreter);
/* A witness checked against the circuit's own constraints, row by row, on the device (csrc/check_rows.hip; DESIGN.md §2 CHECK ROWS):
 * which constraint a trace breaks, and on which row, before a seal is spent on it.  groups = the RAW accum, code, data traces (each
 * W x 2^po2 words; n_groups must be 3); out_global / mix_global = host words, as zkh_accumulate takes mix.  Every constraint is
 * evaluated exactly on every row r of the window [row_lo, row_hi) of the trace domain (no mix, no probability): a tap (g, col, back)
 * reads row (r - back) mod 2^po2, cells and globals are read as residues (raw % P), values are Fp, and Fp4 downstream of a ConstExt.
 * Over the mix steps F = the lowest failing and_eqz step (an index into the ZKC1 step list) or 0xffffffff:
 *   F(true) = none; F(and_eqz(x, v)) = min(F(x), v != 0 ? this step : none); F(and_cond(x, cond, inner)) = min(F(x), cond != 0 ?
 *   F(inner) : none); an Fp4 is non-zero when any component is.  Row r fails when F(ret) is a step.
 * result: row = the lowest failing row of the window (-1: none failed, the other fields are then 0xffffffff, 0, zeros), step = its
 * F(ret), failing_rows = the rows of the window that fail, value = the value that step requires to be zero on that row (canonical,
 * decoded; a base-field value has zero upper components).  per_row (NULL, or a buffer of 2^po2 words): word r = F(ret) of row r for
 * the rows of the window; the other words are not written.
 * A failing row is an ANSWER: the call returns NULL either way.  It fails only for bad shapes, an empty window or one outside
 * [0, 2^po2], a circuit loaded on another context, and a step list whose live values exceed the step interpreter's LDS. */
typedef struct { int64_t row; uint32_t step; uint32_t failing_rows; uint32_t value[4]; } zkh_check_rows_result;
const char* zkh_check_rows(zkh_ctx*, const zkh_circuit*, size_t po2, const zkh_buf* const* groups, size_t n_groups,
                           const uint32_t* out_global, const uint32_t* mix_global, size_t row_lo, size_t row_hi, zkh_buf* per_row,
                           zkh_check_rows_result* result);
/* A witness's bus checked key by key on the device (csrc/bus.hip; DESIGN.md §2 CHECK BUS; host twin: circuits/logup.py reference_bus):
 * which key does not balance, when zkh_accumulate (below) would only say "the bus does not balance".  Needs a circuit with arguments
 * and the RAW code and data traces of 2^po2 rows, A = 2^po2 - zk_cycles active; no mix, no accum.
 * An ENTRY is a (term i, row r < A) of non-zero weight w_i(r) = sel_i(r) m_i(r) in Fp (both read as residues, an absent one is 1: the
 * accumulate's numerator; a selector is a field value here, nothing is refused).  Its KEY is (tag, v_0 .. v_3) as residues, the tuple
 * zero-padded to 4 — the accumulate's denominator, so (x) and (x, 0) are one key.  net(K) = sum over K's entries of sign_i w_i(r) in
 * Fp; K is UNBALANCED when net(K) != 0.  Distinct keys are distinct poles: the bus can balance for a mix only by chance unless every
 * net is 0, and balances for every mix when they all are.  The representative of a key is its entry of smallest (blob term index,
 * row) over all terms.
 * result: term, row = the representative of the unbalanced key whose representative is smallest (-1, -1: every key balances; tag, key,
 * net are then 0), tag, key = that key (canonical), net = its net (canonical), unbalanced_keys, distinct_keys, slots = the final size
 * of the key table: the smallest power of two >= max(64, 2 A), doubled until it is at least twice distinct_keys.
 * per_term (NULL, or n_terms records, n_terms the blob's): record i = what term i holds of the reported key: count of entries, their
 * first and last row, weight = the sum of w_i(r) over them in Fp (unsigned; the sign is the term's).  A term without such an entry, and
 * every term when nothing is unbalanced, gets count 0, rows 0xffffffff, weight 0.
 * An unbalanced bus is an ANSWER: the call returns NULL either way.  It fails only for bad shapes, a circuit without arguments, a
 * missing code trace, a circuit loaded on another context, more distinct keys than a table of 2^31 slots holds, and n_terms x A >= 2^33
 * (a counter could wrap).  Reads code and data, writes neither. */
typedef struct { int64_t row; int32_t term; uint32_t tag; uint32_t key[4]; uint32_t net; uint32_t unbalanced_keys; uint32_t distinct_keys;
                 uint32_t slots; } zkh_check_bus_result;
typedef struct { uint32_t count; uint32_t first_row; uint32_t last_row; uint32_t weight; } zkh_bus_term;
const char* zkh_check_bus(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* data,
                          zkh_bus_term* per_term, size_t n_terms, zkh_check_bus_result* result);

/* ---- CircuitHal::accumulate for arguments described as data (csrc/accumulate.hip; zeth_amd/circuits/logup.py) ----
 * Lookup and permutation arguments as log-derivative sums: a ZKA1 blob lists terms t(r) = sign sel(r) m(r) / (alpha - (tag + beta v_0(r)
 * + ... + beta^w v_{w-1}(r))) per accum Fp4 column; the column holds their running sum over the active rows, the blinding rows hold
 * noise, and all columns' totals must sum to zero (one bus).  The constraints that check it are ordinary steps of the circuit's ZKC1
 * description (emitted by the same builder), so provers and verifiers need nothing else.
 * zkh_circuit_set_arguments validates the blob against the circuit (accum width = 4 k, alpha / beta within the mix globals, columns
 * within their groups, tuple width 1..4, 1..3 terms per column) and keeps a copy; words == 0 removes the arguments.
 * zkh_accumulate fills `accum` (4k x 2^po2) from the raw code and data traces and the mix globals drawn by zkh_prove_begin.  It FAILS
 * — and leaves the accum zeroed, so no seal can be made from it — when a denominator vanishes (the error names the row and column) or
 * when the bus does not balance (the error reports the total): an ordinary refusal of a bad witness. */
const char* zkh_circuit_set_arguments(zkh_circuit*, const uint32_t* blob, size_t words);
int zkh_circuit_has_arguments(const zkh_circuit*);
const char* zkh_accumulate(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const uint32_t noise_key[8], const zkh_buf* code,
                           const zkh_buf* data, const uint32_t* mix_global, zkh_buf* accum);
/* THE OPEN BUS (ZKA1 version 8: version 7's layout and, after every other record, ONE record of kind 5 = OPEN, 16 words: kind, the open
 * tag, the `out` word offsets of alpha, beta and the total (4 words each, disjoint, inside `out`), the circuit's `out` words, the rest
 * reserved; header words 3, 4 repeat the offsets of alpha and beta; header word 7 carries bit 17, and bit 16 exactly when the blob holds a
 * PAGES record).  A bus ACROSS seals (DESIGN.md §2 "THE TIE"): the constraints read alpha and beta from `out`, the terms of the open tag are
 * answered by another seal, and the bus closes on the four `out` words of the total instead of zero.
 * zkh_circuit_open_bus: 1 when the circuit's arguments are open, and then where[4] (if given) = the open tag and the three offsets; else 0.
 * zkh_accumulate_open is zkh_accumulate's pass with `challenge` = alpha (4 words) ‖ beta (4 words), reduced Montgomery words, where the
 * mix globals were.  It refuses a vanishing denominator as zkh_accumulate does; a total that is not zero is no refusal: total[4] = the
 * sum of the accum columns' last active row, 4 reduced Montgomery words, which the caller states in `out` next to the challenge.
 * zkh_accumulate refuses an open blob and zkh_accumulate_open a closed one; zkh_check_bus skips the keys of the open tag. */
/* PORTS (ZKA1 version 9: version 8's layout, the OPEN record no longer required; header word 7 = the READS count | bit 16 exactly when the blob
 * holds a PAGES record | bit 17 exactly when it holds an OPEN record | bit 18 (0x40000, PORTS) exactly when a LINK joins: a version-9 blob
 * without bit 18 is no ZKA1 blob, bit 18 with no joining record is refused).  In LINK word [5] bit 1 = JOINS beside bit 0 = READS, and with
 * JOINS word [31] is the blob record index of the HEAD (without it word [31] stays reserved = 0).  A memory is a run of k <= 8 consecutive LINK
 * records, the head and the records that join it; port q is the record at head + q, with the head's nc, L, nl and READS-ness.  Its accesses
 * are the (row, port) whose record's selector is 1, ordered by (row, port), and the previous access of one is the greatest one before it
 * in that order with the same address, in whichever port.  zkh_derive_links, zkh_derive_links_paged, zkh_derive_links_paged_table and
 * zkh_derive_all* derive such a circuit: destinations stay per record, a refusal names the port's own record and, where the previous access lies
 * in another record, "row R of record Q".  A PAGES record names the head: an unlinked access of any port takes the image's word, the page
 * table's heads and tails are those of the merged order, and a trace that pages more addresses than it has active rows is refused.  A blob
 * without a joiner is what it was, format, launches and messages. */
int zkh_circuit_open_bus(const zkh_circuit*, uint32_t where[4]);
const char* zkh_accumulate_open(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const uint32_t noise_key[8], const zkh_buf* code,
                                const zkh_buf* data, const uint32_t challenge[8], zkh_buf* accum, uint32_t total[4]);
/* THE TABLE'S FINGERPRINT (csrc/tie.hip; host twin: circuits/logup.py table_fingerprint): total[4] = the sum over the D rows (a, in, out)
 * of the table at word `table_at` of `table` (three words a row as a ZKU1 proof holds them: the address an integer, in and out
 * Montgomery words; zkh_page_out_proof leaves it at word 5 + h) of 1 / (alpha - (2 + beta a + beta^2 in + beta^3 out)) in Fp4, as 4
 * reduced Montgomery words; challenge = alpha ‖ beta as zkh_accumulate_open takes it.  It is the open total of the tied paging segment
 * whose page table this is, and minus the sum of the totals of the P2-PAGE-tied parts of its page-out.  D = 0 gives zero without a
 * launch.  It FAILS when the table does not lie in the buffer, when D >= 2^31, and when a denominator vanishes: the error names the
 * lowest such row.  Two launches, one read-back of 5 words; reads the table, writes nothing of the caller's. */
const char* zkh_table_fingerprint(zkh_ctx*, const zkh_buf* table, size_t table_at, size_t D, const uint32_t challenge[8], uint32_t total[4]);
/* Derived multiplicities (ZKA1 version 2: term word 7 bit 0).  A derived term is the table side of a lookup: sign -1, its multiplicity a
 * data column that nothing else in the blob names, every other term of its tag a lookup of sign +1.  zkh_derive_multiplicities writes
 * that column on the active rows [0, 2^po2 - zk_cycles) of `data`: on the representative of each table key (its entry of smallest
 * (blob term index, row)) the number of lookups of that key (the sum of their sel * m, in Fp, Montgomery form), 0 on every other
 * active row; the blinding rows are not touched.  Keys are (tag, v_0 .. v_3) compared as field elements, the tuple zero-padded.  It
 * FAILS and leaves `data` unchanged when a table selector is neither 0 nor 1, or when a lookup of nonzero weight has no table entry
 * (the error names the term, tag, row and key).  zkh_derive_all (below) runs it in its place, last. */
int zkh_circuit_derives_multiplicities(const zkh_circuit*);
const char* zkh_derive_multiplicities(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data);
/* Derived sorted copies (ZKA1 version 3: term word 7 bit 1 marks a term D as the sorted copy of its source term S; bits 4..6 = nkeys
 * (1..3), bits 8 + 2j, 9 + 2j = the tuple position of sort key j, most significant key first; bits 16..31 = the blob index of S; bits
 * 2, 3, 7 and the positions of unused keys are reserved and refused).  D is the permuted side of a multiset equality: sign -1 against
 * S's +1, the same tag, tuple width and selector, constant multiplicities, its tuple columns pairwise distinct data columns that nothing
 * else in the blob names, no derived multiplicity in its tag.  With r_0 < ... < r_{m-1} the active rows (r < 2^po2 - zk_cycles) whose
 * selector is 1 (no selector: all) and pi the STABLE permutation that sorts them by the canonical values of S's key columns
 * (lexicographic, equal keys keep their row order), zkh_derive_sorted writes data[D.v_e][r_j] = the raw word of S.v_e at r_pi(j) for
 * every tuple position e, 0 on the active rows whose selector is 0; the blinding rows are not touched.  The result depends on the
 * traces alone (no atomic arrival order enters it).  It FAILS and leaves `data` unchanged when a selector is neither 0 nor 1 (the
 * error names the term and the row).  zkh_derive_all (below) runs it in its place, first. */
int zkh_circuit_derives_sorted(const zkh_circuit*);
const char* zkh_derive_sorted(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data);
/* Derived columns (ZKA1 version 4: header word 6 = n_records, and n_records records of 16 words follow the terms: kind (1 = LIMBS,
 * 2 = ORDER), L = limb bits (1..16), nl = limbs (1..8, L nl <= 32), n_src (LIMBS: 1; ORDER: 1 or 2), two (group, column) source pairs,
 * eight destination data columns — for ORDER with two keys the flag column first, then nl <= 7 limb columns; unused words 0).  With
 * x(c, r) the canonical value of a cell, zkh_derive_columns writes on the active rows r < 2^po2 - zk_cycles
 *   LIMBS: dst_j[r] = Montgomery((x(src, r) >> jL) & (2^L - 1));
 *   ORDER: zeros on row 0; for r >= 1 the limbs of d = k0[r] - k0[r-1] (one key), or with e = [k0[r] == k0[r-1]] the flag
 *          Montgomery(e) and the limbs of d = e ? k1[r] - k1[r-1] : k0[r] - k0[r-1] - 1 (two keys);
 * the blinding rows are not touched.  A source is a code or data column that no record writes and no derived multiplicity (records
 * never chain); it may be a sorted copy's column.  Destinations are data columns that nothing else writes, that no record and no
 * source term of a sorted copy reads and that no term uses as its multiplicity; lookup tuples read them freely.  It FAILS and leaves
 * `data` unchanged — the error names the lowest (record, row) and the value — when a LIMBS value or an ORDER difference does not fit
 * L nl bits, or when an ORDER difference is negative ("not ordered").  Like its siblings it is an error on a circuit without records.
 * zkh_derive_all (below) runs it in its place, second. */
int zkh_circuit_derives_columns(const zkh_circuit*);
const char* zkh_derive_columns(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data);
/* Linked accesses (ZKA1 version 5: a record of kind 3 = LINK takes 32 words and follows every LIMBS / ORDER record: kind, L = limb bits
 * (1..16), nl = limbs (0..4, L nl <= 29), nc = carried columns (1..3), sel (a code column, or 0xffffffff = every active row), 0, the
 * key's (group, column), three (group, column) pairs of the carried columns c_0 .. c_{nc-1} (c_0 is the clock), 0, 0, then from word 16
 * the 2 + nc + nl destination data columns linked, last, prev_0 .. prev_{nc-1}, limb_0 .. limb_{nl-1}; unused words 0).  This is the
 * witness of a memory argument without a sorted copy: every access carries the previous access to its own address.  A row
 * r < 2^po2 - zk_cycles is an access when its selector is 1.  With x(c, r) the canonical value of a cell, K = x(key, r) and r' the
 * greatest access below r with key K, zkh_derive_links writes on the access rows
 *   linked[r] = Montgomery([r' exists]), last[r] = Montgomery([no access above r has key K]),
 *   prev_j[r] = the raw word of c_j at r' (0 when not linked), limb_j[r] = Montgomery(limb j of d = x(c_0, r) - x(c_0, r') - 1) (0 when
 *   not linked),
 * zeros in every destination on the active rows that are no access; the blinding rows are not touched.  The result depends on the
 * traces alone.  Sources are code or data columns that no derive writes; destinations are data columns that nothing else writes and
 * that no record and no source term of a sorted copy reads; lookup tuples read them freely, and linked and last (only they) may be
 * the multiplicity of a term that is not derived.  It FAILS and leaves `data` unchanged when a selector is neither 0 nor 1 (checked
 * over all records before any clock), when d < 0 ("clock not increasing") or when d >= 2^(L nl); the error names the lowest (record,
 * row) and the values.  Like its siblings it is an error on a circuit without LINK records.  zkh_derive_all (below) runs it in its
 * place, third.
 * The read rule (ZKA1 version 6; versions 1..5 are word for word what they were): LINK word 5 is a flag word, bit 0 = READS, every other
 * bit refused; with READS words 14, 15 are the (group, column) of the write flag w, a source of the record like the key and the carried
 * columns, and nc >= 2; without READS they are 0.  Header word 7 = the number of LINK records with READS: a version-6 blob in which it
 * is 0 is no ZKA1 blob, and one in which it is not that number is refused.  A record with READS states that a load returns the last
 * store: on every access r, x(w, r) must be 0 or 1; a store (1) is free; a load (0) needs, for every carried column j = 1 .. nc - 1 (the
 * clock c_0 is exempt), x(c_j, r) = x(c_j, r') when r is linked and x(c_j, r) = 0 when it is not (memory starts zeroed), compared as
 * residues mod P.  The rule adds no destination.  zkh_derive_links FAILS and leaves `data` unchanged on the lowest (record, row) over
 * clock and read-rule refusals together; on one row it names the write flag first, then the clock, then the read rule, lowest j first,
 * with the value read and the value last stored and its row.  Records without READS behave as in version 5.
 * zkh_circuit_links_check_reads: the number of LINK records with READS (0: none, or no arguments). */
int zkh_circuit_derives_links(const zkh_circuit*);
int zkh_circuit_links_check_reads(const zkh_circuit*);
const char* zkh_derive_links(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data);
/* PAGING (ZKA1 version 7; versions 1..6 are word for word what they were): the arguments may hold ONE PAGES record (kind 4, 32 words, after
 * every LINK record; header word 7 carries bit 16 beside the READS count).  Its words: kind, L = limb bits (1..16), ng = limbs (1..4,
 * L ng <= 29), the blob index of the LINK record it pages (one with READS and nc = 2: a clock and one value column), twelve zeros, then
 * the 5 + 2 ng destination data columns p_on, p_addr, p_in, p_out, p_time, alimb_0 .., gap_0 ...  zkh_circuit_pages: 1 with such a
 * record, else 0.  The memory of that LINK then starts from an IMAGE, W raw Montgomery words, image[a] the word of address a (the
 * canonical value of the key), and zkh_derive_links_paged (zkh_derive_links with that image) differs from zkh_derive_links in this:
 *   an unlinked access r of the paged record takes the image as its previous access: prev_1[r] = the raw word image[a], prev_0[r] = 0
 *   (clock 0 is the image's), limb_j[r] = limb j of x(clock, r) - 0 - 1; linked and last are what they were;
 *   it FAILS, leaving `data` unchanged, also when an access has a >= W ("address A outside the image of W words"), when an unlinked
 *   access has clock 0, when its clock - 1 does not fit the limbs, and when an unlinked load does not return image[a] (residues); on one
 *   row the order is write flag, address, clock, read rule, and the lowest (record, row) over all refusals is the one reported;
 *   with a_0 < .. < a_{D-1} the distinct addresses of the record's accesses it writes the page table on the active rows i < D:
 *   p_on = Montgomery(1), p_addr = the raw key word of a_i's first access, p_in = the raw word image[a_i], p_out, p_time = the raw value
 *   and clock words of a_i's last access, alimb_j = limb j of a_i (refused when a_i >= 2^(L ng)), gap_j = limb j of a_i - a_{i-1} - 1
 *   (zeros on row 0); active rows [D, A) get zeros in all thirteen, rows [A, n) are never touched.
 * One address sort serves the links and the table; the result is a function of the traces and the image alone.  zkh_derive_links and
 * zkh_derive_all REFUSE a circuit with a PAGES record ("the arguments page memory: an image is required (zkh_derive_all_paged)"); with no
 * PAGES record the paged entry points ignore the image (NULL or not) and are the plain ones.
 * zkh_page_out writes the table back: image[x(p_addr, i)] = the raw word p_out[i] on every active row i with p_on = 1.  A check pass
 * comes first and a refusal leaves the image unchanged: the lowest row whose p_on is not 0 / 1, whose address is >= W, or whose address
 * does not follow a smaller one on a row with p_on = 1 (the table is a prefix of strictly increasing addresses, as the circuit demands:
 * a host-made table that repeats an address is refused, not resolved).  It is a call of its own so that a refused or aborted seal never
 * touches the image.  The prover can commit to the image, prove a page-out between two roots and seal that step (below: P2-PAGE); a
 * tied group (P2-PAGE-tied, P2-TREE-tied: zkh_accumulate_open, zkh_tie_challenge) ties p_in / p_out of a paging segment's OWN seal to
 * that commitment over one shared bus, so the verifier of the group learns which image (THE TIE).
 * PAGING IN FROM A PAGE TABLE (zkh_derive_links_paged_table, zkh_derive_all_paged_table): a rank that does not hold the image derives the
 * same witness from the page table a ZKU1 proof ships.  The words of `table` from `table_at` on are D rows of 3 words (a_i, in_i, out_i),
 * as zkh_table_fingerprint and zkh_page_tree_plan_device take them (for a proof table_at = 5 + h), over an image of image_words words; the
 * table stands for the image: image[a_i] is the raw word table[3 i + 1].  Only an unlinked access of the paged record uses the image's word
 * (the read rule of a first load, prev_1 of a first access, p_in of its page), and it knows its page i from the page scan: one indexed read
 * and one address comparison per first access, no search, no W-word buffer.  EQUIVALENCE: for every (code, data, image) that
 * zkh_derive_links_paged accepts, the table (a_i, image[a_i] % P, anything) of its own page table makes this call leave `data` equal to the
 * image variant's, cell for cell as residues, and word for word when every image word it read is below P; after zkh_reduce_elem the two
 * traces are the same bytes.  REFUSALS: the image variant's, with the same text and precedence (`image_words` in W's place; "the image holds
 * .. at its address" for a first load the table contradicts), and three of its own, reported under the PAGES record's index R, the first two
 * tested on a row after "outside the image" and before the clock:
 *   "derive_links: record R at row r: address A is page I of the trace, but row I of the page table holds address B: the witness is refused"
 *   "derive_links: record R at row r: address A is page I of the trace, but the page table has D rows: the witness is refused"
 *   and, when no row is refused, "derive_links: record R: the trace pages D' addresses, but the page table has D rows: the witness is refused".
 * Before any launch: "a table of D rows of 3 words at word T does not fit a buffer of N words"; "an image of W words (1 .. 2^32 - 1)".  A
 * refusal leaves `data` unchanged; `table` and `code` are only read, rows [A, n) never touched; for a message the host reads single words of
 * the table, never the table.  Without a PAGES record the table is ignored (NULL or not) and the call is the plain one; with one, a NULL
 * table is refused ("a page table is required").
 * WIDE (ZKA1 version 10; versions 1..9 are word for word what they were): a paged memory of V = 2 value words per address, the two 16-bit
 * halves of a 32-bit machine word.  The PAGES record may name a LINK with READS and nc = 3 (a clock and two value columns; its ports, if
 * any, carry the same).  PAGES word 4 holds V - 1 (0 in every earlier blob; a value that is not the LINK's nc - 2 is refused), and the
 * record has 3 + 2 V + 2 ng destinations: p_on, p_addr, p_in_0 .. p_in_{V-1}, p_out_0 .. p_out_{V-1}, p_time, alimb_*, gap_*.  Header word 7
 * carries bit 19 (WIDE) exactly when V = 2: a version-10 blob without it is no ZKA1 blob, and bit 19 with V = 1 is refused; bits 16, 17
 * and 18 are set exactly when the blob holds a PAGES record, an OPEN record, a LINK that joins.  zkh_circuit_page_words: V, and 0 without
 * a PAGES record.  THE IMAGE IS FLAT: V W raw Montgomery words, word j of address a at image[V a + j]; a length that is no multiple of V
 * is refused before any launch ("an image of N words is not a whole number of addresses of V value words"), and "address A outside the
 * image of W words" counts W in addresses.  An unlinked access takes prev_{1+j} = image[V a + j] and prev_0 = 0, an unlinked load must
 * return both words (residues; a refusal names the lowest j first); the head of page i writes p_in_j = image[V a_i + j], the tail
 * p_out_j from its value columns.  zkh_page_out sets image[V a_i + j] = p_out_j[i].  THE FLAT TABLE: to the tree update, the ZKU1
 * proof, the walk, ZKN1 and the page-out circuits a wide page table of D rows is the table of V D rows (V a_i + j, in_j, out_j), i
 * major, j minor: strictly increasing flat addresses over the flat image, so none of them knows V, and zkh_image_proof_words is asked
 * about (V W, V D).  The proof's fourth refusal says "p_in word j X at address A" when V = 2.  zkh_derive_links_paged_table takes the flat
 * table: D counts its flat rows and image_words the flat image's words, the head of page i reads rows V i + j and checks each address
 * against V a + j, the trace's D' pages must meet V D' rows, and the three table refusals name the flat row.  The tie of a wide memory
 * (kinds 8 and 9) needs flat-address columns in the trace: its table's rows on the open bus are the flat table's.
 * FLAT (ZKA1 version 11; versions 1..10 are word for word what they were): PAGES word 5 holds F, the number of flat-address destinations,
 * 0 or 2 and 2 only with V = 2 (any other value, and F = 2 with V = 1, is refused); words 6, 7 hold the data columns p_flat_0, p_flat_1 (0
 * when F = 0), words 8..15 stay reserved.  Header word 7 carries bit 20 (0x100000, FLAT) exactly when F = 2: a version-11 blob without it
 * is no ZKA1 blob, bit 20 with no record of F = 2 is refused.  The links stage writes p_flat_j[i] = the canonical Montgomery encoding of
 * 2 a_i + j on page i < D (from the decoded address; p_addr stays the raw key word) and 0 on rows D <= i < A, in image and in table
 * mode, with and without ports, in the write pass it always ran: no new launch, the refusals unchanged.  p_flat_j are destinations like
 * the others (one writer, no record reads them, none is a multiplicity; terms may read them).  zkh_circuit_page_flats: F, and 0 without a
 * PAGES record.  A circuit constrains p_on (p_flat_j - 2 p_addr - j) = 0 and puts +p_on (p_flat_j, p_in_j, p_out_j) on the open bus, so
 * that a wide segment's open total is zkh_table_fingerprint of its flat table and kinds 8 and 9 tie it to its page-out as they are. */
int zkh_circuit_pages(const zkh_circuit*);
int zkh_circuit_page_words(const zkh_circuit*);
int zkh_circuit_page_flats(const zkh_circuit*);
const char* zkh_derive_links_paged(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data, const zkh_buf* image);
const char* zkh_derive_links_paged_table(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data, const zkh_buf* table,
                                         size_t table_at, size_t D, size_t image_words);
const char* zkh_page_out(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* data, zkh_buf* image);
/* THE IMAGE'S COMMITMENT: a Merkle root that the prover keeps current from segment to segment.  An image is W >= 1 raw Montgomery words,
 * W <= 2^32 - 1, as zkh_page_out takes it.  The commitment is a function of the RESIDUES, not of the raw words: image[a] and
 * image[a] + P are one memory and give one root.  L = the smallest power of two >= ceil(W / 8).  The tree is 2 L digests in heap order,
 * 16 L words, digest i at words [8 i, 8 i + 8): the `nodes` layout of zkh_merkle_fold_all(nodes, rows = L) and zkh_merkle_open.
 *   digest 0 is eight zero words;
 *   leaf digest L + j, word k, is image[8 j + k] % P for 8 j + k < W and 0 past the end of the image, in the last partial leaf and in
 *   every padding leaf alike: a leaf is eight memory words verbatim, not a hash;
 *   node i, 1 <= i < L, is hash_pair(node 2 i, node 2 i + 1): the Poseidon2 of zkh_hash_fold, the one operation P2-JOIN constrains;
 *   the root is digest 1 (for L = 1 it is the leaf).
 * zkh_image_tree_words: 16 L, and 0 for W = 0.  zkh_image_commit writes the whole tree of `image` into `nodes`: one pass for digest 0
 * and the leaf layer, the layers above as zkh_merkle_fold_all builds them.  It FAILS on W = 0, on W > 2^32 - 1 and on a `nodes` that is
 * not exactly zkh_image_tree_words(W) words.
 * zkh_page_out_tree is zkh_page_out followed by the update of `nodes`, as one call: the same check pass, the same refusals with the same
 * messages (image and nodes then unchanged; a wrong-sized `nodes` is refused before anything is written), the same scatter; then, with D
 * the rows of the table, the dirty leaves are rewritten from the image and only the nodes on the paths of the paged words are hashed
 * again, so that `nodes` equals, word for word, what zkh_image_commit writes for the new image.  `nodes` must hold the tree of `image`
 * as it was before the call.  D = 0 leaves `nodes` as it is.  No atomics: `nodes` is a function of the image alone. */
size_t zkh_image_tree_words(size_t image_words);
const char* zkh_image_commit(zkh_ctx*, const zkh_buf* image, zkh_buf* nodes);
const char* zkh_page_out_tree(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* data, zkh_buf* image, zkh_buf* nodes);
/* THE UPDATE'S PROOF, ZKU1: what takes a holder of root_before to root_after without the image.  W, L, `nodes` and "residue" are as
 * above.  h = log2 L.  Layer k, 0 <= k <= h, is the layer of width w = L >> k: heap indices [w, 2 w); k = 0 is the leaf layer.  A valid
 * page table has rows [0, D) with strictly increasing addresses a_i < W (what zkh_page_out's check pass establishes).
 *   S_0 = the distinct a_i >> 3, increasing; M = |S_0|.   S_{k+1} = the distinct x >> 1 for x in S_k.
 *   C_k, k < h: the clean siblings of layer k, { x ^ 1 : x in S_k, x ^ 1 not in S_k }, increasing; c_k = |C_k|.
 * A clean sibling is the same digest in the tree before and after the page-out, so one proof serves both roots.  A padding leaf can be a
 * clean sibling.  Digest 0 is never read.  The proof is a run of 32-bit words:
 *   word 0                 0x5a4b5531 ('ZKU1', written as ARGS_MAGIC is)
 *   words 1 .. 4           W, D, M, h
 *   words 5 .. 5 + h - 1   c_0 .. c_{h-1}
 *   then 3 D words         row i: a_i as an integer (the canonical value of p_addr), p_in[i] % P, p_out[i] % P (the residues of the raw
 *                          words: the space the tree lives in)
 *   then 8 M words         the leaves S_0, in order, as `nodes` holds them BEFORE the page-out
 *   then 8 sum c_k words   for k = 0 .. h - 1 in that order, the digests of C_k in increasing index
 * Its length is 5 + h + 3 D + 8 M + 8 sum c_k.  D = 0 gives the header alone, L = 1 no sibling section.  zkh_image_proof_words(W, D) is
 * the bound 5 + h + 3 D + 8 min(D, L) + 8 sum_{k<h} min(D, L >> (k + 1)): a clean sibling shares its pair with a dirty node, so c_k is at
 * most D and at most the number of pairs.  The bound is reached for D = 1 and for W <= 8.
 * zkh_page_out_proof writes the proof of the page table of `data` into `proof`.  It only READS data, image and nodes, `nodes` being the
 * tree of `image` as it is: call it BEFORE zkh_page_out_tree (the old leaves are taken from `nodes`).  The check pass is zkh_page_out's,
 * with the same three refusals and the same text after "page_out_proof: " (nothing is written, so no "the image is unchanged"), and one
 * more, tested after them on a row: p_in[i] % P is not the word the tree holds ("record R at row r: p_in X at address A, the tree holds
 * Y").  A `nodes` that is not zkh_image_tree_words(W) words is refused before any launch, and so is, after the check pass has given D, a
 * `proof` shorter than zkh_image_proof_words(W, D).  After a refusal the contents of `proof` are unspecified; words past the proof's
 * length are never written.  No atomics, no read-back after the check pass: the proof is a function of data and nodes alone.
 * zkh_image_proof_verify is HOST ONLY (no context, no GPU): the walk from `proof` and root_before to root_after, hashing through the
 * permutation of zkh_poseidon2_mix_host.
 *   The header is checked against the length; every word of the table's in / out, of the leaves and of the siblings must be < P; the
 *   addresses must increase and lie below W, and lie in M leaves.  Every in_i must equal word a_i & 7 of its old leaf; the new leaves are
 *   the old ones with out_i put in.  On layer k the walk goes through S_k in order: a node whose sibling is the next item pairs with it,
 *   any other takes the next digest of C_k, on the left when the node's index is odd; hash_pair of the old children and of the new ones
 *   give the parent's two digests.  Exactly c_k digests must be taken.  At the top the old digest must equal root_before; the new one is
 *   root_after (L = 1: the leaf is the root; D = 0: root_before).  Zero padding past W is not checked: root_before is the authority.
 * It FAILS with one message per cause, naming what and where: bad magic; an h that is not W's; a length other than what the header
 * describes; a word >= P (its offset); row i whose address does not follow a smaller one or lies outside the image; an M other than the
 * table's; row i whose `in` differs from its leaf's word; layer k with more or fewer siblings than the walk takes; "the proof opens root
 * .., not root_before".  root_after is written only on success.
 * zkh_image_proof_walk is the same walk ON THE DEVICE, for a rank that has a GPU but not the image, and for the prover checking the
 * proof it is about to ship: `proof` is a device buffer whose first `words` words are the proof (words <= the buffer's size, words <=
 * 2^32 - 1: refused before anything is read; the rest of the buffer is never read, so the buffer zkh_page_out_proof wrote goes in as it
 * is with the proof's own length).  `proof` is only read; root_before and root_after are host pointers.  For every (proof, root_before)
 * the call and zkh_image_proof_verify either both succeed with the same root_after or both fail with the same message after
 * "image_proof_walk: " / "image_proof_verify: ", the cause reported being the first in the host verifier's order when several apply.
 * One read-back fetches the header (5 + h words, at most 34), which is checked against the length by the code zkh_image_proof_verify
 * uses; everything after it is enqueued without synchronisation (per layer: the two flags of every item, one counter scan, the
 * parents, one Poseidon2 lane per hash_pair); one read-back fetches a 32-word record: the lowest index of every cause (atomicMin:
 * the result does not depend on arrival order; there are no other atomics), the values its message prints, both top digests.  No
 * kernel reads a proof word at or past `words` whatever the proof holds: a stage does nothing when an earlier refusal removes its
 * precondition.  Scratch comes from the context's pool, a small multiple of the proof's own size.  D = 0 launches nothing.
 * zkh_image_proof_nodes is zkh_image_proof_walk (its stages, its verdicts: the same root_after, or the same message after
 * "image_proof_nodes: "), and on success it also leaves in `dirty` the DIRTY-NODE TABLE of the page-out: every digest the walk
 * recomputes, which is everything a P2-TREE block of any part can ask for (zkh_page_tree_witgen_nodes).  Words (csrc/zkn1.h; the numpy
 * twin: logup.reference_page_out_nodes): 'ZKN1', W, D, h, n_1 .. n_h; then per layer k = 1 .. h (layer 0 the leaves, h the root) the
 * n_k heap ids of the layer's dirty nodes, increasing (the walk's list S_k), and n_k records of 32 words, the four digests of a node's
 * two children: left old ‖ left new ‖ right old ‖ right new.  A clean child has old = new, the proof's sibling; the children of a
 * layer-1 node are two leaves, 16 memory words.  The table's length is 4 + h + 33 sum n_k; zkh_image_dirty_words(W, D) = 4 + h +
 * 33 sum_k min(D, L >> k) bounds it for every table of D rows, a function of (W, D) alone (0 for W = 0).  `dirty` shorter than that
 * bound, or a bound past 2^32 - 1 words, is refused after the header's refusals and before any launch.  root_after and `dirty` are
 * written only on success (the table is built in scratch of the bound's size and copied once the record has come back clean); words of
 * `dirty` past the table's length are never written.  No atomics beyond the walk's record, one writer per word.  An empty table (D = 0)
 * is refused where the walk would succeed: "an empty table (D = 0) has no dirty nodes: its proof is the header alone and holds no
 * node, not even the root's children; such a page-out is sealed from the tree (zkh_page_tree_witgen)". */
size_t zkh_image_proof_words(size_t image_words, size_t pages);
size_t zkh_image_dirty_words(size_t image_words, size_t pages);
const char* zkh_page_out_proof(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* data, const zkh_buf* image, const zkh_buf* nodes,
                               zkh_buf* proof);
const char* zkh_image_proof_verify(const uint32_t* proof, size_t words, const uint32_t root_before[8], uint32_t root_after[8]);
const char* zkh_image_proof_walk(zkh_ctx*, const zkh_buf* proof, size_t words, const uint32_t root_before[8], uint32_t root_after[8]);
const char* zkh_image_proof_nodes(zkh_ctx*, const zkh_buf* proof, size_t words, const uint32_t root_before[8], uint32_t root_after[8], zkh_buf* dirty);
/* P2-PAGE (circuit kind 5, zeth_amd/circuits/p2_page.py; csrc/page_circuit.hip): the circuit that consumes a ZKU1 proof's table.  Its
 * seal proves "D single-word updates, applied one after the other, take root_before to root_after": out = root_before (8) ‖ root_after
 * (8).  Every update is one Merkle path of h = log2 L blocks of 31 rows (P2-JOIN's rows), the old path and the new one side by side;
 * N = ((2^po2 - zk_cycles) / 31) / h paths fit a trace, the slots past D are no-op updates of address 0.  It does NOT constrain that
 * the addresses increase (P2-PAGE-ordered, below, does), nor that the table is the page table of a paging segment's seal.  W > 8 (a path is at least one hash_pair)
 * and h <= 27 (the address is rebuilt in the field).
 * zkh_page_circuit_code writes the code group, a function of (po2, zk_cycles, h of `image_words`): what the control root commits to.
 * zkh_page_circuit_witgen writes the data group and out_roots = digest 1 of both trees.  `proof` is a device buffer whose first
 * `proof_words` words are a ZKU1 proof as zkh_page_out_proof left it; only its header (one read-back, checked as zkh_image_proof_walk
 * checks it) and its 3 D table words are read.  `nodes_before` / `nodes_after`: the tree before and after zkh_page_out_tree, each
 * exactly zkh_image_tree_words(W) words.  `code`: this (po2, zk_cycles, h)'s code group, only read.  noise_key: as zkh_syn_witgen's.
 * The generator reads the memory that update i opens from the two trees (`nodes_after` below a_i, `nodes_before` from a_i on: the
 * addresses increase), so every path is independent; it TRUSTS that the table matches the trees (zkh_image_proof_walk is the check
 * for that, and a table that does not gives a witness that zkh_check_rows refuses), but never reads outside `nodes_*` whatever the
 * table holds: a check pass comes first and no path is walked after a refusal.
 * It FAILS, after "page_circuit_witgen: ", one message per cause, in this order and before any launch: the circuit does not have
 * P2-PAGE's shape; buffer shape mismatch; the proof's header (zkh_image_proof_verify's messages); W <= 8; nodes of another size; D > N
 * (naming D, N, h and po2).  After the launches, from one read-back: the code group was not built for this h; row i whose address lies
 * outside the image or does not follow a smaller one (`data` is then unspecified).  The accum group is zkh_syn_accum's (P2-JOIN's
 * argument: one running product of mix + data column 0); the seal goes through zkh_prove_begin / zkh_prove_finish.
 * PARTS: a table of D > N rows is sealed as a chain.  A PART is the run of updates [first, first + count) of one table, count =
 * min(N, D - first); its trace is the circuit's as it stands, slot s holding update first + s and the slots count .. N - 1 the usual
 * no-ops (only the last part has any, so they still open the tree after the whole page-out); its out is (the root before update
 * `first`) ‖ (the root after update first + count - 1).  Part p + 1 opens the root part p left: the verifier of the chain checks that
 * link, the first root and every seal, all against ONE control root.  The circuit, the code group and the accum are untouched.
 * zkh_page_circuit_witgen_part is zkh_page_circuit_witgen for the part at `first`: the same operands (both trees are the WHOLE
 * page-out's, whichever part is laid out: the memory an update opens is chosen by its address, so the parts are independent and can be
 * generated in any order), the same refusals in the same order with the same text after "page_circuit_witgen_part: ", but no D > N
 * refusal, and in its place "first F, but the table has D rows" for first >= D (first = D = 0 is the empty table's one part).  The
 * check pass still covers the whole table and names a refused row by its index in the table.  For first > 0 the root before the part
 * is computed on the device (h hash_pairs: the new path of update first - 1); still one read-back, no atomics.
 * zkh_page_circuit_witgen is the part at first = 0 behind its D <= N refusal, word for word.
 * zkh_page_circuit_slots is HOST ONLY (no context, no GPU): N for (po2, zk_cycles, an image of `image_words` words), or 0 where
 * zkh_page_circuit_code refuses the shape.  The parts of a table of D rows start at 0, N, 2 N, ... below D (D = 0: one part at 0). */
const char* zkh_page_circuit_code(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, size_t image_words, zkh_buf* code);
const char* zkh_page_circuit_witgen(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* proof, size_t proof_words,
                                    const zkh_buf* nodes_before, const zkh_buf* nodes_after, zkh_buf* data, uint32_t out_roots[16], const uint32_t noise_key[8]);
const char* zkh_page_circuit_witgen_part(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* proof, size_t proof_words,
                                         const zkh_buf* nodes_before, const zkh_buf* nodes_after, size_t first, zkh_buf* data, uint32_t out_roots[16],
                                         const uint32_t noise_key[8]);
size_t zkh_page_circuit_slots(size_t po2, size_t zk_cycles, size_t image_words);
/* P2-PAGE-ordered (circuit kind 6, zeth_amd/circuits/p2_page_ordered.py; csrc/page_circuit.hip): P2-PAGE plus the constraint that the
 * addresses strictly increase.  Its seal proves "the LIVE updates of the part have strictly increasing addresses, all at or above lo;
 * hi is one more than the last of them, or lo if there is none; those updates, in that order, take root_before to root_after": out =
 * root_before (8) ‖ root_after (8) ‖ lo ‖ hi (18 words; lo and hi are field elements as the trace holds them, Montgomery words, which
 * the verifier decodes).  A chain whose part 0 has lo = 0 and whose part p + 1 starts at the root and the hi part p left seals a SET of
 * addresses, each written once, in order.  The trace is P2-PAGE's in a wider buffer: data columns 0 .. 124 and code columns 0 .. 38
 * are P2-PAGE's, written by the same kernels; data 125 live (1 on a real update's path, 0 on a no-op's), 126 lo (one more than the last
 * live address before the slot, in this part or an earlier one; 0 if none), 127 gbit / 128 gacc (the gap addr - lo one bit per row on
 * rows 1 .. 29 of a path's block 0, and its running sum); code 39 gsel, 40 gpow, 41 gend (those rows, 2^(k - 1) on them, the last of
 * them).  Still NOT constrained: that the table is the page table of a paging segment's seal (P2-PAGE-tied, below, adds that).
 * h <= 26 (images of at most 2^29 words), one less than P2-PAGE: the gap is decomposed into 29 bits, and addr = lo + gap is an integer
 * equation only while lo + gap < 2^30 < P.  N, the parts' plan and W > 8 are P2-PAGE's (zkh_page_circuit_slots).
 * zkh_page_ordered_code: zkh_page_circuit_code's operands, `code` of 42 x 2^po2 words.
 * zkh_page_ordered_witgen: zkh_page_circuit_witgen_part's operands, `first` included, `data` of 129 x 2^po2 words, out[18]; first = 0
 * with D <= N is the single-seal case.  One more kernel after P2-PAGE's, one lane per (path row, new column); still one read-back, no
 * atomics.  The refusals are zkh_page_circuit_witgen_part's, in the same order with the same text, after "page_ordered_code: " /
 * "page_ordered_witgen: ", but "the circuit does not have P2-PAGE-ordered's shape (kind 6, 42 / 129 / 4 columns, 18 outputs)", and after
 * P2-PAGE's h <= 27 refusal "an image of W words has h 27; the gap between two addresses is decomposed into 29 bits, which takes
 * addresses below 2^29: h <= 26".  A table whose addresses do not increase is the check pass's refusal as before: no path and no new
 * column is written after it.  The accum group is zkh_syn_accum's, as for kind 5.
 * P2-PAGE-tied (circuit kind 8, zeth_amd/circuits/p2_page_tied.py; DESIGN.md §2 "THE TIE"): P2-PAGE-ordered's code and data groups column
 * for column, so both calls serve it as they stand (they tell the circuit by its kind, and then ask for 30 outputs); out = these 18 words
 * ‖ alpha ‖ beta ‖ F, of which the witness call writes the 18.  Its accum group is an open bus: zkh_accumulate_open, not zkh_syn_accum. */
const char* zkh_page_ordered_code(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, size_t image_words, zkh_buf* code);
const char* zkh_page_ordered_witgen(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* proof, size_t proof_words,
                                    const zkh_buf* nodes_before, const zkh_buf* nodes_after, size_t first, zkh_buf* data, uint32_t out[18],
                                    const uint32_t noise_key[8]);
/* P2-TREE (circuit kind 7, zeth_amd/circuits/p2_tree.py; csrc/page_tree.hip): a page-out sealed by its DIRTY NODES instead of one path
 * per word.  Its seal proves "a set of pairs of leaves (16 words each), in strictly increasing order, is replaced, and the replacement
 * takes root_before to root_after": out = root_before (8) ‖ root_after (8) ‖ lo ‖ hi (18 words), lo and hi bounding the HEAP IDS of
 * the part's pair blocks (a pair of leaves q of a tree of L = 2^h leaves has id L/2 + q) as P2-PAGE-ordered's bound addresses.  A chain
 * whose part 0 has lo = 2^(h-1), whose part p + 1 opens the root and starts at the hi part p left, and whose last hi is at most 2^h
 * seals a page-out of any size; the verifier is told h.  The trace is B = (2^po2 - zk_cycles) / 31 blocks of P2-JOIN's 31 rows, one
 * tree node each, old and new permutation side by side; a parent reads its children over a bus in the accum group (24 columns), which
 * zkh_accumulate fills from the circuit's ZKA1 arguments (zkh_circuit_set_arguments with p2_tree.arguments()): zkh_syn_accum does not
 * serve kind 7.  The columns, the constraints and why the bus forces a tree: p2_tree.py.  NOT constrained by kind 7: which words of a pair
 * were touched, and that the table is the page table of a paging segment's seal; P2-TREE-tied constrains both.  W > 16, h = 2 .. 27, B >= h.
 * P2-TREE-tied (circuit kind 9, zeth_amd/circuits/p2_tree_tied.py): P2-TREE's code group and data columns 0 .. 105, then ch[16] and wa[16]
 * (138 data columns: on the input row of a pair block, which of its 16 words the part touches, and their addresses), an OPEN bus of 12
 * Fp4 accum columns (48; zkh_accumulate_open) and out = P2-TREE's 18 words ‖ base ‖ alpha ‖ beta ‖ F (31).  Both calls below serve it:
 * the circuit's own kind decides the shape, and a circuit of neither kind is refused in P2-TREE's words.
 * zkh_page_tree_code: `code` of 41 x 2^po2 words, a function of (po2, zk_cycles) alone: one control root for every image size; the
 * same words for kind 7 and kind 9.
 * zkh_page_tree_plan (HOST ONLY): the parts of a table with the addresses addrs[0 .. D) (strictly increasing, below image_words), greedy:
 * a part takes whole pairs of leaves while its nodes stay at most B, its first pair costing h nodes and every later one bit_length(pair
 * index xor the one before).  parts[2 p], parts[2 p + 1] = (first, count) of part p for p < parts_cap; *n_parts is the number of parts
 * whatever parts_cap is (D = 0: the one part (0, 0)).  The addresses are the host's: a host that holds no copy of the table plans with
 * zkh_page_tree_plan_device.
 * zkh_page_tree_plan_device: the same plan over a table where it lies on the device: the words of `table` from `table_at` on are D rows
 * of a ZKU1 table (stride 3, the address first; for a proof table_at = 5 + h), in any buffer, with no proof needed around them.  The plan
 * as a prefix sum and a search (DESIGN.md "THE PLAN AS A SCAN"): a costs pass of 256 rows a workgroup, a scan of the workgroups' sums,
 * one wave that walks from part to part; no atomics, one writer per cell.  parts, parts_cap and n_parts as zkh_page_tree_plan's; nodes
 * (may be NULL): nodes[p] = the dirty nodes of part p (at most B), for p < parts_cap.  What is read back is the record and the parts
 * written, never a word per row.  Refusals after "page_tree_plan_device: ", in this order: "null argument"; "po2 P out of range for Z
 * zk_cycles"; the image's shape as zkh_page_tree_plan; "a table of D rows of 3 words at word T does not fit a buffer of N words"; "a
 * table of D rows (at most 1073741824: ...)" (no table of more rows increases below the 2^30 words of the largest image); then the
 * LOWEST row of the whole table that breaks the table's rule, in zkh_page_tree_witgen's words: "row R: address A outside the image of
 * W words" or "row R: address A does not follow a smaller one (row R-1: address A')".  On a refusal nothing is written, *n_parts
 * included.
 * zkh_page_tree_witgen: zkh_page_ordered_witgen's operands with the part as (first, count), `data` of 106 x 2^po2 words (kind 9: 138 x
 * 2^po2, the 32 word columns by one more kernel, one lane per cell), out[18] for both kinds (kind 9: the caller appends base =
 * Montgomery(2^(h+3)), the challenge and the total).  Both trees are the WHOLE page-out's for every part.  One read-back at the end, no atomics, one writer per cell.  Refusals after
 * "page_tree_witgen: " (the shape ones also after "page_tree_code: " / "page_tree_plan: "): "the circuit does not have P2-TREE's shape
 * (kind 7, 41 / 106 / 24 columns, 18 outputs)"; "an image of W words has a single pair of leaves (W > 16: ...)"; "no room for the h H
 * nodes of one path in B block slots"; the proof header's and the tree buffers' as zkh_page_circuit_witgen; "the part [F, E) of a table
 * of D rows"; then, from the check pass over the whole table and before any tree is indexed: "row R: address A outside the image of W
 * words", "row R: address A does not follow a smaller one (row R-1: address A')", "the part [F, E) splits a pair of leaves: rows R-1
 * and R write the same 16 words", "the part [F, E) has N dirty nodes, but po2 P leaves B block slots".  A table that does not match
 * the trees is not refused here: its bus does not balance, zkh_accumulate refuses it and zkh_check_bus names the key.
 * zkh_page_tree_witgen_nodes: the same witness, cell for cell, from (proof, dirty) alone: zkh_page_tree_witgen's operands with the
 * dirty-node table zkh_image_proof_nodes left (THE UPDATE'S PROOF above) in place of the two trees, for a rank that holds neither.
 * The source rule is the same (a child below the part's edge address is the new tree's, one above it the old tree's, the one that
 * holds it comes from the edge chain); a block finds its node by ONE binary search of its layer's ids and takes the record's old or
 * new digest.  Refusals after "page_tree_witgen_nodes: ": zkh_page_tree_witgen's in its order, with, in the place of the tree
 * buffers', the table's header against the buffer's length and the proof, all on the host before any launch: "dirty nodes of N
 * words: the header alone has 4"; "dirty nodes: bad magic .."; "dirty nodes: h H, but an image of W words has h H'"; "dirty nodes: N
 * nodes on layer K, but D rows dirty at most C of its X"; "dirty nodes of N words, but the header describes at least M"; "dirty nodes
 * of D rows over W words (h H), but the proof has D' rows over W' words (h H')"; "an empty table (D = 0) has no dirty nodes; such a
 * page-out is sealed from the tree"; and last, from the one read-back: "node N of layer K is not in the dirty nodes (the table is
 * another proof's)", N the lowest such heap id (one atomicMin on the record), after which no cell of a block is written.  No index
 * read from `dirty` is used before it is bounded by a count the host has checked.  A table with the right ids and other digests is
 * not refused here, as a tree that does not match is not: the bus does not balance. */
const char* zkh_page_tree_code(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, zkh_buf* code);
const char* zkh_page_tree_plan(size_t po2, size_t zk_cycles, size_t image_words, const uint32_t* addrs, size_t D, size_t* parts, size_t parts_cap,
                               size_t* n_parts);
const char* zkh_page_tree_plan_device(zkh_ctx*, size_t po2, size_t zk_cycles, size_t image_words, const zkh_buf* table, size_t table_at, size_t D, size_t* parts,
                                      size_t parts_cap, size_t* n_parts, uint32_t* nodes);
const char* zkh_page_tree_witgen(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* proof, size_t proof_words,
                                 const zkh_buf* nodes_before, const zkh_buf* nodes_after, size_t first, size_t count, zkh_buf* data, uint32_t out[18],
                                 const uint32_t noise_key[8]);
const char* zkh_page_tree_witgen_nodes(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* proof, size_t proof_words,
                                       const zkh_buf* dirty, size_t first, size_t count, zkh_buf* data, uint32_t out[18], const uint32_t noise_key[8]);
/* Everything a circuit's arguments derive, in the one order in which it is sound: sorted copies, then columns, then links, then
 * multiplicities (a LIMBS / ORDER record may read a sorted copy's column, and the multiplicities count the limbs that the records and
 * the links derive).  Call it after the data upload and before zkh_prove_begin: what it writes belongs to the data group.  It runs
 * every stage whose zkh_circuit_derives_* holds, with the arguments as given, and launches nothing of its own; a circuit without
 * arguments, or whose arguments derive nothing, is a no-op that looks at no other argument, so the call needs no guard.  A NULL
 * circuit is its only own error.  The first stage that fails ends the call with that stage's error; that stage has left `data` as it
 * found it, the stages before it have written their columns. */
const char* zkh_derive_all(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data);
/* ... and the same with the memory image that the links stage of a paging circuit reads (zkh_derive_links_paged); zkh_derive_all is this
 * call with no image.  A paging circuit without an image is refused before any stage has written. */
const char* zkh_derive_all_paged(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data, const zkh_buf* image);
/* ... and with the page table of a ZKU1 proof in the image's place (zkh_derive_links_paged_table, PAGING above): the links stage gets the
 * table where zkh_derive_all_paged hands it the image; every other stage is the same. */
const char* zkh_derive_all_paged_table(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data, const zkh_buf* table,
                                       size_t table_at, size_t D, size_t image_words);
/* The data columns that zkh_derive_sorted, zkh_derive_columns, zkh_derive_links and zkh_derive_multiplicities write on the active rows: their sorted
 * union in cols[0 .. *n) (cap = room in cols; *n is set even when the call fails for lack of room).
 * zkh_upload_data_trace copies a caller's data trace (`host`, W_data x 2^po2 words) into `data` without what the library derives:
 * columns outside that set whole, runs of adjacent columns as one copy; the derived columns on the blinding rows [2^po2 - zk_cycles,
 * 2^po2) only (the host still supplies those), one strided copy per run.  What it does not copy it does not write: derive before
 * use.  pinned_async != 0: `host` lies in a zkh_host_alloc block and the copies are enqueued without a host sync (zkh_write_async);
 * 0: any host memory, consumed before the call returns (zkh_write).
 * zkh_ctx_h2d_bytes: the bytes this context has copied host to device since it was created (zkh_write, zkh_copy_from, zkh_write_async,
 * zkh_upload_data_trace and the library's own uploads through them; not the tables of context and circuit set-up). */
const char* zkh_circuit_derived_data_columns(const zkh_circuit*, uint32_t* cols, size_t cap, size_t* n);
const char* zkh_upload_data_trace(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, zkh_buf* data, const uint32_t* host, int pinned_async);
size_t zkh_ctx_h2d_bytes(const zkh_ctx*);

/* ---- built-in witness generators on the device, by circuit kind (desc word 13) ----
 *   kind 1 SYN-AIR   stands in for risc0-circuit-rv32im's witgen (declared synthetic)
 *   kind 2 KECCAK-F  every 25 active rows are one real keccak-f[1600] permutation (zeth_amd/circuits/keccak_f.py; stands
 *                    in for risc0-circuit-keccak 4.0.2, /root/reference/Cargo.lock:5289).  For this kind `pub` is the optional
 *                    input state of the LAST permutation (25 lanes = 50 words, low word first; NULL = seeded like the others)
 *                    and out_global receives its output state as 100 16-bit limbs (lane l, limb j at 4 l + j).
 *   kind 3 P2-JOIN   every 31 active rows are one Poseidon2 permutation; block 0 = hash_pair(left, right) (zeth_amd/circuits/
 *                    p2_join.py; stands in for the in-circuit hashing of risc0-circuit-recursion 4.0.2, Cargo.lock:5305).
 *                    `pub` = the two child claims (16 words, required); out_global = parent (8) ‖ left (8) ‖ right (8).
 *   kind 5 P2-PAGE   has a generator of its own, zkh_page_circuit_code / zkh_page_circuit_witgen above (its inputs are a proof and
 *                    two trees, not a seed); zkh_syn_accum builds its accum group, which is P2-JOIN's.
 *   kind 6 P2-PAGE-ordered  likewise: zkh_page_ordered_code / zkh_page_ordered_witgen above, and zkh_syn_accum.
 *   kind 7 P2-TREE   zkh_page_tree_code / zkh_page_tree_witgen above; its accum group is a bus: zkh_accumulate, not zkh_syn_accum.
 *   kind 9 P2-TREE-tied  the same two calls; its accum group is an open bus: zkh_accumulate_open. */
/* BLINDING ROWS.  The last zk_cycles rows of every data / accum column are zero-knowledge blinding noise.  Upstream draws each
 * cell from the OS RNG (`Elem::random(&mut rng)`); here the randomness enters once per call as a 256-bit key — `noise_key`, 8
 * words — and every cell is ChaCha12(key; counter = (row, column), nonce = (group, "ZKN1")) folded mod P the way upstream's
 * Elem::random folds six u32 draws (csrc/noise.h; CPU twin oracle/noise.h).  noise_key == NULL or all-zero: 256 fresh bits from
 * getrandom() for this call — the product default; the call FAILS if the OS cannot deliver.  A fixed key makes seals reproducible
 * (tests, bench.py, golden fixtures).
 * The two host functions below expose the generator itself (no GPU): one blinding cell, and the underlying RFC 8439 block function
 * with `double_rounds` double rounds (10 = ChaCha20: what the RFC's test vector pins; the stream uses 6). */
uint32_t zkh_noise_cell_host(const uint32_t noise_key[8], uint32_t group, uint32_t column, uint32_t row);
void zkh_chacha_block_host(const uint32_t key[8], const uint32_t counter_nonce[4], int double_rounds, uint32_t out[16]);
/* code group only: a function of (circuit, po2, zk_cycles) — what the control root commits to */
const char* zkh_syn_code(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, zkh_buf* code);
/* pub: OUTPUT_SIZE - 4 public input words (Montgomery; NULL if the circuit has none); out_global: OUTPUT_SIZE words;
 * code may be NULL for kinds 1 and 2 (the caller already holds this size's code group, e.g. resident in its prover) */
const char* zkh_syn_witgen(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, uint64_t seed,
                           const uint32_t noise_key[8], const uint32_t* pub, zkh_buf* code, zkh_buf* data, uint32_t* out_global);
const char* zkh_syn_accum(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const uint32_t noise_key[8],
                          const zkh_buf* data, const uint32_t* mix_global, zkh_buf* accum);
/* Chained sessions (SYN-C: a kind-1 circuit with ONE public input = the segment's pre-state; out = (post, 0, 0, 0, pre)): what each
 * of n segments (seed, po2) adds to the running state — its post-state when started from state 0 — in one launch.  The executor's
 * part: with these a host fixes every segment's pre-state before any segment is proven (upstream's executor fixes
 * ReceiptClaim.pre / .post the same way), which keeps the segments independent for the provers. */
const char* zkh_syn_chain_contributions(zkh_ctx*, const zkh_circuit*, const uint64_t* seeds, const uint32_t* po2s, size_t n,
                                        size_t zk_cycles, uint32_t* contributions);

/* ---- trace-driven witness (csrc/preflight.hip).  Upstream: the rv32im preflight replays a segment's cycles
 * on one host thread into per-cycle records, witgen kernels fill the trace rows from them (one lane per cycle) and Hal::scatter
 * places the preloaded memory image (risc0-circuit-rv32im 4.0.2 prove/witgen, un-vendored: /root/reference/Cargo.lock:5320; the
 * guest input enters at /root/reference/crates/host/src/lib.rs:132-136).  Here the same pipeline for SYN-AIR circuits (kind 1,
 * no public inputs) with a stand-in machine: zkh_syn_preflight is the SEQUENTIAL host producer — 4 words (16 bytes) per active
 * cycle (value, operand, pc | op | rd | address, running state digest), all valid Elem words, plus the 1024-word RAM image before
 * the first cycle — and zkh_syn_witgen_trace expands records
 * that are already on the device (zkh_write_async from pinned memory: 16.7 MB per po2-20 segment instead of the 0.94 GB full
 * trace) into the data group: one row-fill launch, the running-sum scan, the preload through zkh_scatter. ---- */
size_t zkh_syn_preflight_ram_words(void);
const char* zkh_syn_preflight(uint64_t seed, size_t po2, size_t zk_cycles, uint32_t* records, uint32_t* ram_image,
                              double* cpu_seconds);
const char* zkh_syn_witgen_trace(zkh_ctx*, const zkh_circuit*, size_t po2, size_t zk_cycles, const uint32_t noise_key[8],
                                 const zkh_buf* records, const uint32_t* ram_image, zkh_buf* code, zkh_buf* data,
                                 uint32_t* out_global);

/* ---- segment prover: SegmentProver::prove_segment + risc0_zkp::prove::Prover ---- */
const char* zkh_prover_create(zkh_ctx*, const zkh_circuit*, zkh_prover** out);
void zkh_prover_destroy(zkh_prover*);   /* before zkh_ctx_destroy: a prover may hold device buffers (zkh_prover_cache_code) */
/* Seal one segment of a SYN-AIR-family circuit (kind 1: the accum witness generator is zkh_syn_accum) whose code/data
 * traces are already resident in HBM (W x 2^po2 each); out_global has OUTPUT_SIZE words.  On success *seal is a
 * malloc'd word array (release with zkh_free_seal). */
const char* zkh_prove_segment(zkh_prover*, size_t po2, size_t zk_cycles, const uint32_t noise_key[8], const zkh_buf* code,
                              const zkh_buf* data, const uint32_t* out_global, uint32_t** seal,
                              size_t* seal_words);
void zkh_free_seal(uint32_t* seal);
/* The same seal in the two halves upstream's SegmentProver drives `Prover` in, for ANY circuit and for traces the caller
 * produced itself (uploaded with zkh_copy_from / zkh_write_async):
 *   zkh_prove_begin : header, Prover::commit_group(code), commit_group(data); returns the accum mix challenges
 *                     (global_size[mix] words into mix_global, may be NULL) drawn from the transcript;
 *   (caller)        : fills the accum trace (W_accum x 2^po2) from data + mix — CircuitHal::accumulate, circuit-specific;
 *   zkh_prove_finish: commit_group(accum) + Prover::finalize (eval_check, DEEP, FRI, queries).  Consumes the job whether
 *                     or not it succeeds; zkh_prove_abort drops a job that will not be finished. */
typedef struct zkh_seal_job zkh_seal_job;
/* The code (control) group is a function of (circuit, po2) alone — it is what the control ID commits to — yet upstream's
 * SegmentProver re-commits it for every segment.  A prover that seals many segments of one size can keep that group's
 * committed form (coefficients, 4n evaluations, Merkle nodes: 0.6 GB at po2 20, W_code 16) resident in HBM:
 * zkh_prover_cache_code commits `code` once for this po2 (replacing an earlier entry); afterwards zkh_prove_begin /
 * zkh_prove_segment accept code == NULL for that po2 and share the resident group read-only.  Seals are byte-identical
 * to the ones made from the same code trace.  The caller vouches that the trace is the circuit's code trace for that
 * size (the verifier still checks the root against the control root).  zkh_prover_drop_code_cache releases the entries.
 * REDUCED WORDS IN.  zkh_prove_begin, zkh_prove_segment, zkh_prover_cache_code and zkh_code_root take device-resident traces of
 * reduced words (< P), like the Hal-level ops they drive (the NTTs, hash_rows, hash_fold, the eltwise ops): a raw word >= P is not
 * refused, it seals to something no verifier accepts.  A caller whose traces may hold such words (the entry points over arguments
 * as data read a cell as its residue, and the derives copy raw words) calls zkh_reduce_elem on code and data after zkh_derive_all
 * and before zkh_prove_begin, as zkh_session_prove does for a segment with host traces. */
const char* zkh_prover_cache_code(zkh_prover*, size_t po2, const zkh_buf* code);
void zkh_prover_drop_code_cache(zkh_prover*);
/* Root of the resident code group of this size.  The entry is keyed by po2 alone although a code trace also depends on
 * zk_cycles: a host that changes zk_cycles must re-cache, and can compare this root with the control root it expects. */
const char* zkh_prover_cached_code_root(zkh_prover*, size_t po2, uint32_t root[8]);
const char* zkh_prove_begin(zkh_prover*, size_t po2, const zkh_buf* code, const zkh_buf* data, const uint32_t* out_global,
                            zkh_seal_job** job, uint32_t* mix_global);
const char* zkh_prove_finish(zkh_seal_job*, const zkh_buf* accum, uint32_t** seal, size_t* seal_words);
void zkh_prove_abort(zkh_seal_job*);
/* Control root = Merkle root of the committed code group (the control-ID analogue: risc0-zkp verify/mod.rs check_code).
 * zkh_code_root commits a caller-supplied code trace; zkh_syn_control_root generates SYN-AIR's for (po2, zk_cycles). */
const char* zkh_code_root(zkh_prover*, const zkh_buf* code, size_t po2, uint32_t root[8]);
/* zkh_data_root commits a data trace as zkh_prove_begin will: the root the seal of this trace carries, known before the seal is made
 * (the shared challenge of a tied group hashes the data roots of all its seals: zkh_tie_challenge).  zkh_prove_begin commits the group
 * again; to commit it ONCE, hold the commitment:
 *   zkh_commit_data      : zkh_data_root that keeps what it built (REDUCED WORDS IN, as above).  The commitment holds three device
 *                          buffers of its own (coefficients, 4n evaluations, Merkle nodes) and does not alias `data`: the caller may
 *                          overwrite or release the trace afterwards.  zkh_data_root is this call and a release.
 *   zkh_commitment_root  : the root zkh_data_root gives.
 *   zkh_commitment_bytes : the device bytes of the three buffers as zkh_ctx_memory's live_bytes counts them: 4 n (5 W + 64) for W
 *                          columns at n = 2^po2 rows (0 for NULL).
 *   zkh_prove_begin_held : zkh_prove_begin with the data group shared from the commitment instead of committed from a trace: the same
 *                          header, transcript order (code, then data) and mix draw, code == NULL with a resident code group as there,
 *                          hence the same seal byte for byte.  It SHARES and does not consume: the job takes its own references, so the
 *                          commitment may be released before zkh_prove_finish, and one commitment may seed several jobs.  It refuses,
 *                          before any launch and before a job exists, each with its own message naming both values: a NULL argument; a
 *                          commitment made by a prover of another context; one whose column count is not this circuit's W_data; one
 *                          whose po2 is not the call's; and what zkh_prove_begin refuses of po2 and out_global, in the same words after
 *                          the prefix.  A refusal leaves the commitment untouched and usable.
 *   zkh_commitment_release: drops the commitment's references (NULL is a no-op).
 * DESTRUCTION ORDER: a commitment holds its buffers by reference count and keeps no pointer to the prover that made it, so it may be
 * released after zkh_prover_destroy; like every zkh_buf it must be released before zkh_ctx_destroy. */
typedef struct zkh_commitment zkh_commitment;
const char* zkh_data_root(zkh_prover*, size_t po2, const zkh_buf* data, uint32_t root[8]);
const char* zkh_commit_data(zkh_prover*, size_t po2, const zkh_buf* data, zkh_commitment** out);
const char* zkh_commitment_root(const zkh_commitment*, uint32_t root[8]);
size_t zkh_commitment_bytes(const zkh_commitment*);
void zkh_commitment_release(zkh_commitment*);
const char* zkh_prove_begin_held(zkh_prover*, size_t po2, const zkh_buf* code, const zkh_commitment* data, const uint32_t* out_global,
                                 zkh_seal_job** job, uint32_t* mix_global);
const char* zkh_syn_control_root(zkh_prover*, size_t po2, size_t zk_cycles, uint32_t root[8]);

/* ---- verifier: risc0_zkp::verify::verify — what `receipt.verify(image_id)` (cli.rs:103) runs per segment ----
 * Pure host code, no GPU needed: the circuit may be loaded with ctx == NULL (zkh_circuit_load(NULL, ...)).
 * control_root: the expected code commitment for (circuit, po2) — REQUIRED (check_code: a seal whose code group is
 * anything else, e.g. all-zero selectors, is rejected).  rc / diag: canonical Poseidon2 tables (24*29 / 24 words) or
 * NULL for the shipped ones.  NULL = seal accepted. */
/* THE TIE, HOST ONLY.  zkh_seal_data_root: the root of the data group a seal commits to, folded from the top layer the seal carries as
 * zkh_verify_segment folds it; it reads the header and the two tree tops only, so verify the seal first.
 * zkh_tie_challenge: challenge[8] = alpha ‖ beta of a tied group from its n data roots in order (the segment's, then the parts'): the hash
 * suite's digest of ('ZKT1', n, the roots) seeds a fresh transcript generator, and eight random elements follow.  Prover and verifier
 * call this one function. */
const char* zkh_seal_data_root(const zkh_circuit*, const uint32_t* seal, size_t seal_words, uint32_t root[8]);
const char* zkh_tie_challenge(const uint32_t* roots, size_t n, uint32_t challenge[8]);
const char* zkh_verify_segment(const zkh_circuit*, const uint32_t* seal, size_t seal_words, const uint32_t control_root[8],
                               const uint32_t* rc, const uint32_t* diag);

/* Claim digest of a sealed segment = Poseidon2(out globals, po2, control root): what a join receipt commits to for each
 * of its two children (zeth_amd/host.py; upstream: ReceiptClaim digests inside risc0-zkvm's lift/join).  Host only. */
const char* zkh_receipt_claim(const zkh_circuit*, const uint32_t* seal, size_t seal_words, const uint32_t control_root[8],
                              const uint32_t* rc, const uint32_t* diag, uint32_t claim[8]);

/* Receipt container: a versioned little-endian word envelope around a seal carrying what upstream's SegmentReceipt does
 * (circuit hash, po2, hash function, segment index, control root, claim digest, seal, checksum; layout: csrc/verifier.hip).
 * Stands in for the bincode `SegmentReceipt` inside `ProveInfo` (risc0-zkvm 3.0.3, decoded by zeth at
 * /root/reference/crates/host/src/lib.rs:137).  Host only.  *blob is malloc'd: release with zkh_free_seal. */
const char* zkh_receipt_encode(const zkh_circuit*, const uint32_t* seal, size_t seal_words, uint32_t segment_index,
                               const uint32_t control_root[8], uint32_t** blob, size_t* blob_words);
/* Parse + integrity-check (checksum, version, hash-suite, and with a circuit: desc hash, output size, po2, claim digest).
 * The checksum is FNV-1a: it detects corruption, not forgery; with circuit == NULL only the envelope is checked and NOTHING
 * is authenticated.  Authenticity comes from zkh_verify_segment on the seal against the EXPECTED control root, never from here.
 * info receives header words [0, 26); the seal sits at blob + *seal_offset (info[9] words).  Does NOT verify the seal. */
const char* zkh_receipt_decode(const zkh_circuit*, const uint32_t* blob, size_t blob_words, uint32_t info[26],
                               size_t* seal_offset);

/* ---- RECURSION circuit (kind 4): lift / join as programs of an in-circuit STARK verifier ----
 * Replaces risc0-circuit-recursion 4.0.2 src/prove/{mod.rs Prover::run, program.rs} + its witness generator (un-vendored:
 * /root/reference/Cargo.lock:5305), reached from default_prover().prove (/root/reference/crates/host/src/lib.rs:137) once per
 * lift and per join (BASELINE.json config 5).  The circuit: zeth_amd/circuits/recursion.py (six Fp4 wires + one gate per row,
 * Poseidon2 blocks, a copy argument in the accum group); a PROGRAM = the code group, produced by
 * zeth_amd/circuits/rec_verify.py (build_lift / build_lift2 / build_join = this library's verifier restated gate by gate) as a u32 blob.
 * zkh_rec_program_load validates the blob, sorts its witness schedule into dependency levels, uploads it, generates the code
 * group and commits it (resident); `circuit` = the RECURSION description loaded on the same context.  zkh_rec_prove runs the
 * program on `inputs` (raw Montgomery words: the child seal(s) and the program's other witness words), which FAILS unless every
 * assertion of the in-circuit verifier holds, and seals the trace; out_global (16 words) = claim (8) ‖ allowed-programs root.
 * A program handle owns its witness buffers and the hipGraph of its schedule: one zkh_rec_witgen / zkh_rec_prove at a time per
 * handle (every lane loads its own). */
typedef struct zkh_rec_program zkh_rec_program;
/* The circuit DESCRIPTIONS compiled into the library (the shipped circuits of zeth_amd/circuits/: syn_a, syn_small, syn_tiny, syn_join,
 * syn_chain, syn_heavy, keccak_f, p2_join, recursion), for hosts without Python; the words are static data (do not free). */
size_t zkh_shipped_circuit_count(void);
const char* zkh_shipped_circuit_name(size_t i);                       /* NULL past the end */
const char* zkh_shipped_circuit_desc(const char* name, const uint32_t** words, size_t* n_words);
/* The program BUILDER on the host, in C++ (csrc/rec_builder.hip; no GPU, no Python): what zeth_amd/circuits/rec_verify.py +
 * recursion.py Program.finish produce, word for word (upstream ships its lift / join programs as precompiled .zkr files; a host
 * without Python builds them here).  kind 0 lift: child_desc = the SEGMENT circuit, po2s[0], control_roots = the 8 words of
 * its control root at that size as the library hands them out (zkh_syn_control_root: Montgomery form); kind 2 lift2: po2s[0..2),
 * control_roots = 16 words (left, right); kind 1 join /
 * kind 3 join3: child_desc = the RECURSION circuit, po2s[0..2) / [0..3), control_roots = NULL; kind 4 union (two receipts of any
 * claims -> the digest of the sorted pair; inputs: seal, membership path per child, then the swap bit) / kind 5 resolve (the
 * conditional receipt, opened, bound to its assumption receipt): child_desc = the RECURSION circuit, po2s[0..2).  The program is placed at the
 * smallest po2 that holds it (blob[2]); *blob is malloc'd: release with zkh_free_seal. */
const char* zkh_rec_build_program(uint32_t kind, const uint32_t* child_desc, size_t child_desc_words, const uint32_t* po2s,
                                  const uint32_t* control_roots, uint32_t zk_cycles, uint32_t** blob, size_t* words);
const char* zkh_rec_program_load(zkh_ctx*, const zkh_circuit* circuit, const uint32_t* blob, size_t words, zkh_rec_program** out);
void zkh_rec_program_destroy(zkh_rec_program*);
/* root: the program's control root (Merkle root of its code group); info: po2, zk_cycles, input words, permutations, gates,
 * witness ops, dependency levels, variables */
const char* zkh_rec_program_info(const zkh_rec_program*, uint32_t root[8], uint32_t info[8]);
/* > 0: the witness schedule is replayed as a hipGraph (opt-in: ZKH_REC_GRAPH=1 when the program is loaded); the value is the
 * number of steps of its launch plan (runs of narrow levels in one persistent workgroup + single wide levels).  0: the plan is
 * launched kernel by kernel (the default: measured equal, and profilers cope with it). */
int zkh_rec_program_has_graph(const zkh_rec_program*);
const char* zkh_rec_code(const zkh_rec_program*, zkh_buf* code /* 58 x 2^po2 */);
const char* zkh_rec_witgen(const zkh_rec_program*, const uint32_t* inputs, size_t n_inputs, const uint32_t noise_key[8],
                           zkh_buf* data /* 72 x 2^po2 */, uint32_t out_global[16]);
const char* zkh_rec_accum(const zkh_rec_program*, const uint32_t noise_key[8], const zkh_buf* data, const uint32_t* mix_global /* 20 */,
                          zkh_buf* accum /* 12 x 2^po2 */);
const char* zkh_rec_prove(const zkh_rec_program*, const uint32_t* inputs, size_t n_inputs, const uint32_t noise_key[8],
                          uint32_t out_global[16] /* may be NULL */, uint32_t** seal, size_t* seal_words);

/* ---- session executor: ProverServer::prove_session / ProverImpl::{prove_segment, join} (risc0-zkvm 3.0.3, un-vendored:
 * /root/reference/Cargo.lock:5418) — what default_prover().prove(env, elf) runs once the executor has cut the guest's run
 * into segments (/root/reference/crates/host/src/lib.rs:137), as ONE call: every segment sealed on G devices x K lanes through
 * one shared work index (segments are independent: no exchange between devices), receipts in index order, optionally folded
 * through the P2-JOIN tree to one root receipt; zkh_session_verify is receipt.verify (cli.rs:103) for the result.
 * A session owns its lanes (one zkh_ctx + circuit + prover each) and runs one zkh_session_prove at a time. ---- */
typedef struct zkh_session zkh_session;
typedef struct {
    uint32_t po2;                 /* segment size 2^po2 cycles */
    uint64_t seed;                /* built-in witness generators (circuit kind 1..3): witness seed */
    uint32_t noise_key[8];        /* blinding rows: 256-bit ChaCha12 key; all-zero = fresh OS randomness per segment (the product default, like upstream) */
    const uint32_t* pub;          /* public inputs of the built-in generators (see zkh_syn_witgen), may be NULL */
    size_t n_pub;
    /* caller-produced traces instead (CPU preflight + witgen, upstream's flow): W_code x 2^po2, W_data x 2^po2 words and
     * OUTPUT_SIZE out globals; accum comes from the session's accumulate callback if one is set, else the built-in generator of
     * kinds 1..3, else zkh_accumulate when the circuit carries arguments (zkh_circuit_set_arguments on every lane's circuit) */
    const uint32_t* host_code;
    const uint32_t* host_data;
    const uint32_t* out_global;
} zkh_segment;
typedef struct {
    size_t n_segments;
    uint32_t** seals;             /* n_segments malloc'd seals in index order (the composite receipt) */
    size_t* seal_words;
    uint32_t* root_seal;          /* the root join receipt, or NULL (no join tree requested / one segment) */
    size_t root_seal_words;
    size_t n_joins;
    double wall_s, leaves_s, join_s;            /* whole call, leaf phase, join tree */
    double witgen_s_sum, seal_s_sum;            /* summed over segments (lane seconds) */
    size_t n_lifts;                             /* join_tree == 2: proofs of the bottom level (lifts, or lift2 per pair) + one lift per assumption receipt; the root is a RECURSION seal (n_joins then counts joins, join3s, unions and the resolve) */
    size_t root_program;                        /* ... and the index of the program the root was sealed under */
    double lift_s;                              /* ... the bottom level (join_s is then the joins alone) — with the streamed fold: what
                                                 * each still took AFTER the last segment was sealed (most of it overlapped the leaves) */
    size_t n_retries;                           /* segments handed to another lane after a failed attempt (ZKH_SEGMENT_RETRIES, default 1) */
    double fold_tail_s;                         /* join_tree == 2: last segment sealed -> root receipt */
    double fold_busy_s_sum;                     /* ... lane seconds spent inside lift / lift2 / join proofs */
    int streamed;                               /* ... 1 = fold nodes were proven as soon as their children existed (the default) */
    double preflight_cpu_s_sum;                 /* witness source 1: host CPU seconds spent in the sequential preflight, summed over segments */
    double trace_bytes;                         /* ... bytes that crossed PCIe as witness input (16 per cycle + the RAM image), summed */
    uint32_t root_core[8];                      /* join_tree == 2: the OPENING of the claim' the root seal publishes (claim' = hash_pair(core, */
    uint32_t root_pre, root_post;               /* (pre, post, 0..))): what a further join needs as witness for this receipt; never trusted */
} zkh_prove_info;
/* CircuitHal::accumulate for circuits without a built-in accum generator: fill `accum` (W_accum x 2^po2) from data + mix */
typedef const char* (*zkh_accumulate_fn)(void* user, zkh_ctx*, const zkh_circuit*, size_t po2, const zkh_buf* data,
                                         const uint32_t* mix_global, zkh_buf* accum);
/* devices[n_devices] x lanes_per_device lanes; join_desc: a P2-JOIN description (kind 3) or NULL */
const char* zkh_session_create(const int* devices, size_t n_devices, size_t lanes_per_device, const uint32_t* desc,
                               size_t desc_words, const uint32_t* join_desc, size_t join_desc_words, zkh_session** out);
void zkh_session_destroy(zkh_session*);
size_t zkh_session_lanes(const zkh_session*);
/* the circuit handle of a lane (join != 0: its join circuit), e.g. to attach code objects before proving */
zkh_circuit* zkh_session_circuit(zkh_session*, size_t lane, int join);
void zkh_session_set_accumulate(zkh_session*, zkh_accumulate_fn fn, void* user);
/* Built-in circuits (kinds 1, 2): every lane commits the code (control) group of a segment size ONCE and keeps the committed form
 * resident in HBM (zkh_prover_cache_code) — the default; seals are byte-identical.  on = 0: re-commit it per segment, as
 * upstream's SegmentProver does. */
void zkh_session_set_resident_code(zkh_session*, int on);
/* The lift / join programs of the RECURSION circuit (zkh_rec_program_*; blobs from `python -m zeth_amd.circuits.rec_verify dir`):
 * rec_desc = the RECURSION description; program i is blobs[i] (words[i] words) of kind kinds[3 i .. 3 i + 3) = {0, segment po2,
 * circuit family (0 = the session's)} for a lift, {1, left po2, right po2} for a join of two recursion seals, {2, left po2,
 * right po2} for a lift2 (two SEGMENT seals verified by one program: lift + lift + join fused; used for the bottom level when
 * every pair of the session has one), {3, po2 of the first two children, po2 of the third} for a join3 (three recursion seals,
 * out = what join(join(a, b), c) publishes: used above the bottom level wherever three neighbours have these sizes).
 * Every lane loads every program (code groups resident). */
const char* zkh_session_set_recursion(zkh_session*, const uint32_t* rec_desc, size_t rec_desc_words, const uint32_t* const* blobs,
                                      const size_t* words, const uint32_t* kinds, size_t n_programs);
/* The same, with the programs BUILT by the library (zkh_rec_build_program; the RECURSION description is compiled in): for a block
 * whose segments have the sizes po2s[0] > po2s[1] > .. (built-in circuits, kinds 1..3: the control roots come from their own code
 * generators) — a lift per size, a lift2 per pair, joins until the set of program sizes closes, and (with_join3) the join3 of the
 * largest size if it fits that size again: the set and the order of zeth_amd/recursion.py build_programs.  No Python, no files. */
const char* zkh_session_build_recursion(zkh_session*, const uint32_t* po2s, size_t n_po2s, int with_join3);
/* ASSUMPTION receipts of the session (upstream: the keccak batch receipts a guest's accelerator calls leave behind; ProverServer::
 * {prove_keccak, lift, union, resolve}, risc0-zkvm 3.0.3, /root/reference/Cargo.lock:5418): n seals of the circuit `desc` (no state
 * words; KECCAK-F), sizes po2s[i], proven beforehand (zkh_prove_segment), control_roots = n x 8 words (that circuit's control root at
 * each size).  Every receipt is VERIFIED here on the host; the session keeps copies.  With join_tree == 2 they are lifted (lift
 * programs of family 1), united pairwise into one receipt (kind 4: every node the digest of the SORTED pair; an odd one moves up) and
 * the session's join-tree root is resolved against the union root (kind 5): the root receipt of zkh_session_prove is the RESOLVED
 * one, zkh_session_verify recomputes its claim from the segments AND these receipts (zkh_succinct_verify_resolved: the same from
 * claims alone).  Call BEFORE zkh_session_build_recursion, which then also builds those programs (zkh_session_set_recursion: kinds
 * {0, po2, 1}, {4, a, b}, {5, session size, union size}).  n = 0 clears. */
const char* zkh_session_set_assumptions(zkh_session*, const uint32_t* desc, size_t desc_words, const uint32_t* const* seals,
                                        const size_t* seal_words, const uint32_t* po2s, const uint32_t* control_roots, size_t n);
/* join_tree == 2 runs as ONE pipeline by default: a lift2 / join is proven the moment both children exist, on the fold lanes while
 * the sealing lanes are still busy with segments, on every lane afterwards (upstream joins as receipts arrive too).  on = 0: two
 * phases (seal everything, then fold).  Same tree, same receipts either way. */
void zkh_session_set_streamed_fold(zkh_session*, int on);
/* Chained session (SYN-C circuits): zkh_session_prove runs the executor's pass first (zkh_syn_chain_contributions), gives segment i
 * the pre-state initial + sum of the contributions of segments 0 .. i-1 as its public input (any `pub` of the caller is replaced),
 * and zkh_session_verify additionally checks CONTINUITY on the seals: the first segment starts from initial_state (canonical
 * residue), every segment's pre-state (out[4]) is its predecessor's post-state (out[0]) — `CompositeReceipt::verify_integrity`.
 * SYN-S circuits additionally get their exit-code pair and journal-digest limbs here and have them checked (see below). */
const char* zkh_session_set_chained(zkh_session*, int on, uint32_t initial_state);
/* The journal of a chained SYN-S session: the bytes the guest commits — zeth's guest commits the 32-byte block hash
 * (/root/reference/guests/stateless-client/src/lib.rs:33 `env::commit_slice(block_hash)`), which the CLI then compares with the hash
 * it computed itself (/root/reference/crates/host/src/bin/cli.rs:103-107).  The last seal binds Output{SHA-256(journal), assumptions};
 * zkh_session_verify checks the seals against THESE bytes.  journal == NULL (default): the session's final state word, 4 bytes LE.
 * journal != NULL with journal_len == 0: an empty journal.  Call before zkh_session_prove. */
const char* zkh_session_set_journal(zkh_session*, const uint8_t* journal, size_t journal_len);
/* Where a segment's witness comes from (SYN-AIR circuits without public inputs).  0 (default): the closed-form generator on the
 * device (zkh_syn_witgen).  1: upstream's shape — a SEQUENTIAL host preflight per segment (zkh_syn_preflight) running ahead of the
 * seals on `producers_per_lane` host threads per sealing lane (0 = 2), its compact records (16 bytes per cycle) uploaded from pinned
 * memory and expanded on the GPU (zkh_syn_witgen_trace).  zkh_prove_info reports the host CPU seconds and the PCIe bytes. */
const char* zkh_session_set_witness_source(zkh_session*, int source, size_t producers_per_lane);
/* join_tree == 1: fold the receipts through the P2-JOIN tree (joins at 2^join_po2; join_noise_key NULL = a fresh OS key per proof);
 * join_tree == 2: lift every receipt and join level by level with the RECURSION programs - every node verifies its child
 * seal(s) in-circuit; the root receipt is a RECURSION seal with out = claim tree root ‖ allowed-programs root.  The tree: the
 * first level pairs the segments, every level above takes three nodes at a time (a remainder of two is a join, of one moves up);
 * a group of three is ONE proof where the session has a join3 program for its sizes, else join(join(a, b), c) - the same node. */
const char* zkh_session_prove(zkh_session*, const zkh_segment* segs, size_t n, int join_tree, size_t join_po2,
                              const uint32_t join_noise_key[8], zkh_prove_info* info);
void zkh_prove_info_free(zkh_prove_info*);
/* every leaf seal against the control root of its size; with a root receipt also the root seal and the claim tree
 * (hash_pair over the leaf claims, recomputed on the host) against the root's public output */
const char* zkh_session_verify(zkh_session*, const zkh_segment* segs, const zkh_prove_info* info, size_t join_po2);

/* Sessions that TERMINATE (SYN-S circuits: zeth_amd/circuits/syn_air.py syn_session; shipped as "syn_session").  Upstream's ReceiptClaim
 * carries an exit code and an output (journal) digest per segment, and `receipt.verify(image_id)` + the journal comparison
 * (/root/reference/crates/host/src/bin/cli.rs:103-107) rely on them: every segment but the last ends in SystemSplit, the last in
 * Halted(0) with the digest of the journal (risc0-zkvm 3.0.3 receipt/composite.rs verify_integrity, recalled).  A SYN-S segment
 * publishes out = (post, 0, 0, 0, pre, exit_sys, exit_user, j_0 .. j_15) — j = the session's OUTPUT digest
 * tagged_struct("risc0.Output", [SHA-256(journal), Assumptions digest]) as sixteen 16-bit limbs (round 6; until then SHA-256(journal)
 * alone) — every word a bound public input; zkh_session_set_chained fills them (the journal of a session = its final state word, 4 bytes
 * LE; the assumptions = the receipts handed to zkh_session_set_assumptions, in that order) and zkh_session_verify checks them.
 * zkh_session_check_output is that check for a verifier that holds VERIFIED seals: a receipt whose trailing segments were cut off ends in
 * a SystemSplit and is refused; journal == NULL: the final state word; assumptions_digest == NULL: the session assumed nothing —
 * otherwise zkh_assumptions_digest over (claim digest = zkh_receipt_claim, control root) of the assumption receipts THE VERIFIER holds:
 * a session cannot be resolved against other receipts than the ones its own seal names.  zkh_session_check_termination = the same with
 * no assumptions.  Host only. */
void zkh_sha256(const uint8_t* data, size_t len, uint8_t out[32]);
const char* zkh_session_check_termination(const zkh_circuit*, const uint32_t* const* seals, const size_t* seal_words, size_t n,
                                          const uint8_t* journal, size_t journal_len);
const char* zkh_session_check_output(const zkh_circuit*, const uint32_t* const* seals, const size_t* seal_words, size_t n,
                                     const uint8_t* journal, size_t journal_len, const uint32_t assumptions_digest[8]);
/* Assumptions([Assumption{claim, control_root}, ..]).digest() (recalled layout): claims / control_roots = n x 8 words; n == 0: zero digest */
void zkh_assumptions_digest(const uint32_t* claims, const uint32_t* control_roots, size_t n, uint32_t out[8]);

/* `receipt.verify` for a SUCCINCT receipt on the host alone — no GPU, no session (upstream: SuccinctReceipt::verify_integrity, reached
 * from /root/reference/crates/host/src/bin/cli.rs:103): ONE seal of the RECURSION circuit (description compiled in) under the control
 * root of program `root_program` of the allowed set (allowed_roots: n_allowed x 8 words, in the order the prover loaded its
 * programs), the allowed-programs root the receipt carries, and its claim = the root of the leaves' claim tree.  leaves: n_leaves x
 * 10 words = (receipt claim digest [8], pre, post) per segment, taken from VERIFIED segment receipts or from the statement being
 * checked; ranks = 1, or N when the block was folded as N contiguous equal ranges whose roots were folded again (§7). */
const char* zkh_succinct_verify(const uint32_t* root_seal, size_t root_words, const uint32_t* allowed_roots, size_t n_allowed,
                                size_t root_program, const uint32_t* leaves, size_t n_leaves, size_t ranks);
/* The same for a RESOLVED receipt (upstream: ProverServer::{union, resolve}, risc0-zkvm 3.0.3, /root/reference/Cargo.lock:5418 — the
 * session's assumption receipts, e.g. keccak batches, are lifted, united pairwise into one receipt whose claim is the digest of the
 * SORTED pair at every node, and the session's root is resolved against it; recursion programs of kinds 4 / 5, zkh_rec_build_program):
 * assumption_claims = n_assumptions x 8 words, the receipt claim digests of the assumption receipts (any order within a pair: the
 * union sorts).  The claim must be wrap(hash_pair(claim' of the leaves' join tree, claim' of the union tree), pre, post of the
 * session).  n_leaves == 0 (leaves may be NULL): the receipt is the union-tree root alone. */
const char* zkh_succinct_verify_resolved(const uint32_t* root_seal, size_t root_words, const uint32_t* allowed_roots, size_t n_allowed,
                                         size_t root_program, const uint32_t* leaves, size_t n_leaves, size_t ranks,
                                         const uint32_t* assumption_claims, size_t n_assumptions);

/* ---- host placement (topology.hip): one process per GPU / one lane thread per context should run on the cores of the NUMA node
 * the GPU's root port hangs off, and allocate its pinned witness blocks there (upstream leaves placement to the operator:
 * /root/reference/run-parallel.sh:15 starts one prover per GPU and pins nothing).  Host only; sysfs + sched_setaffinity. ---- */
/* "0-15,64-79" -> sorted CPU ids (cpus may be NULL to count); anything that is not a cpulist is an error */
const char* zkh_parse_cpulist(const char* text, int* cpus, size_t cap, size_t* n);
/* NUMA node of PCI function bdf ("0000:c1:00.0") and that node's CPUs, read under sysfs_root ("/sys"); *node = -1 and
 * *n_cpus = 0 when the kernel reports none */
const char* zkh_pci_numa_cpus(const char* sysfs_root, const char* bdf, int* node, int* cpus, size_t cap, size_t* n_cpus);
/* NUMA node of a HIP device (-1 = unknown) and, optionally, its PCI bus id */
const char* zkh_device_numa_node(int device, int* node, char pci_bus_id[32]);
/* What tells one GPU from another across processes (bench.py gathers it from every rank: an N-GPU line lists N distinct devices):
 * PCI bus id, the device UUID as 32 hex digits (independent of HIP_VISIBLE_DEVICES renumbering; empty if the runtime has none),
 * NUMA node (-1 = unknown), marketing name, and the number of devices this process sees.  Any out pointer may be NULL. */
const char* zkh_device_identity(int device, char pci_bus_id[32], char uuid_hex[40], int* numa_node, char name[64], int* visible_devices);
/* Bind the CALLING thread (and the threads it creates afterwards) to slice `slot` of `share` equal slices of the device's
 * NUMA-node CPUs (share <= 1: the whole node) and make that node its preferred memory node.  ZKH_AFFINITY=off, or a host that
 * reports no node: nothing is changed and *node = -1. */
const char* zkh_bind_thread_to_device(int device, size_t slot, size_t share, int* node, size_t* n_cpus);

/* ---- profiling: per-kernel HIP-event timing on the ctx stream ---- */
const char* zkh_prof_enable(zkh_ctx*, int on);
/* writes up to cap records; returns count via *n.  Each record: name (<=47 chars), calls, total_ms */
typedef struct { char name[48]; uint64_t calls; double total_ms; double alg_bytes; } zkh_prof_rec;
const char* zkh_prof_get(zkh_ctx*, zkh_prof_rec* recs, size_t cap, size_t* n);
const char* zkh_prof_reset(zkh_ctx*);

#ifdef __cplusplus
}
#endif
#endif
