// hash.hip — Poseidon2 (BabyBear, t = 24, rate 16, out 8) Merkle hashing for gfx950:
// Hal::hash_rows / Hal::hash_fold and the fused tree build (risc0-zkp 3.0.2 src/hal/mod.rs; hash semantics
// src/core/hash/poseidon2/mod.rs; un-vendored: /root/reference/Cargo.lock:5393).  Reached from
// /root/reference/crates/host/src/lib.rs:137 (MerkleTreeProver::new inside Prover::commit_group).
//
// This is 31-bit modular integer work: a product of two VARIABLES has no use for the matrix cores.  A constant matrix
// applied to 64 states at once has: in k_hash_rows and k_hash_fold the linear part of the 21 partial rounds is two int8
// digit products on v_mfma_i32_32x32x32_i8 (poseidon2_linear.h; 54 MFMAs per wave-permutation, on a pipe of their own), and
// only the serial cell-0 chain of those rounds stays on the VALU.  Every other caller keeps the grouped partial rounds.
// One lane owns one sponge; the 24-word state lives in VGPRs for
// the whole permutation (all cell loops are fully unrolled, round constants arrive through scalar loads), rows
// are read column-major so a wave's 64 lanes read 64 consecutive words per column; four resident workgroups per CU
// hide the column loads behind other waves' permutations (no software prefetch: it only cost VGPRs).  VALU-bound
// by construction (~1356 Montgomery products per 64 absorbed bytes); the HBM side only has to keep up with
// 16*W*n bytes per tree.  The permutation is poseidon2.h's lane-per-permutation form: signed Montgomery s-boxes with
// no canonicalisation, M_ext on exact doubles (v_add_f64 / v_fma_f64 issue at the rate of a 32-bit multiply and have
// the headroom a 31-bit prime denies a 32-bit word); partial rounds three at a time with unreduced weighted sums
// (6.4 k VALU instructions per 64 permutations) or, in the two kernels above, as matrix products (5.0 k).
#include "common.h"
#include "image_tree.h"
#include "poseidon2.h"
#include "poseidon2_wide.h"

using namespace zkh;

// common.h sizes the host / device / verifier copies of the partial-round table by hand; poseidon2.h lays the table out.
static_assert(zkh::ZKH_P2_PTAB == zkh::P2_TAB_WORDS, "common.h ZKH_P2_PTAB must equal poseidon2.h P2_TAB_WORDS");
static_assert(zkh::ZKH_P2_LIN == zkh::LIN_WORDS, "common.h ZKH_P2_LIN must equal poseidon2_linear.h LIN_WORDS");

namespace {

// Hal::hash_rows — one lane per leaf.
// (register budgets for 2, 3 or 4 workgroups per CU compile to the same speed; capping residency at 2 or 3 workgroups
// with LDS padding is 5 % slower alone and 5 % slower with three seals in flight: no SMT-style gain from leaving room)
// LINEAR (lin: poseidon2_linear.h's table): the partial rounds run as int8 matrix products, wave-wide, so no lane leaves before the
// last permutation: a lane past the end hashes the last row again and only its store is predicated.  Without it (a table the
// builder refused) the grouped form runs.
template <bool LINEAR>
__global__ __launch_bounds__(256, 4) void k_hash_rows(uint32_t* __restrict__ out, const uint32_t* __restrict__ matrix,
                                                   size_t rows, uint32_t cols, const uint32_t* __restrict__ rc,
                                                   const uint32_t* __restrict__ diag, const uint32_t* __restrict__ lin) {
    const size_t lane_row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = lane_row < rows;
    if (!LINEAR && !live) return;
    // The lane's row as (the workgroup's first row: uniform) + (dr < 256): every address below is a scalar base plus one 32-bit
    // per-lane offset, so the only per-lane value live across the block loop is one register, not a 64-bit pointer or two.
    const size_t row0 = (size_t)blockIdx.x * blockDim.x;
    uint32_t dr = live ? threadIdx.x : (uint32_t)(rows - 1 - row0);
    asm("" : "+v"(dr));                          // (one value: not threadIdx.x kept beside it for the live lanes' store)
    uint32_t s[CELLS];
#pragma unroll
    for (int i = 0; i < CELLS; i++) s[i] = 0;
    const uint32_t full = cols / RATE, tail = cols % RATE;
    const uint32_t blocks = full + (tail || cols == 0 ? 1u : 0u);
    // No register double-buffer for the next 16 columns: the partial rounds need the VGPRs (127 with the matrix products'
    // operands and accumulators, 88 in the grouped form), and with 4 or 5 waves per SIMD the loads of one wave hide under
    // the permutations of the others.
    // ONE call site of the permutation serves full blocks and the tail block: interior blocks keep the capacity, the
    // last block the digest, either one in s[16..24) (poseidon2_mix_sponge: a scalar branch around the last eight
    // reductions).  The capacity stays a nearly centred signed word from block to block; only the digest is canonicalised.
    for (uint32_t b = 0; b < blocks; b++) {
        const uint32_t* bsrc = matrix + (size_t)b * RATE * rows + row0;
        if (b < full) {
#pragma unroll
            for (int i = 0; i < RATE; i++) s[i] = (bsrc + (size_t)i * rows)[dr];
        } else {
#pragma unroll
            for (int i = 0; i < RATE; i++) s[i] = (uint32_t)i < tail ? (bsrc + (size_t)i * rows)[dr] : 0u;
        }
        // The table's ~230 uniform words are loaded where they are used, not hoisted out of this loop and spilled: an opaque
        // zero OFFSET makes the address new in every block.  (Laundering the pointer itself loses its address space: every
        // table word then arrives through a per-lane flat load and lands in a VGPR.)
        uint32_t lin_off = 0;
        asm volatile("" : "+s"(lin_off));
        const uint32_t* __restrict__ lin_here = lin + lin_off;
        if (LINEAR) poseidon2_mix_sponge_linear(s, diag, lin_here, b + 1 == blocks);
        else        poseidon2_mix_sponge(s, rc, diag, b + 1 == blocks);
#pragma unroll
        for (int i = RATE; i < CELLS; i++) s[i] = p2_signed(s[i]);
    }
#pragma unroll
    for (int i = 0; i < OUT; i++) s[i] = canon((int32_t)s[RATE + i]);
    if (!live) return;
    uint4* o = (uint4*)(out + row0 * 8) + 2 * dr;
    o[0] = make_uint4(s[0], s[1], s[2], s[3]);
    o[1] = make_uint4(s[4], s[5], s[6], s[7]);
}

// one lane folds one parent of the layer of `output_size` parents: io[out+i] = H(io[in+2i] || io[in+2i+1])
// (LINEAR: as in k_hash_rows; `store` predicates the write of a lane that only keeps its wave whole)
template <bool LINEAR = false>
__device__ __forceinline__ void fold_one(uint32_t* __restrict__ io, size_t input_size, size_t output_size, size_t i,
                                         const uint32_t* __restrict__ rc, const uint32_t* __restrict__ diag,
                                         const uint32_t* __restrict__ lin = nullptr, bool store = true) {
    const uint4* src = (const uint4*)(io + (input_size + 2 * i) * 8);
    uint32_t s[CELLS];
    const uint4 a = src[0], b = src[1], c = src[2], d = src[3];
    s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w; s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
    s[8] = c.x; s[9] = c.y; s[10] = c.z; s[11] = c.w; s[12] = d.x; s[13] = d.y; s[14] = d.z; s[15] = d.w;
#pragma unroll
    for (int k = RATE; k < CELLS; k++) s[k] = 0;
    if (LINEAR) poseidon2_mix_raw_linear<0, OUT, RATE>(s, diag, lin);
    else        poseidon2_mix_raw<0, OUT, RATE>(s, rc, diag);  // the zero capacity is not fed through the first M_ext
#pragma unroll
    for (int k = 0; k < OUT; k++) s[k] = p2_finish(s[k]);
    if (!store) return;
    uint4* o = (uint4*)(io + (output_size + i) * 8);
    o[0] = make_uint4(s[0], s[1], s[2], s[3]);
    o[1] = make_uint4(s[4], s[5], s[6], s[7]);
}
// Hal::hash_fold — one lane per parent
template <bool LINEAR>
__global__ __launch_bounds__(256, 4) void k_hash_fold(uint32_t* __restrict__ io, size_t input_size, size_t output_size,
                                                   const uint32_t* __restrict__ rc, const uint32_t* __restrict__ diag,
                                                   const uint32_t* __restrict__ lin) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < output_size;
    if (!LINEAR && !live) return;
    fold_one<LINEAR>(io, input_size, output_size, live ? i : output_size - 1, rc, diag, lin, live);
}
// The image tree's update (image.hip): the same fold over a LIST of parents of the layer of `width` parents, lane t the parent list[t],
// t < *count (the count is the device's: the compaction that made the list left it).  The lanes are dense: a wave runs a permutation
// only for parents that are dirty, but for the last wave of the list.  Every parent is in the list once: no node is written twice.
__global__ __launch_bounds__(256, 4) void k_hash_fold_list(uint32_t* __restrict__ io, size_t width, const uint32_t* __restrict__ list,
                                                        const uint32_t* __restrict__ count, const uint32_t* __restrict__ rc,
                                                        const uint32_t* __restrict__ diag) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= *count) return;
    fold_one(io, 2 * width, width, list[t], rc, diag);
}
// The walk of a ZKU1 proof (image.hip, zkh_image_proof_walk): layer k's parents [0, *count), TWO lanes per parent, lane parity 0 the
// hash_pair of the old children, 1 of the new ones, so a lane holds one permutation as in k_hash_fold.  Parent r's first child is item
// from[r] of the layer's list, its digests at cur[16 item, +16) (old, new); the other child is the item after it (sib[r] = NONE), or the
// clean sibling at rank sib[r] of the proof's section C_k (word *off; word aligned), the same for old and new, on the left when the
// item's index is odd.  The parent's digests go to next[16 r, +16).  Lanes past the count leave: a refusal leaves a count of 0.
// kKeep (zkh_image_proof_nodes; zkn1.h): the lane also leaves the two children it has just read in the parent's record of the dirty-node
// table, the section of this layer's parents at word *keep_at of `keep`: behind the section's *count ids, record r, the left child at
// words [8 v, +8), the right one at [16 + 8 v, +8).  One writer per word; the records are word aligned.  Without kKeep the kernel is
// the walk's as it was.
template <bool kKeep>
__global__ __launch_bounds__(256, 4) void k_hash_walk(const uint32_t* __restrict__ list, const uint32_t* __restrict__ from, const uint32_t* __restrict__ sib,
                                                   const uint32_t* __restrict__ count, const uint32_t* __restrict__ proof, const uint32_t* __restrict__ off,
                                                   const uint32_t* __restrict__ cur, uint32_t* __restrict__ next, const uint32_t* __restrict__ rc,
                                                   const uint32_t* __restrict__ diag, uint32_t* __restrict__ keep, const uint32_t* __restrict__ keep_at) {
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x, r = lane >> 1, v = lane & 1;
    if (r >= *count) return;
    const uint32_t item = from[r], clean = sib[r];
    const uint32_t* mine = cur + 16 * (size_t)item + 8 * v;
    const uint32_t* other = clean == 0xffffffffu ? mine + 16 : proof + *off + 8 * (size_t)clean;
    const bool odd = clean != 0xffffffffu && (list[item] & 1);
    const uint32_t* left = odd ? other : mine;
    const uint32_t* right = odd ? mine : other;
    uint32_t s[CELLS];
#pragma unroll
    for (int k = 0; k < 8; k++) { s[k] = left[k]; s[8 + k] = right[k]; }
    if (kKeep) {
        uint32_t* record = keep + *keep_at + *count + 32 * (size_t)r + 8 * v;
#pragma unroll
        for (int k = 0; k < 8; k++) { record[k] = s[k]; record[16 + k] = s[8 + k]; }
    }
#pragma unroll
    for (int k = RATE; k < CELLS; k++) s[k] = 0;
    poseidon2_mix_raw<0, OUT, RATE>(s, rc, diag);             // as fold_one: the zero capacity is not fed through the first M_ext
#pragma unroll
    for (int k = 0; k < OUT; k++) s[k] = p2_finish(s[k]);
    uint4* o = (uint4*)(next + 16 * (size_t)r + 8 * v);
    o[0] = make_uint4(s[0], s[1], s[2], s[3]);
    o[1] = make_uint4(s[4], s[5], s[6], s[7]);
}

// ---------------------------------------------------------------------------------------------------------
// Wavefront-cooperative permutation for the narrow layers of a tree.  With one lane per permutation a layer
// cannot finish faster than one serial permutation (~36k VALU cycles, ~20-30 us) however few parents it has, and
// a 2^22-leaf tree has 16 such layers.  Here EIGHT lanes share one permutation: lane j < 6 owns state cells
// 4j..4j+3 (one M4 block), the column sums of M_ext and the partial-round state sum are 3-step DPP butterflies
// (quad_perm xor 1, xor 2, row_half_mirror) that never touch LDS, round constants sit in LDS (one ds_read_b128 per
// full round).  ~3.5x lower latency per layer; used only where the layer is too narrow to fill the chip.
// (The permutation itself: poseidon2_wide.h.)
// ---------------------------------------------------------------------------------------------------------
// one 8-lane group folds one parent: io[out + parent] = H(io[in + 2 parent] || io[in + 2 parent + 1]); rcs = rc in LDS
__device__ __forceinline__ void wide_fold_one(uint32_t* __restrict__ io, size_t input_size, size_t output_size, uint32_t gid,
                                              const uint32_t* rcs, const uint32_t* __restrict__ pc) {
    const uint32_t j = gid & 7;
    size_t parent = gid >> 3;
    const bool live = parent < output_size;
    if (!live) parent = output_size - 1;                        // keep the whole wave in the butterflies
    uint32_t c[4] = {0, 0, 0, 0};
    if (j < 4) {
        const uint4 v = *(const uint4*)(io + (input_size + 2 * parent) * 8 + 4 * j);
        c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
    }
    wide_permute(c, j, rcs, pc);
    if (live && j < 2) *(uint4*)(io + (output_size + parent) * 8 + 4 * j) = make_uint4(c[0], c[1], c[2], c[3]);
}
// (WIDE_LOG, image_tree.h: layers with <= 2^15 parents use the 8-lane permutation)
constexpr int TAIL_LOG = 7;       // a 1024-lane workgroup = 2^7 eight-lane groups; the last 8 layers (<= 2^7 parents) are one launch
// Middle of the tree: workgroup b owns the 128 consecutive parents [128 b, 128 b + 128) of the layer with `first_parents`
// parents and the `levels` - 1 layers above them (64, 32, ... parents of its own subtree), so the layers with
// 2^15 .. 2^8 parents are ONE launch.  Each level still costs one 8-lane permutation of latency; what disappears is the
// launch round trip between them.
__global__ __launch_bounds__(8 << TAIL_LOG) void k_hash_fold_subtree(uint32_t* __restrict__ io, size_t first_parents, uint32_t levels,
                                                                     const uint32_t* __restrict__ rc, const uint32_t* __restrict__ pc) {
    __shared__ __attribute__((aligned(16))) uint32_t rcs[ROUNDS_TOTAL * CELLS + 8];
    for (uint32_t w = threadIdx.x; w < ROUNDS_TOTAL * CELLS; w += blockDim.x) rcs[w] = rc[w];
    __syncthreads();
    for (uint32_t l = 0; l < levels; l++) {
        const size_t parents = first_parents >> l;
        const uint32_t local = (1u << TAIL_LOG) >> l;           // parents of this level inside the workgroup
        if ((threadIdx.x >> 6) * 8 < local) {                   // wave-uniform
            // lanes beyond `local` groups alias the last parent of the level (no write): live == false there
            const uint32_t grp = threadIdx.x >> 3;
            const uint32_t gid = grp < local ? (uint32_t)((blockIdx.x * local + grp) * 8 + (threadIdx.x & 7)) : 0xffffffffu;
            wide_fold_one(io, 2 * parents, parents, gid, rcs, pc);
        }
        __threadfence_block();
        __syncthreads();
    }
}
// Tree top: parents = first_parents, first_parents / 2, ..., 1 inside one workgroup (each layer reads what the previous
// one wrote: __syncthreads orders the global writes of a workgroup for its own later reads).
__global__ __launch_bounds__(8 << TAIL_LOG) void k_hash_fold_tail(uint32_t* __restrict__ io, size_t first_parents,
                                                                  const uint32_t* __restrict__ rc, const uint32_t* __restrict__ pc) {
    __shared__ __attribute__((aligned(16))) uint32_t rcs[ROUNDS_TOTAL * CELLS + 8];
    for (uint32_t w = threadIdx.x; w < ROUNDS_TOTAL * CELLS; w += blockDim.x) rcs[w] = rc[w];
    __syncthreads();
    for (size_t parents = first_parents; parents >= 1; parents >>= 1) {
        if ((threadIdx.x >> 6) * 8 < parents)                    // wave-uniform: waves with no live group skip the layer
            wide_fold_one(io, 2 * parents, parents, threadIdx.x, rcs, pc);
        __threadfence_block();
        __syncthreads();
    }
}

// the bare permutation, one lane per state (24 words each)
__global__ __launch_bounds__(256) void k_poseidon2_mix(uint32_t* __restrict__ io, size_t count, const uint32_t* __restrict__ rc,
                                                       const uint32_t* __restrict__ diag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint4* p = (uint4*)(io + i * CELLS);
    uint32_t s[CELLS];
#pragma unroll
    for (int q = 0; q < CELLS / 4; q++) { const uint4 v = p[q]; s[4 * q] = v.x; s[4 * q + 1] = v.y; s[4 * q + 2] = v.z; s[4 * q + 3] = v.w; }
    poseidon2_mix(s, rc, diag);
#pragma unroll
    for (int q = 0; q < CELLS / 4; q++) p[q] = make_uint4(s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
}

// Test hook: ONE tile product of poseidon2_linear.h through the helpers the kernels use.  a: a 32 x 32 int8 matrix, row-major;
// b: lane l's own eight words (the bytes k = 0..31 of column l); out[32 l + 4 o + (0, 1)] = (lo, hi) of output o (rows lin_row(o, 0..3)) of column l, gathered by the swaps (8 o < 32: 16 words used).
__global__ __launch_bounds__(64) void k_lin_tile(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)               // (the matrix helpers exist in the device pass only)
    const uint32_t lane = threadIdx.x;
    uint32_t v[8];
#pragma unroll
    for (int q = 0; q < 8; q++) v[q] = b[8 * lane + q];
    lin_operands(v);
    const lin_v4 af = ((const lin_v4*)a)[2 * (lane & 31) + (lane >> 5)];      // row lane & 31, bytes 16 (lane >> 5) + 0..15
    lin_v16 c0 = {0}, c1 = {0};
    c0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, lin_b(v, 0, 0), c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, lin_b(v, 0, 1), c1, 0, 0, 0);
    // lin_gather2 with the weights (1, 0) and then (0, 1) returns lo = r_0 + (r_1 << 8) and hi = r_2 + (r_3 << 8) of two outputs
#pragma unroll
    for (int g = 0; g < 4; g++) {
        int64_t lo0, lo1, hi0, hi1;
        lin_gather2(lo0, lo1, c0, c1, g, 1, 0);
        lin_gather2(hi0, hi1, c0, c1, g, 0, 1);
        out[32 * lane + 8 * g] = (uint32_t)lo0; out[32 * lane + 8 * g + 1] = (uint32_t)hi0;
        out[32 * lane + 8 * g + 4] = (uint32_t)lo1; out[32 * lane + 8 * g + 5] = (uint32_t)hi1;
    }
#endif
}

}  // namespace

extern "C" const char* zkh_test_lin_tile(zkh_ctx* c, const zkh_buf* a, const zkh_buf* b, zkh_buf* out) {
    ZKH_REQUIRE(a && b && out && a->len == 256 && b->len == 512 && out->len == 2048, "test_lin_tile: a 256, b 512, out 2048 words");
    bind_thread(c);
    k_lin_tile<<<1, 64, 0, c->stream>>>(a->ptr(), b->ptr(), out->ptr());
    return last_launch_error("test_lin_tile");
}
extern "C" const char* zkh_poseidon2_mix(zkh_ctx* c, zkh_buf* states, size_t count) {
    ZKH_REQUIRE(states && states->len == count * CELLS, "poseidon2_mix: buffer is not count x 24 words");
    if (!count) return nullptr;
    bind_thread(c);
    k_poseidon2_mix<<<(unsigned)((count + 255) / 256), 256, 0, c->stream>>>(states->ptr(), count, c->tab.rc, c->tab.diag);
    return last_launch_error("poseidon2_mix");
}
extern "C" const char* zkh_hash_rows(zkh_ctx* c, zkh_buf* out, const zkh_buf* matrix) {
    ZKH_REQUIRE(out->len % 8 == 0 && out->len, "hash_rows: output is not a digest array");
    const size_t rows = out->len / 8;
    ZKH_REQUIRE(matrix->len % rows == 0, "hash_rows: matrix size %zu not a multiple of rows %zu", matrix->len, rows);
    const size_t cols = matrix->len / rows;
    ProfScope prof(c, "hash_rows", 4.0 * matrix->len + 32.0 * rows);
    const dim3 grid((unsigned)((rows + 255) / 256));
    if (c->lin_ok) k_hash_rows<true><<<grid, 256, 0, c->stream>>>(out->ptr(), matrix->ptr(), rows, (uint32_t)cols, c->tab.rc, c->tab.diag, c->tab.lin);
    else           k_hash_rows<false><<<grid, 256, 0, c->stream>>>(out->ptr(), matrix->ptr(), rows, (uint32_t)cols, c->tab.rc, c->tab.diag, c->tab.lin);
    return last_launch_error("hash_rows");
}
extern "C" const char* zkh_hash_fold(zkh_ctx* c, zkh_buf* io, size_t input_size, size_t output_size) {
    ZKH_REQUIRE(io->len % 8 == 0, "hash_fold: not a digest array");
    ZKH_REQUIRE((input_size + 2 * output_size) * 8 <= io->len && output_size * 2 <= input_size, "hash_fold: ranges out of bounds");
    if (!output_size) return nullptr;
    ProfScope prof(c, "hash_fold", 96.0 * output_size);
    const dim3 grid((unsigned)((output_size + 255) / 256));
    if (c->lin_ok) k_hash_fold<true><<<grid, 256, 0, c->stream>>>(io->ptr(), input_size, output_size, c->tab.rc, c->tab.diag, c->tab.lin);
    else           k_hash_fold<false><<<grid, 256, 0, c->stream>>>(io->ptr(), input_size, output_size, c->tab.rc, c->tab.diag, c->tab.lin);
    return last_launch_error("hash_fold");
}
extern "C" const char* zkh_merkle_fold_all(zkh_ctx* c, zkh_buf* nodes, size_t rows) {
    ZKH_REQUIRE(nodes->len == rows * 16 && rows && (rows & (rows - 1)) == 0, "merkle_fold_all: nodes must hold 2*rows digests");
    return merkle_fold_from(c, nodes, rows);
}
// MerkleTreeProver::new: leaves = hash_rows(matrix), then every layer above.  (A fused leaves + first-layer pass was built in
// round 4, measured slower — 17.81 vs 17.68 ms of Poseidon2 per seal, profiles/r04_merkle_fused_ab.txt — and removed in round 6.)
extern "C" const char* zkh_merkle_build(zkh_ctx* c, zkh_buf* nodes, const zkh_buf* matrix, size_t rows) {
    ZKH_REQUIRE(nodes && matrix && nodes->len == rows * 16 && rows && (rows & (rows - 1)) == 0, "merkle_build: nodes must hold 2*rows digests");
    ZKH_REQUIRE(matrix->len % rows == 0, "merkle_build: matrix size %zu not a multiple of rows %zu", matrix->len, rows);
    zkh_buf* leaves = nullptr;
    ZKH_TRY(zkh_slice(nodes, rows * 8, rows * 8, &leaves));
    const char* err = zkh_hash_rows(c, leaves, matrix);
    zkh_release(leaves);
    ZKH_TRY(err);
    return merkle_fold_from(c, nodes, rows);
}
const char* zkh::merkle_fold_from(zkh_ctx* c, zkh_buf* nodes, size_t first_layer) {
    for (size_t layer = first_layer; layer >= 2; layer /= 2) {       // layer = current input width, layer/2 parents
        const size_t parents = layer / 2;
        if (parents > ((size_t)1 << WIDE_LOG)) {
            ZKH_TRY(zkh_hash_fold(c, nodes, layer, parents));
        } else if (parents > ((size_t)1 << TAIL_LOG)) {
            uint32_t levels = 0;
            while ((parents >> levels) > ((size_t)1 << TAIL_LOG)) levels++;      // down to the layer with 2^(TAIL_LOG+1) parents
            ProfScope prof(c, "hash_fold_wide", 96.0 * (2 * parents - (parents >> (levels - 1))));
            k_hash_fold_subtree<<<(unsigned)(parents >> TAIL_LOG), 8 << TAIL_LOG, 0, c->stream>>>(nodes->ptr(), parents, levels, c->tab.rc,
                                                                                                   c->tab.diag);
            ZKH_TRY(last_launch_error("hash_fold_wide"));
            layer >>= (levels - 1);                              // the loop's own /2 steps over the last fused level
        } else {
            ProfScope prof(c, "hash_fold_tail", 96.0 * (2 * parents - 1));
            k_hash_fold_tail<<<1, 8 << TAIL_LOG, 0, c->stream>>>(nodes->ptr(), parents, c->tab.rc, c->tab.diag);
            ZKH_TRY(last_launch_error("hash_fold_tail"));
            break;
        }
    }
    return nullptr;
}
const char* zkh::hash_fold_listed(zkh_ctx* c, zkh_buf* nodes, size_t width, const uint32_t* list, const uint32_t* count, uint32_t bound) {
    ZKH_REQUIRE(bound && bound <= width && 32 * width <= nodes->len, "hash_fold_listed: %u parents of %zu in %zu words", bound, width, nodes->len);
    ProfScope prof(c, "image_sparse", 100.0 * bound);
    k_hash_fold_list<<<(bound + 255) / 256, 256, 0, c->stream>>>(nodes->ptr(), width, list, count, c->tab.rc, c->tab.diag);
    return last_launch_error("image_sparse");
}
const char* zkh::hash_walk_layer(zkh_ctx* c, const uint32_t* list, const uint32_t* from, const uint32_t* sib, const uint32_t* count, const uint32_t* proof,
                                 const uint32_t* off, const uint32_t* cur, uint32_t* next, uint32_t bound, uint32_t* keep, const uint32_t* keep_at) {
    ZKH_REQUIRE(bound && bound <= 0x7fffffffu, "hash_walk_layer: %u parents", bound);
    ProfScope prof(c, "walk_hash", (keep ? 328.0 : 200.0) * bound);
    const unsigned grid = (unsigned)((2 * (size_t)bound + 255) / 256);
    if (keep) k_hash_walk<true><<<grid, 256, 0, c->stream>>>(list, from, sib, count, proof, off, cur, next, c->tab.rc, c->tab.diag, keep, keep_at);
    else k_hash_walk<false><<<grid, 256, 0, c->stream>>>(list, from, sib, count, proof, off, cur, next, c->tab.rc, c->tab.diag, nullptr, nullptr);
    return last_launch_error("walk_hash");
}
