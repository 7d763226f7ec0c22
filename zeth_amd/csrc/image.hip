// image.hip — the committed memory image (include/zkhal.h "THE IMAGE'S COMMITMENT"; zeth_amd/circuits/logup.py `reference_image_tree`;
// DESIGN.md §2 ARGUMENTS): a Merkle tree over the residues of an image of W raw Montgomery words, built on the device
// (zkh_image_commit) and kept current by a page-out (zkh_page_out_tree, page_out.hip -> image_tree_update).
//
// L = the smallest power of two >= ceil(W / 8).  `nodes` is 2 L digests in heap order (digest i at words [8 i, 8 i + 8)): digest 0 eight
// zeros; leaf L + j, word k = image[8 j + k] % P where 8 j + k < W, else 0 (a leaf is eight memory words verbatim, no hash); node i
// (1 <= i < L) = hash_pair(node 2 i, node 2 i + 1); the root is digest 1.
//
// COMMIT: one coalesced pass writes digest 0 and the leaf layer, hash.hip's merkle_fold_from every layer above.
//
// UPDATE, after the page-out's scatter.  The check pass has established that the table's rows [0, D) hold strictly increasing addresses
// a_i < W, so the dirty leaves a_i >> 3 do not decrease, and on every layer the dirty nodes are a sorted list with adjacent duplicates.
//   image_leaves : lane i < D whose leaf differs from the row below's rewrites the whole leaf from the image (residues, zero padding);
//   then per layer of `width` parents, from the widest (L / 2) up, while the layer is LISTED:
//   image_list   : the layer's dirty parents = the adjacent-unique of (the layer below's list >> 1); the first list comes from the table
//                  (a_i >> 4).  Flag, scan, scatter as the page scan of links.hip does: k_image_heads runs the heads stage (scan.h
//                  scan_heads) on "my key differs from the one before", the sort's counter scan leaves the count, k_image_compact writes the
//                  heads' keys at their ranks.  The count stays on the device: the grids are sized by its bound min(D, width), lanes past it leave.
//   image_sparse : hash.hip's k_hash_fold_list, one lane per listed parent: dense lanes, a permutation per dirty parent and no other.
//   A layer is listed when D + 2^16 <= width (listed(): a function of (D, width) alone, the constant measured; since D only grows
//   against width on the way up, the listed layers are the lowest ones).  From the first layer that is not, merkle_fold_from rebuilds
//   that layer and everything above it densely: at most 2^17 - 1 permutations when D is small, one lane-per-parent launch for the layer of 2^16
//   parents and two launches of the 8-lane kernels above it.
// No atomics: every node is written by one lane, and a layer reads what the launch before wrote, in stream order.  Every route writes
// hash_pair of the same children, so `nodes` is a function of the image alone.
#include "image_tree.h"
#include "scan.h"
#include "sort.h"
#include "zku1.h"
#include "zkn1.h"

#include <cstring>
#include <vector>

using namespace zkh;

namespace {

constexpr uint32_t IMG_THREADS = 256;
// A layer is listed when D + LIST_COST <= width.  Measured (DESIGN.md §2 ARGUMENTS, M18): a dense layer of `width` parents takes
// max(26 us, 0.21 ns x width) — one permutation's latency, or the chip's rate —, a listed one the same for its count of at most D plus
// 11 .. 14 us for its list: what 2^16 permutations cost at that rate.  So a layer of 2^16 parents is never listed (it is one
// permutation's latency either way), and no layer is whose D is within 2^16 of its width.  (An experiment build, ZKH_BUILD_FLAGS,
// may set another cost.)
#ifndef ZKH_IMAGE_LIST_COST
#define ZKH_IMAGE_LIST_COST 65536
#endif
constexpr size_t LIST_COST = ZKH_IMAGE_LIST_COST;
static_assert(LIST_COST >= ((size_t)1 << WIDE_LOG), "the layers of hash.hip's 8-lane kernels are never listed");
bool listed(size_t D, size_t width) { return D + LIST_COST <= width; }

__device__ __forceinline__ uint32_t image_word(const uint32_t* __restrict__ image, uint32_t W, size_t a) { return a < W ? image[a] % P : 0u; }

// grid ceil(2 L / IMG_THREADS): lane i writes words [4 i, 4 i + 4) of the leaf layer; the first two lanes also digest 0
__global__ __launch_bounds__(IMG_THREADS) void k_image_leaves(const uint32_t* __restrict__ image, uint32_t W, size_t L, uint32_t* __restrict__ nodes) {
    const size_t i = (size_t)blockIdx.x * IMG_THREADS + threadIdx.x;
    if (i >= 2 * L) return;
    const size_t a = 4 * i;
    *(uint4*)(nodes + 8 * L + a) = make_uint4(image_word(image, W, a), image_word(image, W, a + 1), image_word(image, W, a + 2), image_word(image, W, a + 3));
    if (i < 2) *(uint4*)(nodes + a) = make_uint4(0, 0, 0, 0);
}

// grid ceil(D / IMG_THREADS) over the table's rows: the first row of every dirty leaf rewrites it
__global__ __launch_bounds__(IMG_THREADS) void k_image_dirty_leaves(const uint32_t* __restrict__ addrs, uint32_t D, const uint32_t* __restrict__ image, uint32_t W,
                                                                    size_t L, uint32_t* __restrict__ nodes) {
    const uint32_t t = blockIdx.x * IMG_THREADS + threadIdx.x;
    if (t >= D) return;
    const uint32_t leaf = canonical(addrs[t]) >> 3;
    if (t && (canonical(addrs[t - 1]) >> 3) == leaf) return;
    const size_t a = (size_t)leaf * 8;
    uint4* o = (uint4*)(nodes + (L + leaf) * 8);
    o[0] = make_uint4(image_word(image, W, a), image_word(image, W, a + 1), image_word(image, W, a + 2), image_word(image, W, a + 3));
    o[1] = make_uint4(image_word(image, W, a + 4), image_word(image, W, a + 5), image_word(image, W, a + 6), image_word(image, W, a + 7));
}

// The dirty parent that item t of the layer below names.  kTable: the items are the table's rows, a row's parent on the widest parent
// layer is its address >> 4; else the items are the list of the layer below, and a node's parent is its index >> 1.
// kShift: what a table row's address is shifted by: 4 names its parent on the widest parent layer, 3 its leaf (the proof's first list).
template <bool kTable, int kShift = 4>
__device__ __forceinline__ uint32_t parent_of(const uint32_t* __restrict__ src, uint32_t t) { return kTable ? canonical(src[t]) >> kShift : src[t] >> 1; }

// grid ceil(bound / IMG_THREADS) over the items [0, m) of the layer below, m = *count (kTable: the host's D, count = NULL): the heads stage,
// a head being an item whose parent differs from the item before's; the totals from sums[1].  Workgroups past m leave a total of 0.
template <bool kTable, int kShift = 4>
__global__ __launch_bounds__(IMG_THREADS) void k_image_heads(const uint32_t* __restrict__ src, const uint32_t* __restrict__ count, uint32_t D,
                                                             uint32_t* __restrict__ local, uint32_t* __restrict__ sums) {
    __shared__ uint32_t buf[2][IMG_THREADS];
    const uint32_t m = kTable ? D : *count;
    const uint32_t t = blockIdx.x * IMG_THREADS + threadIdx.x;
    const uint32_t head = t < m && (t == 0 || parent_of<kTable, kShift>(src, t - 1) != parent_of<kTable, kShift>(src, t));
    scan_heads<IMG_THREADS>(head, t, m, buf, local, sums + 1);
}
// ... and after the counter scan (sums[1 + workgroup] = the heads of the workgroups before it): every head writes its parent at its rank.
// `count` is the count k_image_heads read: the layer below's, in the other counter run than `sums` (whose word 0 is now this layer's).
template <bool kTable>
__global__ __launch_bounds__(IMG_THREADS) void k_image_compact(const uint32_t* __restrict__ src, uint32_t m_table, const uint32_t* __restrict__ count,
                                                               const uint32_t* __restrict__ local, const uint32_t* __restrict__ sums, uint32_t* __restrict__ list) {
    const uint32_t m = kTable ? m_table : *count;
    const uint32_t t = blockIdx.x * IMG_THREADS + threadIdx.x;
    if (t >= m) return;
    const uint32_t v = parent_of<kTable>(src, t);
    if (t == 0 || parent_of<kTable>(src, t - 1) != v) list[head_rank(local, sums + 1, t)] = v;
}

// ---- THE UPDATE'S PROOF (include/zkhal.h; the header comment of zkh::image_proof_build below; its layout: zku1.h) ----
// A layer whose list holds at most 2^PROOF_TOP_LOG items for certain (min(D, its nodes): the bound only falls on the way up) is walked,
// with every layer above it, by ONE workgroup in one launch (k_proof_top): the list fits its lanes, and a layer costs barriers instead
// of three launches.  Measured (DESIGN.md §2 ARGUMENTS, M19): a layer of three launches takes 12 us whatever its list holds up to 2^19
// items (16 us with 6 x 10^5 digests to copy), a layer inside the top kernel 1.8 us; so the top starts as low as its lanes allow.
constexpr int PROOF_TOP_LOG = 10;
constexpr uint32_t TOP_THREADS = 1u << PROOF_TOP_LOG;
// the counts on the device, three words per layer k: the items of S_k, c_k, and the word of `proof` where C_k's digests start
enum { PM_ITEMS = 0, PM_CLEAN = 1, PM_OFF = 2, PM_WORDS = 3 };

// A digest from `nodes` (16-byte aligned: two 16-byte loads) to the proof (word aligned: its sections start where the counts put them)
__device__ __forceinline__ void copy_digest(const uint32_t* __restrict__ from, uint32_t* __restrict__ to) {
    const uint4 a = ((const uint4*)from)[0], b = ((const uint4*)from)[1];
    to[0] = a.x; to[1] = a.y; to[2] = a.z; to[3] = a.w;
    to[4] = b.x; to[5] = b.y; to[6] = b.z; to[7] = b.w;
}

// The two flags of item t of a sorted list S_k of m node indices, given its neighbours (NONE past either end): bit 0 "my sibling is not
// my neighbour in the list" (its digest is a clean sibling), bit 16 "my parent differs from the item before's" (a head of S_{k+1}).
__device__ __forceinline__ uint32_t proof_flags(uint32_t before, uint32_t x, uint32_t after) {
    const bool paired = x & 1 ? before == x - 1 : after == x + 1;          // before / after = NONE never match: x < 2^29
    const bool head = before == NONE || (before >> 1) != (x >> 1);
    return (paired ? 0u : 1u) | (head ? 0x10000u : 0u);
}

// grid ceil(D / IMG_THREADS): row i of the table as three words (the address as an integer, the residues of p_in and p_out); lane 0
// the header's words that the host knows
__global__ __launch_bounds__(IMG_THREADS) void k_proof_table(const uint32_t* __restrict__ addrs, const uint32_t* __restrict__ in, const uint32_t* __restrict__ out,
                                                             uint32_t D, uint32_t W, uint32_t h, uint32_t* __restrict__ proof) {
    const uint32_t t = blockIdx.x * IMG_THREADS + threadIdx.x;
    if (t >= D) return;
    uint32_t* row = table_row(proof + proof_table_at(h), t);
    row[ROW_ADDR] = canonical(addrs[t]);
    row[ROW_IN] = in[t] % P;
    row[ROW_OUT] = out[t] % P;
    if (t == 0) { proof[0] = PROOF_MAGIC; proof[PROOF_W] = W; proof[PROOF_D] = D; proof[PROOF_H] = h; }
}

// After k_image_heads<true, 3> and its counter scan (meta[PM_ITEMS] = M): every row that is the first of its leaf writes the leaf's
// index at its rank into `list` (S_0) and copies the leaf, as `nodes` holds it, to the proof's leaf section at that rank.  Lane 0 writes
// M to the header and the word where the sibling digests start.
__global__ __launch_bounds__(IMG_THREADS) void k_proof_leaves(const uint32_t* __restrict__ addrs, uint32_t D, const uint32_t* __restrict__ local,
                                                              const uint32_t* __restrict__ sums, const uint32_t* __restrict__ nodes, size_t L, uint32_t h,
                                                              uint32_t* __restrict__ list, uint32_t* __restrict__ meta, uint32_t* __restrict__ proof) {
    const uint32_t t = blockIdx.x * IMG_THREADS + threadIdx.x;
    if (t >= D) return;
    const size_t leaves0 = proof_leaves_at(h, D);
    if (t == 0) {
        const uint32_t M = meta[PM_ITEMS];
        proof[PROOF_M] = M;
        meta[PM_OFF] = (uint32_t)(leaves0 + 8 * (size_t)M);
    }
    const uint32_t leaf = canonical(addrs[t]) >> 3;
    if (t && (canonical(addrs[t - 1]) >> 3) == leaf) return;
    const uint32_t rank = head_rank(local, sums + 1, t);
    list[rank] = leaf;
    copy_digest(nodes + (L + leaf) * 8, proof + leaves0 + 8 * (size_t)rank);
}

// One layer below the top kernel's, three launches.  First, grid ceil(bound / IMG_THREADS) over the items [0, m) of S_k,
// m = meta[PM_ITEMS]: both flags of every item, scanned in the workgroup as one packed word (a workgroup's counts are <= 256: 16 bits
// each), local[t] = the packed inclusive counts, the workgroup's totals to its place in the two runs of `sums` ([0, nb) clean, [nb, 2 nb) heads).
__global__ __launch_bounds__(IMG_THREADS) void k_proof_flags(const uint32_t* __restrict__ list, const uint32_t* __restrict__ meta, uint32_t* __restrict__ local,
                                                             uint32_t* __restrict__ sums, uint32_t nb) {
    __shared__ uint32_t buf[2][IMG_THREADS];
    const uint32_t m = meta[PM_ITEMS];
    const uint32_t t = blockIdx.x * IMG_THREADS + threadIdx.x;
    uint32_t f = 0;
    if (t < m) f = proof_flags(t ? list[t - 1] : NONE, list[t], t + 1 < m ? list[t + 1] : NONE);
    const uint32_t incl = block_scan<IMG_THREADS>(f, buf, AddWrap());
    if (t < m) local[t] = incl;
    if (threadIdx.x == IMG_THREADS - 1) { sums[blockIdx.x] = incl & 0xffff; sums[nb + blockIdx.x] = incl >> 16; }
}
// ... then the counter scan over both runs (c_k to meta[PM_CLEAN], the items of S_{k+1} to the next layer's meta[PM_ITEMS]), then: an
// item whose sibling is clean copies that digest from `nodes` to the proof at its rank, a head writes its parent into `next` at its
// rank.  Lane 0 writes c_k to the header and the next layer's offset.  `width` = the nodes of layer k.
__global__ __launch_bounds__(IMG_THREADS) void k_proof_gather(const uint32_t* __restrict__ list, uint32_t* __restrict__ meta, const uint32_t* __restrict__ local,
                                                              const uint32_t* __restrict__ sums, uint32_t nb, const uint32_t* __restrict__ nodes, size_t width,
                                                              uint32_t k, uint32_t* __restrict__ next, uint32_t* __restrict__ proof) {
    const uint32_t m = meta[PM_ITEMS], off = meta[PM_OFF];
    const uint32_t t = blockIdx.x * IMG_THREADS + threadIdx.x;
    if (t >= m) return;
    if (t == 0) {
        const uint32_t c = meta[PM_CLEAN];
        proof[PROOF_HEADER + k] = c;
        meta[PM_WORDS + PM_OFF] = off + 8 * c;
    }
    const uint32_t x = list[t];
    const uint32_t f = proof_flags(t ? list[t - 1] : NONE, x, t + 1 < m ? list[t + 1] : NONE);
    const uint32_t ranks = local[t];
    if (f & 1) copy_digest(nodes + (width + (x ^ 1)) * 8, proof + off + 8 * (size_t)((ranks & 0xffff) + sums[blockIdx.x] - 1));
    if (f >> 16) next[(ranks >> 16) + sums[nb + blockIdx.x] - 1] = x >> 1;
}

// The narrow top: ONE workgroup walks every layer k0 <= k < h (S_k0 and so every list above it fits its lanes), the list in
// LDS: flag, scan, gather, parents, a barrier between the layers.  meta: layer k0's three words.
__global__ __launch_bounds__(TOP_THREADS) void k_proof_top(const uint32_t* __restrict__ list, const uint32_t* __restrict__ meta, const uint32_t* __restrict__ nodes,
                                                           size_t L, uint32_t k0, uint32_t h, uint32_t* __restrict__ proof) {
    __shared__ uint32_t items[2][TOP_THREADS];
    __shared__ uint32_t buf[2][TOP_THREADS];
    __shared__ uint32_t totals;
    const uint32_t t = threadIdx.x;
    uint32_t m = meta[PM_ITEMS], off = meta[PM_OFF];
    if (t < m) items[0][t] = list[t];
    __syncthreads();
    int cur = 0;
    for (uint32_t k = k0; k < h; k++, cur ^= 1) {
        const uint32_t x = t < m ? items[cur][t] : 0;
        uint32_t f = 0;
        if (t < m) f = proof_flags(t ? items[cur][t - 1] : NONE, x, t + 1 < m ? items[cur][t + 1] : NONE);
        const uint32_t incl = block_scan<TOP_THREADS>(f, buf, AddWrap());
        if (t == TOP_THREADS - 1) totals = incl;
        __syncthreads();
        const uint32_t c = totals & 0xffff;
        if (f & 1) copy_digest(nodes + ((L >> k) + (x ^ 1)) * 8, proof + off + 8 * (size_t)((incl & 0xffff) - 1));
        if (f >> 16) items[cur ^ 1][(incl >> 16) - 1] = x >> 1;
        if (t == 0) proof[PROOF_HEADER + k] = c;
        m = totals >> 16;
        off += 8 * c;
        __syncthreads();
    }
}

}  // namespace

// THE UPDATE'S PROOF on the device (zkh_page_out_proof, page_out.hip -> image_proof_build), after the check pass: the table's rows [0, D)
// hold strictly increasing addresses a_i < W and p_in is what the tree holds.  `nodes` is only read.
//   proof_table  : the header's W, D, h and the 3 D table words, one pass over D lanes;
//   proof_leaves : S_0 = the adjacent-unique of a_i >> 3, flag / scan / compact as image_list does for a_i >> 4 (k_image_heads with the
//                  shift 3, the counter scan, k_proof_leaves): a head lane copies its 32-byte leaf to its rank; M and the siblings'
//                  first word are written from the count;
//   proof_layer  : per layer whose list may hold more than 2^PROOF_TOP_LOG items (min(D, its nodes)): k_proof_flags, ONE counter scan
//                  over two runs, k_proof_gather;
//   proof_top    : every layer from the first whose list cannot, in one launch of one workgroup.  L = 1 has no layer.
// No atomics and no read-back: every count stays on the device (`meta`), every section's offset comes from counts an earlier launch
// (or, in the top, an earlier barrier) wrote, every word of the proof is written by one lane.  The grids are sized by the bounds
// min(D, the layer's nodes); lanes past the count leave.
const char* zkh::image_proof_build(zkh_ctx* ctx, const uint32_t* addrs, const uint32_t* in, const uint32_t* out, uint32_t D, size_t image_words,
                                   const zkh_buf* nodes, zkh_buf* proof) {
    const size_t L = image_leaves(image_words);
    const uint32_t W = (uint32_t)image_words;
    const uint32_t h = image_height(image_words);
    if (!D) {                                           // the header alone: nothing to launch
        std::vector<uint32_t> header(PROOF_HEADER + h, 0);
        header[0] = PROOF_MAGIC; header[PROOF_W] = W; header[PROOF_H] = h;
        return zkh_write(ctx, proof, header.data(), 0, header.size());
    }
    const uint32_t nb0 = (D + IMG_THREADS - 1) / IMG_THREADS;
    Tmp lists[2], local, sums, meta;
    for (int i = 0; i < 2; i++) ZKH_TRY(new_buf(ctx, D, false, lists[i].out()));
    ZKH_TRY(new_buf(ctx, D, false, local.out()));
    ZKH_TRY(new_buf(ctx, 1 + 2 * (size_t)nb0, false, sums.out()));
    ZKH_TRY(new_buf(ctx, PM_WORDS * ((size_t)h + 2), false, meta.out()));
    {
        ProfScope prof(ctx, "proof_table", 24.0 * D);
        k_proof_table<<<nb0, IMG_THREADS, 0, ctx->stream>>>(addrs, in, out, D, W, h, proof->ptr());
        ZKH_TRY(last_launch_error("proof_table"));
    }
    {
        ProfScope prof(ctx, "proof_leaves", 16.0 * D + 8.0 * nb0 + 68.0 * (D < L ? D : L));
        k_image_heads<true, 3><<<nb0, IMG_THREADS, 0, ctx->stream>>>(addrs, nullptr, D, local->ptr(), sums->ptr());
        ZKH_TRY(last_launch_error("proof_heads"));
        scan_counters(ctx, sums->ptr() + 1, 1, nb0, meta->ptr() + PM_ITEMS, 0);
        ZKH_TRY(last_launch_error("proof_carry"));
        k_proof_leaves<<<nb0, IMG_THREADS, 0, ctx->stream>>>(addrs, D, local->ptr(), sums->ptr(), nodes->ptr(), L, h, lists[0]->ptr(), meta->ptr(), proof->ptr());
        ZKH_TRY(last_launch_error("proof_leaves"));
    }
    uint32_t k0 = 0;                                    // layers [0, k0): S_k may hold more items than the top kernel has lanes
    while (k0 < h && (D < (L >> k0) ? D : (L >> k0)) > TOP_THREADS) k0++;
    int cur = 0;
    for (uint32_t k = 0; k < k0; k++, cur ^= 1) {
        const size_t width = L >> k;
        const uint32_t items = (uint32_t)(D < width ? D : width);
        const uint32_t nb = (items + IMG_THREADS - 1) / IMG_THREADS;
        uint32_t* mk = meta->ptr() + PM_WORDS * (size_t)k;
        ProfScope prof(ctx, "proof_layer", 20.0 * items + 16.0 * nb + 64.0 * (items < width / 2 ? items : width / 2));
        k_proof_flags<<<nb, IMG_THREADS, 0, ctx->stream>>>(lists[cur]->ptr(), mk, local->ptr(), sums->ptr(), nb);
        ZKH_TRY(last_launch_error("proof_flags"));
        scan_counters(ctx, sums->ptr(), 2, nb, mk + PM_CLEAN, PM_WORDS - PM_CLEAN + PM_ITEMS);
        ZKH_TRY(last_launch_error("proof_carry"));
        k_proof_gather<<<nb, IMG_THREADS, 0, ctx->stream>>>(lists[cur]->ptr(), mk, local->ptr(), sums->ptr(), nb, nodes->ptr(), width, k, lists[cur ^ 1]->ptr(),
                                                            proof->ptr());
        ZKH_TRY(last_launch_error("proof_gather"));
    }
    if (k0 < h) {
        const size_t width = L >> k0;
        const size_t items = D < width ? D : width;
        double digests = 0;                             // at most min(items, the layer's pairs) clean siblings per layer
        for (uint32_t k = k0; k < h; k++) digests += (double)(items < (L >> k) / 2 ? items : (L >> k) / 2);
        ProfScope prof(ctx, "proof_top", 4.0 * items + 64.0 * digests);
        k_proof_top<<<1, TOP_THREADS, 0, ctx->stream>>>(lists[cur]->ptr(), meta->ptr() + PM_WORDS * (size_t)k0, nodes->ptr(), L, k0, h, proof->ptr());
        ZKH_TRY(last_launch_error("proof_top"));
    }
    // the temporaries go back to the pool on return: the stream orders their next use after these launches
    return nullptr;
}

const char* zkh::image_tree_update(zkh_ctx* ctx, const uint32_t* addrs, uint32_t D, const zkh_buf* image, zkh_buf* nodes) {
    const size_t L = image_leaves(image->len);
    const uint32_t W = (uint32_t)image->len;
    ZKH_REQUIRE(nodes->len == 16 * L, "image_tree_update: nodes of %zu words for an image of %zu", nodes->len, image->len);
    if (!D) return nullptr;
    {
        ProfScope prof(ctx, "image_leaves", 8.0 * D + 64.0 * D);
        k_image_dirty_leaves<<<(D + IMG_THREADS - 1) / IMG_THREADS, IMG_THREADS, 0, ctx->stream>>>(addrs, D, image->ptr(), W, L, nodes->ptr());
        ZKH_TRY(last_launch_error("image_leaves"));
    }
    size_t width = L / 2;                               // the parents of the layer in hand
    if (listed(D, width)) {
        // two lists (a layer reads the one below's), the local ranks, and two counter runs: a layer's counter scan leaves its count in
        // word 0 of its own run while the compaction still reads the count of the layer below from the other
        const uint32_t nb0 = (D + IMG_THREADS - 1) / IMG_THREADS;
        Tmp lists[2], local, sums[2];
        for (int i = 0; i < 2; i++) {
            ZKH_TRY(new_buf(ctx, D, false, lists[i].out()));
            ZKH_TRY(new_buf(ctx, 1 + (size_t)nb0, false, sums[i].out()));
        }
        ZKH_TRY(new_buf(ctx, D, false, local.out()));
        int cur = 0;
        const uint32_t* src = addrs;                    // the items of the layer below: the table, then the lists
        const uint32_t* count = nullptr;                // ... and their number, on the device (the table's is D)
        uint32_t items = D;                             // ... and its bound: min(D, the layer below's width)
        for (bool table = true; listed(D, width); table = false, width /= 2, cur ^= 1) {
            const uint32_t nb = (items + IMG_THREADS - 1) / IMG_THREADS;
            uint32_t* list = lists[cur]->ptr();
            uint32_t* sm = sums[cur]->ptr();
            {
                ProfScope prof(ctx, "image_list", 16.0 * items + 8.0 * nb);
                if (table) k_image_heads<true><<<nb, IMG_THREADS, 0, ctx->stream>>>(src, count, D, local->ptr(), sm);
                else k_image_heads<false><<<nb, IMG_THREADS, 0, ctx->stream>>>(src, count, D, local->ptr(), sm);
                ZKH_TRY(last_launch_error("image_heads"));
                scan_counters(ctx, sm + 1, 1, nb, sm, 0);
                ZKH_TRY(last_launch_error("image_carry"));
                if (table) k_image_compact<true><<<nb, IMG_THREADS, 0, ctx->stream>>>(src, D, count, local->ptr(), sm, list);
                else k_image_compact<false><<<nb, IMG_THREADS, 0, ctx->stream>>>(src, D, count, local->ptr(), sm, list);
                ZKH_TRY(last_launch_error("image_compact"));
            }
            items = (uint32_t)(items < width ? items : width);
            ZKH_TRY(hash_fold_listed(ctx, nodes, width, list, sm, items));
            src = list;
            count = sm;
        }
    }
    // the temporaries go back to the pool on return: the stream orders their next use after these launches
    return width ? merkle_fold_from(ctx, nodes, 2 * width) : nullptr;
}

extern "C" size_t zkh_image_tree_words(size_t image_words) { return image_words ? 16 * image_leaves(image_words) : 0; }

extern "C" const char* zkh_image_commit(zkh_ctx* ctx, const zkh_buf* image, zkh_buf* nodes) {
    ZKH_REQUIRE(ctx && image && nodes, "image_commit: null argument");
    ZKH_REQUIRE(image->len >= 1 && image->len <= 0xffffffffull, "image_commit: an image of %zu words (1 .. 2^32 - 1)", image->len);
    const size_t L = image_leaves(image->len);
    ZKH_REQUIRE(nodes->len == 16 * L, "image_commit: nodes of %zu words; an image of %zu words has a tree of %zu (zkh_image_tree_words)", nodes->len, image->len, 16 * L);
    {
        ProfScope prof(ctx, "image_leaves", 4.0 * image->len + 32.0 * L);
        k_image_leaves<<<(unsigned)((2 * L + IMG_THREADS - 1) / IMG_THREADS), IMG_THREADS, 0, ctx->stream>>>(image->ptr(), (uint32_t)image->len, L, nodes->ptr());
        ZKH_TRY(last_launch_error("image_leaves"));
    }
    return merkle_fold_from(ctx, nodes, L);
}

extern "C" size_t zkh_image_proof_words(size_t image_words, size_t pages) {
    const size_t L = image_leaves(image_words), D = pages;
    size_t words = PROOF_HEADER + PROOF_ROW * D + 8 * (D < L ? D : L);
    for (size_t w = L; w > 1; w >>= 1) words += 1 + 8 * (D < w / 2 ? D : w / 2);
    return words;
}

// ---- THE UPDATE'S PROOF, WALKED (zkh_image_proof_verify on the host, zkh_image_proof_walk on the device) ----
// One source for every refusal of the two walks: `who` is the call's name, the text after it is the same for both (the header's
// and the table's refusals are zku1.h's: the page-out circuits share them).
namespace {

const char* refuse_word(const char* who, size_t i, uint32_t v) { return make_err("%s: word %zu is %u, not below P", who, i, v); }
const char* refuse_root_range(const char* who) { return make_err("%s: root_before is not 8 words below P", who); }
const char* refuse_leaves(const char* who, uint32_t M, size_t leaves) { return make_err("%s: M %u, but the table's rows lie in %zu leaves", who, M, leaves); }
const char* refuse_layer(const char* who, uint32_t k, uint32_t c, uint32_t take) { return make_err("%s: layer %u: %u siblings, but the walk takes %u", who, k, c, take); }
const char* refuse_in(const char* who, uint32_t i, uint32_t in, uint32_t a, uint32_t held) {
    return make_err("%s: row %u: in %u at address %u, but its leaf holds %u", who, i, in, a, held);
}
const char* refuse_root(const char* who, const uint32_t* top) {
    return make_err("%s: the proof opens root %08x %08x %08x %08x %08x %08x %08x %08x, not root_before", who, top[0], top[1], top[2], top[3], top[4], top[5], top[6], top[7]);
}

// zkh_image_proof_nodes alone, where the walk of an empty table would pass
const char* refuse_empty_nodes(const char* who) {
    return make_err("%s: an empty table (D = 0) has no dirty nodes: its proof is the header alone and holds no node, not even the root's children; "
                    "such a page-out is sealed from the tree (zkh_page_tree_witgen)", who);
}

// D = 0 after the header, the words and root_before have passed: the header must describe nothing
const char* proof_empty(const char* who, const uint32_t* head) {
    if (head[PROOF_M]) return refuse_leaves(who, head[PROOF_M], 0);
    for (uint32_t k = 0; k < head[PROOF_H]; k++)
        if (head[PROOF_HEADER + k]) return refuse_layer(who, k, head[PROOF_HEADER + k], 0);
    return nullptr;
}

}  // namespace

// The walk of include/zkhal.h "THE UPDATE'S PROOF" on the host: no context, no GPU; every layer is one batch through the permutation
// zkh_poseidon2_mix_host uses, the old children first, the new ones after them.
extern "C" const char* zkh_image_proof_verify(const uint32_t* proof, size_t words, const uint32_t root_before[8], uint32_t root_after[8]) {
    static const char who[] = "image_proof_verify";
    ZKH_REQUIRE(proof && root_before && root_after, "%s: null argument", who);
    ZKH_TRY(image_proof_header(who, proof, words));
    const ProofShape ps = proof_shape(proof);
    const uint32_t W = ps.W, D = ps.D, M = ps.M, h = ps.h;
    const uint32_t* c = proof + PROOF_HEADER;
    const size_t t0 = ps.table, l0 = ps.leaves, s0 = ps.siblings;
    for (size_t i = t0; i < words; i++)
        if (!(proof[i] < P || proof_word_is_address(i, t0, l0))) return refuse_word(who, i, proof[i]);
    for (int j = 0; j < 8; j++)
        if (root_before[j] >= P) return refuse_root_range(who);
    if (!D) {
        ZKH_TRY(proof_empty(who, proof));
        memmove(root_after, root_before, 32);
        return nullptr;
    }
    const uint32_t* table = proof + t0;
    std::vector<uint32_t> S, rank(D);                   // the dirty nodes of the layer in hand; every row's leaf among S_0
    for (uint32_t i = 0; i < D; i++) {
        const uint32_t a = table_addr(table, i), before = i ? table_addr(table, i - 1) : 0;
        if (table_row_refused(i, a, before, W)) return refuse_row(who, i, a, before, W);
        if (S.empty() || S.back() != a >> 3) S.push_back(a >> 3);
        rank[i] = (uint32_t)S.size() - 1;
    }
    if (S.size() != M) return refuse_leaves(who, M, S.size());
    // the digests of the layer in hand, 16 words per item: the old one, then the new one
    std::vector<uint32_t> cur(16 * (size_t)M), st;
    for (size_t j = 0; j < M; j++) {
        memcpy(&cur[16 * j], proof + l0 + 8 * j, 32);
        memcpy(&cur[16 * j + 8], proof + l0 + 8 * j, 32);
    }
    for (uint32_t i = 0; i < D; i++) {
        const uint32_t a = table_addr(table, i), held = cur[16 * (size_t)rank[i] + (a & 7)];
        if (held != table_in(table, i)) return refuse_in(who, i, table_in(table, i), a, held);
        cur[16 * (size_t)rank[i] + 8 + (a & 7)] = table_out(table, i);
    }
    size_t at = s0;
    for (uint32_t k = 0; k < h; k++) {
        const size_t m = S.size();
        uint32_t take = 0;
        for (size_t j = 0; j < m; j++) take += !(S[j] & 1 ? j && S[j - 1] == S[j] - 1 : j + 1 < m && S[j + 1] == S[j] + 1);
        if (take != c[k]) return refuse_layer(who, k, c[k], take);
        std::vector<uint32_t> up;
        st.clear();                                     // per parent two states of 24 words: (old left, old right, 0), (new left, new right, 0)
        for (size_t j = 0; j < m; j++) {
            const uint32_t x = S[j];
            const bool pair = !(x & 1) && j + 1 < m && S[j + 1] == x + 1;
            const uint32_t* left[2] = {&cur[16 * j], &cur[16 * j + 8]};
            const uint32_t* right[2] = {left[0], left[1]};
            if (pair) { right[0] = &cur[16 * (j + 1)]; right[1] = &cur[16 * (j + 1) + 8]; }
            else if (x & 1) { left[0] = left[1] = proof + at; at += 8; }
            else { right[0] = right[1] = proof + at; at += 8; }
            for (int v = 0; v < 2; v++) {
                st.insert(st.end(), left[v], left[v] + 8);
                st.insert(st.end(), right[v], right[v] + 8);
                st.insert(st.end(), 8, 0u);
            }
            up.push_back(x >> 1);
            j += pair;
        }
        ZKH_TRY(zkh_poseidon2_mix_host(nullptr, nullptr, st.data(), st.size() / 24));
        cur.resize(16 * up.size());
        for (size_t j = 0; j < up.size(); j++) {
            memcpy(&cur[16 * j], &st[48 * j], 32);
            memcpy(&cur[16 * j + 8], &st[48 * j + 24], 32);
        }
        S.swap(up);
    }
    if (memcmp(cur.data(), root_before, 32)) return refuse_root(who, cur.data());
    memcpy(root_after, &cur[8], 32);
    return nullptr;
}

// THE WALK ON THE DEVICE (zkh_image_proof_walk): what zkh_image_proof_verify computes, from a proof that sits in device memory.
//
// SAFETY AGAINST ANY INPUT.  The proof is hostile until shown otherwise, and nothing below may read a proof word at or past `words`,
// or a scratch item past its count, whatever the proof holds.  The reasoning, stage by stage:
//   header     : the host reads min(words, PROOF_HEAD_MAX) words once and runs image_proof_header (zku1.h) on them: after it, h is W's (<= 29),
//                words = t0 + 3 D + 8 M + 8 sum c_k exactly, so the table [t0, l0), the leaves [l0, s0) and the siblings [s0, words) are
//                sections of the proof, and 3 D + 8 M <= words: the scratch, sized by min(D, M, L), is a small multiple of the proof.
//   walk_check : k_walk_range reads the words [t0, words), k_walk_rows the address words t0 + 3 i, i < D: inside the table.  They
//                gate nothing and are gated by nothing; each leaves the LOWEST index it refuses (atomicMin), so the result does
//                not depend on the order in which lanes arrive.  The counter scan leaves the number of distinct leaves in the record.
//   walk_leaves: gated on what the launches BEFORE it left (a word >= P, a refused row, a count of leaves other than M).  No leaf is
//                read before M has been found to be the table's count ON THE DEVICE: a rank is then below M and the leaf inside
//                [l0, s0); with a wrong M a rank could run into the siblings or past the proof.  Lane 0 hands layer 0 its count: M, or
//                0 when the gate is shut, so that every later stage has nothing to do.  The gate does not include the stage's own
//                refusal (an `in` that differs): lanes that saw it early would leave, and the lowest row would depend on timing.
//   walk_layer : k_proof_flags reads list[0, m), m the count the stage before left (<= the list's size by the above).  k_walk_parents
//                is gated on every earlier refusal AND on the layer's taken-count being c_k; lane 0 hands the next layer |S_{k+1}|, or 0
//                when the gate is shut.  hash.hip's k_hash_walk runs one lane per permutation of the parents below that count, so
//                it does nothing after a refusal, and its sibling ranks are below take = c_k: the reads stay inside C_k's section,
//                which ends at or before `words` because the length was what the header describes.  With take > c_k and no gate a
//                lane would read past the section.
//   walk_top   : copies the two top digests into the record only when the last count is 1, and the values a message prints (read at
//                indices the check stages refused, which they had read themselves).
// The only atomics are the atomicMin's on the record; every scratch word has one writer (a leaf's two digests: the lane of the leaf's
// first row; a parent's digest: the lane of that permutation; lists and ranks: the head lanes, as in image_proof_build); a launch reads
// what earlier launches wrote, in stream order.  Two calls give the same record.
//
// THE DIRTY NODES (zkh_image_proof_nodes; zkn1.h).  The same stages, and nothing above changes: no stage reads a word it did not read
// before, and what it keeps it writes into a scratch buffer of the table's BOUND, never into the caller's.  A section's count is the
// count the walk itself runs the layer's parents under (|S_{k+1}| <= min(D, M, L, the layer's nodes), 0 once a gate is shut), and the
// bound counts min(D, its nodes) items for layer k: whatever the proof holds, the packed sections end inside the scratch buffer.
// Writers: a section's ids the head lanes of k_walk_parents (the lanes that write `next`), its records the two lanes of each
// permutation of k_hash_walk (the children they have just read), its count and the next section's first word lane 0 of
// k_walk_parents, the header lane 0 of k_walk_leaves: one writer per word, no atomic.  The caller's buffer takes one device copy of
// the table's words after the record has come back clean.
//
// NARROW LAYERS.  Every layer is its own four launches (flags, the counter scan, parents, hash) whatever its list holds: the simplest
// of the three candidates (one launch per layer; one workgroup walking the narrow layers with barriers; hash.hip's 8-lane permutation),
// and the only one built.  No constant switches a code path but the workgroup size.  What it reads: DESIGN.md §2 ARGUMENTS, M20.
namespace {

// the result record, 32 words.  Two 64-bit keys (index << 32 | the value the message prints), then words.
enum {
    WR_RANGE = 0,       // 64 bits: the lowest word >= P and the word
    WR_IN = 2,          // 64 bits: the lowest row whose `in` differs and what its leaf holds
    WR_ROW = 4,         // the lowest refused row
    WR_COUNT = 5,       // the distinct leaves of the table
    WR_LAYER = 6, WR_LAYER_C = 7, WR_LAYER_TAKE = 8,    // the lowest layer whose taken-count is not c_k, c_k, the count
    WR_ROW_A = 9, WR_ROW_BEFORE = 10,                   // the refused row's address and the one before it
    WR_IN_IN = 11, WR_IN_A = 12,                        // that row's `in` and address
    WR_TOP_ITEMS = 13,  // the items of the top layer (1 after a walk that went through)
    WR_DIRTY_END = 14,  // the word where the dirty-node table ends (zkh_image_proof_nodes)
    WR_DIGESTS = 16,    // the old and the new top digest
    WR_WORDS = 32
};
// per layer on the device: the items of S_k, the word where C_k starts, the two totals of the layer's counter scan, and the word of the
// dirty-node table (zkn1.h) where the section of S_{k+1} starts
enum { WM_ITEMS = 0, WM_OFF = 1, WM_TAKE = 2, WM_HEADS = 3, WM_DIRTY = 4, WM_WORDS = 5 };
static_assert(WM_ITEMS == PM_ITEMS, "k_proof_flags reads the layer's count at PM_ITEMS");

__device__ __forceinline__ void lowest(unsigned long long* slot, uint32_t index, uint32_t value) {
    const unsigned long long key = ((unsigned long long)index << 32) | value;
    if (key < *(volatile unsigned long long*)slot) atomicMin(slot, key);       // entries only decrease
}
__device__ __forceinline__ bool clean64(const uint32_t* st, int at) { return (st[at] & st[at + 1]) == NONE; }

// grid ceil((words - t0) / IMG_THREADS): every word of the table's in / out, of the leaves and of the siblings is below P
__global__ __launch_bounds__(IMG_THREADS) void k_walk_range(const uint32_t* __restrict__ proof, size_t t0, size_t l0, size_t words, uint32_t* __restrict__ st) {
    const size_t i = t0 + (size_t)blockIdx.x * IMG_THREADS + threadIdx.x;
    if (i >= words) return;
    const uint32_t v = proof[i];
    if (v >= P && !proof_word_is_address(i, t0, l0)) lowest((unsigned long long*)(st + WR_RANGE), (uint32_t)i, v);
}

// grid ceil(D / IMG_THREADS) over the rows of the proof's table (stride 3, addresses as integers): the lowest row whose address lies
// outside the image or does not follow a smaller one; and what k_image_heads<true, 3> leaves for a raw column: local[t] = the heads
// (rows whose leaf differs from the row before's) of t's workgroup up to t, sums[1 + workgroup] its total.
__global__ __launch_bounds__(IMG_THREADS) void k_walk_rows(const uint32_t* __restrict__ table, uint32_t D, uint32_t W, uint32_t* __restrict__ local,
                                                           uint32_t* __restrict__ sums, uint32_t* __restrict__ st) {
    __shared__ uint32_t buf[2][IMG_THREADS];
    const uint32_t t = blockIdx.x * IMG_THREADS + threadIdx.x;
    const uint32_t a = t < D ? table_addr(table, t) : 0, before = t && t < D ? table_addr(table, t - 1) : 0;
    if (t < D && table_row_refused(t, a, before, W)) atomicMin(st + WR_ROW, t);
    const uint32_t head = t < D && (t == 0 || (before >> 3) != (a >> 3));
    scan_heads<IMG_THREADS>(head, t, D, buf, local, sums + 1);
}

// grid ceil(D / IMG_THREADS), after the counter scan (st[WR_COUNT]).  The lane of a leaf's first row owns the leaf: its index to
// list[rank], the old digest (the proof's leaf) and the new one (the rows' `out` put in) to dig[16 rank, +16), every `in` of the leaf's
// rows (at most 8, consecutive) compared with the old word.  Lane 0 hands layer 0 its count, the siblings' first word and the dirty-node
// table's first section, and writes that table's header (`dirty`, or null: W, D, h are the proof's).
__global__ __launch_bounds__(IMG_THREADS) void k_walk_leaves(const uint32_t* __restrict__ proof, uint32_t t0, uint32_t D, uint32_t M, const uint32_t* __restrict__ local,
                                                             const uint32_t* __restrict__ sums, uint32_t* __restrict__ st, uint32_t* __restrict__ list,
                                                             uint32_t* __restrict__ dig, uint32_t* __restrict__ meta, uint32_t W, uint32_t h, uint32_t* __restrict__ dirty) {
    const uint32_t t = blockIdx.x * IMG_THREADS + threadIdx.x;
    const size_t l0 = (size_t)t0 + PROOF_ROW * (size_t)D;
    const bool ok = clean64(st, WR_RANGE) && st[WR_ROW] == NONE && st[WR_COUNT] == M;
    if (t == 0) {
        meta[WM_ITEMS] = ok ? M : 0; meta[WM_OFF] = (uint32_t)(l0 + 8 * (size_t)M); meta[WM_DIRTY] = NODES_HEADER + h;
        if (dirty) { dirty[0] = NODES_MAGIC; dirty[NODES_W] = W; dirty[NODES_D] = D; dirty[NODES_H] = h; }
    }
    if (t >= D || !ok) return;
    const uint32_t* table = proof + t0;
    const uint32_t leaf = table_addr(table, t) >> 3;
    if (t && (table_addr(table, t - 1) >> 3) == leaf) return;
    const uint32_t rank = head_rank(local, sums + 1, t);         // < M: the count is M
    list[rank] = leaf;
    const uint32_t* from = proof + l0 + 8 * (size_t)rank;
    uint32_t o[8], n[8];
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = n[j] = from[j];
    uint32_t bad = NONE, held = 0;
    for (uint32_t u = t; u < D && u - t < 8; u++) {
        const uint32_t* row = table_row(table, u);
        const uint32_t a = row[ROW_ADDR];
        if ((a >> 3) != leaf) break;
        uint32_t was = 0;
#pragma unroll
        for (int j = 0; j < 8; j++)
            if ((a & 7) == (uint32_t)j) { was = o[j]; n[j] = row[ROW_OUT]; }
        if (was != row[ROW_IN] && bad == NONE) { bad = u; held = was; }
    }
    if (bad != NONE) lowest((unsigned long long*)(st + WR_IN), bad, held);
    uint4* d = (uint4*)(dig + 16 * (size_t)rank);
    d[0] = make_uint4(o[0], o[1], o[2], o[3]); d[1] = make_uint4(o[4], o[5], o[6], o[7]);
    d[2] = make_uint4(n[0], n[1], n[2], n[3]); d[3] = make_uint4(n[4], n[5], n[6], n[7]);
}

// grid ceil(bound / IMG_THREADS) over the items of S_k, after k_proof_flags and the counter scan over its two runs (meta[WM_TAKE], the
// siblings the walk takes; meta[WM_HEADS] = |S_{k+1}|).  Gated on every earlier refusal and on take = c_k.  A head writes, at its
// parent's rank: the parent's index (next), its own item (from) and the rank of the clean sibling it takes, NONE when it pairs with
// the item after it (sib).  Lane 0 hands the next layer its count (0: the gate is shut) and the word where C_{k+1} starts, and records
// the layer when its count is the first that differs.  `dirty` (or null; zkn1.h): lane 0 writes the count to its header as n_{k+1} and
// hands the next layer the word where this section ends; a head writes its parent's heap id, `up` + the parent's index (`up` = the
// nodes of layer k + 1), at its rank into the section's ids.
__global__ __launch_bounds__(IMG_THREADS) void k_walk_parents(const uint32_t* __restrict__ list, uint32_t* __restrict__ meta, const uint32_t* __restrict__ local,
                                                              const uint32_t* __restrict__ sums, uint32_t nb, uint32_t k, const uint32_t* __restrict__ proof,
                                                              uint32_t* __restrict__ st, uint32_t* __restrict__ next, uint32_t* __restrict__ from, uint32_t* __restrict__ sib,
                                                              uint32_t up, uint32_t* __restrict__ dirty) {
    const uint32_t m = meta[WM_ITEMS], take = meta[WM_TAKE], c = proof[PROOF_HEADER + k];
    const uint32_t t = blockIdx.x * IMG_THREADS + threadIdx.x;
    const bool before = clean64(st, WR_RANGE) && clean64(st, WR_IN) && st[WR_ROW] == NONE, ok = before && take == c;
    if (t == 0) {
        const uint32_t heads = ok ? meta[WM_HEADS] : 0;
        meta[WM_WORDS + WM_ITEMS] = heads;
        meta[WM_WORDS + WM_OFF] = meta[WM_OFF] + 8 * c;
        meta[WM_WORDS + WM_DIRTY] = meta[WM_DIRTY] + NODES_ITEM * heads;
        if (dirty) dirty[NODES_HEADER + k] = heads;
        if (before && m && take != c && st[WR_LAYER] == NONE) { st[WR_LAYER] = k; st[WR_LAYER_C] = c; st[WR_LAYER_TAKE] = take; }
    }
    if (t >= m || !ok) return;
    const uint32_t x = list[t];
    const uint32_t f = proof_flags(t ? list[t - 1] : NONE, x, t + 1 < m ? list[t + 1] : NONE);
    if (!(f >> 16)) return;
    const uint32_t ranks = local[t], r = (ranks >> 16) + sums[nb + blockIdx.x] - 1;
    next[r] = x >> 1;
    from[r] = t;
    sib[r] = f & 1 ? (ranks & 0xffff) + sums[blockIdx.x] - 1 : NONE;
    if (dirty) dirty[meta[WM_DIRTY] + r] = up + (x >> 1);
}

// one workgroup of 64: the top digests when the walk went through (items = the count of the top layer), and the values the messages of
// a refused row and of a differing `in` print; and the word where the dirty-node table ends (`items` is the top layer's meta)
__global__ __launch_bounds__(64) void k_walk_top(const uint32_t* __restrict__ proof, uint32_t t0, const uint32_t* __restrict__ items, const uint32_t* __restrict__ dig,
                                                 uint32_t* __restrict__ st) {
    const uint32_t t = threadIdx.x, n = *items;
    if (t < 16 && n == 1) st[WR_DIGESTS + t] = dig[t];
    if (t == 16) st[WR_TOP_ITEMS] = n;
    if (t == 19) st[WR_DIRTY_END] = items[WM_DIRTY];
    if (t == 17 && st[WR_ROW] != NONE) {
        const uint32_t i = st[WR_ROW];
        st[WR_ROW_A] = table_addr(proof + t0, i);
        st[WR_ROW_BEFORE] = i ? table_addr(proof + t0, i - 1) : 0;
    }
    if (t == 18 && !clean64(st, WR_IN)) {
        const uint32_t i = st[WR_IN + 1];
        st[WR_IN_A] = table_addr(proof + t0, i);
        st[WR_IN_IN] = table_in(proof + t0, i);
    }
}

}  // namespace

// Both entry points; `dirty` is zkh_image_proof_nodes' (null for the walk: THE DIRTY NODES above)
static const char* proof_walk(const char* who, zkh_ctx* ctx, const zkh_buf* proof, size_t words, const uint32_t root_before[8], uint32_t root_after[8], zkh_buf* dirty) {
    ZKH_REQUIRE(words <= proof->len, "%s: a proof of %zu words in a buffer of %zu", who, words, proof->len);
    ZKH_REQUIRE(words <= 0xffffffffull, "%s: a proof of %zu words (at most 2^32 - 1)", who, words);
    bind_thread(ctx);
    uint32_t head[PROOF_HEAD_MAX] = {0};
    ZKH_TRY(zkh_read(ctx, proof, head, 0, words < PROOF_HEAD_MAX ? words : PROOF_HEAD_MAX));
    ZKH_TRY(image_proof_header(who, head, words));
    const ProofShape ps = proof_shape(head);
    const uint32_t W = ps.W, D = ps.D, M = ps.M, h = ps.h;
    const size_t L = image_leaves(W), t0 = ps.table, l0 = ps.leaves;
    const unsigned long long bound = image_nodes_bound(W, D);
    if (dirty) {
        ZKH_REQUIRE(bound <= 0xffffffffull, "%s: the dirty nodes of %u rows over %u words may take %llu words (at most 2^32 - 1)", who, D, W, bound);
        ZKH_REQUIRE(dirty->len >= bound, "%s: dirty nodes of %zu words; %u rows over %u words may take %llu (zkh_image_dirty_words)", who, dirty->len, D, W, bound);
    }
    bool root_ok = true;
    for (int j = 0; j < 8; j++) root_ok = root_ok && root_before[j] < P;
    if (words == t0) {                                  // D = 0 and nothing after the header: nothing to launch
        if (!root_ok) return refuse_root_range(who);
        if (dirty) return refuse_empty_nodes(who);
        memmove(root_after, root_before, 32);
        return nullptr;
    }
    uint32_t rec[WR_WORDS] = {0};
    rec[WR_RANGE] = rec[WR_RANGE + 1] = rec[WR_IN] = rec[WR_IN + 1] = rec[WR_ROW] = rec[WR_LAYER] = NONE;
    Tmp st;
    ZKH_TRY(zkh_copy_from(ctx, "walk_record", rec, WR_WORDS, st.out()));
    const uint32_t* pw = proof->ptr();
    // the scratch: the items of any layer are at most min(D, M, L) once the leaf stage's gate has passed, and nothing runs when it has not
    size_t items0 = D < M ? D : M;
    if (L < items0) items0 = L;
    if (!items0) items0 = 1;                            // M = 0 on a table with rows: the gate stays shut, the stages still report
    const bool rows = D && root_ok;                     // a root_before that is not below P: only a word >= P is reported before it
    const uint32_t nb0 = (D + IMG_THREADS - 1) / IMG_THREADS;
    Tmp lists[2], local, sums, meta, from, sib, dig[2], kept;
    uint32_t* keep = nullptr;
    if (dirty && rows) {
        ZKH_TRY(new_buf(ctx, (size_t)bound, false, kept.out()));
        keep = kept->ptr();
    }
    {
        ProfScope prof(ctx, "walk_check", 4.0 * (words - t0) + (rows ? 12.0 * D + 8.0 * nb0 : 0.0));
        k_walk_range<<<(unsigned)((words - t0 + IMG_THREADS - 1) / IMG_THREADS), IMG_THREADS, 0, ctx->stream>>>(pw, t0, l0, words, st->ptr());
        ZKH_TRY(last_launch_error("walk_range"));
        if (rows) {
            ZKH_TRY(new_buf(ctx, D, false, local.out()));
            ZKH_TRY(new_buf(ctx, 1 + 2 * (size_t)nb0, false, sums.out()));
            k_walk_rows<<<nb0, IMG_THREADS, 0, ctx->stream>>>(pw + t0, D, W, local->ptr(), sums->ptr(), st->ptr());
            ZKH_TRY(last_launch_error("walk_rows"));
            scan_counters(ctx, sums->ptr() + 1, 1, nb0, st->ptr() + WR_COUNT, 0);
            ZKH_TRY(last_launch_error("walk_carry"));
        }
    }
    if (rows) {
        for (int i = 0; i < 2; i++) {
            ZKH_TRY(new_buf(ctx, items0, false, lists[i].out()));
            ZKH_TRY(new_buf(ctx, 16 * items0, false, dig[i].out()));
        }
        ZKH_TRY(new_buf(ctx, items0, false, from.out()));
        ZKH_TRY(new_buf(ctx, items0, false, sib.out()));
        ZKH_TRY(new_buf(ctx, WM_WORDS * ((size_t)h + 2), false, meta.out()));
        {
            ProfScope prof(ctx, "walk_leaves", 20.0 * D + 100.0 * items0);
            k_walk_leaves<<<nb0, IMG_THREADS, 0, ctx->stream>>>(pw, (uint32_t)t0, D, M, local->ptr(), sums->ptr(), st->ptr(), lists[0]->ptr(), dig[0]->ptr(), meta->ptr(), W, h,
                                                                keep);
            ZKH_TRY(last_launch_error("walk_leaves"));
        }
        int cur = 0;
        for (uint32_t k = 0; k < h; k++, cur ^= 1) {
            const size_t width = L >> k;
            const uint32_t items = (uint32_t)(items0 < width ? items0 : width), parents = (uint32_t)(items0 < width / 2 ? items0 : width / 2);
            const uint32_t nb = (items + IMG_THREADS - 1) / IMG_THREADS;
            uint32_t* mk = meta->ptr() + WM_WORDS * (size_t)k;
            {
                ProfScope prof(ctx, "walk_layer", 24.0 * items + 16.0 * nb + 12.0 * parents);
                k_proof_flags<<<nb, IMG_THREADS, 0, ctx->stream>>>(lists[cur]->ptr(), mk, local->ptr(), sums->ptr(), nb);
                ZKH_TRY(last_launch_error("walk_flags"));
                scan_counters(ctx, sums->ptr(), 2, nb, mk + WM_TAKE, 1);
                ZKH_TRY(last_launch_error("walk_carry"));
                k_walk_parents<<<nb, IMG_THREADS, 0, ctx->stream>>>(lists[cur]->ptr(), mk, local->ptr(), sums->ptr(), nb, k, pw, st->ptr(), lists[cur ^ 1]->ptr(), from->ptr(),
                                                                    sib->ptr(), (uint32_t)(width >> 1), keep);
                ZKH_TRY(last_launch_error("walk_parents"));
            }
            ZKH_TRY(hash_walk_layer(ctx, lists[cur]->ptr(), from->ptr(), sib->ptr(), mk + WM_WORDS + WM_ITEMS, pw, mk + WM_OFF, dig[cur]->ptr(), dig[cur ^ 1]->ptr(), parents, keep,
                                    mk + WM_DIRTY));
        }
        {
            ProfScope prof(ctx, "walk_top", 128.0);
            k_walk_top<<<1, 64, 0, ctx->stream>>>(pw, (uint32_t)t0, meta->ptr() + WM_WORDS * (size_t)h + WM_ITEMS, dig[cur]->ptr(), st->ptr());
            ZKH_TRY(last_launch_error("walk_top"));
        }
    }
    ZKH_TRY(zkh_read(ctx, st.b, rec, 0, WR_WORDS));
    // the causes in the host verifier's order
    if (!((rec[WR_RANGE] & rec[WR_RANGE + 1]) == NONE)) return refuse_word(who, rec[WR_RANGE + 1], rec[WR_RANGE]);
    if (!root_ok) return refuse_root_range(who);
    if (!D) return proof_empty(who, head);              // words past the header: M or a c_k is not 0
    if (rec[WR_ROW] != NONE) return refuse_row(who, rec[WR_ROW], rec[WR_ROW_A], rec[WR_ROW_BEFORE], W);
    if (rec[WR_COUNT] != M) return refuse_leaves(who, M, rec[WR_COUNT]);
    if (!((rec[WR_IN] & rec[WR_IN + 1]) == NONE)) return refuse_in(who, rec[WR_IN + 1], rec[WR_IN_IN], rec[WR_IN_A], rec[WR_IN]);
    if (rec[WR_LAYER] != NONE) return refuse_layer(who, rec[WR_LAYER], rec[WR_LAYER_C], rec[WR_LAYER_TAKE]);
    ZKH_REQUIRE(rec[WR_TOP_ITEMS] == 1, "%s: the walk ended on %u nodes (a fault of the walk, not of the proof)", who, rec[WR_TOP_ITEMS]);
    if (memcmp(rec + WR_DIGESTS, root_before, 32)) return refuse_root(who, rec + WR_DIGESTS);
    if (dirty) {
        ZKH_REQUIRE(rec[WR_DIRTY_END] <= bound, "%s: the dirty nodes ended at word %u of %llu (a fault of the walk, not of the proof)", who, rec[WR_DIRTY_END], bound);
        ProfScope prof(ctx, "walk_keep", 8.0 * rec[WR_DIRTY_END]);
        ZKH_HIP(hipMemcpyAsync(dirty->ptr(), keep, 4 * (size_t)rec[WR_DIRTY_END], hipMemcpyDeviceToDevice, ctx->stream));
    }
    memcpy(root_after, rec + WR_DIGESTS + 8, 32);
    return nullptr;
}

extern "C" const char* zkh_image_proof_walk(zkh_ctx* ctx, const zkh_buf* proof, size_t words, const uint32_t root_before[8], uint32_t root_after[8]) {
    static const char who[] = "image_proof_walk";
    ZKH_REQUIRE(ctx && proof && root_before && root_after, "%s: null argument", who);
    return proof_walk(who, ctx, proof, words, root_before, root_after, nullptr);
}

extern "C" const char* zkh_image_proof_nodes(zkh_ctx* ctx, const zkh_buf* proof, size_t words, const uint32_t root_before[8], uint32_t root_after[8], zkh_buf* dirty) {
    static const char who[] = "image_proof_nodes";
    ZKH_REQUIRE(ctx && proof && root_before && root_after && dirty, "%s: null argument", who);
    return proof_walk(who, ctx, proof, words, root_before, root_after, dirty);
}

extern "C" size_t zkh_image_dirty_words(size_t image_words, size_t pages) { return image_words ? (size_t)image_nodes_bound(image_words, pages) : 0; }
