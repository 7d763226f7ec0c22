// image.hip — the committed memory image (include/zkhal.h "THE IMAGE'S COMMITMENT"; zeth_amd/circuits/logup.py `reference_image_tree`;
// DESIGN.md §2 ARGUMENTS): a Merkle tree over the residues of an image of W raw Montgomery words, built on the device
// (zkh_image_commit) and kept current by a page-out (zkh_page_out_tree, links.hip -> image_tree_update).
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
//                  (a_i >> 4).  Flag, scan, scatter as the page scan of links.hip does: k_image_heads flags a lane whose key differs from
//                  the one before and scans the flags in its workgroup (scan.h), the sort's counter scan (sort.h scan_counters, ONE
//                  workgroup) turns the workgroups' totals into carries and leaves the count, k_image_compact writes the heads' keys at
//                  their ranks.  The count stays on the device: the grids are sized by its bound min(D, width) and lanes past it leave.
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
template <bool kTable>
__device__ __forceinline__ uint32_t parent_of(const uint32_t* __restrict__ src, uint32_t t) { return kTable ? canonical(src[t]) >> 4 : src[t] >> 1; }

// grid ceil(bound / IMG_THREADS) over the items [0, m) of the layer below, m = *count (kTable: the host's D, count = NULL): local[t] = the
// heads among the items of t's workgroup up to t (a head: its parent differs from the item before's), sums[1 + workgroup] = the
// workgroup's heads.  Workgroups past m leave a total of 0.
template <bool kTable>
__global__ __launch_bounds__(IMG_THREADS) void k_image_heads(const uint32_t* __restrict__ src, const uint32_t* __restrict__ count, uint32_t D,
                                                             uint32_t* __restrict__ local, uint32_t* __restrict__ sums) {
    __shared__ uint32_t buf[2][IMG_THREADS];
    const uint32_t m = kTable ? D : *count;
    const uint32_t t = blockIdx.x * IMG_THREADS + threadIdx.x;
    const uint32_t head = t < m && (t == 0 || parent_of<kTable>(src, t - 1) != parent_of<kTable>(src, t));
    const uint32_t incl = block_scan<IMG_THREADS>(head, buf, AddWrap());
    if (t < m) local[t] = incl;
    if (threadIdx.x == IMG_THREADS - 1) sums[1 + blockIdx.x] = incl;
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
    if (t == 0 || parent_of<kTable>(src, t - 1) != v) list[local[t] + sums[1 + blockIdx.x] - 1] = v;
}

}  // namespace

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
