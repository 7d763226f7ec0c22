// zkn1.h — the DIRTY-NODE TABLE of a page-out (include/zkhal.h "THE UPDATE'S PROOF", zkh_image_proof_nodes; zeth_amd/circuits/logup.py
// `reference_page_out_nodes`): what the walk of a ZKU1 proof (zku1.h) recomputes on its way from root to root, kept.  The one place that
// knows where a word of the table lies.  image.hip and hash.hip write it (the walk's own stages), page_tree.hip reads it
// (zkh_page_tree_witgen_nodes).
//   word 0 the magic, then W (the image's words), D (the page table's rows), h (the tree's height), n_1 .. n_h (the dirty nodes of each
//   layer: layer k has L >> k nodes, layer 0 the leaves, layer h the root, so n_h = 1); then, layer by layer for k = 1 .. h, a SECTION:
//   the n_k heap ids (L >> k) + x of the layer's dirty nodes, increasing (the walk's list S_k), then n_k RECORDS of 32 words, record p
//   for id p: the four digests of the node's two children, left old ‖ left new ‖ right old ‖ right new.  A clean child has old = new
//   (the proof's sibling); the children of a node of layer 1 are leaves, eight memory words verbatim.  Sections are packed: the table
//   holds NODES_HEADER + h + 33 (n_1 + .. + n_h) words, and one search of a layer's ids gives a P2-TREE block both of its inputs on
//   both sides.
// THE BOUND.  n_k <= min(D, L >> k): a row dirties one node per layer.  zkh_image_dirty_words(W, D) = NODES_HEADER + h + 33 sum_k min(D,
// L >> k) words hold the table of any page-out of D rows, a function of (W, D) alone; at most 33 (L - 1) + h + 4 words, whatever D is.  Every
// word index is 32 bits: a table whose BOUND passes 2^32 - 1 words is refused where it would be written.
#pragma once
#include "image_tree.h"

namespace zkh {

constexpr uint32_t NODES_MAGIC = 0x5a4b4e31;            // 'ZKN1'
enum : uint32_t { NODES_W = 1, NODES_D = 2, NODES_H = 3, NODES_HEADER = 4, NODES_RECORD = 32, NODES_ITEM = NODES_RECORD + 1 };   // n_k at NODES_HEADER + k - 1
constexpr uint32_t NODES_MAX_H = 29, NODES_HEAD_MAX = NODES_HEADER + NODES_MAX_H;                // the longest header, as PROOF_HEAD_MAX
constexpr uint32_t NODES_NONE = 0xffffffffu;            // no such id in a section

inline unsigned long long image_nodes_bound(size_t W, size_t D) {
    const size_t L = image_leaves(W);
    unsigned long long items = 0;
    for (size_t w = L >> 1; w; w >>= 1) items += D < w ? D : w;
    return NODES_HEADER + image_height(W) + NODES_ITEM * items;
}

// The sections of a table whose header has passed: layer k's n[k] ids at word at[k], its records behind them (index 0 is unused).
// Passed to the kernels by value: every index they form is below a count the host has checked.
struct NodesShape {
    uint32_t n[NODES_MAX_H + 1], at[NODES_MAX_H + 1];
    // the rank of `id` among layer k's ids, NODES_NONE if it is not there: a binary search over [at[k], at[k] + n[k])
    __device__ __forceinline__ uint32_t find(const uint32_t* __restrict__ dirty, uint32_t k, uint32_t id) const {
        const uint32_t* ids = dirty + at[k];
        uint32_t lo = 0, hi = n[k];
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (ids[mid] < id) lo = mid + 1; else hi = mid;
        }
        return lo < n[k] && ids[lo] == id ? lo : NODES_NONE;
    }
    // record p < n[k] of layer k: 32 words
    __device__ __forceinline__ const uint32_t* record(const uint32_t* __restrict__ dirty, uint32_t k, uint32_t p) const {
        return dirty + at[k] + n[k] + NODES_RECORD * (size_t)p;
    }
};

// The header of a table against the length `len` of the buffer that holds it, after "`who`: ".  `head` holds its first min(len,
// NODES_HEAD_MAX) words.  After it: h is W's, every count is within its bound, and the sections of `s` lie inside the first s->at[0]
// words (the table's length), which the buffer holds.
inline const char* image_nodes_header(const char* who, const uint32_t* head, size_t len, NodesShape* s) {
    ZKH_REQUIRE(len >= NODES_HEADER, "%s: dirty nodes of %zu words: the header alone has %u", who, len, NODES_HEADER);
    ZKH_REQUIRE(head[0] == NODES_MAGIC, "%s: dirty nodes: bad magic 0x%08x (ZKN1 is 0x%08x)", who, head[0], NODES_MAGIC);
    const uint32_t W = head[NODES_W], D = head[NODES_D], h = head[NODES_H];
    ZKH_REQUIRE(W && h == image_height(W), "%s: dirty nodes: h %u, but an image of %u words has h %u", who, h, W, W ? image_height(W) : 0);
    ZKH_REQUIRE(len >= NODES_HEADER + (size_t)h, "%s: dirty nodes of %zu words, but the header alone has %u", who, len, NODES_HEADER + h);
    const size_t L = image_leaves(W);
    unsigned long long at = NODES_HEADER + h;
    *s = NodesShape{};
    for (uint32_t k = 1; k <= h; k++) {
        const uint32_t n = head[NODES_HEADER + k - 1];
        const size_t width = L >> k, cap = D < width ? D : width;
        ZKH_REQUIRE(n <= cap, "%s: dirty nodes: %u nodes on layer %u, but %u rows dirty at most %zu of its %zu", who, n, k, D, cap, width);
        s->n[k] = n;
        s->at[k] = (uint32_t)at;                        // <= the buffer's length, checked below, before any use
        at += (unsigned long long)NODES_ITEM * n;
        ZKH_REQUIRE(at <= len && at <= 0xffffffffull, "%s: dirty nodes of %zu words, but the header describes at least %llu", who, len, at);
    }
    s->at[0] = (uint32_t)at;
    return nullptr;
}

}  // namespace zkh
