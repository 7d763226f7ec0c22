// image_tree.h — the committed memory image (include/zkhal.h "THE IMAGE'S COMMITMENT"; DESIGN.md §2 ARGUMENTS): what image.hip,
// hash.hip and page_out.hip share.  image.hip owns the leaf layer and the lists of dirty nodes, hash.hip every permutation (its build
// flags), page_out.hip the page-out that drives the update and the proof, zku1.h the proof's layout.
#pragma once
#include "common.h"

namespace zkh {

constexpr int WIDE_LOG = 15;      // tree layers with <= 2^15 parents use hash.hip's 8-lane permutation; the image update lists no such layer

// L of an image of W >= 1 words: the smallest power of two >= ceil(W / 8); the tree is 2 L digests, 16 L words
inline size_t image_leaves(size_t W) {
    size_t L = 1;
    while (L * 8 < W) L <<= 1;
    return L;
}
// h = log2 L: the hash_pairs of a path from a leaf to the root
inline uint32_t image_height(size_t W) {
    uint32_t h = 0;
    while (((size_t)1 << h) < image_leaves(W)) h++;
    return h;
}

// hash.hip: every layer above the one of `first_layer` digests (a power of two; 1: nothing), the widest with one lane per parent, the
// narrow ones with the 8-lane kernels
const char* merkle_fold_from(zkh_ctx* c, zkh_buf* nodes, size_t first_layer);
// hash.hip: the parents list[0 .. *count) of the layer of `width` parents, one lane per listed parent, nothing else of the layer touched.
// `bound` >= *count sizes the grid (the count lives on the device); every list[t] < width.  Profiler scope image_sparse.
const char* hash_fold_listed(zkh_ctx* c, zkh_buf* nodes, size_t width, const uint32_t* list, const uint32_t* count, uint32_t bound);
// hash.hip: one layer of the walk of a ZKU1 proof (image.hip, zkh_image_proof_walk): the parents [0, *count) of the layer, two lanes
// each (hash_pair of the old children, of the new ones).  Parent r's children: item from[r] of `list` with its two digests at
// cur[16 item, +16), and the item after it (sib[r] = all ones) or the clean sibling at rank sib[r] of the proof's section at word *off.
// The two digests of parent r go to next[16 r, +16).  `bound` >= *count sizes the grid.  Profiler scope walk_hash.  `keep` (or null):
// the dirty-node table (zkn1.h) whose section at word *keep_at takes, behind its *count ids, the parents' records: the children as read.
const char* hash_walk_layer(zkh_ctx* c, const uint32_t* list, const uint32_t* from, const uint32_t* sib, const uint32_t* count, const uint32_t* proof,
                            const uint32_t* off, const uint32_t* cur, uint32_t* next, uint32_t bound, uint32_t* keep, const uint32_t* keep_at);

// image.hip: after a page-out has scattered into `image`: `addrs` is the page table's address column (raw words), its rows [0, D) strictly
// increasing addresses below image->len; `nodes` becomes what zkh_image_commit writes for the new image.  D = 0: nothing is launched.
const char* image_tree_update(zkh_ctx* c, const uint32_t* addrs, uint32_t D, const zkh_buf* image, zkh_buf* nodes);

// image.hip: THE UPDATE'S PROOF (include/zkhal.h), after the proof's check pass: `addrs`, `in`, `out` are the page table's p_addr, p_in
// and p_out columns (raw words), their rows [0, D) strictly increasing addresses below `image_words`, `nodes` the tree of the image
// before the page-out (only read), `proof` at least zkh_image_proof_words(image_words, D) words.
const char* image_proof_build(zkh_ctx* c, const uint32_t* addrs, const uint32_t* in, const uint32_t* out, uint32_t D, size_t image_words, const zkh_buf* nodes,
                              zkh_buf* proof);
// The proof's layout, its header's check and its table's rule are zku1.h's.

}  // namespace zkh
