// zku1.h — the ZKU1 proof of a page-out (include/zkhal.h "THE UPDATE'S PROOF"; zeth_amd/circuits/logup.py `reference_page_out_proof`) on
// the device side: the one place that knows where a word of the proof lies.  image.hip builds, verifies and walks the proof; the
// page-out circuits (p2_rows.h, page_circuit.hip, page_tree.hip) read its header and its table.
//   word 0 the magic, then W (the image's words), D (the table's rows), M (the dirty leaves), h (the tree's height), c_0 .. c_{h-1} (the
//   clean siblings of each layer); the table, D rows of (address as an integer, residue of p_in, residue of p_out); the leaves, M
//   digests; the siblings, c_0 + .. + c_{h-1} digests, layer by layer.
#pragma once
#include "image_tree.h"

namespace zkh {

constexpr uint32_t PROOF_MAGIC = 0x5a4b5531;            // 'ZKU1'
enum : uint32_t { PROOF_W = 1, PROOF_D = 2, PROOF_M = 3, PROOF_H = 4, PROOF_HEADER = 5 };      // the header's words; c_k at PROOF_HEADER + k
constexpr uint32_t PROOF_HEAD_MAX = PROOF_HEADER + 29;  // the longest header: an h that passes is at most 29
enum : uint32_t { ROW_ADDR = 0, ROW_IN = 1, ROW_OUT = 2, PROOF_ROW = 3 };                       // a table row's words

// where the sections start (word indices), and a header read into them
__host__ __device__ __forceinline__ size_t proof_table_at(uint32_t h) { return (size_t)PROOF_HEADER + h; }
__host__ __device__ __forceinline__ size_t proof_leaves_at(uint32_t h, uint32_t D) { return proof_table_at(h) + PROOF_ROW * (size_t)D; }
struct ProofShape { uint32_t W, D, M, h; size_t table, leaves, siblings; };
inline ProofShape proof_shape(const uint32_t* head) {
    const uint32_t D = head[PROOF_D], M = head[PROOF_M], h = head[PROOF_H];
    return {head[PROOF_W], D, M, h, proof_table_at(h), proof_leaves_at(h, D), proof_leaves_at(h, D) + 8 * (size_t)M};
}
// word i >= table of a proof is a row's address (an integer: any value), not a residue (below P)
__host__ __device__ __forceinline__ bool proof_word_is_address(size_t i, size_t table, size_t leaves) { return i < leaves && (i - table) % PROOF_ROW == 0; }

// row i of a table (`table`: the proof's words from the table on): its words, its address, in, out
template <class T> __host__ __device__ __forceinline__ T* table_row(T* table, size_t i) { return table + PROOF_ROW * i; }
__host__ __device__ __forceinline__ uint32_t table_addr(const uint32_t* table, size_t i) { return table_row(table, i)[ROW_ADDR]; }
__host__ __device__ __forceinline__ uint32_t table_in(const uint32_t* table, size_t i) { return table_row(table, i)[ROW_IN]; }
__host__ __device__ __forceinline__ uint32_t table_out(const uint32_t* table, size_t i) { return table_row(table, i)[ROW_OUT]; }

// THE TABLE'S RULE: row i, with address a and `before` the address of row i - 1 (anything for row 0), is refused unless a lies below W
// and strictly above `before`; and the message of a refused row after "`who`: ", for the host verifier, the walk and the circuits alike
__host__ __device__ __forceinline__ bool table_row_refused(uint32_t i, uint32_t a, uint32_t before, uint32_t W) { return a >= W || (i && before >= a); }
static inline const char* refuse_row(const char* who, uint32_t i, uint32_t a, uint32_t before, uint32_t W) {
    if (a >= W) return make_err("%s: row %u: address %u outside the image of %u words", who, i, a, W);
    return make_err("%s: row %u: address %u does not follow a smaller one (row %u: address %u)", who, i, a, i - 1, before);
}

// The header of a ZKU1 proof against the proof's length, with the messages of zkh_image_proof_verify after "`who`: ".  `head` holds the
// proof's first min(words, PROOF_HEAD_MAX) words: enough, since the counts c_k are read only once h has been found to be W's.  After
// it proof_shape(head) holds: h is W's, and the three sections lie inside the proof, which ends where the siblings do.
inline const char* image_proof_header(const char* who, const uint32_t* head, size_t words) {
    ZKH_REQUIRE(words >= PROOF_HEADER, "%s: a proof of %zu words: the header alone has %u", who, words, PROOF_HEADER);
    ZKH_REQUIRE(head[0] == PROOF_MAGIC, "%s: bad magic 0x%08x (ZKU1 is 0x%08x)", who, head[0], PROOF_MAGIC);
    const ProofShape s = proof_shape(head);
    ZKH_REQUIRE(s.h == image_height(s.W), "%s: h %u, but an image of %u words has h %u", who, s.h, s.W, image_height(s.W));
    ZKH_REQUIRE(words >= s.table, "%s: a proof of %zu words, but the header describes at least %zu", who, words, s.table);
    unsigned long long want = s.siblings;
    for (uint32_t k = 0; k < s.h; k++) want += 8ull * head[PROOF_HEADER + k];
    ZKH_REQUIRE(words == want, "%s: a proof of %zu words, but the header describes %llu", who, words, want);
    return nullptr;
}

}  // namespace zkh
