// p2_rows.h — the Poseidon2 permutation as TRACE ROWS (zeth_amd/circuits/p2_blocks.py, p2_join.py block_rows), and what the witness
// generators built on it share: P2-JOIN (circuit.hip k_p2join_*), P2-PAGE and P2-PAGE-ordered (page_circuit.hip k_page_*), P2-TREE
// (page_tree.hip k_tree_*).  A block is 31 rows: the input, the state before each of the 29 rounds with the cubes of that round, the
// output.  The rounds are literal (the trace needs every intermediate state).
//
// WHO SHARES WHAT.  k_page_paths writes its blocks through pj_block_rows, and k_page_code and k_tree_code take their round columns
// from pj_code_cell.  k_p2join_blocks and k_p2join_code do NOT: they keep their loop and their switch written out in circuit.hip.
// They are on the benchmarked join path, and through the shared functions they compile to other instructions than the ones that
// were measured (k_p2join_blocks: 1036 instead of 1043 at the same registers and scratch), so sharing them would be a change of the
// join's kernels that nobody has timed.  k_tree_blocks and k_tree_edges (page_tree.hip) do not either: through the functions of this
// file they measured 2 % and 4 to 7 % slower than written out (profiles/r26_page_refactor.json), so they stand as they were; whoever
// changes the block rows or the address rule changes them there too.  The page-out generators also share the address rule of the two-tree shortcut
// (page_circuit.hip's header: pj_pair_words, pj_node_beside, pj_join_sibling), the table's check (pj_table_scan, pj_table_lowest,
// table_refusal) and the opening of their entry points (page_open).  The tail rows of all three are k_rows_tail's (p2_rows_tail).
#pragma once
#include "circuit.h"
#include "zku1.h"
#include "poseidon2.h"

namespace zkh {

constexpr uint32_t PJ_T = 24, PJ_HALF = 4, PJ_RP = 21, PJ_ROUNDS = 29, PJ_BLOCK = 31;
constexpr uint32_t PJ_NONE = 0xffffffffu;                             // no row of the table is refused
__device__ __forceinline__ bool pj_is_full(uint32_t rnd) { return rnd < PJ_HALF || rnd >= PJ_HALF + PJ_RP; }
__device__ __forceinline__ uint32_t pj_encode(uint32_t x) { return mul_mod(R2, x); }    // x < P
static __device__ void pj_m_ext(uint32_t (&c)[PJ_T]) {
    uint32_t sums[4] = {0, 0, 0, 0};
    for (uint32_t b = 0; b < PJ_T; b += 4) {
        m4(c[b], c[b + 1], c[b + 2], c[b + 3]);
        for (uint32_t i = 0; i < 4; i++) sums[i] = add_mod(sums[i], c[b + i]);
    }
    for (uint32_t k = 0; k < PJ_T; k++) c[k] = add_mod(c[k], sums[k & 3]);
}

// One block from the input state `s`: the rows [r0, r0 + 31) of the columns S = [s_col, s_col + 24) and Q = [q_col, q_col + 24) of a
// data group of n rows; `s` is left holding the output.  tab = rc[24 * 29] then diag[24] (p2_rows_tables).
static __device__ __forceinline__ void pj_block_rows(uint32_t* __restrict__ data, uint32_t n, size_t r0, uint32_t s_col, uint32_t q_col, uint32_t (&s)[PJ_T],
                                                     const uint32_t* __restrict__ tab) {
    const uint32_t* diag = tab + PJ_T * PJ_ROUNDS;
    for (uint32_t j = 0; j < PJ_T; j++) { data[(size_t)(s_col + j) * n + r0] = s[j]; data[(size_t)(q_col + j) * n + r0] = 0; }
    pj_m_ext(s);
    for (uint32_t rnd = 0; rnd < PJ_ROUNDS; rnd++) {
        const size_t r = r0 + 1 + rnd;
        for (uint32_t j = 0; j < PJ_T; j++) data[(size_t)(s_col + j) * n + r] = s[j];
        if (pj_is_full(rnd)) {
            for (uint32_t j = 0; j < PJ_T; j++) {
                const uint32_t u = add_mod(s[j], tab[rnd * PJ_T + j]);
                const uint32_t q = mul_mod(mul_mod(u, u), u);
                data[(size_t)(q_col + j) * n + r] = q;
                s[j] = mul_mod(mul_mod(q, q), u);
            }
            pj_m_ext(s);
        } else {
            const uint32_t u = add_mod(s[0], tab[rnd * PJ_T]);
            const uint32_t q = mul_mod(mul_mod(u, u), u);
            data[(size_t)q_col * n + r] = q;
            for (uint32_t j = 1; j < PJ_T; j++) data[(size_t)(q_col + j) * n + r] = 0;
            const uint32_t x7 = mul_mod(mul_mod(q, q), u);
            uint32_t tot = x7;
            for (uint32_t j = 1; j < PJ_T; j++) tot = add_mod(tot, s[j]);
            s[0] = add_mod(tot, mul_mod(diag[0], x7));
            for (uint32_t j = 1; j < PJ_T; j++) s[j] = add_mod(tot, mul_mod(diag[j], s[j]));
        }
    }
    const size_t rl = r0 + PJ_BLOCK - 1;
    for (uint32_t j = 0; j < PJ_T; j++) { data[(size_t)(s_col + j) * n + rl] = s[j]; data[(size_t)(q_col + j) * n + rl] = 0; }
}

// The code columns every block circuit has, by ROLE: active, first, body, then the round selectors, in the columns 0 .. 7 of P2-PAGE
// and P2-TREE; PJ_RC0 + j is round constant j.  r: the row, k = r % 31, in_blocks: r lies in a block.
enum : uint32_t { PJ_ACTIVE = 0, PJ_FIRST, PJ_BODY, PJ_LIN, PJ_FULLR, PJ_PARTR, PJ_LF, PJ_LP, PJ_RC0 };
static __device__ __forceinline__ uint32_t pj_code_cell(uint32_t role, uint32_t r, uint32_t A, uint32_t k, bool in_blocks, const uint32_t* __restrict__ tab) {
    const bool round_row = in_blocks && k >= 1 && k <= PJ_ROUNDS;
    const bool full = round_row && pj_is_full(k - 1), part = round_row && !pj_is_full(k - 1);
    switch (role) {
    case PJ_ACTIVE: return r < A ? R1 : 0;
    case PJ_FIRST: return r == 0 ? R1 : 0;
    case PJ_BODY: return (r > 0 && r < A) ? R1 : 0;
    case PJ_LIN: return (in_blocks && k == 1) ? R1 : 0;
    case PJ_FULLR: return full ? R1 : 0;
    case PJ_PARTR: return part ? R1 : 0;
    case PJ_LF: return (in_blocks && k >= 2 && pj_is_full(k - 2)) ? R1 : 0;
    case PJ_LP: return (in_blocks && k >= 2 && !pj_is_full(k - 2)) ? R1 : 0;
    default: return (full || (part && role == PJ_RC0)) ? tab[(k - 1) * PJ_T + (role - PJ_RC0)] : 0;
    }
}

// ---- THE ADDRESS RULE of the two-tree shortcut (page_circuit.hip's header; page_tree.hip SOURCES BY ADDRESS ALONE).  Against an
// address a of the table, memory below a is `written`'s (the tree after the page-out), memory above it `open`'s: the tree before the
// page-out, or, for a no-op slot of k_page_paths, the tree after it.  with_a: a's own word counts as written (a new side).
// L = the tree's leaves; the words of layer t's node x are at 8 ((L >> t) + x), the leaf layer is the memory itself at [8 L, 16 L).

// the 16 words of the pair of leaves at x0 (a multiple of 16; all below 8 L: L >= 2)
static __device__ __forceinline__ void pj_pair_words(uint32_t* s, uint32_t x0, uint32_t a, bool with_a, const uint32_t* open, const uint32_t* written, size_t L) {
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
        const uint32_t x = x0 + j;
        const bool done = with_a ? x <= a : x < a;
        s[j] = (done ? written : open)[8 * L + x];
    }
}
// node x of layer t >= 1, for an x that does not hold a: it lies wholly below a (`below`) or wholly above it
static __device__ __forceinline__ const uint32_t* pj_node_beside(uint32_t x, uint32_t t, bool below, const uint32_t* open, const uint32_t* written, size_t L) {
    return (below ? written : open) + 8 * ((L >> t) + x);
}
// the input of block t >= 1 of a's path: the digest in s[0, 8), the on-path node of layer t, beside its sibling (a right node's
// sibling lies below a)
static __device__ __forceinline__ void pj_join_sibling(uint32_t* s, uint32_t t, uint32_t a, const uint32_t* open, const uint32_t* written, size_t L) {
    const uint32_t x = a >> (3 + t);
    const bool right = x & 1;
    const uint32_t* sib = pj_node_beside(x ^ 1, t, right, open, written, L);
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        const uint32_t own = s[j], other = sib[j];
        s[j] = right ? other : own;
        s[8 + j] = right ? own : other;
    }
}
// NOT shared: the walk of one path as h bare hash_pairs (k_page_root lane 0, k_tree_edges lanes 0 and 1).  As one function that also
// stored every layer's digest, k_tree_edges measured 4 to 7 % slower than the parent's (M24: 0.342 against 0.329 ms at h = 17, 0.474
// against 0.442 ms at h = 23), so it keeps the rule written out; k_page_root walks with the two helpers above.  pj_node_beside has
// pj_join_sibling as its one caller since k_tree_blocks went back to its own text.

// ---- THE TABLE'S CHECK.  Block-wide, THREADS lanes: the lowest row of the table's D rows that the table's rule refuses (zku1.h
// table_row_refused: an address outside the image of W words, or one that does not follow a smaller one), PJ_NONE if there is none.  In two steps, so that a kernel can read
// the table for sums of its own in between (k_tree_check: what it reads last is what the next kernel finds in the cache).
// pj_table_scan: the lowest such row among the lane's own, i = lane, lane + THREADS, ...
template <uint32_t THREADS>
static __device__ __forceinline__ uint32_t pj_table_scan(const uint32_t* __restrict__ table, uint32_t D, uint32_t W) {
    uint32_t bad = PJ_NONE;
    for (uint32_t i = threadIdx.x; i < D && bad == PJ_NONE; i += THREADS) {
        if (table_row_refused(i, table_addr(table, i), i ? table_addr(table, i - 1) : 0, W)) bad = i;
    }
    return bad;
}
// pj_table_lowest: the lowest of the lanes' rows `bad` (an LDS minimum over `low`, no atomics).  Lane 0 writes it into rec[0] with its
// address (rec[1]) and the address before it (rec[2]); every lane returns it.  also(t, s): the caller's own LDS sums, stored before
// the call, ride the same reduction: cell t takes in cell t + s.
enum : uint32_t { TABLE_ROW = 0, TABLE_A = 1, TABLE_BEFORE = 2 };
template <uint32_t THREADS, class Also>
static __device__ __forceinline__ uint32_t pj_table_lowest(uint32_t bad, const uint32_t* __restrict__ table, uint32_t (&low)[THREADS], uint32_t* __restrict__ rec, Also also) {
    const uint32_t t = threadIdx.x;
    low[t] = bad;
    __syncthreads();
    for (uint32_t s = THREADS / 2; s; s >>= 1) {
        if (t < s) {
            low[t] = low[t] < low[t + s] ? low[t] : low[t + s];
            also(t, s);
        }
        __syncthreads();
    }
    const uint32_t i = low[0];
    if (t == 0) {
        rec[TABLE_ROW] = i;
        rec[TABLE_A] = i != PJ_NONE ? table_addr(table, i) : 0;
        rec[TABLE_BEFORE] = i != PJ_NONE && i ? table_addr(table, i - 1) : 0;
    }
    return i;
}
// HOST: the refusal the record's words 0 .. 2 stand for, after "`who`: "; nullptr if no row is refused
inline const char* table_refusal(const char* who, const uint32_t* r, uint32_t W) {
    return r[TABLE_ROW] == PJ_NONE ? nullptr : refuse_row(who, r[TABLE_ROW], r[TABLE_A], r[TABLE_BEFORE], W);
}

// ---- HOST: what the entry points share
// circuit.hip: the SHIPPED round constants and diagonal as Montgomery words on the device, rc[24 * 29] then diag[24]: the `tab` of every generator
const char* p2_rows_tables(zkh_ctx* ctx, Tmp& tab);
// circuit.hip: launches k_rows_tail over the rows [first_row, n) of the `wd` columns of a data group: zero while active, blinding noise
// after.  The rows past the last block of every generator; the caller asks for the launch error.
void p2_rows_tail(zkh_ctx* ctx, zkh_buf* data, uint32_t wd, size_t n, uint32_t A, uint32_t first_row, const NoiseKey& nk);

inline bool page_po2_ok(size_t po2, size_t zk_cycles) { return po2 >= 1 && po2 <= 30 && ((size_t)1 << po2) > zk_cycles + 1; }
// the shape of the circuit an entry point serves; `buffers`: what its witness call adds to "buffer shape mismatch"
struct PageShape { const char* name; uint32_t kind, wc, wd, wa, out, max_h; const char* buffers; };
inline const char* page_circuit_shape(const char* who, const PageShape& sh, const zkh_circuit* c, size_t po2, size_t zk_cycles) {
    ZKH_REQUIRE(c->kind == sh.kind && c->group_size[GROUP_CODE] == sh.wc && c->group_size[GROUP_DATA] == sh.wd && c->group_size[GROUP_ACCUM] == sh.wa &&
                c->global_size[GLOBAL_OUT] == sh.out, "%s: the circuit does not have %s's shape (kind %u, %u / %u / %u columns, %u outputs)", who, sh.name, sh.kind,
                sh.wc, sh.wd, sh.wa, sh.out);
    ZKH_REQUIRE(page_po2_ok(po2, zk_cycles), "%s: po2 %zu out of range for %zu zk_cycles", who, po2, zk_cycles);
    return nullptr;
}
// What a witness call of a page-out circuit opens with, in the order of its refusals: null arguments, the circuit's shape, the
// buffers', the proof's head (read back: one small copy), the image's shape by `image_shape(W)` (the circuit's own refusals), the
// trees' length.  Nothing is launched or written.  -> n rows, the image's W words, h and L leaves, the table (3 D words inside the
// proof: its length is what the header describes), the noise key.
// page_open_proof is all of it but the trees: what a call that reads no tree opens with (zkh_page_tree_witgen_nodes).
struct PageOpen { size_t n, L; uint32_t W, D, h; const uint32_t* table; NoiseKey nk; };
template <class ImageShape>
const char* page_open_proof(const char* who, const PageShape& sh, zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code,
                            const zkh_buf* proof, size_t proof_words, const zkh_buf* data, const uint32_t* out, const uint32_t* noise_key, ImageShape image_shape,
                            PageOpen* o) {
    ZKH_REQUIRE(ctx && c && code && proof && data && out, "%s: null argument", who);
    ZKH_TRY(page_circuit_shape(who, sh, c, po2, zk_cycles));
    o->n = (size_t)1 << po2;
    ZKH_REQUIRE(code->len == (size_t)sh.wc * o->n && data->len == (size_t)sh.wd * o->n, "%s: buffer shape mismatch%s", who, sh.buffers);
    ZKH_REQUIRE(proof_words <= proof->len && proof_words <= 0xffffffffull, "%s: a proof of %zu words in a buffer of %zu", who, proof_words, proof->len);
    ZKH_TRY(resolve_noise_key(noise_key, &o->nk));
    bind_thread(ctx);
    uint32_t head[PROOF_HEAD_MAX] = {0};
    ZKH_TRY(zkh_read(ctx, proof, head, 0, proof_words < PROOF_HEAD_MAX ? proof_words : PROOF_HEAD_MAX));
    ZKH_TRY(image_proof_header(who, head, proof_words));
    const ProofShape ps = proof_shape(head);
    o->W = ps.W;
    o->D = ps.D;
    ZKH_TRY(image_shape(o->W));
    o->h = ps.h;                                        // the header passed: h is W's
    o->L = image_leaves(o->W);
    o->table = proof->ptr() + ps.table;
    return nullptr;
}
template <class ImageShape>
const char* page_open(const char* who, const PageShape& sh, zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* proof,
                      size_t proof_words, const zkh_buf* nodes_before, const zkh_buf* nodes_after, const zkh_buf* data, const uint32_t* out, const uint32_t* noise_key,
                      ImageShape image_shape, PageOpen* o) {
    ZKH_REQUIRE(ctx && c && code && proof && nodes_before && nodes_after && data && out, "%s: null argument", who);
    ZKH_TRY(page_open_proof(who, sh, ctx, c, po2, zk_cycles, code, proof, proof_words, data, out, noise_key, image_shape, o));
    ZKH_REQUIRE(nodes_before->len == 16 * o->L && nodes_after->len == 16 * o->L, "%s: nodes of %zu and %zu words; an image of %u words has a tree of %zu (zkh_image_tree_words)",
                who, nodes_before->len, nodes_after->len, o->W, 16 * o->L);
    return nullptr;
}

}  // namespace zkh
