// page_tree.hip — the witness of P2-TREE (zeth_amd/circuits/p2_tree.py; include/zkhal.h "P2-TREE"; DESIGN.md §2 ARGUMENTS): a page-out
// of the committed memory image sealed by its DIRTY NODES.  B = A / 31 block slots of P2-JOIN's 31 rows, the old and the new
// permutation side by side; a block computes one node of the tree, its id is the node's heap index (image_tree.h), and parents read
// their children over the circuit's bus, wherever they lie in the trace.
//
// SOURCES BY ADDRESS ALONE (the proof: DESIGN.md, next to THE TWO-TREE SHORTCUT).  A part replaces the updates [first, first + count) of
// the table; a_f and a_l are its first and last address.  Every part reads the two trees of the WHOLE page-out.  Old side: what the
// updates [0, first) left; new side: what [0, first + count) left.  The table increases, so a memory word x is `nodes_after`'s on the
// old side when x < a_f (new side: x <= a_l), else `nodes_before`'s; nodes are aligned intervals, so a child node that does not hold
// a_f (a_l) lies wholly on one side of it and is a node of one of the two trees as it stands: `nodes_after` below, `nodes_before`
// above.  The one child per layer that holds a_f (a_l) is neither: it comes from the EDGE CHAIN, a_f's old path (a_l's new path) walked
// as h bare hash_pairs by k_tree_edges.  Every block is then independent of every other.  An empty part (the table has no row) is the
// root block over the tree as it stands.
//
// KERNELS.  k_tree_check: ONE workgroup; k_page_check's refusals over the whole table, a part that splits a pair of leaves, the part's
// node and pair counts (LDS sums, no atomics).  Every other kernel returns at once when the record holds a refusal, so no address at
// or past W ever indexes `nodes_*` and no slot past B is written.  k_tree_edges: one wave, lane 0 the old chain, lane 1 the new one.
// k_tree_words (P2-TREE-tied only): one lane per (row, word column).  k_tree_place: ONE workgroup, one lane per update, 256 at a time: the slot list (p2_tree.py slot order) by two block scans with a
// carry.  k_tree_blocks: one lane per (slot, side), the literal round loop of k_p2join_blocks.  k_tree_book: one lane per (row,
// bookkeeping column).  The tail rows are k_rows_tail's (circuit.hip, p2_rows_tail).  One writer per cell (of the record and the slot list
// too), one read-back of the record at the end.  The plan of the parts, on the host (zkh_page_tree_plan) and over the table where it
// lies (zkh_page_tree_plan_device: k_plan_costs, k_plan_scan, k_plan_walk, many workgroups), is described above those kernels.
//
// FROM THE DIRTY NODES (zkh_page_tree_witgen_nodes; zkn1.h; DESIGN.md §2 "P2-TREE from the proof alone").  The same witness without the
// two trees.  The source rule above does not change, only the fetch: a block's node is dirty, so the dirty-node table of the page-out's
// proof holds its record, both children on both sides, and "the NEW tree's" is the record's new digest, "the OLD tree's" its old one (a
// clean child has both equal).  k_tree_find: one lane per slot, ONE binary search of the layer's ids, the record's rank into `pos`; a
// miss (the table is another proof's) leaves the lowest missing id in the record (atomicMin, the one atomic of this file: which lane
// arrives first must not choose the message).  k_tree_edges_nodes: k_tree_edges over the records; it shuts the gate (TR_REFUSED) after
// a miss, so no block, bookkeeping or word cell is written.  k_tree_blocks_nodes: k_tree_blocks' inputs from the record at pos[slot],
// the rows through p2_rows.h pj_block_rows.  Every index into the table is below a count the host has checked (NodesShape, by value).
// The order of the launches is check, place, find, edges, blocks; the rest is shared with the two-tree call.
#include <vector>

#include "p2_rows.h"
#include "scan.h"
#include "zkn1.h"

using namespace zkh;

namespace {

constexpr uint32_t PT_KIND = 7, PT_WC = 41, PT_WD = 106, PT_WA = 24, PT_OUT = 18, PT_MIN_H = 2, PT_MAX_H = 27, PT_GAP_BITS = 29;
constexpr PageShape TREE = {"P2-TREE", PT_KIND, PT_WC, PT_WD, PT_WA, PT_OUT, PT_MAX_H, ""},     // p2_rows.h
                    // P2-TREE-tied (p2_tree_tied.py): P2-TREE's code group and data columns 0 .. 105 column for column, then ch[16] and wa[16]; its
                    // out is P2-TREE's 18 words ‖ base ‖ alpha ‖ beta ‖ F, of which the generator writes the 18
                    TREE_TIED = {"P2-TREE-tied", 9, PT_WC, PT_WD + 2 * 16, 48, 31, PT_MAX_H, ""};
// the shape both P2-TREE calls serve: the circuit's own kind decides
inline const PageShape& tree_shape(const zkh_circuit* c) { return c && c->kind == TREE_TIED.kind ? TREE_TIED : TREE; }
// code columns (p2_tree.py C_*)
enum : uint32_t { TC_LIN = 3, TC_FULLR, TC_PARTR, TC_LF, TC_LP, TC_IN_ROW, TC_OUT_ROW, TC_BLOCK_FIRST, TC_CARRY, TC_LAST_TOP, TC_GSEL, TC_GPOW, TC_GEND, TC_RC, TC_LAST = 40 };
// data columns (p2_tree.py D_*)
enum : uint32_t { TD_SO = 0, TD_QO = 24, TD_SN = 48, TD_QN = 72, TD_ID = 96, TD_IDL, TD_IDR, TD_LEAF, TD_UP, TD_DL, TD_DR, TD_LO, TD_GBIT, TD_GACC };
// P2-TREE-tied's word columns (p2_tree_tied.py D_CH, D_WA): 16 each, behind P2-TREE's
enum : uint32_t { TD_CH = 106, TD_WA = 122, PT_PAIR_WORDS = 16 };
// the record: k_page_check's refusal (row, its address, the one before), the row at which the part splits a pair of leaves, the part's
// nodes (saturated) and pairs, lo and hi as the trace holds them, whether anything is refused, both roots, both edge chains (h digests
// each: step t's is the node of layer t + 1)
// (TR_MISS, the dirty-node path alone: the lowest id of a block that the table does not hold)
enum : uint32_t { TR_ROW = 0, TR_A, TR_BEFORE, TR_SPLIT, TR_NODES, TR_PAIRS, TR_LO, TR_HI, TR_REFUSED, TR_MISS, TR_ROOTS = 16, TR_EDGES = 32, TR_WORDS = TR_EDGES + 16 * PT_MAX_H };
constexpr uint32_t PT_THREADS = 256;

__device__ __forceinline__ uint32_t bit_length(uint32_t x) { return 32u - (uint32_t)__clz((int)x); }   // __clz(0) = 32
// the nodes update i of the part starts: all h of its path when it is the part's first, else those below the fork from the update before
__device__ __forceinline__ uint32_t started(const uint32_t* __restrict__ table, uint32_t first, uint32_t i, uint32_t h) {
    if (i == 0) return h;
    return bit_length((table_addr(table, first + i) >> 4) ^ (table_addr(table, first + i - 1) >> 4));
}

// grid (ceil(n / 256), 41): a function of (po2, zk_cycles) alone
__global__ void k_tree_code(uint32_t* code, uint32_t n, uint32_t A, uint32_t B, const uint32_t* __restrict__ tab) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x, col = blockIdx.y;
    if (r >= n) return;
    uint32_t v = 0;
    const bool in_blocks = r < PJ_BLOCK * B;
    const uint32_t k = r % PJ_BLOCK, slot = r / PJ_BLOCK;
    const bool round_row = in_blocks && k >= 1 && k <= PJ_ROUNDS;
    switch (col) {
    case TC_IN_ROW: v = (in_blocks && k == 0) ? R1 : 0; break;
    case TC_OUT_ROW: v = (in_blocks && k == PJ_BLOCK - 1) ? R1 : 0; break;
    case TC_BLOCK_FIRST: v = (in_blocks && k == 0 && slot > 0) ? R1 : 0; break;
    case TC_CARRY: v = (in_blocks && k > 0) ? R1 : 0; break;
    case TC_LAST_TOP: v = (in_blocks && k == PJ_BLOCK - 1 && slot == B - 1) ? R1 : 0; break;
    case TC_GSEL: v = round_row ? R1 : 0; break;                       // rows 1 .. 29: the 29 gap bits
    case TC_GPOW: v = round_row ? pj_encode(1u << (k - 1)) : 0; break;
    case TC_GEND: v = (round_row && k == PT_GAP_BITS) ? R1 : 0; break;
    case TC_LAST: v = r == A - 1 ? R1 : 0; break;
    default: v = pj_code_cell(col < TC_RC ? col : PJ_RC0 + col - TC_RC, r, A, k, in_blocks, tab);    // columns 0 .. 7 are their roles
    }
    code[(size_t)col * n + r] = v;
}

// ONE workgroup over the table's D rows (stride 3, the address first): the WHOLE table, whichever part is laid out, then the part
// [first, first + count) (inside the table: the host has checked it)
__global__ __launch_bounds__(PT_THREADS) void k_tree_check(const uint32_t* __restrict__ table, uint32_t D, uint32_t W, uint32_t h, uint32_t B, uint32_t first,
                                                           uint32_t count, uint32_t* __restrict__ rec) {
    __shared__ uint32_t low[PT_THREADS], pairs[PT_THREADS];
    __shared__ unsigned long long nodes[PT_THREADS];
    const uint32_t t = threadIdx.x;
    const uint32_t bad = pj_table_scan<PT_THREADS>(table, D, W);
    unsigned long long sum = 0;
    uint32_t fresh = 0;
    for (uint32_t u = t; u < count; u += PT_THREADS) {
        const uint32_t c = started(table, first, u, h);
        sum += c;
        fresh += c != 0;
    }
    nodes[t] = sum; pairs[t] = fresh;
    const uint32_t i = pj_table_lowest<PT_THREADS>(bad, table, low, rec, [&](uint32_t t, uint32_t s) { nodes[t] += nodes[t + s]; pairs[t] += pairs[t + s]; });
    if (t == 0) {
        const uint32_t end = first + count;
        uint32_t split = PJ_NONE;
        if (end && end < D && table_addr(table, end - 1) >> 4 == table_addr(table, end) >> 4) split = end;
        if (first && first < D && table_addr(table, first - 1) >> 4 == table_addr(table, first) >> 4) split = first;
        const unsigned long long total = count ? nodes[0] : 1;          // an empty part is the root block alone
        rec[TR_SPLIT] = split;
        rec[TR_NODES] = total > 0xfffffffeull ? 0xfffffffeu : (uint32_t)total;
        rec[TR_PAIRS] = pairs[0];
        rec[TR_REFUSED] = i != PJ_NONE || split != PJ_NONE || total > B;
    }
}

// ONE wave.  Lane 0: a_f's OLD path, lane 1: a_l's NEW path, each h bare hash_pairs (as k_page_root's lane 0) whose digests go into
// the record; the tops are the part's two roots.  An empty part: both roots are digest 1 of the tree as it stands.
__global__ __launch_bounds__(64) void k_tree_edges(uint32_t h, const uint32_t* __restrict__ table, uint32_t first, uint32_t count, const uint32_t* __restrict__ nodes_before,
                                                   const uint32_t* __restrict__ nodes_after, size_t L, uint32_t* rec, const uint32_t* __restrict__ rc,
                                                   const uint32_t* __restrict__ diag) {
    const uint32_t lane = threadIdx.x;
    if (rec[TR_REFUSED]) return;
    if (count == 0) {
        if (lane < 16) rec[TR_ROOTS + lane] = nodes_after[8 + (lane & 7)];
        return;
    }
    if (lane >= 2) return;
    const uint32_t side = lane;
    const uint32_t a = table_addr(table, side ? first + count - 1 : first);      // < W <= 8 L: the record holds no refusal
    uint32_t s[CELLS];
    // the address rule written out, not p2_rows.h's pj_pair_words and pj_join_sibling: through them this one-lane kernel measured 4 to
    // 7 % slower (M24, medians of six runs: 0.342 against 0.329 ms at h = 17, 0.474 against 0.442 ms at h = 23)
    for (uint32_t t = 0; t < h; t++) {
        if (t == 0) {
            const uint32_t x0 = a & ~15u;
#pragma unroll
            for (uint32_t j = 0; j < 16; j++) {
                const bool done = side ? x0 + j <= a : x0 + j < a;
                s[j] = (done ? nodes_after : nodes_before)[8 * L + x0 + j];
            }
        } else {
            const uint32_t x = a >> (3 + t);
            const bool right = x & 1;
            const uint32_t* sib = (right ? nodes_after : nodes_before) + 8 * ((L >> t) + (x ^ 1));
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) {
                const uint32_t own = s[j], other = sib[j];
                s[j] = right ? other : own;
                s[8 + j] = right ? own : other;
            }
        }
#pragma unroll
        for (int j = RATE; j < CELLS; j++) s[j] = 0;
        poseidon2_mix_raw<0, OUT, RATE>(s, rc, diag);
#pragma unroll
        for (int j = 0; j < OUT; j++) s[j] = p2_finish(s[j]);
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) rec[TR_EDGES + 8 * (side * h + t) + j] = s[j];
    }
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) rec[TR_ROOTS + 8 * side + j] = s[j];
}

// ONE workgroup, one lane per update of the part, 256 updates at a time.  An update that opens a new pair of leaves q takes the next
// pair slot (a scan of the "new pair" flags) and writes the ids of the nodes it starts above the pair, bottom up, behind the pair slots
// (a scan of their numbers); the root is not among them: it is slot B - 1.  The record's node count has passed the check, so every
// slot written is below B - 1.  The dead slots and the root slot are written by the lanes' first loop: one writer per slot.
__global__ __launch_bounds__(PT_THREADS) void k_tree_place(uint32_t* __restrict__ ids, uint32_t B, uint32_t h, const uint32_t* __restrict__ table, uint32_t first,
                                                           uint32_t count, const uint32_t* __restrict__ rec) {
    __shared__ uint32_t buf[2][PT_THREADS];
    __shared__ uint32_t tot[2];
    const uint32_t t = threadIdx.x;
    if (rec[TR_REFUSED]) return;
    const uint32_t live = rec[TR_NODES] - 1, m = rec[TR_PAIRS], half = 1u << (h - 1);       // live slots but the root: [0, live)
    for (uint32_t s = live + t; s < B; s += PT_THREADS) ids[s] = s == B - 1 ? 1u : 0u;
    uint32_t pair_base = 0, over_base = m;
    for (uint32_t i0 = 0; i0 < count; i0 += PT_THREADS) {
        const uint32_t i = i0 + t;
        const uint32_t c = i < count ? started(table, first, i, h) : 0;
        const uint32_t above = c ? (c < h - 1 ? c : h - 1) - 1 : 0;                        // t = 1 .. min(c, h - 1) - 1
        const uint32_t p_incl = block_scan<PT_THREADS>(c ? 1u : 0u, buf, AddWrap());
        const uint32_t o_incl = block_scan<PT_THREADS>(above, buf, AddWrap());
        if (t == PT_THREADS - 1) { tot[0] = p_incl; tot[1] = o_incl; }
        __syncthreads();
        if (c) {
            const uint32_t id = half + (table_addr(table, first + i) >> 4);
            ids[pair_base + p_incl - 1] = id;
            const uint32_t at = over_base + o_incl - above;
            for (uint32_t k = 1; k <= above; k++) ids[at + k - 1] = id >> k;
        }
        pair_base += tot[0];
        over_base += tot[1];
        __syncthreads();
    }
}

// One lane per (slot, side): side 0 the old permutation, 1 the new one.  The 16 input words by the address rule at the top of this
// file, then the round loop of k_p2join_blocks (circuit.hip) on this side's columns.  A dead slot (id 0) hashes zeros.  Written out,
// not through p2_rows.h's pj_pair_words, pj_node_beside and pj_block_rows: through them this kernel measured 2 % slower on every
// row of M24 (medians of five runs: 1.341 against 1.311 ms, 1.343 against 1.321, 1.333 against 1.314, 1.341 against 1.319).
__global__ __launch_bounds__(64) void k_tree_blocks(uint32_t* __restrict__ data, uint32_t n, uint32_t h, uint32_t B, const uint32_t* __restrict__ ids,
                                                    const uint32_t* __restrict__ table, uint32_t first, uint32_t count, const uint32_t* __restrict__ nodes_before,
                                                    const uint32_t* __restrict__ nodes_after, size_t L, const uint32_t* __restrict__ rec, const uint32_t* __restrict__ tab) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * B || rec[TR_REFUSED]) return;
    const uint32_t slot = i >> 1, side = i & 1, id = ids[slot];
    const uint32_t s_col = side ? TD_SN : TD_SO, q_col = side ? TD_QN : TD_QO;
    const uint32_t* diag = tab + PJ_T * PJ_ROUNDS;
    uint32_t s[PJ_T];
    for (uint32_t j = 0; j < PJ_T; j++) s[j] = 0;
    if (id && count == 0) {                                                // the root block over the tree as it stands
        for (uint32_t j = 0; j < 16; j++) s[j] = nodes_after[16 * (size_t)id + j];
    } else if (id) {
        // the part's edge: its first address on the old side (words below it are written), its last on the new side (words up to it are)
        const uint32_t a = table_addr(table, side ? first + count - 1 : first);
        if (id >= L / 2) {                                                 // a pair block: 16 memory words
            const uint32_t x0 = (id - (uint32_t)(L / 2)) << 4;
            for (uint32_t j = 0; j < 16; j++) {
                const uint32_t x = x0 + j;
                const bool done = side ? x <= a : x < a;
                s[j] = (done ? nodes_after : nodes_before)[8 * L + x];
            }
        } else {                                                           // children 2 id, 2 id + 1: nodes of layer t >= 1
            const uint32_t t = h - bit_length(id);
            const uint32_t on_edge = a >> (3 + t);                         // the node of layer t that holds the edge address
            for (uint32_t c = 0; c < 2; c++) {
                const size_t child = 2 * (size_t)id + c;
                const uint32_t x = (uint32_t)(child - (L >> t));
                const uint32_t* src = x == on_edge ? rec + TR_EDGES + 8 * (side * h + t - 1) : (x < on_edge ? nodes_after : nodes_before) + 8 * child;
                for (uint32_t j = 0; j < 8; j++) s[8 * c + j] = src[j];
            }
        }
    }
    const size_t r0 = (size_t)PJ_BLOCK * slot;
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

// ---- the same from the dirty nodes (the header of this file, FROM THE DIRTY NODES).  count > 0: an empty table has no dirty-node table.
// The layer of the node with heap id `id` (1 <= id < L): h + 1 - bit_length(id); a pair block's is 1.

// grid ceil(B / 256), one lane per slot: the rank of the slot's id among its layer's ids into pos[slot]; a dead slot (id 0) takes 0
__global__ __launch_bounds__(PT_THREADS) void k_tree_find(const uint32_t* __restrict__ ids, uint32_t B, uint32_t h, const uint32_t* __restrict__ dirty, const NodesShape ns,
                                                          uint32_t* __restrict__ pos, uint32_t* __restrict__ rec) {
    const uint32_t slot = blockIdx.x * PT_THREADS + threadIdx.x;
    if (slot >= B || rec[TR_REFUSED]) return;
    const uint32_t id = ids[slot];
    uint32_t p = 0;
    if (id) {
        p = ns.find(dirty, h + 1 - bit_length(id), id);
        if (p == NODES_NONE) atomicMin(rec + TR_MISS, id);
    }
    pos[slot] = p;
}

// ONE wave, k_tree_edges' two chains: the node of layer t + 1 on the edge address's path is a block of the part, its record holds the
// path's child (recomputed here) beside its sibling.  All lanes stay to the end: lane 0 shuts the gate after a miss, k_tree_find's or
// (it cannot happen once every slot was found: the path's nodes are slots) one of the two chains'.
__global__ __launch_bounds__(64) void k_tree_edges_nodes(uint32_t h, const uint32_t* __restrict__ table, uint32_t first, uint32_t count, const uint32_t* __restrict__ dirty,
                                                         const NodesShape ns, size_t L, uint32_t* rec, const uint32_t* __restrict__ rc, const uint32_t* __restrict__ diag) {
    const uint32_t lane = threadIdx.x;
    if (rec[TR_REFUSED]) return;
    bool missed = rec[TR_MISS] != PJ_NONE;
    if (lane < 2 && !missed) {
        const uint32_t side = lane;
        const uint32_t a = table_addr(table, side ? first + count - 1 : first);
        uint32_t s[CELLS];
        for (uint32_t t = 0; t < h && !missed; t++) {
            const uint32_t id = (uint32_t)(L >> (t + 1)) + (a >> (4 + t));
            const uint32_t p = ns.find(dirty, t + 1, id);
            if (p == NODES_NONE) { atomicMin(rec + TR_MISS, id); missed = true; break; }
            const uint32_t* r = ns.record(dirty, t + 1, p);
            if (t == 0) {
                const uint32_t x0 = a & ~15u;
#pragma unroll
                for (uint32_t j = 0; j < 16; j++) {
                    const bool done = side ? x0 + j <= a : x0 + j < a;
                    s[j] = r[16 * (j >> 3) + (done ? 8 : 0) + (j & 7)];
                }
            } else {
                const bool right = (a >> (3 + t)) & 1;                     // a right node's sibling lies below the edge: the new digest
                const uint32_t* sib = r + (right ? 8 : 16);
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) {
                    const uint32_t own = s[j], other = sib[j];
                    s[j] = right ? other : own;
                    s[8 + j] = right ? own : other;
                }
            }
#pragma unroll
            for (int j = RATE; j < CELLS; j++) s[j] = 0;
            poseidon2_mix_raw<0, OUT, RATE>(s, rc, diag);
#pragma unroll
            for (int j = 0; j < OUT; j++) s[j] = p2_finish(s[j]);
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) rec[TR_EDGES + 8 * (side * h + t) + j] = s[j];
        }
        if (!missed) {
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) rec[TR_ROOTS + 8 * side + j] = s[j];
        }
    }
    if (__any(missed) && lane == 0) rec[TR_REFUSED] = 1;
}

// One lane per (slot, side), as k_tree_blocks; the 16 input words from the record at pos[slot]: a child below the edge address its new
// digest, one above it its old one, the one that holds it from the edge chain.  The rows are pj_block_rows' (p2_rows.h).
__global__ __launch_bounds__(64) void k_tree_blocks_nodes(uint32_t* __restrict__ data, uint32_t n, uint32_t h, uint32_t B, const uint32_t* __restrict__ ids,
                                                          const uint32_t* __restrict__ pos, const uint32_t* __restrict__ table, uint32_t first, uint32_t count,
                                                          const uint32_t* __restrict__ dirty, const NodesShape ns, const uint32_t* __restrict__ rec,
                                                          const uint32_t* __restrict__ tab) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * B || rec[TR_REFUSED]) return;
    const uint32_t slot = i >> 1, side = i & 1, id = ids[slot], half = 1u << (h - 1);
    uint32_t s[PJ_T];
    for (uint32_t j = 0; j < PJ_T; j++) s[j] = 0;
    if (id) {
        const uint32_t a = table_addr(table, side ? first + count - 1 : first);
        const uint32_t k = h + 1 - bit_length(id);
        const uint32_t* r = ns.record(dirty, k, pos[slot]);                // pos[slot] < n[k]: k_tree_find found it, or the gate is shut
        if (id >= half) {                                                  // a pair block: 16 memory words
            const uint32_t x0 = (id - half) << 4;
            for (uint32_t j = 0; j < 16; j++) {
                const uint32_t x = x0 + j;
                const bool done = side ? x <= a : x < a;
                s[j] = r[16 * (j >> 3) + (done ? 8 : 0) + (j & 7)];
            }
        } else {                                                           // children 2 id, 2 id + 1: nodes of layer t = k - 1 >= 1
            const uint32_t t = k - 1;
            const uint32_t on_edge = a >> (3 + t);
            for (uint32_t c = 0; c < 2; c++) {
                const uint32_t x = 2 * id + c - (1u << (h - t));
                const uint32_t* src = x == on_edge ? rec + TR_EDGES + 8 * (side * h + t - 1) : r + 16 * c + (x < on_edge ? 8 : 0);
                for (uint32_t j = 0; j < 8; j++) s[8 * c + j] = src[j];
            }
        }
    }
    pj_block_rows(data, n, (size_t)PJ_BLOCK * slot, side ? TD_SN : TD_SO, side ? TD_QN : TD_QO, s, tab);
}

// whether an address of the part lies in [x, y): a binary search of its `count` increasing addresses
__device__ __forceinline__ bool part_touches(const uint32_t* __restrict__ table, uint32_t first, uint32_t count, uint32_t x, uint32_t y) {
    uint32_t lo = 0, hi = count;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (table_addr(table, first + mid) < x) lo = mid + 1; else hi = mid;
    }
    return lo < count && table_addr(table, first + lo) < y;
}

// grid (ceil(31 B / 256), 10): the bookkeeping columns id .. gacc of the rows of the blocks, stores coalesced along the rows.  The lane
// of row 0 and `lo` writes out[16] into the record, the lane of the root block's last row and `lo` writes out[17] = hi (the root block
// is no pair block, and lo behind the pair blocks is one more than the last of them).  `rec` is read and written here (distinct cells).
__global__ __launch_bounds__(PT_THREADS) void k_tree_book(uint32_t* __restrict__ data, uint32_t n, uint32_t h, uint32_t B, const uint32_t* __restrict__ ids,
                                                          const uint32_t* __restrict__ table, uint32_t first, uint32_t count, uint32_t* rec) {
    const uint32_t r = blockIdx.x * PT_THREADS + threadIdx.x, col = TD_ID + blockIdx.y, rows = PJ_BLOCK * B;
    if (r >= rows || rec[TR_REFUSED]) return;
    const uint32_t k = r % PJ_BLOCK, slot = r / PJ_BLOCK, id = ids[slot], half = 1u << (h - 1), m = rec[TR_PAIRS];
    const bool leaf = id >= half;
    uint32_t v = 0;
    if (col == TD_ID) v = pj_encode(id);
    else if (col == TD_IDL) v = pj_encode(2 * id);
    else if (col == TD_IDR) v = pj_encode(2 * id + 1);
    else if (col == TD_LEAF) v = leaf ? R1 : 0;
    else if (col == TD_UP) v = id > 1 ? R1 : 0;
    else if (col == TD_DL || col == TD_DR) {
        if (id && !leaf && count) {
            const uint32_t t = h - bit_length(id);                         // the children are nodes of layer t >= 1: 2^(3 + t) words each
            const uint32_t x = (2 * id + (col == TD_DR)) - (1u << (h - t));
            v = part_touches(table, first, count, x << (3 + t), (x + 1) << (3 + t)) ? R1 : 0;
        }
    } else {
        const uint32_t base = first ? half + (table_addr(table, first - 1) >> 4) + 1 : half;
        const uint32_t lo = leaf ? (slot ? ids[slot - 1] + 1 : base) : (m ? ids[m - 1] + 1 : base);
        const uint32_t g = leaf ? id - lo : 0;
        if (col == TD_LO) {
            v = pj_encode(lo);
            if (r == 0) rec[TR_LO] = v;
            if (r == rows - 1) rec[TR_HI] = v;
        } else if (col == TD_GBIT) v = (k >= 1 && k <= PT_GAP_BITS && ((g >> (k - 1)) & 1)) ? R1 : 0;
        else v = k == 0 ? 0 : pj_encode(k <= PT_GAP_BITS ? g & ((1u << k) - 1) : g);
    }
    data[(size_t)col * n + r] = v;
}

// P2-TREE-tied only.  grid (ceil(31 B / 256), 32): the word columns ch[16] ‖ wa[16] of the rows of the blocks, stores coalesced along the
// rows, one writer per cell.  Only the input row of a pair block holds anything: wa[j] = the address 16 (id - 2^(h-1)) + j of word j,
// ch[j] = whether the part touches it.  Every other lane (30 rows in 31, and the blocks that are no pair blocks) stores its zero on a
// path of its own that never enters the binary search; which side of that branch a wave runs first is the compiler's choice, and the
// kernel is right either way.  Measured (M28): 0.11 ms for the 32 columns at po2 20.
__global__ __launch_bounds__(PT_THREADS) void k_tree_words(uint32_t* __restrict__ data, uint32_t n, uint32_t h, uint32_t B, const uint32_t* __restrict__ ids,
                                                           const uint32_t* __restrict__ table, uint32_t first, uint32_t count, const uint32_t* __restrict__ rec) {
    const uint32_t r = blockIdx.x * PT_THREADS + threadIdx.x, y = blockIdx.y, rows = PJ_BLOCK * B;
    if (r >= rows || rec[TR_REFUSED]) return;
    uint32_t* cell = data + (size_t)(TD_CH + y) * n + r;
    const uint32_t slot = r / PJ_BLOCK, half = 1u << (h - 1);
    const uint32_t id = r % PJ_BLOCK == 0 ? ids[slot] : 0;                 // only an input row asks for its block's id
    if (id < half) { *cell = 0; return; }
    const uint32_t a = ((id - half) << 4) + (y & (PT_PAIR_WORDS - 1));     // id < 2^27: below 2^31
    *cell = y >= PT_PAIR_WORDS ? pj_encode(a) : (part_touches(table, first, count, a, a + 1) ? R1 : 0);
}

// ---- THE PLAN ON THE DEVICE (zkh_page_tree_plan_device; DESIGN.md "THE PLAN AS A SCAN").  Row i costs c_i = bit_length(q_i xor q_{i-1})
// for the pair indices q = a >> 4 (c_0 = 0; 0 inside a pair), S_i = c_0 + .. + c_i, and the part that starts at row f ends before the first
// row i with S_i > S_f + B - h.  S_i = base[i / 256] + local[i]: k_plan_costs leaves the locals and every workgroup's sum, k_plan_scan
// turns the sums into the bases (base[nb] is S_{D-1}), k_plan_walk follows f.  32 bits hold every S that is read: a table that passes
// the table's rule starts every node of the tree of pairs at most once, so S_{D-1} < 2^h <= 2^27, and the sums of a table that does not
// pass are never read (they may wrap).  The record: the table's refusal in words 0 .. 2 (p2_rows.h TABLE_*), the number of parts, then
// per part written (first, count, nodes).
constexpr uint32_t PLAN_MAX_ROWS = 1u << 30;              // the words of the largest image (h = 27): no longer table can increase below W
enum : uint32_t { PL_PARTS = 3, PL_WORDS = 4, PL_PART = 3, PL_EAGER = 20 };     // PL_EAGER: the parts the first read-back brings along
struct MinOf { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; } };

// grid ceil(D / 256), one lane per row: the row's cost into the workgroup's scan (scan_heads, with costs for heads: local[i] and
// sums[workgroup]) and the workgroup's lowest refused row, PJ_NONE if it has none, into low[workgroup] (a min scan, no atomics)
__global__ __launch_bounds__(PT_THREADS) void k_plan_costs(const uint32_t* __restrict__ table, uint32_t D, uint32_t W, uint32_t* __restrict__ local,
                                                           uint32_t* __restrict__ sums, uint32_t* __restrict__ low) {
    __shared__ uint32_t buf[2][PT_THREADS];
    const uint32_t i = blockIdx.x * PT_THREADS + threadIdx.x;
    uint32_t c = 0, bad = PJ_NONE;
    if (i < D) {
        const uint32_t a = table_addr(table, i), before = i ? table_addr(table, i - 1) : 0;
        if (table_row_refused(i, a, before, W)) bad = i;
        if (i) c = bit_length((a >> 4) ^ (before >> 4));
    }
    scan_heads<PT_THREADS>(c, i, D, buf, local, sums);
    const uint32_t lowest = block_scan<PT_THREADS>(bad, buf, MinOf());
    if (threadIdx.x == PT_THREADS - 1) low[blockIdx.x] = lowest;
}

// ONE workgroup, k_sort_scan's shape (a contiguous chunk of the nb workgroups per lane): the exclusive scan of `sums` in place with
// the total behind it (sums[nb]), and the minimum of `low` riding along: the lowest refused row of the whole table into the record,
// as pj_table_lowest leaves it
__global__ __launch_bounds__(PT_THREADS) void k_plan_scan(uint32_t* __restrict__ sums, const uint32_t* __restrict__ low, uint32_t nb, const uint32_t* __restrict__ table,
                                                          uint32_t* __restrict__ rec) {
    __shared__ uint32_t buf[2][PT_THREADS];
    const uint32_t t = threadIdx.x, chunk = (nb + PT_THREADS - 1) / PT_THREADS;
    const uint32_t lo = min(t * chunk, nb), hi = min(lo + chunk, nb);
    uint32_t sum = 0, bad = PJ_NONE;
    for (uint32_t b = lo; b < hi; b++) {
        sum += sums[b];
        bad = MinOf()(bad, low[b]);
    }
    const uint32_t incl = block_scan<PT_THREADS>(sum, buf, AddWrap());
    const uint32_t lowest = block_scan<PT_THREADS>(bad, buf, MinOf());
    uint32_t run = incl - sum;
    for (uint32_t b = lo; b < hi; b++) {
        const uint32_t c = sums[b];
        sums[b] = run;
        run += c;
    }
    if (t == PT_THREADS - 1) {
        sums[nb] = incl;
        rec[TABLE_ROW] = lowest;
        rec[TABLE_A] = lowest != PJ_NONE ? table_addr(table, lowest) : 0;
        rec[TABLE_BEFORE] = lowest != PJ_NONE && lowest ? table_addr(table, lowest - 1) : 0;
    }
}

// ONE wave follows f_0 = 0, f_{k+1} = the first row i with S_i > S_{f_k} + B - h (D if there is none); the lanes search together.
// First for the workgroup that holds i, the first b with base[b + 1] > limit: 64 probes a round over [lo, hi], of which hi is known to
// pass (64-ary: two rounds for 4096 workgroups); then among that workgroup's 256 locals, four loads a lane.  S does not fall and
// limit >= S_f (B >= h), so i > f: the walk ends after at most D parts.  Lane 0 writes the parts below `slots` and, last, their number.
__global__ __launch_bounds__(64) void k_plan_walk(const uint32_t* __restrict__ local, const uint32_t* __restrict__ base, uint32_t nb, uint32_t D, uint32_t h, uint32_t B,
                                                  uint32_t slots, uint32_t* __restrict__ rec) {
    if (rec[TABLE_ROW] != PJ_NONE) return;
    const uint32_t lane = threadIdx.x, total = base[nb];
    uint32_t f = 0, k = 0;
    while (f < D) {
        const uint32_t s_f = base[f / PT_THREADS] + local[f], limit = s_f + (B - h);
        uint32_t next = D;
        if (total > limit) {
            uint32_t lo = f / PT_THREADS, hi = nb - 1;
            while (lo < hi) {
                const uint32_t step = (hi - lo) / 64 + 1, p = lo + lane * step + step - 1;      // lane 63's probe is at or past hi
                const uint32_t j = (uint32_t)__ffsll((long long)__ballot(p >= hi || base[p + 1] > limit)) - 1;
                hi = min(lo + j * step + step - 1, hi);
                lo += j * step;
            }
            const uint32_t row0 = lo * PT_THREADS, s0 = base[lo];
            uint32_t s[PT_THREADS / 64];
#pragma unroll
            for (uint32_t j = 0; j < PT_THREADS / 64; j++) {
                const uint32_t i = row0 + 64 * j + lane;
                s[j] = i < D ? s0 + local[i] : 0;                                                // 0 never passes a limit
            }
#pragma unroll
            for (uint32_t j = PT_THREADS / 64; j-- > 0;) {
                const unsigned long long over = __ballot(s[j] > limit);
                if (over) next = row0 + 64 * j + (uint32_t)__ffsll((long long)over) - 1;
            }
        }
        const uint32_t s_last = next < D ? base[(next - 1) / PT_THREADS] + local[next - 1] : total;
        if (lane == 0 && k < slots) {
            uint32_t* part = rec + PL_WORDS + PL_PART * (size_t)k;
            part[0] = f;
            part[1] = next - f;
            part[2] = h + s_last - s_f;
        }
        k++;
        f = next;
    }
    if (lane == 0) rec[PL_PARTS] = k;
}

// the image's shape -> h, B
const char* tree_image_shape(const char* who, size_t po2, size_t zk_cycles, size_t W, uint32_t* h_out, uint32_t* B_out) {
    ZKH_REQUIRE(W > 16, "%s: an image of %zu words has a single pair of leaves (W > 16: the root block is not a pair block)", who, W);
    const uint32_t h = image_height(W);
    ZKH_REQUIRE(h >= PT_MIN_H && h <= PT_MAX_H, "%s: an image of %zu words has h %u (%u .. %u: ids and gaps stay below 2^%u)", who, W, h, PT_MIN_H, PT_MAX_H, PT_GAP_BITS);
    *h_out = h;
    *B_out = (uint32_t)((((size_t)1 << po2) - zk_cycles) / PJ_BLOCK);
    ZKH_REQUIRE(*B_out >= h, "%s: no room for the h %u nodes of one path in %u block slots (po2 %zu, %zu zk_cycles)", who, h, *B_out, po2, zk_cycles);
    return nullptr;
}

}  // namespace

extern "C" const char* zkh_page_tree_code(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, zkh_buf* code) {
    const char* who = "page_tree_code";
    ZKH_REQUIRE(ctx && c && code, "%s: null argument", who);
    ZKH_TRY(page_circuit_shape(who, tree_shape(c), c, po2, zk_cycles));
    const size_t n = (size_t)1 << po2;
    ZKH_REQUIRE(code->len == (size_t)PT_WC * n, "%s: buffer shape mismatch", who);
    const uint32_t A = (uint32_t)(n - zk_cycles), B = A / PJ_BLOCK;
    Tmp tab;
    ZKH_TRY(p2_rows_tables(ctx, tab));
    ProfScope prof(ctx, "tree_code", 4.0 * PT_WC * n);
    k_tree_code<<<dim3((unsigned)((n + 255) / 256), PT_WC), 256, 0, ctx->stream>>>(code->ptr(), (uint32_t)n, A, B, tab->ptr());
    return last_launch_error("tree_code");
}

// HOST ONLY: the plan of p2_tree.parts over a host array of the table's addresses
extern "C" const char* zkh_page_tree_plan(size_t po2, size_t zk_cycles, size_t image_words, const uint32_t* addrs, size_t D, size_t* parts, size_t parts_cap,
                                          size_t* n_parts) {
    const char* who = "page_tree_plan";
    ZKH_REQUIRE((addrs || D == 0) && (parts || parts_cap == 0) && n_parts, "%s: null argument", who);
    ZKH_REQUIRE(page_po2_ok(po2, zk_cycles), "%s: po2 %zu out of range for %zu zk_cycles", who, po2, zk_cycles);
    uint32_t h, B;
    ZKH_TRY(tree_image_shape(who, po2, zk_cycles, image_words, &h, &B));
    size_t count = 0, first = 0, nodes = 0;
    auto emit = [&](size_t from, size_t to) {
        if (count < parts_cap) { parts[2 * count] = from; parts[2 * count + 1] = to - from; }
        count++;
    };
    bool any = false;
    uint32_t before = 0;
    for (size_t i = 0; i < D; i++) {
        ZKH_REQUIRE(addrs[i] < image_words && (i == 0 || addrs[i - 1] < addrs[i]), "%s: row %zu: address %u does not follow a smaller one below %zu", who, i, addrs[i],
                    image_words);
        const uint32_t q = addrs[i] >> 4;
        if (any && q == before) continue;
        uint32_t cost = any ? 32u - (uint32_t)__builtin_clz(q ^ before) : h;
        if (nodes + cost > B) { emit(first, i); first = i; nodes = 0; cost = h; }
        nodes += cost;
        before = q;
        any = true;
    }
    emit(first, D);
    *n_parts = count;
    return nullptr;
}

// The same plan over a table that lies on the device (stride 3 from word `table_at` of `table` on, as in a ZKU1 proof): three launches,
// and what comes back is the record and the parts written, never a word per row.  nodes[k]: part k's dirty nodes, under the same cap.
extern "C" const char* zkh_page_tree_plan_device(zkh_ctx* ctx, size_t po2, size_t zk_cycles, size_t image_words, const zkh_buf* table, size_t table_at, size_t D,
                                                 size_t* parts, size_t parts_cap, size_t* n_parts, uint32_t* nodes) {
    const char* who = "page_tree_plan_device";
    ZKH_REQUIRE(ctx && table && (parts || parts_cap == 0) && n_parts, "%s: null argument", who);
    ZKH_REQUIRE(page_po2_ok(po2, zk_cycles), "%s: po2 %zu out of range for %zu zk_cycles", who, po2, zk_cycles);
    uint32_t h, B;
    ZKH_TRY(tree_image_shape(who, po2, zk_cycles, image_words, &h, &B));
    ZKH_REQUIRE(table_at <= table->len && D <= (table->len - table_at) / PROOF_ROW, "%s: a table of %zu rows of %u words at word %zu does not fit a buffer of %zu words", who,
                D, PROOF_ROW, table_at, table->len);
    ZKH_REQUIRE(D <= PLAN_MAX_ROWS, "%s: a table of %zu rows (at most %u: the words of the largest image, and what keeps the sums of the costs in 32 bits)", who, D,
                PLAN_MAX_ROWS);
    if (D == 0) {                                       // the one empty part, the root block alone: nothing to launch
        if (parts_cap) { parts[0] = parts[1] = 0; if (nodes) nodes[0] = 1; }
        *n_parts = 1;
        return nullptr;
    }
    const uint32_t rows = (uint32_t)D, W = (uint32_t)image_words, nb = (rows + PT_THREADS - 1) / PT_THREADS;      // h <= 27: W <= 2^30
    const uint32_t slots = (uint32_t)(parts_cap < D ? parts_cap : D);                                              // a part has a row: at most D parts
    const uint32_t* rows_at = table->ptr() + table_at;
    bind_thread(ctx);
    Tmp local, sums, rec;
    ZKH_TRY(new_buf(ctx, rows, false, local.out()));
    ZKH_TRY(new_buf(ctx, 2 * (size_t)nb + 1, false, sums.out()));       // the nb sums, their total, then the nb lowest refused rows
    ZKH_TRY(new_buf(ctx, PL_WORDS + PL_PART * (size_t)slots, false, rec.out()));
    uint32_t* low = sums->ptr() + nb + 1;
    {
        ProfScope prof(ctx, "tree_plan_costs", 16.0 * rows + 8.0 * nb);
        k_plan_costs<<<nb, PT_THREADS, 0, ctx->stream>>>(rows_at, rows, W, local->ptr(), sums->ptr(), low);
        ZKH_TRY(last_launch_error("tree_plan_costs"));
    }
    {
        ProfScope prof(ctx, "tree_plan_scan", 12.0 * nb);
        k_plan_scan<<<1, PT_THREADS, 0, ctx->stream>>>(sums->ptr(), low, nb, rows_at, rec->ptr());
        ZKH_TRY(last_launch_error("tree_plan_scan"));
    }
    {
        ProfScope prof(ctx, "tree_plan_walk", 4.0 * PL_PART * slots);
        k_plan_walk<<<1, 64, 0, ctx->stream>>>(local->ptr(), sums->ptr(), nb, rows, h, B, slots, rec->ptr());
        ZKH_TRY(last_launch_error("tree_plan_walk"));
    }
    const uint32_t eager = slots < PL_EAGER ? slots : PL_EAGER;
    std::vector<uint32_t> r(PL_WORDS + PL_PART * (size_t)eager);
    ZKH_TRY(zkh_read(ctx, rec.b, r.data(), 0, r.size()));
    ZKH_TRY(table_refusal(who, r.data(), W));
    const uint32_t count = r[PL_PARTS], written = count < slots ? count : slots;
    if (written > eager) {                              // a long plan: the parts written, in a second read-back
        r.resize(PL_WORDS + PL_PART * (size_t)written);
        ZKH_TRY(zkh_read(ctx, rec.b, r.data() + PL_WORDS, PL_WORDS, PL_PART * (size_t)written));
    }
    for (uint32_t k = 0; k < written; k++) {
        const uint32_t* part = r.data() + PL_WORDS + PL_PART * (size_t)k;
        parts[2 * k] = part[0];
        parts[2 * k + 1] = part[1];
        if (nodes) nodes[k] = part[2];
    }
    *n_parts = count;
    return nullptr;
}

namespace {

// Both witness calls.  `dirty` null: the two trees (nodes_before, nodes_after); else the dirty-node table of the proof, and no tree.
const char* tree_witgen(const char* who, zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* proof, size_t proof_words,
                        const zkh_buf* nodes_before, const zkh_buf* nodes_after, const zkh_buf* dirty, size_t first_row, size_t count_rows, zkh_buf* data,
                        uint32_t out[18], const uint32_t* noise_key) {
    uint32_t h, B;
    PageOpen o;
    NodesShape ns;
    const PageShape& sh = tree_shape(c);
    const auto image_shape = [&](size_t W) { return tree_image_shape(who, po2, zk_cycles, W, &h, &B); };
    if (dirty) {
        ZKH_TRY(page_open_proof(who, sh, ctx, c, po2, zk_cycles, code, proof, proof_words, data, out, noise_key, image_shape, &o));
        uint32_t head[NODES_HEAD_MAX] = {0};
        ZKH_TRY(zkh_read(ctx, dirty, head, 0, dirty->len < NODES_HEAD_MAX ? dirty->len : NODES_HEAD_MAX));
        ZKH_TRY(image_nodes_header(who, head, dirty->len, &ns));
        ZKH_REQUIRE(head[NODES_W] == o.W && head[NODES_D] == o.D && head[NODES_H] == o.h, "%s: dirty nodes of %u rows over %u words (h %u), but the proof has %u rows over %u words (h %u)",
                    who, head[NODES_D], head[NODES_W], head[NODES_H], o.D, o.W, o.h);
        ZKH_REQUIRE(o.D, "%s: an empty table (D = 0) has no dirty nodes; such a page-out is sealed from the tree (zkh_page_tree_witgen)", who);
    } else {
        ZKH_TRY(page_open(who, sh, ctx, c, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, data, out, noise_key, image_shape, &o));
    }
    const size_t n = o.n, L = o.L;
    const uint32_t W = o.W, D = o.D, *table = o.table;
    const NoiseKey& nk = o.nk;
    ZKH_REQUIRE(first_row <= D && count_rows <= D - first_row && (count_rows || D == 0), "%s: the part [%zu, %zu) of a table of %u rows (an empty part only of an empty table)",
                who, first_row, first_row + count_rows, D);
    const uint32_t first = (uint32_t)first_row, count = (uint32_t)count_rows;     // 3 D words fit the proof: D < 2^31
    const uint32_t A = (uint32_t)(n - zk_cycles), rows = PJ_BLOCK * B;
    Tmp tab, rec, ids, pos;
    ZKH_TRY(p2_rows_tables(ctx, tab));
    if (dirty) {                                        // the record starts with no miss
        std::vector<uint32_t> init(TR_WORDS, 0);
        init[TR_MISS] = PJ_NONE;
        ZKH_TRY(zkh_copy_from(ctx, "tree_record", init.data(), TR_WORDS, rec.out()));
        ZKH_TRY(new_buf(ctx, B, false, pos.out()));
    } else {
        ZKH_TRY(new_buf(ctx, TR_WORDS, false, rec.out()));
    }
    ZKH_TRY(new_buf(ctx, B, false, ids.out()));
    {
        ProfScope prof(ctx, "tree_check", 12.0 * D + 12.0 * count);
        k_tree_check<<<1, PT_THREADS, 0, ctx->stream>>>(table, D, W, h, B, first, count, rec->ptr());
        ZKH_TRY(last_launch_error("tree_check"));
    }
    if (!dirty) {
        ProfScope prof(ctx, "tree_edges", 4.0 * 32 * h);
        k_tree_edges<<<1, 64, 0, ctx->stream>>>(h, table, first, count, nodes_before->ptr(), nodes_after->ptr(), L, rec->ptr(), ctx->tab.rc, ctx->tab.diag);
        ZKH_TRY(last_launch_error("tree_edges"));
    }
    {
        ProfScope prof(ctx, "tree_place", 12.0 * count + 4.0 * B);
        k_tree_place<<<1, PT_THREADS, 0, ctx->stream>>>(ids->ptr(), B, h, table, first, count, rec->ptr());
        ZKH_TRY(last_launch_error("tree_place"));
    }
    if (dirty) {
        {
            ProfScope prof(ctx, "tree_find", 8.0 * B + 4.0 * h * B);
            k_tree_find<<<(B + PT_THREADS - 1) / PT_THREADS, PT_THREADS, 0, ctx->stream>>>(ids->ptr(), B, h, dirty->ptr(), ns, pos->ptr(), rec->ptr());
            ZKH_TRY(last_launch_error("tree_find"));
        }
        {
            ProfScope prof(ctx, "tree_edges", 4.0 * 32 * h);
            k_tree_edges_nodes<<<1, 64, 0, ctx->stream>>>(h, table, first, count, dirty->ptr(), ns, L, rec->ptr(), ctx->tab.rc, ctx->tab.diag);
            ZKH_TRY(last_launch_error("tree_edges"));
        }
    }
    {
        ProfScope prof(ctx, "tree_blocks", 4.0 * 96 * rows);
        if (dirty) k_tree_blocks_nodes<<<(2 * B + 63) / 64, 64, 0, ctx->stream>>>(data->ptr(), (uint32_t)n, h, B, ids->ptr(), pos->ptr(), table, first, count, dirty->ptr(), ns,
                                                                                  rec->ptr(), tab->ptr());
        else k_tree_blocks<<<(2 * B + 63) / 64, 64, 0, ctx->stream>>>(data->ptr(), (uint32_t)n, h, B, ids->ptr(), table, first, count, nodes_before->ptr(),
                                                                      nodes_after->ptr(), L, rec->ptr(), tab->ptr());
        ZKH_TRY(last_launch_error("tree_blocks"));
    }
    {
        ProfScope prof(ctx, "tree_book", 4.0 * (PT_WD - TD_ID) * rows + 4.0 * sh.wd * (n - rows));
        k_tree_book<<<dim3((rows + PT_THREADS - 1) / PT_THREADS, PT_WD - TD_ID), PT_THREADS, 0, ctx->stream>>>(data->ptr(), (uint32_t)n, h, B, ids->ptr(), table, first,
                                                                                                               count, rec->ptr());
        ZKH_TRY(last_launch_error("tree_book"));
        if (rows < n) {
            p2_rows_tail(ctx, data, sh.wd, n, A, rows, nk);
            ZKH_TRY(last_launch_error("page_tail"));
        }
    }
    if (sh.wd > PT_WD) {                                // P2-TREE-tied: the 32 word columns
        ProfScope prof(ctx, "tree_words", 4.0 * (sh.wd - PT_WD) * rows);
        k_tree_words<<<dim3((rows + PT_THREADS - 1) / PT_THREADS, sh.wd - PT_WD), PT_THREADS, 0, ctx->stream>>>(data->ptr(), (uint32_t)n, h, B, ids->ptr(), table, first,
                                                                                                                count, rec->ptr());
        ZKH_TRY(last_launch_error("tree_words"));
    }
    uint32_t r[TR_ROOTS + 16];
    ZKH_TRY(zkh_read(ctx, rec, r, 0, TR_ROOTS + 16));
    ZKH_TRY(table_refusal(who, r, W));
    ZKH_REQUIRE(r[TR_SPLIT] == PJ_NONE, "%s: the part [%u, %u) splits a pair of leaves: rows %u and %u write the same 16 words (zkh_page_tree_plan)", who, first,
                first + count, r[TR_SPLIT] - 1, r[TR_SPLIT]);
    ZKH_REQUIRE(r[TR_NODES] <= B, "%s: the part [%u, %u) has %u%s dirty nodes, but po2 %zu leaves %u block slots (zkh_page_tree_plan)", who, first, first + count,
                r[TR_NODES], r[TR_NODES] == 0xfffffffeu ? " or more" : "", po2, B);
    if (dirty) {
        const uint32_t miss = r[TR_MISS];
        ZKH_REQUIRE(miss == PJ_NONE, "%s: node %u of layer %u is not in the dirty nodes (the table is another proof's)", who, miss, h + 1 - (32u - (uint32_t)__builtin_clz(miss | 1)));
    }
    memcpy(out, r + TR_ROOTS, 4 * 16);
    out[16] = r[TR_LO];
    out[17] = r[TR_HI];
    return nullptr;
}

}  // namespace

extern "C" const char* zkh_page_tree_witgen(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* proof,
                                            size_t proof_words, const zkh_buf* nodes_before, const zkh_buf* nodes_after, size_t first_row, size_t count_rows,
                                            zkh_buf* data, uint32_t out[18], const uint32_t* noise_key) {
    return tree_witgen("page_tree_witgen", ctx, c, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, nullptr, first_row, count_rows, data, out, noise_key);
}

extern "C" const char* zkh_page_tree_witgen_nodes(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* proof,
                                                  size_t proof_words, const zkh_buf* dirty, size_t first_row, size_t count_rows, zkh_buf* data, uint32_t out[18],
                                                  const uint32_t* noise_key) {
    const char* who = "page_tree_witgen_nodes";
    ZKH_REQUIRE(dirty, "%s: null argument", who);
    return tree_witgen(who, ctx, c, po2, zk_cycles, code, proof, proof_words, nullptr, nullptr, dirty, first_row, count_rows, data, out, noise_key);
}
