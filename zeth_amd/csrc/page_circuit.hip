// page_circuit.hip — the witness of P2-PAGE (zeth_amd/circuits/p2_page.py; include/zkhal.h "P2-PAGE"; DESIGN.md §2 ARGUMENTS): a
// page-out of the committed memory image as a trace, D single-word updates applied one after the other from root_before to
// root_after, every update one Merkle path of h blocks of 31 rows, the old path and the new one side by side in every row.
//
// THE TWO-TREE SHORTCUT.  Update i opens its word under the tree as updates 0 .. i - 1 have left it, so the paths form a chain.  The
// generator does not walk that chain: it holds the tree BEFORE the page-out and the tree AFTER it, and the table's addresses strictly
// increase.  So the memory update i opens is `nodes_after` at every address below a_i and `nodes_before` from a_i on: updates before
// i wrote only below a_i, and nothing above a_i has been written yet.  A subtree that lies wholly on one side of a_i is therefore a
// node of one of the two trees as it stands:
//   leaf block : each of the 16 words of the pair of leaves comes from `nodes_after` when its address is below a_i (new side: at or
//                below a_i), else from `nodes_before`;
//   block t>=1 : the sibling is a left one (all its addresses below a_i) from `nodes_after`, or a right one from `nodes_before`;
//   the on-path digests come from the lane's own permutation chain.
// Every path is then independent of every other.  The slots D .. N - 1 are no-op updates of address 0 under the tree after the
// page-out.  The Python yardstick (p2_page.reference_page_trace) applies the updates one at a time to one tree and shares nothing
// with this.
//
// PARTS.  A table of D > N rows is sealed as a chain of parts (zkh_page_circuit_witgen_part): the part at `first` lays out the updates
// [first, first + count), count = min(N, D - first), slot s holding update first + s.  The memory an update opens is chosen by its
// ADDRESS alone, so a part reads the same two trees as the whole table would and needs no tree of its own; what it does need is the
// root its first path opens, the tree with the updates [0, first) applied.  That root is the top of the NEW path of update first - 1
// under the same shortcut: k_page_root walks it, h hash_pairs in one lane, and writes no rows.  Only the last part has slots left
// over, so a no-op still opens the tree after the whole page-out.  The root a part that is not the last leaves is the top of its slot
// N - 1's new path, which k_page_root copies out of the rows.
//
// KERNELS.  k_page_check: ONE workgroup; the lowest row of the table whose address is outside the image or does not follow a smaller
// one (an LDS minimum, no atomics), whether the code group was built for this h, and digest 1 of both trees, into a record of 24 words.
// k_page_paths: one lane per (slot, old / new) walks its h blocks, every block by pj_block_rows (p2_rows.h); it returns at once
// when the record holds a refusal, so no address at or past W ever indexes `nodes_*`.  k_page_root (parts only: first > 0, or a part
// that is not the last): the record's roots that k_page_check does not own.  k_page_book: one lane per (row, bookkeeping column);
// `cur` of slot 0 is the record's first root, of slot s > 0 it is read from the output row the path kernel wrote for slot s - 1.
// k_rows_tail (circuit.hip, p2_rows_tail): zero rows, then the blinding rows.  No atomics, every cell (of the record too) has one
// writer; one read-back fetches the record at the end.
//
// P2-PAGE-ORDERED (zeth_amd/circuits/p2_page_ordered.py; include/zkhal.h "P2-PAGE-ordered"): the same trace in a wider buffer, columns
// 0 .. 124 of the data group and 0 .. 38 of the code group written by the kernels above as they stand (every one of them strides by n,
// and the tail's width is a grid dimension), then the columns live, lo, gbit, gacc by k_page_order and gsel, gpow, gend by
// k_page_order_code.  The order the circuit constrains is the one the two-tree shortcut already relies on and k_page_check already
// refuses a table without: lo of a slot is one more than the address of the table's row before it, and the gap to it is >= 0.
#include "p2_rows.h"

using namespace zkh;

namespace {

constexpr uint32_t PG_WC = 39, PG_WD = 125, PG_OUT = 16, PG_MAX_H = 27;
// P2-PAGE-ordered (p2_page_ordered.py): three more code columns, four more data columns, out = the roots ‖ lo ‖ hi; the gap between two
// addresses is decomposed into 29 bits, which takes addr < 2^29: h <= 26
constexpr uint32_t PO_WC = 42, PO_WD = 129, PO_OUT = 18, PO_MAX_H = 26, PO_GAP_BITS = 29;
enum : uint32_t { PC_GSEL = 39, PC_GPOW = 40, PC_GEND = 41 };
enum : uint32_t { PD_LIVE = 125, PD_LO = 126, PD_GBIT = 127, PD_GACC = 128 };
// the shape of the circuit an entry point serves (p2_rows.h PageShape)
constexpr PageShape PAGE = {"P2-PAGE", 5, PG_WC, PG_WD, 4, PG_OUT, PG_MAX_H, " (the code group is an input of this generator)"},
                    ORDERED = {"P2-PAGE-ordered", 6, PO_WC, PO_WD, 4, PO_OUT, PO_MAX_H, " (the code group is an input of this generator)"},
                    // P2-PAGE-tied (p2_page_tied.py): P2-PAGE-ordered's code and data groups column for column, so both of its calls serve it; its out
                    // is those 18 words ‖ alpha ‖ beta ‖ F, of which the generator writes the 18
                    TIED = {"P2-PAGE-tied", 8, PO_WC, PO_WD, 4, 30, PO_MAX_H, " (the code group is an input of this generator)"};
// the shape the P2-PAGE-ordered calls serve: the circuit's own kind decides
inline const PageShape& ordered_shape(const zkh_circuit* c) { return c && c->kind == TIED.kind ? TIED : ORDERED; }
// code columns (p2_page.py C_*)
enum : uint32_t { PC_LIN = 3, PC_FULLR, PC_PARTR, PC_LF, PC_LP, PC_LEAF_IN, PC_NODE_IN, PC_PATH_FIRST, PC_TOP_OUT, PC_LAST_TOP, PC_CARRY, PC_POW, PC_RC };
// data columns (p2_page.py D_*)
enum : uint32_t { PD_SO = 0, PD_QO = 24, PD_SN = 48, PD_QN = 72, PD_E = 96, PD_B = 112, PD_ADDR = 113, PD_W_IN = 114, PD_W_OUT = 115, PD_ACC = 116, PD_CUR = 117 };
// the record: the lowest refused row (PJ_NONE: none), its address, the address before it, whether the code group is this h's, both roots
// (the one the trace's first path opens, the one its last path leaves); P2-PAGE-ordered: lo and hi as the trace holds them (k_page_order)
enum : uint32_t { PR_ROW = TABLE_ROW, PR_CODE_OK = 3, PR_LO = 4, PR_HI = 5, PR_ROOTS = 8, PR_WORDS = 24 };
constexpr uint32_t PG_THREADS = 256;

__global__ void k_page_code(uint32_t* code, uint32_t n, uint32_t A, uint32_t h, uint32_t N, const uint32_t* __restrict__ tab) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x, col = blockIdx.y;
    if (r >= n) return;
    uint32_t v = 0;
    const bool in_paths = r < PJ_BLOCK * h * N;
    const uint32_t k = r % PJ_BLOCK, blk = r / PJ_BLOCK, t = blk % h, s = blk / h;
    const bool top = in_paths && k == PJ_BLOCK - 1 && t == h - 1;
    switch (col) {
    case PC_LEAF_IN: v = (in_paths && k == 0 && t == 0) ? R1 : 0; break;
    case PC_NODE_IN: v = (in_paths && k == 0 && t > 0) ? R1 : 0; break;
    case PC_PATH_FIRST: v = (in_paths && k == 0 && t == 0 && s > 0) ? R1 : 0; break;
    case PC_TOP_OUT: v = top ? R1 : 0; break;
    case PC_LAST_TOP: v = (top && s == N - 1) ? R1 : 0; break;
    case PC_CARRY: v = (in_paths && (k > 0 || t > 0)) ? R1 : 0; break;
    case PC_POW: v = (in_paths && k == 0 && t > 0) ? pj_encode(1u << (3 + t)) : 0; break;
    default: v = pj_code_cell(col < PC_RC ? col : PJ_RC0 + col - PC_RC, r, A, k, in_paths, tab);     // columns 0 .. 7 are their roles
    }
    code[(size_t)col * n + r] = v;
}

// P2-PAGE-ordered's code columns gsel, gpow, gend: grid (ceil(n / 256), 3), after k_page_code has written columns 0 .. 38
__global__ void k_page_order_code(uint32_t* code, uint32_t n, uint32_t h, uint32_t N) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x, col = PC_GSEL + blockIdx.y;
    if (r >= n) return;
    const uint32_t k = r % PJ_BLOCK, t = (r / PJ_BLOCK) % h;
    const bool bits = r < PJ_BLOCK * h * N && t == 0 && k >= 1 && k <= PO_GAP_BITS;       // rows 1 .. 29 of a path's block 0
    uint32_t v = 0;
    if (col == PC_GSEL) v = bits ? R1 : 0;
    else if (col == PC_GPOW) v = bits ? pj_encode(1u << (k - 1)) : 0;
    else v = (bits && k == PO_GAP_BITS) ? R1 : 0;
    code[(size_t)col * n + r] = v;
}

// ONE workgroup over the table's D rows (stride 3, the address first): the WHOLE table, whichever part is laid out.  No kernel reads
// `nodes_*` at an address of the table before this record says that every address is below W.  The roots: digest 1 of the tree before
// when the part starts the table (first = 0), of the tree after when it ends it (D - first <= N); k_page_root owns the others.
__global__ __launch_bounds__(PG_THREADS) void k_page_check(const uint32_t* __restrict__ table, uint32_t D, uint32_t W, const uint32_t* __restrict__ code, uint32_t n,
                                                           uint32_t h, uint32_t N, uint32_t first, const uint32_t* __restrict__ nodes_before,
                                                           const uint32_t* __restrict__ nodes_after, uint32_t* __restrict__ rec) {
    __shared__ uint32_t low[PG_THREADS];
    const uint32_t t = threadIdx.x;
    pj_table_lowest<PG_THREADS>(pj_table_scan<PG_THREADS>(table, D, W), table, low, rec, [](uint32_t, uint32_t) {});
    if (t == 0) {
        // a code group of another h' has its first top_out row at 31 h' - 1 and 2^(3 + t) on the input row of its blocks t = block % h'
        const bool top = code[(size_t)PC_TOP_OUT * n + PJ_BLOCK * h - 1] == R1;
        const bool pow = h == 1 || code[(size_t)PC_POW * n + PJ_BLOCK * (h - 1)] == pj_encode(1u << (2 + h));
        rec[PR_CODE_OK] = top && pow;
    }
    if (t >= 8 && t < 16 && first == 0) rec[t] = nodes_before[t];     // digest 1 = words [8, 16)
    if (t >= 16 && t < 24 && D - first <= N) rec[t] = nodes_after[t - 8];
}

// One lane per (slot, side): side 0 the old path, 1 the new one.  Slot s holds the table's row first + s (first < D < 2^31, s < N <
// 2^26: the sum does not wrap).  The sources of its h blocks by the address rule (p2_rows.h), the rows by pj_block_rows.
__global__ __launch_bounds__(64) void k_page_paths(uint32_t* __restrict__ data, uint32_t n, uint32_t h, uint32_t N, const uint32_t* __restrict__ table, uint32_t D,
                                                   uint32_t first, const uint32_t* __restrict__ nodes_before, const uint32_t* __restrict__ nodes_after, size_t L,
                                                   const uint32_t* __restrict__ rec, const uint32_t* __restrict__ tab) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * N || rec[PR_ROW] != PJ_NONE) return;
    const uint32_t slot = i >> 1, side = i & 1;
    const bool real = first + slot < D;
    const uint32_t a = real ? table_addr(table, first + slot) : 0;   // < W <= 8 L: the record holds no refusal
    const uint32_t* open = real ? nodes_before : nodes_after;          // a no-op opens the tree after the page-out
    uint32_t s[PJ_T];
    for (uint32_t t = 0; t < h; t++) {
        if (t == 0) pj_pair_words(s, a & ~15u, a, side, open, nodes_after, L);
        else pj_join_sibling(s, t, a, open, nodes_after, L);           // the lane's own digest is in s[0, 8)
        for (uint32_t j = 16; j < PJ_T; j++) s[j] = 0;
        pj_block_rows(data, n, (size_t)PJ_BLOCK * ((size_t)slot * h + t), side ? PD_SN : PD_SO, side ? PD_QN : PD_QO, s, tab);
    }
}

// ONE wave, after k_page_paths, launched only for a part that does not start the table or does not end it: the roots of the record
// that are not digest 1 of a tree.  Lane 0, first > 0: the root BEFORE the part = the tree with the updates [0, first) applied = the
// top of the new path of update first - 1, walked as k_page_paths walks a new side but as h bare hash_pairs: no rows.  Lanes 8 .. 15, a
// part that is not the last: the root AFTER it, the output row of slot N - 1's new path.  It returns at once on a refusal, as the
// path kernel does; `rec` is read and written here (distinct cells), hence no __restrict__ on it.
__global__ __launch_bounds__(64) void k_page_root(const uint32_t* __restrict__ data, uint32_t n, uint32_t h, uint32_t N, const uint32_t* __restrict__ table, uint32_t D,
                                                  uint32_t first, const uint32_t* __restrict__ nodes_before, const uint32_t* __restrict__ nodes_after, size_t L,
                                                  uint32_t* rec, const uint32_t* __restrict__ rc, const uint32_t* __restrict__ diag) {
    const uint32_t lane = threadIdx.x;
    if (rec[PR_ROW] != PJ_NONE) return;
    if (lane >= 8 && lane < 16 && D - first > N) rec[PR_ROOTS + lane] = data[(size_t)(PD_SN + lane - 8) * n + (size_t)PJ_BLOCK * h * N - 1];
    if (lane != 0 || first == 0) return;
    const uint32_t a = table_addr(table, first - 1);                 // < W <= 8 L: the record holds no refusal
    uint32_t s[CELLS];
    for (uint32_t t = 0; t < h; t++) {
        if (t == 0) pj_pair_words(s, a & ~15u, a, true, nodes_before, nodes_after, L);
        else pj_join_sibling(s, t, a, nodes_before, nodes_after, L);
#pragma unroll
        for (int j = RATE; j < CELLS; j++) s[j] = 0;
        poseidon2_mix_raw<0, OUT, RATE>(s, rc, diag);
#pragma unroll
        for (int j = 0; j < OUT; j++) s[j] = p2_finish(s[j]);
    }
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) rec[PR_ROOTS + j] = s[j];
}

// grid (ceil(31 h N / 256), 29): the bookkeeping columns e, b, addr, w_in, w_out, acc, cur of the rows of the paths, after k_page_paths
// (and k_page_root, where it runs: `cur` of slot 0 is the record's first root)
__global__ __launch_bounds__(PG_THREADS) void k_page_book(uint32_t* __restrict__ data, uint32_t n, uint32_t h, uint32_t N, const uint32_t* __restrict__ table, uint32_t D,
                                                          uint32_t first, const uint32_t* __restrict__ nodes_after, size_t L, const uint32_t* __restrict__ rec) {
    const uint32_t r = blockIdx.x * PG_THREADS + threadIdx.x, col = PD_E + blockIdx.y;
    if (r >= PJ_BLOCK * h * N || rec[PR_ROW] != PJ_NONE) return;
    const uint32_t k = r % PJ_BLOCK, blk = r / PJ_BLOCK, t = blk % h, slot = blk / h;
    const bool real = first + slot < D;
    const size_t row = (size_t)first + slot;
    const uint32_t a = real ? table_addr(table, row) : 0;
    uint32_t v = 0;
    if (col < PD_B) v = (k == 0 && t == 0 && (a & 15) == col - PD_E) ? R1 : 0;
    else if (col == PD_B) v = (k == 0 && t > 0 && ((a >> (3 + t)) & 1)) ? R1 : 0;
    else if (col == PD_ADDR) v = pj_encode(a);
    else if (col == PD_W_IN) v = real ? table_row(table, row)[ROW_IN] : nodes_after[8 * L];
    else if (col == PD_W_OUT) v = real ? table_row(table, row)[ROW_OUT] : nodes_after[8 * L];
    else if (col == PD_ACC) v = pj_encode(a & ((1u << (4 + t)) - 1));
    else v = slot ? data[(size_t)(PD_SN + col - PD_CUR) * n + (size_t)PJ_BLOCK * h * slot - 1] : rec[PR_ROOTS + col - PD_CUR];
    data[(size_t)col * n + r] = v;
}

// P2-PAGE-ordered, grid (ceil(31 h N / 256), 4): the columns live, lo, gbit, gacc of the rows of the paths, one lane per (row, column),
// stores coalesced along the rows as k_page_book's.  The record holds no refusal here, so the table's addresses strictly increase below
// W <= 2^29: lo <= 2^29 and the gap a - lo of a live slot is in [0, 2^29).  lo of a slot is one more than the address of the table's row
// before it (a dead slot: before the table's end), 0 where there is none; a dead slot's gap counts as 0.  The lane of slot 0's first
// row and `lo` writes out[16] into the record, the lane of the last path's top row and `lo` writes out[17] = hi: one writer per cell.
// `rec` is read and written here (distinct cells), hence no __restrict__ on it.
__global__ __launch_bounds__(PG_THREADS) void k_page_order(uint32_t* __restrict__ data, uint32_t n, uint32_t h, uint32_t N, const uint32_t* __restrict__ table, uint32_t D,
                                                           uint32_t first, uint32_t* rec) {
    const uint32_t r = blockIdx.x * PG_THREADS + threadIdx.x, col = PD_LIVE + blockIdx.y, rows = PJ_BLOCK * h * N;
    if (r >= rows || rec[PR_ROW] != PJ_NONE) return;
    const uint32_t k = r % PJ_BLOCK, blk = r / PJ_BLOCK, t = blk % h, slot = blk / h;
    const size_t row = (size_t)first + slot;
    const bool live = row < D;
    const size_t before = live ? row : D;                              // the table's rows before this slot
    const uint32_t a = live ? table_addr(table, row) : 0;
    const uint32_t lo = before ? table_addr(table, before - 1) + 1 : 0;
    const uint32_t g = live ? a - lo : 0;
    const bool bits = t == 0 && k >= 1 && k <= PO_GAP_BITS;
    uint32_t v;
    if (col == PD_LIVE) v = live ? R1 : 0;
    else if (col == PD_LO) v = pj_encode(lo);
    else if (col == PD_GBIT) v = (bits && ((g >> (k - 1)) & 1)) ? R1 : 0;
    else v = bits ? pj_encode(g & ((1u << k) - 1)) : 0;
    data[(size_t)col * n + r] = v;
    if (col == PD_LO && r == 0) rec[PR_LO] = v;
    if (col == PD_LO && r == rows - 1) rec[PR_HI] = pj_encode(live ? a + 1 : lo);
}

// the image's shape, after the circuit's (p2_rows.h page_circuit_shape) -> A, h, N
const char* page_image_shape(const char* who, const PageShape& sh, size_t po2, size_t zk_cycles, size_t W, uint32_t* A_out, uint32_t* h_out, uint32_t* N_out) {
    ZKH_REQUIRE(W > 8, "%s: an image of %zu words has a single leaf (W > 8: a path is at least one hash_pair)", who, W);
    const uint32_t h = image_height(W);
    ZKH_REQUIRE(h <= PG_MAX_H, "%s: an image of %zu words has h %u; the address is rebuilt in the field, which takes h <= %u", who, W, h, PG_MAX_H);
    ZKH_REQUIRE(h <= sh.max_h, "%s: an image of %zu words has h %u; the gap between two addresses is decomposed into %u bits, which takes addresses below 2^%u: h <= %u",
                who, W, h, PO_GAP_BITS, PO_GAP_BITS, sh.max_h);
    *A_out = (uint32_t)(((size_t)1 << po2) - zk_cycles);
    *h_out = h;
    *N_out = *A_out / PJ_BLOCK / h;
    ZKH_REQUIRE(*N_out >= 1, "%s: no room for a path of h %u blocks of 31 rows in %u active rows (po2 %zu)", who, h, *A_out, po2);
    return nullptr;
}

// Both generators.  `whole`: zkh_page_circuit_witgen, the table as one trace (first = 0, D <= N or refused); else the part at `first`.
const char* page_witgen(const char* who, const PageShape& sh, bool whole, zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* proof,
                        size_t proof_words, const zkh_buf* nodes_before, const zkh_buf* nodes_after, size_t first_row, zkh_buf* data, uint32_t* out_roots,
                        const uint32_t* noise_key) {
    uint32_t A, h, N;
    PageOpen o;
    ZKH_TRY(page_open(who, sh, ctx, c, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, data, out_roots, noise_key,
                      [&](size_t W) { return page_image_shape(who, sh, po2, zk_cycles, W, &A, &h, &N); }, &o));
    const size_t n = o.n, L = o.L;
    const uint32_t W = o.W, D = o.D, *table = o.table;
    const NoiseKey& nk = o.nk;
    if (whole) ZKH_REQUIRE(D <= N, "%s: D %u updates, but h %u at po2 %zu leaves N %u path slots", who, D, h, po2, N);
    else ZKH_REQUIRE(first_row < D || (first_row == 0 && D == 0), "%s: first %zu, but the table has %u rows", who, first_row, D);
    const uint32_t first = (uint32_t)first_row;                       // < D, and 3 D words fit the proof: D < 2^31
    const bool own_roots = first || D - first > N;                    // a root of this part is not digest 1 of a tree: k_page_root
    Tmp tab, rec;
    ZKH_TRY(p2_rows_tables(ctx, tab));
    ZKH_TRY(new_buf(ctx, PR_WORDS, false, rec.out()));
    const uint32_t rows = PJ_BLOCK * h * N;
    {
        ProfScope prof(ctx, "page_check", 12.0 * D + 4.0 * PR_WORDS);
        k_page_check<<<1, PG_THREADS, 0, ctx->stream>>>(table, D, W, code->ptr(), (uint32_t)n, h, N, first, nodes_before->ptr(), nodes_after->ptr(), rec->ptr());
        ZKH_TRY(last_launch_error("page_check"));
    }
    {
        ProfScope prof(ctx, "page_paths", 4.0 * 96 * rows);
        k_page_paths<<<(2 * N + 63) / 64, 64, 0, ctx->stream>>>(data->ptr(), (uint32_t)n, h, N, table, D, first, nodes_before->ptr(), nodes_after->ptr(), L, rec->ptr(),
                                                                tab->ptr());
        ZKH_TRY(last_launch_error("page_paths"));
    }
    if (own_roots) {
        ProfScope prof(ctx, "page_root", 4.0 * 16 * h);
        k_page_root<<<1, 64, 0, ctx->stream>>>(data->ptr(), (uint32_t)n, h, N, table, D, first, nodes_before->ptr(), nodes_after->ptr(), L, rec->ptr(), ctx->tab.rc,
                                               ctx->tab.diag);
        ZKH_TRY(last_launch_error("page_root"));
    }
    {
        ProfScope prof(ctx, "page_book", 4.0 * (PG_WD - PD_E) * rows + 4.0 * sh.wd * (n - rows));
        k_page_book<<<dim3((rows + PG_THREADS - 1) / PG_THREADS, PG_WD - PD_E), PG_THREADS, 0, ctx->stream>>>(data->ptr(), (uint32_t)n, h, N, table, D, first,
                                                                                                               nodes_after->ptr(), L, rec->ptr());
        if (rows < n) p2_rows_tail(ctx, data, sh.wd, n, A, rows, nk);
        ZKH_TRY(last_launch_error("page_book"));
    }
    if (sh.wd == PO_WD) {
        ProfScope prof(ctx, "page_order", 4.0 * (PO_WD - PD_LIVE) * rows);
        k_page_order<<<dim3((rows + PG_THREADS - 1) / PG_THREADS, PO_WD - PD_LIVE), PG_THREADS, 0, ctx->stream>>>(data->ptr(), (uint32_t)n, h, N, table, D, first, rec->ptr());
        ZKH_TRY(last_launch_error("page_order"));
    }
    uint32_t r[PR_WORDS];
    ZKH_TRY(zkh_read(ctx, rec, r, 0, PR_WORDS));
    ZKH_REQUIRE(r[PR_CODE_OK], "%s: the code group was not built for h %u (zkh_page_circuit_code with this image's size)", who, h);
    ZKH_TRY(table_refusal(who, r, W));
    memcpy(out_roots, r + PR_ROOTS, 4 * PG_OUT);
    if (sh.wd == PO_WD) { out_roots[16] = r[PR_LO]; out_roots[17] = r[PR_HI]; }
    return nullptr;
}

// Both code groups: P2-PAGE's 39 columns, and behind them P2-PAGE-ordered's three
const char* page_code(const char* who, const PageShape& sh, zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, size_t image_words, zkh_buf* code) {
    ZKH_REQUIRE(ctx && c && code, "%s: null argument", who);
    ZKH_TRY(page_circuit_shape(who, sh, c, po2, zk_cycles));
    const size_t n = (size_t)1 << po2;
    ZKH_REQUIRE(code->len == (size_t)sh.wc * n, "%s: buffer shape mismatch", who);
    uint32_t A, h, N;
    ZKH_TRY(page_image_shape(who, sh, po2, zk_cycles, image_words, &A, &h, &N));
    Tmp tab;
    ZKH_TRY(p2_rows_tables(ctx, tab));
    ProfScope prof(ctx, "page_code", 4.0 * sh.wc * n);
    k_page_code<<<dim3((unsigned)((n + 255) / 256), PG_WC), 256, 0, ctx->stream>>>(code->ptr(), (uint32_t)n, A, h, N, tab->ptr());
    if (sh.wc == PO_WC) k_page_order_code<<<dim3((unsigned)((n + 255) / 256), PO_WC - PG_WC), 256, 0, ctx->stream>>>(code->ptr(), (uint32_t)n, h, N);
    return last_launch_error("page_code");
}

}  // namespace

extern "C" const char* zkh_page_circuit_code(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, size_t image_words, zkh_buf* code) {
    return page_code("page_circuit_code", PAGE, ctx, c, po2, zk_cycles, image_words, code);
}

// HOST ONLY: N of (po2, zk_cycles, an image of `image_words` words), 0 where zkh_page_circuit_code refuses the shape
extern "C" size_t zkh_page_circuit_slots(size_t po2, size_t zk_cycles, size_t image_words) {
    uint32_t A, h, N;
    return page_po2_ok(po2, zk_cycles) && !page_image_shape("page_circuit_slots", PAGE, po2, zk_cycles, image_words, &A, &h, &N) ? N : 0;
}

extern "C" const char* zkh_page_circuit_witgen(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* proof,
                                               size_t proof_words, const zkh_buf* nodes_before, const zkh_buf* nodes_after, zkh_buf* data,
                                               uint32_t out_roots[16], const uint32_t* noise_key) {
    return page_witgen("page_circuit_witgen", PAGE, true, ctx, c, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, 0, data, out_roots, noise_key);
}

extern "C" const char* zkh_page_circuit_witgen_part(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* proof,
                                                    size_t proof_words, const zkh_buf* nodes_before, const zkh_buf* nodes_after, size_t first, zkh_buf* data,
                                                    uint32_t out_roots[16], const uint32_t* noise_key) {
    return page_witgen("page_circuit_witgen_part", PAGE, false, ctx, c, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, first, data, out_roots,
                       noise_key);
}

// P2-PAGE-ordered (zeth_amd/circuits/p2_page_ordered.py): the same two calls on the wider circuit
extern "C" const char* zkh_page_ordered_code(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, size_t image_words, zkh_buf* code) {
    return page_code("page_ordered_code", ordered_shape(c), ctx, c, po2, zk_cycles, image_words, code);
}

extern "C" const char* zkh_page_ordered_witgen(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* proof,
                                               size_t proof_words, const zkh_buf* nodes_before, const zkh_buf* nodes_after, size_t first, zkh_buf* data,
                                               uint32_t out[18], const uint32_t* noise_key) {
    return page_witgen("page_ordered_witgen", ordered_shape(c), false, ctx, c, po2, zk_cycles, code, proof, proof_words, nodes_before, nodes_after, first, data, out,
                       noise_key);
}
