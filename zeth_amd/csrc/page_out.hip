// page_out.hip — the page-out of a PAGES record (ZKA1 version 7; zeth_amd/circuits/logup.py `reference_page_out`,
// `reference_page_out_proof`; DESIGN.md §2 ARGUMENTS) over the page table that the paged passes of links.hip left in the trace (its
// header has the table); nothing here reads a LINK record.  PAGE-OUT (zkh_page_out, zkh_page_out_tree): image[x(p_addr, i)] = p_out[i] on
// every active row with p_on = 1, after a check pass that refuses, with the image unchanged, the lowest row whose p_on is not 0 / 1, whose
// address is >= W or does not follow a smaller one on a row with p_on = 1: a table that repeats an address is REFUSED, so the scatter
// never writes one word twice; with `nodes` the update of the image's tree follows (image.hip).  THE PROOF (zkh_page_out_proof) only
// reads: its check pass has a fourth rule, p_in is the word the tree holds, and the ZKU1 proof is built from `nodes` (image.hip).
// WIDE (ZKA1 version 10; logup.py states it once): V = 2 value words per address.  The image is flat, V W words, and the page-out sets
// image[V a_i + j] = p_out_j[i]; the proof's fourth rule is that p_in_j is the word the tree's leaf layer holds at V a_i + j ("word j" in its
// text).  THE FLAT TABLE: to image_tree_update, image_proof_build and everything behind them a wide table of D rows is the table of V D rows
// (V a_i + j, in_j, out_j), i major, j minor: strictly increasing flat addresses over a flat image.  None of that code knows V: k_page_flat
// lays the three flat columns out in temporaries (the addresses Montgomery-encoded, as p_addr is: they are read as a column of raw words)
// and hands them over.  A blob with V = 1 launches what it always launched.
#include "arguments.h"
#include "image_tree.h"

using namespace zkh;

namespace {

constexpr uint32_t PAGE_THREADS = 256;

// The two passes over the active rows of the page table: kWrite = false reduces the lowest refused row into `bad` (under 0),
// and the row with p_on = 1 that has none after it leaves its index in `last` (in a table that passes the rows with p_on = 1 are a prefix
// [0, D): that is row D - 1, one lane, a plain store; no such row: `last` keeps its all ones, D = 0);
// kWrite = true scatters p_out into the image (addresses checked distinct and inside: no word is written twice).
// kProof (zkh_page_out_proof's check pass): `image` is the LEAF LAYER of the image's tree, the residue of word a at image[a], and a row
// that passes the three rules is refused when p_in % P is not that word.
// kV = 2 (WIDE): W counts addresses, `image` is the flat image (kProof: the flat leaf layer), and every row reads or writes its two words.
template <bool kWrite, bool kProof = false, int kV = 1>
__global__ __launch_bounds__(PAGE_THREADS) void k_page_out(const uint32_t* __restrict__ data, const Pages* __restrict__ pg, uint32_t n, uint32_t A, uint32_t* image,
                                                           uint32_t W, unsigned long long* __restrict__ bad, uint32_t* __restrict__ last) {
    const uint32_t t = blockIdx.x * PAGE_THREADS + threadIdx.x;
    const uint32_t* on = data + (size_t)pg->dst[PG_ON] * n;
    const uint32_t* addrs = data + (size_t)pg->dst[PG_ADDR] * n;
    uint32_t mine = NONE;
    if (t < A) {
        const uint32_t v = on[t] % P, a = canonical(addrs[t]);
        if (!kWrite) {
            bool ok = v == 0 || v == R1;
            if (v == R1) ok = a < W && (t == 0 || (on[t - 1] % P == R1 && canonical(addrs[t - 1]) < a));
            if (kProof && ok && v == R1) ok = data[(size_t)pg->dst[PG_IN] * n + t] % P == image[(size_t)kV * a];
            if constexpr (kV == 2) { if (kProof && ok && v == R1) ok = data[(size_t)pg->dst[PG_IN + 1] * n + t] % P == image[(size_t)2 * a + 1]; }
            if (!ok) mine = t;
            if (v == R1 && (t + 1 == A || on[t + 1] % P != R1)) *last = t;
        } else if (v == R1 && a < W) {
            image[(size_t)kV * a] = data[(size_t)pg->dst[pg_out(kV)] * n + t];
            if constexpr (kV == 2) image[(size_t)2 * a + 1] = data[(size_t)pg->dst[pg_out(kV) + 1] * n + t];
        }
    }
    if (!kWrite) report_bad_row(bad, 0, mine);
}

// WIDE: the flat columns of the table's rows [0, D), one lane per row: addr[2 t + j] = Montgomery(2 a_t + j), in[2 t + j] = p_in_j[t],
// out[2 t + j] = p_out_j[t] (raw words, copies).  The check pass has passed: a_t < W, so 2 a_t + 1 < the flat image's words <= P.
__global__ __launch_bounds__(PAGE_THREADS) void k_page_flat(const uint32_t* __restrict__ data, const Pages* __restrict__ pg, uint32_t n, uint32_t D, uint32_t* __restrict__ addr,
                                                            uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * PAGE_THREADS + threadIdx.x;
    if (t >= D) return;
    const uint32_t a = canonical(data[(size_t)pg->dst[PG_ADDR] * n + t]);
#pragma unroll
    for (uint32_t j = 0; j < 2; j++) {
        addr[(size_t)2 * t + j] = fp_encode(2 * a + j).v;
        in[(size_t)2 * t + j] = data[(size_t)pg->dst[PG_IN + j] * n + t];
        out[(size_t)2 * t + j] = data[(size_t)pg->dst[pg_out(2) + j] * n + t];
    }
}

// Which rule the refused row of the page table broke, as the reference names it: `who` and `tail` frame the text.  nodes: the proof's
// check pass, whose fourth rule is that p_in is the word the tree holds.
const char* page_refusal(zkh_ctx* ctx, const char* who, const char* tail, const Pages& g, const zkh_buf* data, size_t n, uint32_t row, uint32_t W, const zkh_buf* nodes) {
    uint32_t on, a, pon = 1, pa = 0;
    ZKH_TRY(read_cell(ctx, data, data, GROUP_DATA, g.dst[PG_ON], n, row, &on));
    ZKH_TRY(read_cell(ctx, data, data, GROUP_DATA, g.dst[PG_ADDR], n, row, &a));
    if (on > 1) return make_err("%s: record %u at row %u: p_on %u, not 0 or 1%s", who, g.index, row, on, tail);
    if (a >= W) return make_err("%s: record %u at row %u: address %u outside the image of %u words%s", who, g.index, row, a, W, tail);
    if (row) {
        ZKH_TRY(read_cell(ctx, data, data, GROUP_DATA, g.dst[PG_ON], n, row - 1, &pon));
        ZKH_TRY(read_cell(ctx, data, data, GROUP_DATA, g.dst[PG_ADDR], n, row - 1, &pa));
    }
    if (!nodes || (row && (pon != 1 || pa >= a)))
        return make_err("%s: record %u at row %u: page address %u does not follow a smaller one (row %u: p_on %u, address %u)%s", who, g.index, row, a, row - 1, pon, pa,
                        tail);
    uint32_t in = 0, held = 0, j = 0;
    for (; j < g.V; j++) {                              // the lowest word that differs; "word j" only where there are two
        ZKH_TRY(read_cell(ctx, data, data, GROUP_DATA, g.dst[PG_IN + j], n, row, &in));
        ZKH_TRY(zkh_read(ctx, nodes, &held, nodes->len / 2 + (size_t)g.V * a + j, 1));
        if (in != canonical(held) || j + 1 == g.V) break;
    }
    if (g.V > 1) return make_err("%s: record %u at row %u: p_in word %u %u at address %u, the tree holds %u%s", who, g.index, row, j, in, a, canonical(held), tail);
    return make_err("%s: record %u at row %u: p_in %u at address %u, the tree holds %u%s", who, g.index, row, in, a, canonical(held), tail);
}

// What all three calls open with, in the order of their refusals: the PAGES record, the trace's shape, the image's length, the length
// of `nodes` (if given); then the record goes up, the check pass runs (proof: the one with the fourth rule, against the leaf layer of
// `nodes`), and its one read-back gives the refused row, named by page_refusal, or D.  `who` and `tail` frame every message.
struct PageOut {
    size_t n;
    uint32_t A, W, D, nb, V;                            // active rows; the image's addresses (V = 1: its words); the table's rows [0, D); the grid; the value words per address
    const Pages* g;                                     // the PAGES record, and its copy on the device
    Tmp dpages;
    const Pages* record() const { return (const Pages*)dpages->ptr(); }
    const uint32_t* column(const zkh_buf* data, int dst) const { return data->ptr() + (size_t)g->dst[dst] * n; }
};
const char* page_out_open(zkh_ctx* ctx, const char* who, const char* tail, bool proof, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* data,
                          const zkh_buf* image, const zkh_buf* nodes, PageOut* o) {
    ZKH_REQUIRE(zkh_circuit_pages(c), "%s: the circuit's arguments hold no PAGES record (ZKA1 version 7)", who);
    ZKH_TRY(trace_rows(who, c, po2, zk_cycles, nullptr, data, nullptr, &o->n, &o->A));
    ZKH_REQUIRE(image->len <= 0xffffffffull, "%s: an image of %zu words (at most 2^32 - 1)", who, image->len);
    ZKH_REQUIRE(!nodes || (image->len && nodes->len == zkh_image_tree_words(image->len)), "%s: nodes of %zu words; an image of %zu words has a tree of %zu (zkh_image_tree_words)%s",
                who, nodes ? nodes->len : 0, image->len, zkh_image_tree_words(image->len), tail);
    o->g = &c->args->pages[0];
    o->V = o->g->V;
    ZKH_REQUIRE(image->len % o->V == 0, "%s: an image of %zu words is not a whole number of addresses of %u value words%s", who, image->len, o->V, tail);
    ZKH_REQUIRE(o->V == 1 || image->len <= P, "%s: an image of %zu words of a memory of two value words per address (at most P: its flat addresses are field elements)%s", who,
                image->len, tail);
    o->W = (uint32_t)(image->len / o->V);
    o->nb = (o->A + PAGE_THREADS - 1) / PAGE_THREADS;
    bind_thread(ctx);
    BadRow bad;
    ZKH_TRY(zkh_copy_from(ctx, "pages_record", (const uint32_t*)o->g, sizeof(Pages) / 4, o->dpages.out()));
    ZKH_TRY(bad.init(ctx));
    {
        ProfScope prof(ctx, "page_out_check", (proof ? 16.0 : 8.0) * o->A);       // p_on and p_addr; the proof's: p_in and the tree's word
        if (proof && o->V == 2) k_page_out<false, true, 2><<<o->nb, PAGE_THREADS, 0, ctx->stream>>>(data->ptr(), o->record(), (uint32_t)o->n, o->A, nodes->ptr() + nodes->len / 2, o->W, bad.ptr(), bad.extra_ptr());
        else if (o->V == 2) k_page_out<false, false, 2><<<o->nb, PAGE_THREADS, 0, ctx->stream>>>(data->ptr(), o->record(), (uint32_t)o->n, o->A, image->ptr(), o->W, bad.ptr(), bad.extra_ptr());
        else if (proof) k_page_out<false, true><<<o->nb, PAGE_THREADS, 0, ctx->stream>>>(data->ptr(), o->record(), (uint32_t)o->n, o->A, nodes->ptr() + nodes->len / 2, o->W, bad.ptr(), bad.extra_ptr());
        else k_page_out<false><<<o->nb, PAGE_THREADS, 0, ctx->stream>>>(data->ptr(), o->record(), (uint32_t)o->n, o->A, image->ptr(), o->W, bad.ptr(), bad.extra_ptr());
        ZKH_TRY(last_launch_error("page_out_check"));
    }
    ZKH_TRY(bad.read(ctx));
    if (bad.found) return page_refusal(ctx, who, tail, *o->g, data, o->n, bad.lo, o->W, proof ? nodes : nullptr);
    o->D = bad.extra + 1;                               // the table passed: its rows are [0, D), and row D - 1 left its index (none: all ones, D = 0)
    ZKH_REQUIRE(o->D <= o->A, "%s: the check pass left %u pages on %u active rows", who, o->D, o->A);
    return nullptr;
}

// WIDE: the flat table of a table that passed, 2 D rows in three temporaries (this file's header), for the tree's update and the proof
struct FlatTable {
    Tmp addr, in, out;
    const char* build(zkh_ctx* ctx, const PageOut& o, const zkh_buf* data) {
        const size_t rows = std::max<size_t>((size_t)2 * o.D, 1);
        ZKH_TRY(new_buf(ctx, rows, false, addr.out()));
        ZKH_TRY(new_buf(ctx, rows, false, in.out()));
        ZKH_TRY(new_buf(ctx, rows, false, out.out()));
        if (!o.D) return nullptr;
        ProfScope prof(ctx, "page_out_flat", 44.0 * o.D);                       // p_addr, two p_in, two p_out; six flat words
        k_page_flat<<<(o.D + PAGE_THREADS - 1) / PAGE_THREADS, PAGE_THREADS, 0, ctx->stream>>>(data->ptr(), o.record(), (uint32_t)o.n, o.D, addr->ptr(), in->ptr(), out->ptr());
        return last_launch_error("page_out_flat");
    }
};

// zkh_page_out (nodes = NULL) and zkh_page_out_tree: the opening, the scatter, and with `nodes` the tree's update over the D addresses
const char* page_out(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* data, zkh_buf* image, zkh_buf* nodes) {
    PageOut o;
    ZKH_TRY(page_out_open(ctx, "page_out", ": the image is unchanged", false, c, po2, zk_cycles, data, image, nodes, &o));
    {
        ProfScope prof(ctx, "page_out_write", 16.0 * o.A);
        if (o.V == 2) k_page_out<true, false, 2><<<o.nb, PAGE_THREADS, 0, ctx->stream>>>(data->ptr(), o.record(), (uint32_t)o.n, o.A, image->ptr(), o.W, nullptr, nullptr);
        else k_page_out<true><<<o.nb, PAGE_THREADS, 0, ctx->stream>>>(data->ptr(), o.record(), (uint32_t)o.n, o.A, image->ptr(), o.W, nullptr, nullptr);
        ZKH_TRY(last_launch_error("page_out_write"));
    }
    if (nodes && o.V == 2) {                            // the tree sees the flat table: 2 D strictly increasing flat addresses
        FlatTable flat;
        ZKH_TRY(flat.build(ctx, o, data));
        return image_tree_update(ctx, flat.addr->ptr(), 2 * o.D, image, nodes);
    }
    return nodes ? image_tree_update(ctx, o.column(data, PG_ADDR), o.D, image, nodes) : nullptr;
}

}  // namespace

// the opening with the fourth rule, then the proof from `nodes`
extern "C" const char* zkh_page_out_proof(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* data, const zkh_buf* image,
                                          const zkh_buf* nodes, zkh_buf* proof) {
    ZKH_REQUIRE(ctx && c && data && image && nodes && proof, "page_out_proof: null argument");
    PageOut o;
    ZKH_TRY(page_out_open(ctx, "page_out_proof", "", true, c, po2, zk_cycles, data, image, nodes, &o));
    const size_t bound = zkh_image_proof_words(image->len, (size_t)o.V * o.D);      // WIDE: asked about the flat image and the flat table
    ZKH_REQUIRE(proof->len >= bound && bound <= 0xffffffffull, "page_out_proof: a proof buffer of %zu words; %u pages over an image of %u words take up to %zu (zkh_image_proof_words)",
                proof->len, o.D, o.W, bound);
    if (o.V == 2) {
        FlatTable flat;
        ZKH_TRY(flat.build(ctx, o, data));
        return image_proof_build(ctx, flat.addr->ptr(), flat.in->ptr(), flat.out->ptr(), 2 * o.D, image->len, nodes, proof);
    }
    return image_proof_build(ctx, o.column(data, PG_ADDR), o.column(data, PG_IN), o.column(data, PG_OUT), o.D, image->len, nodes, proof);
}

extern "C" const char* zkh_page_out(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* data, zkh_buf* image) {
    ZKH_REQUIRE(ctx && c && data && image, "page_out: null argument");
    return page_out(ctx, c, po2, zk_cycles, data, image, nullptr);
}

extern "C" const char* zkh_page_out_tree(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* data, zkh_buf* image, zkh_buf* nodes) {
    ZKH_REQUIRE(ctx && c && data && image && nodes, "page_out: null argument");
    return page_out(ctx, c, po2, zk_cycles, data, image, nodes);
}
