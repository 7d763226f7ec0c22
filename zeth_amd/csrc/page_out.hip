// page_out.hip — the page-out of a PAGES record (ZKA1 version 7; zeth_amd/circuits/logup.py `reference_page_out`,
// `reference_page_out_proof`; DESIGN.md §2 ARGUMENTS) over the page table that the paged passes of links.hip left in the trace (its
// header has the table); nothing here reads a LINK record.  PAGE-OUT (zkh_page_out, zkh_page_out_tree): image[x(p_addr, i)] = p_out[i] on
// every active row with p_on = 1, after a check pass that refuses, with the image unchanged, the lowest row whose p_on is not 0 / 1, whose
// address is >= W or does not follow a smaller one on a row with p_on = 1: a table that repeats an address is REFUSED, so the scatter
// never writes one word twice; with `nodes` the update of the image's tree follows (image.hip).  THE PROOF (zkh_page_out_proof) only
// reads: its check pass has a fourth rule, p_in is the word the tree holds, and the ZKU1 proof is built from `nodes` (image.hip).
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
template <bool kWrite, bool kProof = false>
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
            if (kProof && ok && v == R1) ok = data[(size_t)pg->dst[PG_IN] * n + t] % P == image[a];
            if (!ok) mine = t;
            if (v == R1 && (t + 1 == A || on[t + 1] % P != R1)) *last = t;
        } else if (v == R1 && a < W) {
            image[a] = data[(size_t)pg->dst[PG_OUT] * n + t];
        }
    }
    if (!kWrite) report_bad_row(bad, 0, mine);
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
    uint32_t in, held;
    ZKH_TRY(read_cell(ctx, data, data, GROUP_DATA, g.dst[PG_IN], n, row, &in));
    ZKH_TRY(zkh_read(ctx, nodes, &held, nodes->len / 2 + a, 1));
    return make_err("%s: record %u at row %u: p_in %u at address %u, the tree holds %u%s", who, g.index, row, in, a, canonical(held), tail);
}

// What all three calls open with, in the order of their refusals: the PAGES record, the trace's shape, the image's length, the length
// of `nodes` (if given); then the record goes up, the check pass runs (proof: the one with the fourth rule, against the leaf layer of
// `nodes`), and its one read-back gives the refused row, named by page_refusal, or D.  `who` and `tail` frame every message.
struct PageOut {
    size_t n;
    uint32_t A, W, D, nb;                               // active rows; the image's words; the table's rows [0, D); the grid
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
    o->W = (uint32_t)image->len;
    o->nb = (o->A + PAGE_THREADS - 1) / PAGE_THREADS;
    bind_thread(ctx);
    BadRow bad;
    ZKH_TRY(zkh_copy_from(ctx, "pages_record", (const uint32_t*)o->g, sizeof(Pages) / 4, o->dpages.out()));
    ZKH_TRY(bad.init(ctx));
    {
        ProfScope prof(ctx, "page_out_check", (proof ? 16.0 : 8.0) * o->A);       // p_on and p_addr; the proof's: p_in and the tree's word
        if (proof) k_page_out<false, true><<<o->nb, PAGE_THREADS, 0, ctx->stream>>>(data->ptr(), o->record(), (uint32_t)o->n, o->A, nodes->ptr() + nodes->len / 2, o->W, bad.ptr(), bad.extra_ptr());
        else k_page_out<false><<<o->nb, PAGE_THREADS, 0, ctx->stream>>>(data->ptr(), o->record(), (uint32_t)o->n, o->A, image->ptr(), o->W, bad.ptr(), bad.extra_ptr());
        ZKH_TRY(last_launch_error("page_out_check"));
    }
    ZKH_TRY(bad.read(ctx));
    if (bad.found) return page_refusal(ctx, who, tail, *o->g, data, o->n, bad.lo, o->W, proof ? nodes : nullptr);
    o->D = bad.extra + 1;                               // the table passed: its rows are [0, D), and row D - 1 left its index (none: all ones, D = 0)
    ZKH_REQUIRE(o->D <= o->A, "%s: the check pass left %u pages on %u active rows", who, o->D, o->A);
    return nullptr;
}

// zkh_page_out (nodes = NULL) and zkh_page_out_tree: the opening, the scatter, and with `nodes` the tree's update over the D addresses
const char* page_out(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* data, zkh_buf* image, zkh_buf* nodes) {
    PageOut o;
    ZKH_TRY(page_out_open(ctx, "page_out", ": the image is unchanged", false, c, po2, zk_cycles, data, image, nodes, &o));
    {
        ProfScope prof(ctx, "page_out_write", 16.0 * o.A);
        k_page_out<true><<<o.nb, PAGE_THREADS, 0, ctx->stream>>>(data->ptr(), o.record(), (uint32_t)o.n, o.A, image->ptr(), o.W, nullptr, nullptr);
        ZKH_TRY(last_launch_error("page_out_write"));
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
    const size_t bound = zkh_image_proof_words(o.W, o.D);
    ZKH_REQUIRE(proof->len >= bound && bound <= 0xffffffffull, "page_out_proof: a proof buffer of %zu words; %u pages over an image of %u words take up to %zu (zkh_image_proof_words)",
                proof->len, o.D, o.W, bound);
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
