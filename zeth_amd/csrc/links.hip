// links.hip — LINK records (ZKA1 version 5; zeth_amd/circuits/logup.py `reference_links`; DESIGN.md §2 ARGUMENTS): every memory access
// gets the previous access to its own address, on the device; and (version 6) a load is checked to return the last store.
//
// x(c, r) = the canonical value of the raw Montgomery word of column c at row r (raw words >= P are legal).  A row r < A is an ACCESS
// of a record when its selector is 1 (no selector: every active row).  For an access r with key K = x(key, r), r' = the greatest
// access below r with key K:
//   linked[r] = Montgomery([r' exists]);   last[r] = Montgomery([no access above r has key K]);
//   prev_j[r] = the raw word of carried column c_j at r' (a copy), 0 when r is not linked;
//   limb_j[r] = Montgomery(limb j of d = x(c_0, r) - x(c_0, r') - 1), 0 when r is not linked; refused when d < 0 ("clock not increasing")
//               or d >= 2^(L nl).
// Active rows that are no access get zeros in every destination; rows [A, n) are never touched.
//
// THE READ RULE (a record with READS, ZKA1 version 6): a load returns the last store.  With w(r) = x(write flag, r) on an access r:
// w(r) not 0 / 1 is refused; a store (w = 1) is free; a load (w = 0) is refused unless, for every carried column j = 1 .. nc - 1 (the
// clock c_0 is exempt), x(c_j, r) = x(c_j, r') when r is linked and x(c_j, r) = 0 when it is not (memory starts zeroed).  Residues
// mod P are compared: a raw word P is a zero.  The rule adds no destination.  On one row the order is write flag, clock, read rule
// (lowest j first), and the lowest (record, row) over all of these is the one refusal reported.
//
// sort_rows (sort.h; the passes and kernels of sort.hip) sorts every record's accesses by key, stably: position j of the sorted order
// holds (packed key, row), equal keys in row order, so the previous access of the row at j is the row at j - 1 when the keys are equal,
// and it is the last one when the key at j + 1 differs.  Then two passes of one kernel over all records at once (grid.y = the record),
// one lane per sorted position: the neighbours' keys and rows are coalesced loads, the carried cells at row(j - 1) and the clock at row(j)
// random ones (with READS the check pass also reads the write flag at row(j) and, for a load, the value cells at row(j) and row(j - 1):
// random 4-byte reads like the clock's).  The check pass reads only and reduces the first bad (record, row): one 64-bit atomicMin per
// wave that found one.  The host reads that word back; only a witness that passed is written (the write pass: the destinations at row(j), 4-byte scattered
// stores, and zeros on the active rows that are no access, coalesced), so a refusal leaves `data` unchanged.  Sources are never
// destinations (set_arguments), so both passes see the same sources and no lane reads what another writes.  Selectors are refused by
// the sort's key pass, over all records, before any clock is read.
#include "sort.h"

using namespace zkh;

namespace {

constexpr uint32_t LINK_THREADS = 256;

// grid (ceil(A / LINK_THREADS), records).  kWrite = false: the check pass (bad = the lowest bad record << 32 | row, the record by its place
// among the LINK records); kWrite = true: the write pass over a witness that passed.  kReads: the check pass of a blob in which a
// record has READS; the flag is uniform per record, so the branch is scalar, and which rule a row broke the host finds out by reading
// its few cells back.  The record's words are read through the uniform pointer (scalar loads): nothing is indexed in registers.
template <bool kWrite, bool kReads>
__global__ __launch_bounds__(LINK_THREADS) void k_links(const uint32_t* __restrict__ code, uint32_t* data, const Link* __restrict__ links,
                                                        const uint32_t* __restrict__ status, const unsigned long long* __restrict__ keys,
                                                        const uint32_t* __restrict__ rows, uint32_t n, uint32_t A, unsigned long long* __restrict__ bad) {
    const uint32_t p = blockIdx.y;
    const Link* __restrict__ rec = links + p;
    const uint32_t m = status[ST_HEAD + ST_WORDS * p + ST_M];                 // the record's accesses: m <= A
    const uint32_t t = blockIdx.x * LINK_THREADS + threadIdx.x;             // a sorted position (t < m) and, in the write pass, a row (t < A)
    const size_t base = (size_t)p * A;
    const bool access = t < m;
    uint32_t row = 0, prow = 0;
    bool linked = false, last = false;
    if (access) {
        const unsigned long long key = keys[base + t];
        row = rows[base + t];
        if (t) {
            linked = keys[base + t - 1] == key;
            prow = rows[base + t - 1];
        }
        last = t + 1 >= m || keys[base + t + 1] != key;
    }
    long long d = 0;
    if (linked) {
        const uint32_t* clock = group_ptr(code, data, rec->cg[0]) + (size_t)rec->cc[0] * n;
        d = (long long)canonical(clock[row]) - canonical(clock[prow]) - 1;
    }
    const uint32_t L = rec->L, nl = rec->nl;
    if (!kWrite) {
        uint32_t mine = linked && (d < 0 || (d >> (L * nl)) != 0) ? row : NONE;
        if constexpr (kReads) {
            if ((rec->flags & LINK_READS) && access) {
                const uint32_t w = cell(code, data, rec->wg, rec->wc, n, row);
                bool ok = w == 0 || w == R1;
                if (w == 0) {                             // a load: every value column equals the previous access's, or 0 without one
                    const uint32_t nc = rec->nc;
                    for (uint32_t j = 1; j < nc; j++) {
                        const uint32_t* col = group_ptr(code, data, rec->cg[j]) + (size_t)rec->cc[j] * n;
                        ok &= col[row] % P == (linked ? col[prow] % P : 0);
                    }
                }
                if (!ok) mine = row;
            }
        }
        // report_bad_row (arguments.h) written out: through the helper this kernel's argument loads are scheduled otherwise
        if (__ballot(mine != NONE) != 0) {                // wave-uniform: only a wave that found one reduces and writes
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t o = __shfl_xor(mine, off, 64);
                mine = o < mine ? o : mine;
            }
            if ((threadIdx.x & 63) == 0) atomicMin(bad, ((unsigned long long)p << 32) | mine);
        }
        return;
    }
    const uint32_t nc = rec->nc, n_dst = rec->n_dst;
    if (rec->sel != NONE && t < A && sel_class(code, rec->sel, n, t) != 1)
        for (uint32_t e = 0; e < n_dst; e++) data[(size_t)rec->dst[e] * n + t] = 0;
    if (!access) return;
    data[(size_t)rec->dst[0] * n + row] = linked ? R1 : 0;
    data[(size_t)rec->dst[1] * n + row] = last ? R1 : 0;
    for (uint32_t j = 0; j < nc; j++)
        data[(size_t)rec->dst[2 + j] * n + row] = linked ? group_ptr(code, data, rec->cg[j])[(size_t)rec->cc[j] * n + prow] : 0;
    const uint32_t mask = (1u << L) - 1;                  // L <= 16
    for (uint32_t j = 0; j < nl; j++)
        data[(size_t)rec->dst[2 + nc + j] * n + row] = fp_encode((uint32_t)((unsigned long long)d >> (j * L)) & mask).v;
}

}  // namespace

extern "C" const char* zkh_derive_links(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data) {
    ZKH_REQUIRE(ctx && c && data, "derive_links: null argument");
    ZKH_REQUIRE(code, "derive_links: the raw code trace is required (the selectors and code-group source columns of the records read it)");
    ZKH_REQUIRE(zkh_circuit_derives_links(c), "derive_links: the circuit's arguments hold no LINK record (ZKA1 version 5)");
    size_t n;
    uint32_t A;
    ZKH_TRY(trace_rows("derive_links", c, po2, zk_cycles, code, data, nullptr, &n, &A));
    const std::vector<Link>& links = c->args->links;
    const uint32_t nr = (uint32_t)links.size();
    ZKH_REQUIRE(nr <= 65535, "derive_links: %u LINK records in one blob (at most 65535)", nr);
    std::vector<SortPair> pairs(nr, SortPair{});
    for (uint32_t p = 0; p < nr; p++) {                 // the accesses of a record sorted by their key alone: the sort is stable
        pairs[p].d_term = links[p].index; pairs[p].nkeys = 1; pairs[p].sel = links[p].sel;
        for (uint32_t f = 0; f < MAX_SORT_KEYS; f++) { pairs[p].kg[f] = links[p].kg; pairs[p].kc[f] = links[p].kc; }
        for (uint32_t e = 0; e < MAX_TUPLE; e++) pairs[p].sg[e] = GROUP_DATA;
    }
    bind_thread(ctx);
    SortedRows sorted;
    ZKH_TRY(sort_rows(ctx, code, data, n, A, pairs, &sorted));
    if (sorted.bad_selector) {
        const Link& r = links[sorted.bad_pair];
        uint32_t sel;
        ZKH_TRY(read_cell(ctx, code, data, GROUP_CODE, r.sel, n, sorted.bad_row, &sel));
        return make_err("derive_links: record %u at row %u: selector %u, not 0 or 1: the witness is refused", r.index, sorted.bad_row, sel);
    }
    ZKH_REQUIRE(!sorted.wide, "derive_links: a packed key of more than 64 bits from one 31-bit field");
    static_assert(sizeof(Link) % 4 == 0, "word records");
    Tmp drecs;
    BadRow bad;
    ZKH_TRY(zkh_copy_from(ctx, "link_records", (const uint32_t*)links.data(), links.size() * (sizeof(Link) / 4), drecs.out()));
    ZKH_TRY(bad.init(ctx));
    double carried = 0, dsts = 0;
    for (const Link& r : links) { carried += r.nc; dsts += r.n_dst; }
    const dim3 grid((unsigned)((A + LINK_THREADS - 1) / LINK_THREADS), nr);
    const bool reads = c->args->reads != 0;             // a record has READS: the check pass with the read rule, over all records
    const Link* d_recs = (const Link*)drecs->ptr();
    {
        double cells = 0;                                 // with READS: the write flag and, at most, the value cells at both rows
        for (const Link& r : links) cells += r.flags & LINK_READS ? 1 + 2 * (r.nc - 1) : 0;
        ProfScope prof(ctx, "links_check", (20.0 * nr + 4.0 * cells) * A);   // key and row of every item; the clock at both rows
        (reads ? k_links<false, true> : k_links<false, false>)<<<grid, LINK_THREADS, 0, ctx->stream>>>(code->ptr(), data->ptr(), d_recs, sorted.status->ptr(),
                                                                                                       sorted.keys(), sorted.rows(), (uint32_t)n, A, bad.ptr());
        ZKH_TRY(last_launch_error("links_check"));
    }
    ZKH_TRY(bad.read(ctx));
    if (bad.found) {
        // the refused access and its previous one, found on the host as the reference finds them: the key and the selector of rows [0, row]
        const Link& r = links[bad.hi];
        const uint32_t row = bad.lo;
        std::vector<uint32_t> key(row + 1), sel(row + 1, R1);
        ZKH_TRY(zkh_read(ctx, r.kg == GROUP_CODE ? code : data, key.data(), (size_t)r.kc * n, row + 1));
        if (r.sel != NONE) ZKH_TRY(zkh_read(ctx, code, sel.data(), (size_t)r.sel * n, row + 1));
        uint32_t prow = row;                              // prow == row: no earlier access has its key (unlinked)
        for (uint32_t q = row; q-- > 0;)
            if (sel[q] % P == R1 && key[q] % P == key[row] % P) { prow = q; break; }
        const bool linked = prow != row;
        if (r.flags & LINK_READS) {
            uint32_t w;
            ZKH_TRY(read_cell(ctx, code, data, r.wg, r.wc, n, row, &w));
            if (w > 1) return make_err("derive_links: record %u at row %u: write flag %u, not 0 or 1: the witness is refused", r.index, row, w);
        }
        if (linked) {
            long long now, before;
            ZKH_TRY(read_cell(ctx, code, data, r.cg[0], r.cc[0], n, row, &now));
            ZKH_TRY(read_cell(ctx, code, data, r.cg[0], r.cc[0], n, prow, &before));
            const long long d = now - before - 1;
            if (d < 0)
                return make_err("derive_links: record %u at row %u: clock not increasing (%lld after %lld at row %u): the witness is refused", r.index, row, now, before, prow);
            if ((d >> (r.L * r.nl)) != 0)
                return make_err("derive_links: record %u at row %u: the clock difference %lld (after row %u) does not fit %u limbs of %u bits: the witness is refused",
                                r.index, row, d, prow, r.nl, r.L);
        }
        for (uint32_t j = 1; (r.flags & LINK_READS) && j < r.nc; j++) {     // a load (the write flag is 0, or something above was named)
            uint32_t now, before = 0;
            ZKH_TRY(read_cell(ctx, code, data, r.cg[j], r.cc[j], n, row, &now));
            if (linked) ZKH_TRY(read_cell(ctx, code, data, r.cg[j], r.cc[j], n, prow, &before));
            if (now == before) continue;
            if (linked)
                return make_err("derive_links: record %u at row %u: a load of carried column %u returns %u, but %u was last stored (row %u): the witness is refused",
                                r.index, row, j, now, before, prow);
            return make_err("derive_links: record %u at row %u: a load of carried column %u returns %u, but its address was never accessed: the value must be 0: "
                            "the witness is refused", r.index, row, j, now);
        }
        return make_err("derive_links: record %u at row %u was refused, but the host finds no rule it breaks", r.index, row);
    }
    {
        ProfScope prof(ctx, "links_write", (20.0 * nr + 4.0 * carried + 4.0 * dsts) * A);
        k_links<true, false><<<grid, LINK_THREADS, 0, ctx->stream>>>(code->ptr(), data->ptr(), d_recs, sorted.status->ptr(), sorted.keys(), sorted.rows(),
                                                                   (uint32_t)n, A, bad.ptr());
        ZKH_TRY(last_launch_error("links_write"));
    }
    // the temporaries go back to the pool on return: the stream orders their next use after these launches
    return nullptr;
}
