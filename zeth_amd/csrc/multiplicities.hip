// multiplicities.hip — derived lookup multiplicities (a term's `derive` flag, ZKA1 version 2; zeth_amd/circuits/logup.py; DESIGN.md §2
// ARGUMENTS): the table side's multiplicity column, counted on the device.
//
// A tag t with derived (table) terms D and lookup terms L.  The key of a term at row r is (t, v_0 .. v_3) as field elements, the tuple
// zero-padded to 4 (words compared mod P).  Table entries: the (D, r) with r < A and sel_D(r) = 1; the representative of a key is its
// entry with the smallest (blob term index, row).  count(K) = sum of sel_L(r) m_L(r) over the lookup rows r < A whose key is K (in Fp).
// data[m_D][r] := Montgomery(count(K)) on the representative of K, 0 on every other active row; rows [A, n) are not touched.
//
// Three steps on the context stream:
//   (a) k_derive_build: one lane per (derived term, active row) inserts the packed entry (term << 32 | row) into a power-of-two
//       open-addressing table of at least twice the possible entries, hashed by the key.  Slots hold no key: it is re-read from the
//       trace through the packed entry, which never changes its key once it is in a slot.  An insert is one 64-bit CAS on an empty slot,
//       or an atomicMin on a slot holding an equal key (the lowest entry stays): no lane waits for another.  The lane that fills a slot
//       numbers it (a dense id, 0 .. U-1) for the counters;
//   (b) k_derive_count: one lane per (lookup term, active row) finds its key's slot and adds its weight (canonical, < P) to the slot's
//       u64 counter.  Up to LDS_KEYS distinct keys (byte and 12-bit tables) the counters are a per-workgroup LDS histogram flushed with
//       one global atomic per touched key and workgroup (67 M adds onto 256 addresses are the contended case of Guideline 12); above,
//       the adds go straight to the global counters.  The host picks the path from U, read back after the build;
//   (c) k_derive_write: one lane per (derived term, active row) writes the count of its key on the representative, 0 elsewhere.
// A table selector other than 0 / 1 (after the build) or a lookup of nonzero weight without a table entry (after the count) refuses
// the witness before (c): `data` is left unchanged.  The key, its hash and the probe are keytable.h's, shared with bus.hip.
#include "keytable.h"

#include <algorithm>

using namespace zkh;

namespace {

constexpr uint32_t DERIVE_THREADS = 256;
constexpr uint32_t LDS_KEYS = 4096;              // u64 counters per workgroup in the LDS path: 32 KiB
constexpr uint32_t COUNT_BLOCKS = 1024;          // workgroups of the count (4 per CU); each loops over every lookup term

// status words: [0, 2) the first lookup without a table entry (row << 32 | term), [2, 4) the first bad table selector (the same form),
// [4] U = distinct keys
// (a) grid (x, derived terms)
__global__ __launch_bounds__(DERIVE_THREADS) void k_derive_build(const uint32_t* __restrict__ code, const uint32_t* __restrict__ data,
                                                                const KeyTerm* __restrict__ terms, const uint32_t* __restrict__ derived,
                                                                unsigned long long* __restrict__ slots, uint32_t* __restrict__ sid,
                                                                uint32_t mask, uint32_t n, uint32_t A, uint32_t* __restrict__ status) {
    const uint32_t ti = derived[blockIdx.y];
    const KeyTerm t = terms[ti];
    for (uint32_t r = blockIdx.x * DERIVE_THREADS + threadIdx.x; r < A; r += gridDim.x * DERIVE_THREADS) {
        const uint32_t cls = sel_class(code, t.c.sel, n, r);
        if (cls == 0) continue;
        if (cls == 2) { atomicMin((unsigned long long*)(status + 2), ((unsigned long long)r << 32) | ti); continue; }
        const Key k = read_key(code, data, t, n, r);
        const unsigned long long me = ((unsigned long long)ti << 32) | r;
        for (uint32_t s = key_hash(t.tag, k) & mask;; s = (s + 1) & mask) {
            const unsigned long long cur = atomicCAS(slots + s, SLOT_EMPTY, me);
            if (cur == SLOT_EMPTY) { sid[s] = atomicAdd(status + 4, 1u); break; }
            if (slot_has_key(code, data, terms, cur, t.tag, k, n)) { atomicMin(slots + s, me); break; }
        }
    }
}

// (b) grid COUNT_BLOCKS-or-fewer workgroups; each takes every lookup term over its stride of rows
template <bool kLds>
__global__ __launch_bounds__(DERIVE_THREADS) void k_derive_count(const uint32_t* __restrict__ code, const uint32_t* __restrict__ data,
                                                                const KeyTerm* __restrict__ terms, const uint32_t* __restrict__ lookups,
                                                                uint32_t n_lookups, const unsigned long long* __restrict__ slots,
                                                                const uint32_t* __restrict__ sid, uint32_t mask, uint32_t n, uint32_t A,
                                                                unsigned long long* __restrict__ cnt, uint32_t U, uint32_t* __restrict__ status) {
    __shared__ unsigned long long hist[kLds ? LDS_KEYS : 1];
    if (kLds) {
        for (uint32_t i = threadIdx.x; i < U; i += DERIVE_THREADS) hist[i] = 0;
        __syncthreads();
    }
    for (uint32_t j = 0; j < n_lookups; j++) {
        const uint32_t ti = lookups[j];
        const KeyTerm t = terms[ti];
        for (uint32_t r = blockIdx.x * DERIVE_THREADS + threadIdx.x; r < A; r += gridDim.x * DERIVE_THREADS) {
            const uint32_t w = row_weight(code, data, t, n, r);
            if (w == 0) continue;
            const uint32_t s = find_slot(code, data, terms, slots, mask, t.tag, read_key(code, data, t, n, r), n);
            if (s == NONE) { atomicMin((unsigned long long*)status, ((unsigned long long)r << 32) | ti); continue; }
            if (kLds) atomicAdd(hist + sid[s], (unsigned long long)w);
            else atomicAdd(cnt + sid[s], (unsigned long long)w);
        }
    }
    if (kLds) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < U; i += DERIVE_THREADS)
            if (hist[i]) atomicAdd(cnt + i, hist[i]);
    }
}

// (c) grid (ceil(A / DERIVE_THREADS), derived terms)
__global__ __launch_bounds__(DERIVE_THREADS) void k_derive_write(const uint32_t* __restrict__ code, uint32_t* data, const KeyTerm* __restrict__ terms,
                                                                const uint32_t* __restrict__ derived, const unsigned long long* __restrict__ slots,
                                                                const uint32_t* __restrict__ sid, uint32_t mask, uint32_t n, uint32_t A,
                                                                const unsigned long long* __restrict__ cnt) {
    const uint32_t ti = derived[blockIdx.y];
    const KeyTerm t = terms[ti];
    const uint32_t r = blockIdx.x * DERIVE_THREADS + threadIdx.x;
    if (r >= A) return;
    uint32_t out = 0;
    if (t.c.sel == NONE || cell(code, data, GROUP_CODE, t.c.sel, n, r) != 0) {
        const uint32_t s = find_slot(code, data, terms, slots, mask, t.tag, read_key(code, data, t, n, r), n);
        if (s != NONE && slots[s] == (((unsigned long long)ti << 32) | r)) out = fp_encode((uint32_t)(cnt[sid[s]] % P)).v;
    }
    data[(size_t)t.c.mc * n + r] = out;            // m_D is read by no term (set_arguments): no lane of this grid reads it
}

}  // namespace

extern "C" const char* zkh_derive_multiplicities(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code,
                                                 zkh_buf* data) {
    ZKH_REQUIRE(ctx && c && data, "derive_multiplicities: null argument");
    ZKH_REQUIRE(code, "derive_multiplicities: the raw code trace is required (the keys and selectors of the terms read it)");
    ZKH_REQUIRE(zkh_circuit_derives_multiplicities(c), "derive_multiplicities: the circuit's arguments derive no multiplicity (ZKA1 version 2)");
    size_t n;
    uint32_t A;
    ZKH_TRY(trace_rows("derive_multiplicities", c, po2, zk_cycles, code, data, nullptr, &n, &A));
    const std::vector<Term>& a = c->args->terms;
    const uint32_t n_terms = (uint32_t)a.size();
    std::vector<uint32_t> derived, lookups;
    for (uint32_t i = 0; i < n_terms; i++)
        if (a[i].derive) derived.push_back(i);
    for (uint32_t i = 0; i < n_terms; i++)               // the lookups: the other terms of a derived term's tag
        if (!a[i].derive && std::any_of(derived.begin(), derived.end(), [&](uint32_t j) { return a[j].tag == a[i].tag; })) lookups.push_back(i);
    // counters: at most n_lookups * A adds of < 2^31 each
    ZKH_REQUIRE((uint64_t)lookups.size() * A < (1ull << 33), "derive_multiplicities: %zu lookup terms x %u rows could overflow a counter",
                lookups.size(), A);
    uint64_t slots_n = 64;
    while (slots_n < 2ull * derived.size() * A) slots_n <<= 1;
    ZKH_REQUIRE(slots_n <= (1ull << 31), "derive_multiplicities: %zu table terms x %u rows do not fit one table", derived.size(), A);
    const uint32_t mask = (uint32_t)(slots_n - 1);
    bind_thread(ctx);

    std::vector<uint32_t> table = key_term_table(a, derived.size() + lookups.size());
    uint32_t* lists = table.data() + n_terms * KEY_TERM_WORDS;
    std::copy(derived.begin(), derived.end(), lists);
    std::copy(lookups.begin(), lookups.end(), lists + derived.size());
    Tmp dtab, status, slots, sid, cnt;
    ZKH_TRY(zkh_copy_from(ctx, "derive_terms", table.data(), table.size(), dtab.out()));
    ZKH_TRY(new_buf(ctx, 6, false, status.out()));
    ZKH_TRY(new_buf(ctx, 2 * slots_n, false, slots.out()));
    ZKH_TRY(new_buf(ctx, slots_n, false, sid.out()));                 // read only where a slot is filled: no initialisation
    ZKH_HIP(hipMemsetAsync(status->ptr(), 0xff, 16, ctx->stream));
    ZKH_HIP(hipMemsetAsync(status->ptr() + 4, 0, 8, ctx->stream));
    ZKH_HIP(hipMemsetAsync(slots->ptr(), 0xff, 8 * slots_n, ctx->stream));
    const KeyTerm* d_terms = (const KeyTerm*)dtab->ptr();
    const uint32_t* d_derived = dtab->ptr() + n_terms * KEY_TERM_WORDS;
    const uint32_t* d_lookups = d_derived + derived.size();
    unsigned long long* d_slots = (unsigned long long*)slots->ptr();
    double key_words = 0;                                             // tuple + selector words per row of the derived terms
    for (uint32_t i : derived) key_words += a[i].w + (a[i].sel != NONE);
    const unsigned rows_x = (unsigned)((A + DERIVE_THREADS - 1) / DERIVE_THREADS);
    {
        ProfScope prof(ctx, "derive_build", 4.0 * key_words * A + 8.0 * slots_n);
        k_derive_build<<<dim3(rows_x, (unsigned)derived.size()), DERIVE_THREADS, 0, ctx->stream>>>(
            code->ptr(), data->ptr(), d_terms, d_derived, d_slots, sid->ptr(), mask, (uint32_t)n, A, status->ptr());
        ZKH_TRY(last_launch_error("derive_build"));
    }
    uint32_t st[6];
    ZKH_TRY(zkh_read(ctx, status, st, 0, 6));
    auto entry_of = [&](uint32_t lo, uint32_t hi, uint32_t* term, uint32_t* row) {
        const unsigned long long e = ((unsigned long long)hi << 32) | lo;
        *row = (uint32_t)(e >> 32);
        *term = (uint32_t)e;
        return e != ~0ull;
    };
    uint32_t term, row;
    if (entry_of(st[2], st[3], &term, &row)) {
        uint32_t sel;
        ZKH_TRY(read_cell(ctx, code, data, GROUP_CODE, a[term].sel, n, row, &sel));
        return make_err("derive_multiplicities: table term %u (tag %u) has selector %u at row %u, not 0 or 1: the witness is refused", term,
                        a[term].tag, sel, row);
    }
    const uint32_t U = st[4];
    ZKH_TRY(new_buf(ctx, 2 * (size_t)std::max<uint32_t>(U, 1), true, cnt.out()));
    unsigned long long* d_cnt = (unsigned long long*)cnt->ptr();
    {
        double in_words = 0;                                          // weight + tuple words per lookup row, the key re-reads not counted
        for (uint32_t i : lookups) in_words += entry_words(a[i]);
        const bool lds = U <= LDS_KEYS;
        ProfScope prof(ctx, lds ? "derive_count_lds" : "derive_count_global", 4.0 * in_words * A + 8.0 * U);
        const unsigned bx = std::min<unsigned>(rows_x, COUNT_BLOCKS);
        if (lds)
            k_derive_count<true><<<bx, DERIVE_THREADS, 0, ctx->stream>>>(code->ptr(), data->ptr(), d_terms, d_lookups, (uint32_t)lookups.size(),
                                                                        d_slots, sid->ptr(), mask, (uint32_t)n, A, d_cnt, U, status->ptr());
        else
            k_derive_count<false><<<bx, DERIVE_THREADS, 0, ctx->stream>>>(code->ptr(), data->ptr(), d_terms, d_lookups, (uint32_t)lookups.size(),
                                                                         d_slots, sid->ptr(), mask, (uint32_t)n, A, d_cnt, U, status->ptr());
        ZKH_TRY(last_launch_error("derive_count"));
    }
    ZKH_TRY(zkh_read(ctx, status, st, 0, 2));
    if (entry_of(st[0], st[1], &term, &row)) {
        const Term& t = a[term];
        uint32_t v[MAX_TUPLE] = {0, 0, 0, 0};
        for (uint32_t e = 0; e < t.w; e++) ZKH_TRY(read_cell(ctx, code, data, t.tg[e], t.tc[e], n, row, v + e));
        return make_err("derive_multiplicities: lookup term %u (tag %u) at row %u has no table entry: key (%u, %u, %u, %u): the witness is "
                        "refused", term, t.tag, row, v[0], v[1], v[2], v[3]);
    }
    {
        ProfScope prof(ctx, "derive_write", 4.0 * key_words * A + 4.0 * derived.size() * A);
        k_derive_write<<<dim3(rows_x, (unsigned)derived.size()), DERIVE_THREADS, 0, ctx->stream>>>(
            code->ptr(), data->ptr(), d_terms, d_derived, d_slots, sid->ptr(), mask, (uint32_t)n, A, d_cnt);
        ZKH_TRY(last_launch_error("derive_write"));
    }
    return nullptr;
}
