// bus.hip — zkh_check_bus: which key of a witness's bus does not balance (DESIGN.md §2 CHECK BUS; the definition's host twin:
// zeth_amd/circuits/logup.py reference_bus).  No mix and no accum: the raw code and data traces and the circuit's arguments alone.
//
// An ENTRY is a (term i, row r < A) of non-zero weight w_i(r) = sel_i(r) m_i(r) in Fp (residues; absent = 1: the accumulate's numerator).
// Its KEY is (tag, v_0 .. v_3), residues, the tuple zero-padded to 4 (keytable.h).  net(K) = sum over K's entries of sign_i w_i(r) in Fp;
// K is unbalanced when net(K) != 0.  Distinct keys are distinct poles, so the bus balances for every mix exactly when every net is 0.
// The representative of a key is its entry of smallest (blob term index, row), over all terms; the call reports the unbalanced key of
// smallest representative, and on request what every term holds of that key.
//
//   k_bus_build  one lane per (term, active row).  A lane of non-zero weight finds or claims its key's slot in keytable.h's table —
//       a 64-bit CAS on an empty slot, an atomicMin of (term << 32 | row) on a slot of equal key — and adds its canonical weight to the
//       slot's `pos` or `neg` u64 counter, by the term's sign.  The counters sit at the slot index.  FIND-THEN-ADD IN ONE PASS IS SOUND
//       BECAUSE A SLOT NEVER CHANGES ITS KEY ONCE CLAIMED: the slot a lane found is the slot of its key for good, whatever entry
//       represents it later.  Every global atomic is a CAS-on-empty, a min or an add: the slot a key lands in depends on the order of
//       arrival, the result does not.  A byte table puts tens of millions of adds onto 256 addresses: the lanes of a wave that hold
//       the same slot (one term per workgroup, so one sign) first sum their weights — the leader's slot is broadcast, a ballot finds
//       the equal lanes, repeat — and the leader issues one atomic per slot and wave.
//   The table holds one slot per distinct KEY, not per entry.  It starts at the smallest power of two >= max(64, 2 A); the build counts
//       the slots it claims, and a claim beyond half the table sets an overflow word, after which lanes stop inserting; the host then
//       clears, doubles and builds again, up to 2^31 slots.  More than half the slots are claimed exactly when there are more distinct
//       keys than that, so the final size is a function of the number of distinct keys.  A probe gives up (overflow) after a full
//       turn, so it ends even on a small table that concurrent lanes filled before they saw the overflow word.
//   k_bus_scan   one lane per slot: a filled slot whose residues pos % P and neg % P differ is unbalanced (the 64-bit sums are not
//       compared: P - 1 and 1 on one side are a sum of P); the lowest representative per wave, one 64-bit atomicMin and one atomicAdd
//       of the ballot's popcount per wave that found one (check_rows.hip's pattern).
//   k_bus_report one lane: the reported key (re-read through its representative) and its two sums.
//   k_bus_explain  only when something is unbalanced and the caller asked: one lane per (term of the key's tag, active row); per term
//       the entries of the reported key: their count, weight, first and last row, reduced per wave.
// The counters bound n_terms * A below 2^33 for the reason multiplicities.hip does.  Reads code and data, writes neither.
#include "keytable.h"

#include <algorithm>

using namespace zkh;

// The two choices M16 measured (DESIGN.md §2 CHECK BUS, profiles/r16_check_bus.json); the other settings build the A/B variants.
#ifndef ZKH_BUS_WAVE_COMBINE
#define ZKH_BUS_WAVE_COMBINE 1                   // lanes of a wave that hold one slot combine their weights before one atomic; 0: one atomic per lane
#endif
#ifndef ZKH_BUS_GRID_TERMS
#define ZKH_BUS_GRID_TERMS 1                     // grid (rows, terms); 0: BUILD_BLOCKS workgroups, each looping over every term
#endif

namespace {

constexpr uint32_t BUS_THREADS = 256;
constexpr uint32_t BUILD_BLOCKS = 1024;
// status words
constexpr uint32_t ST_LOWEST = 0;                // [0, 2): the lowest representative of an unbalanced key (u64, all ones = none)
constexpr uint32_t ST_UNBALANCED = 2, ST_KEYS = 3, ST_OVERFLOW = 4;
constexpr uint32_t ST_KEY = 6;                   // [6, 10): the reported key's tuple (Montgomery residues)
constexpr uint32_t ST_POS = 10, ST_NEG = 12;     // its two sums (u64 each)
constexpr uint32_t ST_WORDS = 14;
constexpr uint32_t TERM_OUT_WORDS = 6;           // k_bus_explain, per term: count, first row, last row, -, weight (u64)

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the slot of the key of (t, r), claimed if the key is new; NONE once the table is past half full
__device__ __forceinline__ uint32_t claim_slot(const uint32_t* code, const uint32_t* data, const KeyTerm* terms, unsigned long long* slots,
                                               uint32_t mask, uint32_t half, const KeyTerm& t, uint32_t ti, uint32_t r, uint32_t n,
                                               uint32_t* status) {
    const Key k = read_key(code, data, t, n, r);
    const unsigned long long me = ((unsigned long long)ti << 32) | r;
    uint32_t s = key_hash(t.tag, k) & mask;
    for (uint32_t probes = 0; probes <= mask; probes++, s = (s + 1) & mask) {
        unsigned long long cur = slots[s];                   // a stale word is EMPTY (the CAS then tells) or an older entry of the same key
        if (cur == SLOT_EMPTY) {
            cur = atomicCAS(slots + s, SLOT_EMPTY, me);
            if (cur == SLOT_EMPTY) {
                if (atomicAdd(status + ST_KEYS, 1u) >= half) atomicOr(status + ST_OVERFLOW, 1u);
                return s;
            }
        }
        if (slot_has_key(code, data, terms, cur, t.tag, k, n)) {
            if (me < cur) atomicMin(slots + s, me);          // entries only decrease: me below the current word is below `cur`
            return s;
        }
    }
    atomicOr(status + ST_OVERFLOW, 1u);
    return NONE;
}

// the weights of the lanes of this wave that hold the same slot, added with one atomic per slot (the sign is the wave's: one term)
__device__ __forceinline__ void add_combined(unsigned long long* cnt, uint32_t s, uint32_t neg, uint32_t w) {
    unsigned long long live = __ballot(s != NONE);
    const uint32_t lane = threadIdx.x & 63;
    while (live != 0) {                                      // wave-uniform
        const uint32_t leader = (uint32_t)__ffsll((long long)live) - 1;
        const uint32_t ls = __shfl(s, leader, 64);
        const bool same = s == ls;
        const unsigned long long group = __ballot(same);
        unsigned long long sum = same ? w : 0;
        if (group != (1ull << leader)) sum = wave_sum(sum);
        if (lane == leader) atomicAdd(cnt + 2 * (size_t)ls + neg, sum);
        live &= ~group;
    }
}

// grid (x, y): the workgroups of one y take the terms y, y + gridDim.y, ...; rows in strides of gridDim.x workgroups
constexpr uint32_t BUS_SKIP = 2;                // in place of a term's sign: the term is of the open tag of an OPEN record (ZKA1 version 8) and holds no entry here
__global__ __launch_bounds__(BUS_THREADS) void k_bus_build(const uint32_t* __restrict__ code, const uint32_t* __restrict__ data,
                                                           const KeyTerm* __restrict__ terms, const uint32_t* __restrict__ negs,
                                                           uint32_t n_terms, unsigned long long* slots, unsigned long long* cnt, uint32_t mask,
                                                           uint32_t half, uint32_t n, uint32_t A, uint32_t* status) {
    for (uint32_t ti = blockIdx.y; ti < n_terms; ti += gridDim.y) {
        const KeyTerm t = terms[ti];
        const uint32_t neg = negs[ti];
        if (neg == BUS_SKIP) continue;                                   // a term of the open tag: another seal answers its keys (workgroup-uniform)
        for (uint32_t base = blockIdx.x * BUS_THREADS; base < A; base += gridDim.x * BUS_THREADS) {     // the same trips for every lane
            const uint32_t r = base + threadIdx.x;
            uint32_t s = NONE, w = 0;
            if (r < A && __hip_atomic_load(status + ST_OVERFLOW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
                w = row_weight(code, data, t, n, r);
            if (w != 0) s = claim_slot(code, data, terms, slots, mask, half, t, ti, r, n, status);
#if ZKH_BUS_WAVE_COMBINE
            add_combined(cnt, s, neg, w);
#else
            if (s != NONE) atomicAdd(cnt + 2 * (size_t)s + neg, (unsigned long long)w);
#endif
        }
    }
}

__global__ __launch_bounds__(BUS_THREADS) void k_bus_scan(const unsigned long long* __restrict__ slots, const unsigned long long* __restrict__ cnt,
                                                          uint32_t n_slots, uint32_t* status) {
    const uint32_t s = blockIdx.x * BUS_THREADS + threadIdx.x;
    unsigned long long key = ~0ull;
    if (s < n_slots) {
        const unsigned long long cur = slots[s];
        if (cur != SLOT_EMPTY && (uint32_t)(cnt[2 * (size_t)s] % P) != (uint32_t)(cnt[2 * (size_t)s + 1] % P)) key = cur;
    }
    const unsigned long long bad = __ballot(key != ~0ull);
    if (bad != 0) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(key, off, 64);
            key = o < key ? o : key;
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMin((unsigned long long*)(status + ST_LOWEST), key);
            atomicAdd(status + ST_UNBALANCED, (uint32_t)__popcll(bad));
        }
    }
}

__global__ void k_bus_report(const uint32_t* __restrict__ code, const uint32_t* __restrict__ data, const KeyTerm* __restrict__ terms,
                             const unsigned long long* __restrict__ slots, const unsigned long long* __restrict__ cnt, uint32_t mask,
                             uint32_t n, uint32_t* status) {
    if (threadIdx.x != 0) return;
    const uint32_t ti = status[ST_LOWEST + 1], r = status[ST_LOWEST];
    const KeyTerm t = terms[ti];
    const Key k = read_key(code, data, t, n, r);
    const uint32_t s = find_slot(code, data, terms, slots, mask, t.tag, k, n);     // its own entry is in the table: never NONE
    for (uint32_t e = 0; e < MAX_TUPLE; e++) status[ST_KEY + e] = k.v[e];
    const unsigned long long pos = s != NONE ? cnt[2 * (size_t)s] : 0, neg = s != NONE ? cnt[2 * (size_t)s + 1] : 0;
    status[ST_POS] = (uint32_t)pos; status[ST_POS + 1] = (uint32_t)(pos >> 32);
    status[ST_NEG] = (uint32_t)neg; status[ST_NEG + 1] = (uint32_t)(neg >> 32);
}

// grid (ceil(A / BUS_THREADS), terms); rows ascend with the lane, so a wave's first and last entry are its lowest and highest set lane
__global__ __launch_bounds__(BUS_THREADS) void k_bus_explain(const uint32_t* __restrict__ code, const uint32_t* __restrict__ data,
                                                             const KeyTerm* __restrict__ terms, uint32_t tag, Key key, uint32_t n, uint32_t A,
                                                             uint32_t* out) {
    const uint32_t ti = blockIdx.y;
    const KeyTerm t = terms[ti];
    if (t.tag != tag) return;
    const uint32_t r = blockIdx.x * BUS_THREADS + threadIdx.x;
    uint32_t w = 0;
    bool hit = false;
    if (r < A) {
        w = row_weight(code, data, t, n, r);
        if (w != 0) {
            const Key k = read_key(code, data, t, n, r);
            hit = true;
#pragma unroll
            for (uint32_t e = 0; e < MAX_TUPLE; e++) hit &= k.v[e] == key.v[e];
        }
    }
    const unsigned long long hits = __ballot(hit);
    if (hits == 0) return;                                   // wave-uniform
    const unsigned long long sum = wave_sum(hit ? w : 0);
    const uint32_t lane = threadIdx.x & 63;
    if (lane == 0) {
        uint32_t* o = out + (size_t)ti * TERM_OUT_WORDS;
        atomicAdd(o, (uint32_t)__popcll(hits));
        atomicMin(o + 1, r + (uint32_t)__ffsll((long long)hits) - 1);
        atomicMax(o + 2, r + 63 - (uint32_t)__clzll((long long)hits));
        atomicAdd((unsigned long long*)(o + 4), sum);
    }
}

}  // namespace

extern "C" const char* zkh_check_bus(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* data,
                                     zkh_bus_term* per_term, size_t n_per_term, zkh_check_bus_result* result) {
    ZKH_REQUIRE(ctx && c && data && result, "check_bus: null argument");
    ZKH_REQUIRE(code, "check_bus: the raw code trace is required (the keys and selectors of the terms read it)");
    ZKH_REQUIRE(c->ctx == ctx, "check_bus: circuit was not loaded on this context");
    ZKH_REQUIRE(c->args, "check_bus: the circuit has no arguments (zkh_circuit_set_arguments)");
    size_t n;
    uint32_t A;
    ZKH_TRY(trace_rows("check_bus", c, po2, zk_cycles, code, data, nullptr, &n, &A));
    const std::vector<Term>& a = c->args->terms;
    const uint32_t n_terms = (uint32_t)a.size();
    ZKH_REQUIRE(!per_term || n_per_term == n_terms, "check_bus: the per-term array has %zu records, the arguments have %u terms", n_per_term, n_terms);
    // counters: at most n_terms * A adds of < 2^31 each
    ZKH_REQUIRE((uint64_t)n_terms * A < (1ull << 33), "check_bus: %u terms x %u rows could overflow a counter", n_terms, A);
    bind_thread(ctx);

    std::vector<uint32_t> table = key_term_table(a, n_terms);         // then every term's sign
    for (uint32_t i = 0; i < n_terms; i++) table[n_terms * KEY_TERM_WORDS + i] = c->args->open_tag(a[i].tag) ? BUS_SKIP : a[i].neg ? 1 : 0;
    Tmp dtab, status, slots;
    ZKH_TRY(zkh_copy_from(ctx, "bus_terms", table.data(), table.size(), dtab.out()));
    ZKH_TRY(new_buf(ctx, ST_WORDS, false, status.out()));
    const KeyTerm* d_terms = (const KeyTerm*)dtab->ptr();
    const uint32_t* d_negs = dtab->ptr() + n_terms * KEY_TERM_WORDS;
    double in_words = 0;                                              // weight + tuple words per entry, the key re-reads not counted
    for (const Term& t : a) in_words += entry_words(t);
    const unsigned rows_x = (unsigned)((A + BUS_THREADS - 1) / BUS_THREADS);

    uint64_t slots_n = 64;
    while (slots_n < 2ull * A) slots_n <<= 1;
    uint32_t st[ST_WORDS];
    for (;; slots_n <<= 1) {
        ZKH_REQUIRE(slots_n <= (1ull << 31), "check_bus: the bus has more than 2^30 distinct keys: its table would pass 2^31 slots");
        // per slot: the entry (u64), then at 2 slots_n: pos and neg (u64 each) of slot s at 2 s, 2 s + 1
        ZKH_TRY(new_buf(ctx, 6 * slots_n, false, slots.out()));
        ZKH_HIP(hipMemsetAsync(status->ptr(), 0, 4 * ST_WORDS, ctx->stream));
        ZKH_HIP(hipMemsetAsync(status->ptr() + ST_LOWEST, 0xff, 8, ctx->stream));
        ZKH_HIP(hipMemsetAsync(slots->ptr(), 0xff, 8 * slots_n, ctx->stream));
        ZKH_HIP(hipMemsetAsync(slots->ptr() + 2 * slots_n, 0, 16 * slots_n, ctx->stream));
        unsigned long long* d_slots = (unsigned long long*)slots->ptr();
        unsigned long long* d_cnt = d_slots + slots_n;
        const uint32_t mask = (uint32_t)(slots_n - 1);
        {
            ProfScope prof(ctx, "bus_build", 4.0 * in_words * A + 24.0 * slots_n);
#if ZKH_BUS_GRID_TERMS
            const dim3 grid(rows_x, n_terms);
#else
            const dim3 grid(std::min<unsigned>(rows_x, BUILD_BLOCKS), 1);
#endif
            k_bus_build<<<grid, BUS_THREADS, 0, ctx->stream>>>(code->ptr(), data->ptr(), d_terms, d_negs, n_terms, d_slots, d_cnt, mask,
                                                                (uint32_t)(slots_n / 2), (uint32_t)n, A, status->ptr());
            ZKH_TRY(last_launch_error("bus_build"));
        }
        {
            ProfScope prof(ctx, "bus_scan", 24.0 * slots_n);
            k_bus_scan<<<(unsigned)((slots_n + BUS_THREADS - 1) / BUS_THREADS), BUS_THREADS, 0, ctx->stream>>>(d_slots, d_cnt, (uint32_t)slots_n,
                                                                                                             status->ptr());
            ZKH_TRY(last_launch_error("bus_scan"));
        }
        ZKH_TRY(zkh_read(ctx, status, st, 0, ST_OVERFLOW + 1));
        if (!st[ST_OVERFLOW]) break;
    }
    *result = zkh_check_bus_result{};
    result->row = -1; result->term = -1;
    result->unbalanced_keys = st[ST_UNBALANCED]; result->distinct_keys = st[ST_KEYS]; result->slots = (uint32_t)slots_n;
    for (size_t i = 0; per_term && i < n_per_term; i++) per_term[i] = zkh_bus_term{0, NONE, NONE, 0};
    if ((st[ST_LOWEST] & st[ST_LOWEST + 1]) == NONE) return nullptr;

    const uint32_t term = st[ST_LOWEST + 1], row = st[ST_LOWEST];
    k_bus_report<<<1, 64, 0, ctx->stream>>>(code->ptr(), data->ptr(), d_terms, (const unsigned long long*)slots->ptr(),
                                            (const unsigned long long*)slots->ptr() + slots_n, (uint32_t)(slots_n - 1), (uint32_t)n, status->ptr());
    ZKH_TRY(last_launch_error("bus_report"));
    ZKH_TRY(zkh_read(ctx, status, st, 0, ST_WORDS));
    const uint64_t pos = ((uint64_t)st[ST_POS + 1] << 32) | st[ST_POS], neg = ((uint64_t)st[ST_NEG + 1] << 32) | st[ST_NEG];
    result->term = (int32_t)term; result->row = row; result->tag = a[term].tag;
    for (uint32_t e = 0; e < MAX_TUPLE; e++) result->key[e] = fp_decode(Fp::raw(st[ST_KEY + e]));
    result->net = (uint32_t)((pos % P + P - neg % P) % P);
    if (!per_term) return nullptr;

    std::vector<uint32_t> init((size_t)n_terms * TERM_OUT_WORDS, 0);
    for (uint32_t i = 0; i < n_terms; i++) init[(size_t)i * TERM_OUT_WORDS + 1] = NONE;
    Tmp out;
    ZKH_TRY(zkh_copy_from(ctx, "bus_per_term", init.data(), init.size(), out.out()));
    Key key;
    for (uint32_t e = 0; e < MAX_TUPLE; e++) key.v[e] = st[ST_KEY + e];
    {
        ProfScope prof(ctx, "bus_explain", 4.0 * in_words * A);
        k_bus_explain<<<dim3(rows_x, n_terms), BUS_THREADS, 0, ctx->stream>>>(code->ptr(), data->ptr(), d_terms, a[term].tag, key, (uint32_t)n, A,
                                                                               out->ptr());
        ZKH_TRY(last_launch_error("bus_explain"));
    }
    ZKH_TRY(zkh_read(ctx, out, init.data(), 0, init.size()));
    for (uint32_t i = 0; i < n_terms; i++) {
        const uint32_t* o = init.data() + (size_t)i * TERM_OUT_WORDS;
        if (!o[0]) continue;
        const uint64_t weight = ((uint64_t)o[5] << 32) | o[4];
        per_term[i] = zkh_bus_term{o[0], o[1], o[2], (uint32_t)(weight % P)};
    }
    return nullptr;
}
