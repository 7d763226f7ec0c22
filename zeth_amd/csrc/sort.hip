// sort.hip — derived sorted copies (a term's `sorted_from`, ZKA1 version 3; zeth_amd/circuits/logup.py; DESIGN.md §2 ARGUMENTS): the
// permuted side of a multiset equality, filled on the device.
//
// A pair (D, S): D the sorted copy, S its source (set_arguments has checked the rules).  r_0 < ... < r_{m-1} the active rows r < A
// with selector 1, pi the STABLE permutation that sorts them by the canonical values of S's key columns (most significant key first).
//   data[D.v_e][r_j] := raw word of S.v_e at r_pi(j)   for every tuple position e;   0 on the active rows with selector 0;
// rows [A, n) are not touched.  A selector other than 0 / 1 refuses the witness before anything is written.
//
// The device work, plain launches on the context stream, grid.y (or grid.x of the scans) = the pair, all pairs in the same launches:
//   (a) k_sort_keys   : every active row once: the selector check, the number of selected rows of every 64-row group, and per key
//                       field the OR and the AND of its canonical values.  A bit on which all keys agree (OR == AND) cannot change
//                       an order: it is dropped from the packed key, so that only LIVE bits are sorted — every digit on which all
//                       keys agree disappears (SYN-LOOKUP: addr < 2^20, time < 2^20 -> 40 bits, five byte digits);
//       k_sort_scan   : the exclusive scan of the group counts -> the rank of every selected row (the selector compaction);
//       one read-back : the bad selector, the live masks (the host sizes the key and the number of passes);
//   (b) k_sort_pack   : key = the live bits of the fields, packed (64 bits, or 96 when more are live), + the source row, at the rank;
//   (c) per 8-bit digit, least significant first (LSD; each pass is stable):
//       k_sort_hist   : digit histogram of every tile of SORT_TILE consecutive items, stored bin-major (bin, tile), and added to
//                       the pass's 256 bin totals (integer adds: the sum does not depend on their order);
//       k_sort_offsets: one workgroup per bin: the items of all smaller bins (from the totals) + the exclusive scan of its row of
//                       tile counts = where every (bin, tile) starts in the output;
//       k_sort_scatter: the tile again; a wave ranks its 64 items per round among themselves with 8 ballots (the lanes of equal
//                       digit), a per-wave LDS counter carries the rank from round to round, the four waves' counts are stacked in wave
//                       order: rank = the number of earlier items of the tile with the same digit, by construction.
//   (d) k_sort_gather : row r of rank j reads the sorted source row and copies S's tuple (coalesced writes, random reads).
// (a) .. (c) are `sort_rows` (sort.h), which zkh_derive_links (links.hip) calls as well: it ends with (packed key, source row) in stable order.
// Nothing depends on the order in which workgroups or atomics arrive (the only global atomics are OR / AND / min, which commute), and
// no workgroup waits for another: the placement of every item is a function of the keys alone.
#include "sort.h"
#include "scan.h"

#include <algorithm>

using namespace zkh;

namespace {

constexpr uint32_t SORT_THREADS = 256, SORT_WAVES = SORT_THREADS / 64;
// 8-bit digits: 256 counters per wave are 4 KiB of LDS for the block's four waves plus 4 KiB for their bases, far below what limits
// occupancy, and a wave finds its lanes of equal digit with 8 ballots; 11-bit digits would save one pass in three at 8 x the LDS and
// counters and 11 ballots.  16 items per thread: a tile of 4096 items keeps the offsets at 256 x A / 4096 counters (65536 at 2^20
// rows: one row of 256 per bin and workgroup) and the keys, source rows and ranks of a thread in 64 VGPRs.
constexpr uint32_t SORT_IPT = 16, SORT_TILE = SORT_THREADS * SORT_IPT, SORT_BINS = 256;
static_assert(SORT_BINS == SORT_THREADS, "one thread per bin in the histogram and in the stacking of the waves' counts");
constexpr uint32_t SCAN_THREADS = 1024;
constexpr uint32_t KEYS_ROUNDS = 8;                     // k_sort_keys: rows per thread

// the bits of v under mask, packed towards bit 0 in their order
__device__ __forceinline__ uint32_t extract_bits(uint32_t v, uint32_t mask) {
    uint32_t out = 0, k = 0;
    for (; mask; mask &= mask - 1, k++) out |= ((v >> (__ffs(mask) - 1)) & 1u) << k;
    return out;
}

// (a) grid (ceil(A / (SORT_THREADS * KEYS_ROUNDS)), pairs).  selcnt: groups words per pair.
// kPorts (a run holds the accesses of the k pairs from runs[run].first on: the ports of one memory, links.hip): grid (ceil(cap / ..), runs), one
// lane per VIRTUAL ROW v = row * k + port, so that the ballot compaction ranks a run's items in (row, port) order; the selector and the key
// are the port's own pair's, the counts, the rank and the OR / AND masks the run's: packed keys of different ports are comparable.
template <bool kPorts>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_keys(const uint32_t* __restrict__ code, const uint32_t* __restrict__ data,
                                                           const SortPair* __restrict__ pairs, uint32_t n, uint32_t A, uint32_t groups,
                                                           uint32_t* __restrict__ selcnt, uint32_t* __restrict__ status,
                                                           const Memory* __restrict__ runs, uint32_t cap) {
    __shared__ uint32_t red[2 * MAX_SORT_KEYS];
    const uint32_t p = blockIdx.y;
    const uint32_t first = kPorts ? runs[p].first : p, k = kPorts ? runs[p].k : 1;
    const SortPair t = pairs[first];
    if (threadIdx.x < 2 * MAX_SORT_KEYS) red[threadIdx.x] = threadIdx.x < MAX_SORT_KEYS ? 0u : ~0u;
    __syncthreads();
    uint32_t vor[MAX_SORT_KEYS] = {0, 0, 0}, vand[MAX_SORT_KEYS] = {~0u, ~0u, ~0u};
    for (uint32_t j = 0; j < KEYS_ROUNDS; j++) {
        const uint32_t at = (blockIdx.x * KEYS_ROUNDS + j) * SORT_THREADS + threadIdx.x;     // a wave = one 64-row group
        uint32_t r = at, pair = p;
        if constexpr (kPorts) { r = at / k; pair = first + (at - r * k); }
        const SortPair& u = kPorts ? pairs[pair] : t;    // the lane's pair: its port's
        const uint32_t cls = r < A ? sel_class(code, u.sel, n, r) : 0;
        if (cls == 2) atomicMin((unsigned long long*)status, ((unsigned long long)pair << 32) | r);
        const unsigned long long on = __ballot(cls == 1);
        if ((threadIdx.x & 63) == 0 && at < (kPorts ? cap : A)) selcnt[(size_t)p * groups + at / 64] = __popcll(on);
        if (cls == 1) {
#pragma unroll
            for (uint32_t f = 0; f < MAX_SORT_KEYS; f++) {
                if (f < u.nkeys) {
                    const uint32_t v = fp_decode(Fp::raw(cell(code, data, u.kg[f], u.kc[f], n, r)));
                    vor[f] |= v;
                    vand[f] &= v;
                }
            }
        }
    }
#pragma unroll
    for (uint32_t f = 0; f < MAX_SORT_KEYS; f++) {
        atomicOr(red + f, vor[f]);
        atomicAnd(red + MAX_SORT_KEYS + f, vand[f]);
    }
    __syncthreads();
    uint32_t* st = status + ST_HEAD + ST_WORDS * p;
    if (threadIdx.x < MAX_SORT_KEYS) atomicOr(st + ST_OR + threadIdx.x, red[threadIdx.x]);
    else if (threadIdx.x < 2 * MAX_SORT_KEYS) atomicAnd(st + ST_AND + threadIdx.x - MAX_SORT_KEYS, red[threadIdx.x]);
}

// exclusive scan in place of `len` counters per segment (grid.x = segment), one workgroup per segment, each thread a contiguous chunk;
// the segment's total goes to total[segment * total_stride] (if total is given)
__global__ __launch_bounds__(SCAN_THREADS) void k_sort_scan(uint32_t* __restrict__ v, uint32_t len, uint32_t* __restrict__ total, uint32_t total_stride) {
    __shared__ uint32_t buf[2][SCAN_THREADS];
    uint32_t* seg = v + (size_t)blockIdx.x * len;
    const uint32_t t = threadIdx.x, chunk = (len + SCAN_THREADS - 1) / SCAN_THREADS;
    const uint32_t lo = min(t * chunk, len), hi = min(lo + chunk, len);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += seg[i];
    const uint32_t incl = block_scan<SCAN_THREADS>(sum, buf, AddWrap());
    uint32_t run = incl - sum;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t c = seg[i];
        seg[i] = run;
        run += c;
    }
    if (total && t == SCAN_THREADS - 1) total[(size_t)blockIdx.x * total_stride] = incl;
}

// (b) grid (ceil(A / SORT_THREADS), pairs): the packed key and the source row of every selected row, at its rank.
// kPorts: grid (ceil(cap / SORT_THREADS), runs), one lane per virtual row v = row * k + port as in k_sort_keys; the item's source id is v,
// and run p's items start at p * cap.
template <bool kWide, bool kPorts>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_pack(const uint32_t* __restrict__ code, const uint32_t* __restrict__ data,
                                                           const SortPair* __restrict__ pairs, uint32_t n, uint32_t A, uint32_t groups,
                                                           const uint32_t* __restrict__ selbase, const uint32_t* __restrict__ status,
                                                           unsigned long long* __restrict__ klo, uint32_t* __restrict__ khi,
                                                           uint32_t* __restrict__ idx, const Memory* __restrict__ runs, uint32_t cap) {
    const uint32_t p = blockIdx.y;
    const uint32_t at0 = blockIdx.x * SORT_THREADS + threadIdx.x;
    uint32_t r = at0, pair = p;
    if constexpr (kPorts) {
        const uint32_t k = runs[p].k;
        r = at0 / k;
        pair = runs[p].first + (at0 - r * k);
    }
    const SortPair t = pairs[pair];
    const bool on = r < A && sel_class(code, t.sel, n, r) == 1;
    const unsigned long long mask = __ballot(on);
    if (!on) return;
    const uint32_t rank = selbase[(size_t)p * groups + at0 / 64] + __popcll(mask & ((1ull << (threadIdx.x & 63)) - 1));
    const uint32_t* st = status + ST_HEAD + ST_WORDS * p;
    unsigned long long lo = 0;
    uint32_t hi = 0;
#pragma unroll
    for (uint32_t f = 0; f < MAX_SORT_KEYS; f++) {
        if (f < t.nkeys) {
            const uint32_t live = st[ST_OR + f] & ~st[ST_AND + f];
            const uint32_t b = __popc(live);
            if (b) {                                     // (hi : lo) = (hi : lo) << b | field; b <= 31
                const uint32_t v = extract_bits(fp_decode(Fp::raw(cell(code, data, t.kg[f], t.kc[f], n, r))), live);
                if (kWide) hi = (hi << b) | (uint32_t)(lo >> (64 - b));
                lo = (lo << b) | v;
            }
        }
    }
    const size_t at = (size_t)p * (kPorts ? cap : A) + rank;
    klo[at] = lo;
    if (kWide) khi[at] = hi;
    idx[at] = at0;
}

template <bool kWide>
__device__ __forceinline__ uint32_t digit_of(unsigned long long lo, uint32_t hi, uint32_t shift) {
    return kWide && shift >= 64 ? (hi >> (shift - 64)) & (SORT_BINS - 1) : (uint32_t)(lo >> shift) & (SORT_BINS - 1);
}

// (c) grid (tiles, pairs).  hist: [pair][bin][tile]
template <bool kWide>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_hist(const unsigned long long* __restrict__ klo, const uint32_t* __restrict__ khi,
                                                           const uint32_t* __restrict__ status, uint32_t A, uint32_t tiles, uint32_t shift,
                                                           uint32_t* __restrict__ hist, uint32_t* __restrict__ totals) {
    __shared__ uint32_t h[SORT_BINS];
    const uint32_t p = blockIdx.y, m = status[ST_HEAD + ST_WORDS * p + ST_M];
    h[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)p * A;
    for (uint32_t j = 0; j < SORT_IPT; j++) {
        const uint32_t i = blockIdx.x * SORT_TILE + j * SORT_THREADS + threadIdx.x;
        if (i < m) atomicAdd(h + digit_of<kWide>(klo[base + i], kWide && shift >= 64 ? khi[base + i] : 0, shift), 1u);
    }
    __syncthreads();
    hist[((size_t)p * SORT_BINS + threadIdx.x) * tiles + blockIdx.x] = h[threadIdx.x];
    if (h[threadIdx.x]) atomicAdd(totals + p * SORT_BINS + threadIdx.x, h[threadIdx.x]);
}

// grid (SORT_BINS, pairs): hist[pair][bin][tile] := the output position of the first item of (bin, tile), in place
__global__ __launch_bounds__(SORT_THREADS) void k_sort_offsets(uint32_t* __restrict__ hist, const uint32_t* __restrict__ totals, uint32_t tiles) {
    __shared__ uint32_t buf[2][SORT_THREADS];
    __shared__ uint32_t carry;
    const uint32_t bin = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
    const uint32_t below = block_scan<SORT_THREADS>(t < bin ? totals[p * SORT_BINS + t] : 0, buf, AddWrap());
    if (t == SORT_THREADS - 1) carry = below;            // the items of all smaller bins
    __syncthreads();
    uint32_t* row = hist + ((size_t)p * SORT_BINS + bin) * tiles;
    for (uint32_t t0 = 0; t0 < tiles; t0 += SORT_THREADS) {
        const uint32_t i = t0 + t, c = i < tiles ? row[i] : 0;
        const uint32_t incl = block_scan<SORT_THREADS>(c, buf, AddWrap()), base = carry;
        if (i < tiles) row[i] = base + incl - c;
        __syncthreads();
        if (t == SORT_THREADS - 1) carry = base + incl;
        __syncthreads();
    }
}

template <bool kWide>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_scatter(const unsigned long long* __restrict__ klo_in, const uint32_t* __restrict__ khi_in,
                                                              const uint32_t* __restrict__ idx_in, unsigned long long* __restrict__ klo_out,
                                                              uint32_t* __restrict__ khi_out, uint32_t* __restrict__ idx_out,
                                                              const uint32_t* __restrict__ status, uint32_t A, uint32_t tiles, uint32_t shift,
                                                              const uint32_t* __restrict__ offs) {
    __shared__ uint32_t cnt[SORT_WAVES][SORT_BINS], start[SORT_WAVES][SORT_BINS];
    const uint32_t p = blockIdx.y, m = status[ST_HEAD + ST_WORDS * p + ST_M];
    const uint32_t tile0 = blockIdx.x * SORT_TILE;
    if (tile0 >= m) return;                              // the whole workgroup: no barrier is left behind
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (uint32_t w = 0; w < SORT_WAVES; w++) cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)p * A;
    const unsigned long long below = (1ull << lane) - 1;
    volatile uint32_t* mine = cnt[wave];
    unsigned long long lo[SORT_IPT];
    uint32_t hi[SORT_IPT], src[SORT_IPT], off[SORT_IPT];
    // a wave owns SORT_IPT * 64 consecutive items and takes them 64 at a time: item order = (wave, round, lane)
#pragma unroll
    for (uint32_t j = 0; j < SORT_IPT; j++) {
        const uint32_t i = tile0 + (wave * SORT_IPT + j) * 64 + lane;
        const bool valid = i < m;
        lo[j] = valid ? klo_in[base + i] : 0;
        hi[j] = kWide && valid ? khi_in[base + i] : 0;
        src[j] = valid ? idx_in[base + i] : 0;
        const uint32_t d = digit_of<kWide>(lo[j], hi[j], shift);
        unsigned long long peers = __ballot(valid);      // the valid lanes of this round with my digit
#pragma unroll
        for (uint32_t b = 0; b < 8; b++) {
            const unsigned long long has = __ballot(valid && ((d >> b) & 1));
            peers &= (d >> b) & 1 ? has : ~has;
        }
        const uint32_t before = __popcll(peers & below);
        const uint32_t prior = valid ? mine[d] : 0;      // the wave's earlier rounds; read by every peer before the first one adds
        if (valid && before == 0) mine[d] = prior + __popcll(peers);
        off[j] = prior + before;
    }
    __syncthreads();
    {
        const uint32_t d = threadIdx.x;
        uint32_t run = offs[((size_t)p * SORT_BINS + d) * tiles + blockIdx.x];
#pragma unroll
        for (uint32_t w = 0; w < SORT_WAVES; w++) {
            start[w][d] = run;
            run += cnt[w][d];
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < SORT_IPT; j++) {
        const uint32_t i = tile0 + (wave * SORT_IPT + j) * 64 + lane;
        if (i < m) {
            const size_t at = base + start[wave][digit_of<kWide>(lo[j], hi[j], shift)] + off[j];
            klo_out[at] = lo[j];
            if (kWide) khi_out[at] = hi[j];
            idx_out[at] = src[j];
        }
    }
}

// (d) grid (ceil(A / SORT_THREADS), pairs)
__global__ __launch_bounds__(SORT_THREADS) void k_sort_gather(const uint32_t* __restrict__ code, uint32_t* data, const SortPair* __restrict__ pairs,
                                                             uint32_t n, uint32_t A, uint32_t groups, const uint32_t* __restrict__ selbase,
                                                             const uint32_t* __restrict__ idx) {
    const uint32_t p = blockIdx.y;
    const SortPair t = pairs[p];
    const uint32_t r = blockIdx.x * SORT_THREADS + threadIdx.x;
    const bool on = r < A && sel_class(code, t.sel, n, r) == 1;
    const unsigned long long mask = __ballot(on);
    if (r >= A) return;
    uint32_t from = 0;
    if (on) from = idx[(size_t)p * A + selbase[(size_t)p * groups + r / 64] + __popcll(mask & ((1ull << (threadIdx.x & 63)) - 1))];
#pragma unroll
    for (uint32_t e = 0; e < MAX_TUPLE; e++)             // D's columns are named nowhere else (set_arguments): no lane reads them
        if (e < t.w) data[(size_t)t.dc[e] * n + r] = on ? group_ptr(code, data, t.sg[e])[(size_t)t.sc[e] * n + from] : 0;
}

}  // namespace

void zkh::scan_counters(zkh_ctx* ctx, uint32_t* v, uint32_t segments, uint32_t len, uint32_t* total, uint32_t total_stride) {
    k_sort_scan<<<segments, SCAN_THREADS, 0, ctx->stream>>>(v, len, total, total_stride);
}

// (a) .. (c) for both callers.  The launches, uploads and read-back of a call are a function of (pairs, A) and the live key bits alone.
// With `runs` (the memories of links.hip: run r holds the accesses of the runs[r].k pairs from runs[r].first on) every "pair" of the launches
// below is a run of capacity cap = kmax * A items, kmax the most ports of a run: the histogram, offsets and scatter kernels see runs of `cap`
// items where they saw pairs of A, and only the keys and the pack kernels know what a port is.  Without it cap = A and np = the pairs.
const char* zkh::sort_rows(zkh_ctx* ctx, const zkh_buf* code, const zkh_buf* data, size_t n, uint32_t A0, const std::vector<SortPair>& pairs, SortedRows* out,
                           const std::vector<Memory>* runs) {
    const uint32_t np = runs ? (uint32_t)runs->size() : (uint32_t)pairs.size();
    uint32_t kmax = 1;
    for (uint32_t r = 0; runs && r < np; r++) kmax = std::max(kmax, (*runs)[r].k);
    const uint32_t A = out->cap = kmax * A0;             // the items a run can hold (A0 <= 2^24 rows, kmax <= MAX_PORTS)
    const uint32_t groups = out->groups = (A + 63) / 64, tiles = (A + SORT_TILE - 1) / SORT_TILE;
    static_assert(sizeof(SortPair) % 4 == 0, "word records");
    Tmp &dtab = out->pairs, &status = out->status, &selcnt = out->selbase;
    ZKH_TRY(zkh_copy_from(ctx, "sort_pairs", (const uint32_t*)pairs.data(), pairs.size() * (sizeof(SortPair) / 4), dtab.out()));
    static_assert(sizeof(Memory) == 8, "word records");
    if (runs) ZKH_TRY(zkh_copy_from(ctx, "sort_runs", (const uint32_t*)runs->data(), runs->size() * 2, out->runs.out()));
    const Memory* d_runs = runs ? (const Memory*)out->runs->ptr() : nullptr;
    const size_t st_words = ST_HEAD + (size_t)ST_WORDS * np;
    std::vector<uint32_t>& st = out->st;
    st.assign(st_words, 0);
    st[0] = st[1] = ~0u;
    for (uint32_t p = 0; p < np; p++)
        for (uint32_t f = 0; f < MAX_SORT_KEYS; f++) st[ST_HEAD + ST_WORDS * p + ST_AND + f] = ~0u;
    ZKH_TRY(zkh_copy_from(ctx, "sort_status", st.data(), st.size(), status.out()));
    ZKH_TRY(new_buf(ctx, (size_t)np * groups, false, selcnt.out()));
    const SortPair* d_pairs = (const SortPair*)dtab->ptr();
    const unsigned rows_x = (unsigned)((A + SORT_THREADS - 1) / SORT_THREADS);
    double key_words = 0;                                // the ProfScope bytes count the rows read and the items a run can have, k A0, not its capacity
    for (const SortPair& q : pairs) key_words += q.nkeys + (q.sel != NONE);
    double alg_items = 0;
    for (uint32_t r = 0; r < np; r++) alg_items += (double)(runs ? (*runs)[r].k : 1) * A0;
    {
        ProfScope prof(ctx, "sort_keys", 4.0 * key_words * A0);
        const unsigned bx = (unsigned)((A + SORT_THREADS * KEYS_ROUNDS - 1) / (SORT_THREADS * KEYS_ROUNDS));
        if (runs)
            k_sort_keys<true><<<dim3(bx, np), SORT_THREADS, 0, ctx->stream>>>(code->ptr(), data->ptr(), d_pairs, (uint32_t)n, A0, groups, selcnt->ptr(), status->ptr(),
                                                                              d_runs, A);
        else
            k_sort_keys<false><<<dim3(bx, np), SORT_THREADS, 0, ctx->stream>>>(code->ptr(), data->ptr(), d_pairs, (uint32_t)n, A, groups, selcnt->ptr(), status->ptr(),
                                                                               nullptr, A);
        scan_counters(ctx, selcnt->ptr(), np, groups, status->ptr() + ST_HEAD + ST_M, ST_WORDS);
        ZKH_TRY(last_launch_error("sort_keys"));
    }
    ZKH_TRY(zkh_read(ctx, status, st.data(), 0, st.size()));
    if (st[0] != ~0u || st[1] != ~0u) {
        out->bad_selector = true;
        out->bad_pair = st[1];
        out->bad_row = st[0];
        return nullptr;
    }
    uint32_t bits = 0;                                   // the widest packed key over the pairs
    for (uint32_t p = 0; p < np; p++) {
        uint32_t b = 0;
        const uint32_t* s = st.data() + ST_HEAD + ST_WORDS * p;
        for (uint32_t f = 0; f < pairs[runs ? (*runs)[p].first : p].nkeys; f++) b += (uint32_t)__builtin_popcount(s[ST_OR + f] & ~s[ST_AND + f]);
        bits = std::max(bits, b);
    }
    const bool wide = out->wide = bits > 64;
    const uint32_t passes = (bits + 7) / 8;
    const size_t items = (size_t)np * A;
    Tmp (&klo)[2] = out->klo, (&khi)[2] = out->khi, (&idx)[2] = out->idx, &hist = out->hist, &totals = out->totals;
    for (int i = 0; i < (passes ? 2 : 1); i++) {
        ZKH_TRY(new_buf(ctx, 2 * items, false, klo[i].out()));
        ZKH_TRY(new_buf(ctx, wide ? items : 1, false, khi[i].out()));
        ZKH_TRY(new_buf(ctx, items, false, idx[i].out()));
    }
    auto lo_of = [&](int i) { return (unsigned long long*)klo[i]->ptr(); };
    {
        ProfScope prof(ctx, "sort_pack", 4.0 * key_words * A0 + (wide ? 16.0 : 12.0) * alg_items);
        auto pack = [&](auto* kernel, uint32_t rows) {
            kernel<<<dim3(rows_x, np), SORT_THREADS, 0, ctx->stream>>>(code->ptr(), data->ptr(), d_pairs, (uint32_t)n, rows, groups, selcnt->ptr(), status->ptr(), lo_of(0),
                                                                      khi[0]->ptr(), idx[0]->ptr(), d_runs, A);
        };
        if (runs) pack(wide ? k_sort_pack<true, true> : k_sort_pack<false, true>, A0);
        else pack(wide ? k_sort_pack<true, false> : k_sort_pack<false, false>, A);
        ZKH_TRY(last_launch_error("sort_pack"));
    }
    int cur = 0;
    if (passes) {
        ZKH_TRY(new_buf(ctx, (size_t)np * SORT_BINS * tiles, false, hist.out()));
        ZKH_TRY(new_buf(ctx, (size_t)passes * np * SORT_BINS, true, totals.out()));       // the bin totals of every pass, zeroed once
        // per pass: the items read twice and written once, the counters written, scanned and read
        ProfScope prof(ctx, "sort_passes", passes * (3.0 * (wide ? 16.0 : 12.0) * alg_items + 16.0 * np * SORT_BINS * tiles));
        for (uint32_t d = 0; d < passes; d++, cur ^= 1) {
            const dim3 grid(tiles, np);
            uint32_t* tot = totals->ptr() + (size_t)d * np * SORT_BINS;
            if (wide) {
                k_sort_hist<true><<<grid, SORT_THREADS, 0, ctx->stream>>>(lo_of(cur), khi[cur]->ptr(), status->ptr(), A, tiles, 8 * d, hist->ptr(), tot);
                k_sort_offsets<<<dim3(SORT_BINS, np), SORT_THREADS, 0, ctx->stream>>>(hist->ptr(), tot, tiles);
                k_sort_scatter<true><<<grid, SORT_THREADS, 0, ctx->stream>>>(lo_of(cur), khi[cur]->ptr(), idx[cur]->ptr(), lo_of(cur ^ 1), khi[cur ^ 1]->ptr(),
                                                                           idx[cur ^ 1]->ptr(), status->ptr(), A, tiles, 8 * d, hist->ptr());
            } else {
                k_sort_hist<false><<<grid, SORT_THREADS, 0, ctx->stream>>>(lo_of(cur), khi[cur]->ptr(), status->ptr(), A, tiles, 8 * d, hist->ptr(), tot);
                k_sort_offsets<<<dim3(SORT_BINS, np), SORT_THREADS, 0, ctx->stream>>>(hist->ptr(), tot, tiles);
                k_sort_scatter<false><<<grid, SORT_THREADS, 0, ctx->stream>>>(lo_of(cur), khi[cur]->ptr(), idx[cur]->ptr(), lo_of(cur ^ 1), khi[cur ^ 1]->ptr(),
                                                                            idx[cur ^ 1]->ptr(), status->ptr(), A, tiles, 8 * d, hist->ptr());
            }
        }
        ZKH_TRY(last_launch_error("sort_passes"));
    }
    out->cur = cur;
    return nullptr;
}

extern "C" const char* zkh_derive_sorted(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data) {
    ZKH_REQUIRE(ctx && c && data, "derive_sorted: null argument");
    ZKH_REQUIRE(code, "derive_sorted: the raw code trace is required (the selectors and code-group source columns of the terms read it)");
    ZKH_REQUIRE(zkh_circuit_derives_sorted(c), "derive_sorted: the circuit's arguments derive no sorted copy (ZKA1 version 3)");
    size_t n;
    uint32_t A;
    ZKH_TRY(trace_rows("derive_sorted", c, po2, zk_cycles, code, data, nullptr, &n, &A));
    const std::vector<Term>& a = c->args->terms;
    std::vector<SortPair> pairs;
    for (uint32_t i = 0; i < a.size(); i++) {
        if (!a[i].sorted) continue;
        const TermCols d = term_cols(a[i]), s = term_cols(a[a[i].sorted_from]);
        SortPair q{};
        q.d_term = i; q.w = d.w; q.nkeys = a[i].nkeys; q.sel = d.sel;
        for (uint32_t f = 0; f < MAX_SORT_KEYS; f++) {
            const uint32_t pos = f < q.nkeys ? a[i].key[f] : 0;
            q.kg[f] = s.tg[pos]; q.kc[f] = s.tc[pos];
        }
        for (uint32_t e = 0; e < MAX_TUPLE; e++) { q.sg[e] = s.tg[e]; q.sc[e] = s.tc[e]; q.dc[e] = d.tc[e]; }
        pairs.push_back(q);
    }
    const uint32_t np = (uint32_t)pairs.size();
    ZKH_REQUIRE(np <= 65535, "derive_sorted: %u sorted copies in one blob (at most 65535)", np);
    bind_thread(ctx);
    SortedRows sorted;
    ZKH_TRY(sort_rows(ctx, code, data, n, A, pairs, &sorted));
    if (sorted.bad_selector) {
        const SortPair& q = pairs[sorted.bad_pair];
        const uint32_t row = sorted.bad_row;
        uint32_t sel;
        ZKH_TRY(read_cell(ctx, code, data, GROUP_CODE, q.sel, n, row, &sel));
        return make_err("derive_sorted: sorted-copy term %u (tag %u) has selector %u at row %u, not 0 or 1: the witness is refused", q.d_term,
                        a[q.d_term].tag, sel, row);
    }
    double tuple_words = 0;
    for (const SortPair& q : pairs) tuple_words += q.w;
    {
        ProfScope prof(ctx, "sort_gather", 4.0 * (size_t)np * A + 8.0 * tuple_words * A);
        k_sort_gather<<<dim3((unsigned)((A + SORT_THREADS - 1) / SORT_THREADS), np), SORT_THREADS, 0, ctx->stream>>>(
            code->ptr(), data->ptr(), sorted.d_pairs(), (uint32_t)n, A, sorted.groups, sorted.selbase->ptr(), sorted.rows());
        ZKH_TRY(last_launch_error("sort_gather"));
    }
    // the temporaries go back to the pool on return: the stream orders their next use after these launches
    return nullptr;
}
