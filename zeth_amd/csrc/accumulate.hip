// accumulate.hip — the built-in CircuitHal::accumulate for circuits whose accum group is described as DATA: lookup and
// permutation arguments as log-derivative sums (ZKA1 blob, zeth_amd/circuits/logup.py; DESIGN.md §2 ARGUMENTS).
//
//   t_i(r)  = sign_i sel_i(r) m_i(r) / (alpha - (tag_i + beta v_0(r) + ... + beta^w v_{w-1}(r)))        (Fp4)
//   S_c[r]  = sum_{r' <= r} sum_{terms i of column c} t_i(r')        on the active rows [0, A); blinding noise on [A, n)
//   bus     : sum_c S_c[A-1] = 0
//
// Three steps on the context stream:
//   (a) k_args_terms: one thread owns ARGS_BATCH rows of one accum column, interleaved by the block width so that a wave's column
//       loads are coalesced.  Per row the column's terms (at most 3) are folded into one fraction N / D; the batch's D are inverted
//       with ONE fp4_inv (Montgomery's trick) and N / D is written in place into the column's four Fp planes of `accum`;
//   (b) an inclusive prefix sum over the A active rows of all 4k Fp planes in one set of launches (the batched sibling of
//       circuit.hip's k_prefix_sum_chunks / _fp / _carry), which also leaves every plane's total;
//   (c) the blinding rows (noise_cell(GROUP_ACCUM, column, row), as k_syn_accum_store writes them).
// The host then reads back the totals and the first vanishing denominator (one sync) and refuses the witness if either is wrong:
// the accum is zeroed and an error names the row and column, or the bus total.
#include "circuit.h"

using namespace zkh;

namespace {

constexpr uint32_t ARGS_MAGIC = 0x5a4b4131u;        // 'ZKA1'
constexpr uint32_t ARGS_HEADER = 8, TERM_WORDS = 16, MAX_TUPLE = 4, MAX_TERMS = 3, NONE = 0xffffffffu;
constexpr uint32_t ARGS_THREADS = 256;
// Rows per thread.  The batch keeps D, the running product before each row and N (3 Fp4 = 12 VGPRs per row) in registers, which needs
// the batch loops fully unrolled (build.py passes a higher pragma-unroll threshold for this file; without it the arrays go to
// scratch).  hipcc -Rpass-analysis=kernel-resource-usage, no scratch in either case: 4 rows -> 68 VGPRs = 7 waves per SIMD,
// 6 rows -> 104 VGPRs = 4 waves, 8 rows -> 134 VGPRs = 3 waves (512 VGPRs per SIMD lane, allocated in steps of 8).  4 rows: one fp4_inv
// (~65 Fp products) costs ~16 products per row against ~110 for the row itself at 3 terms.
constexpr uint32_t ARGS_BATCH = 4;

// one term, prepared on the host: Montgomery words, columns resolved to (group, column)
struct ArgTerm {
    uint32_t am[4];                 // alpha - tag (Fp4)
    uint32_t w, neg, sel, mg, mc;   // tuple width; sign; selector code column or NONE; multiplicity group (NONE = 1) and column
    uint32_t tg[MAX_TUPLE], tc[MAX_TUPLE];
};
struct ArgCols { uint32_t begin, count; };
struct BetaPows { uint32_t b[MAX_TUPLE][4]; };      // beta^1 .. beta^4

__device__ __forceinline__ const uint32_t* group_ptr(const uint32_t* code, const uint32_t* data, uint32_t g) { return g == GROUP_CODE ? code : data; }
__device__ __forceinline__ bool fp4_is_zero(const Fp4& x) { return (x.c[0].v | x.c[1].v | x.c[2].v | x.c[3].v) == 0; }

// N / D of one row: the column's terms folded as N / D + f / d = (N d + f D) / (D d); rows past A give 0 / 1.  Fixed trip counts
// (MAX_TERMS, MAX_TUPLE) with guards, so that the batch arrays of the caller stay in registers.
__device__ __forceinline__ void row_fraction(const uint32_t* __restrict__ code, const uint32_t* __restrict__ data, const ArgTerm* __restrict__ terms,
                                             const ArgCols cc, const BetaPows& bp, uint32_t n, uint32_t A, uint32_t r, uint32_t c,
                                             unsigned long long* __restrict__ bad, Fp4& D, Fp4& N) {
    D = Fp4::one();
    N = Fp4::zero();
    if (r >= A) return;
#pragma unroll
    for (uint32_t i = 0; i < MAX_TERMS; i++) {
        if (i < cc.count) {
            const ArgTerm& t = terms[cc.begin + i];
            Fp4 d(Fp::raw(t.am[0]), Fp::raw(t.am[1]), Fp::raw(t.am[2]), Fp::raw(t.am[3]));
#pragma unroll
            for (uint32_t e = 0; e < MAX_TUPLE; e++) {
                if (e < t.w) {
                    const Fp v = Fp::raw(group_ptr(code, data, t.tg[e])[(size_t)t.tc[e] * n + r]);
                    const Fp4 b(Fp::raw(bp.b[e][0]), Fp::raw(bp.b[e][1]), Fp::raw(bp.b[e][2]), Fp::raw(bp.b[e][3]));
                    d = d - b * v;
                }
            }
            Fp f = Fp::one();
            if (t.sel != NONE) f = Fp::raw(code[(size_t)t.sel * n + r]);
            if (t.mg != NONE) f = f * Fp::raw(group_ptr(code, data, t.mg)[(size_t)t.mc * n + r]);
            if (t.neg) f = -f;
            if (fp4_is_zero(d)) atomicMin(bad, ((unsigned long long)r << 32) | (c << 2) | i);
            if (i == 0) { N = Fp4(f); D = d; }
            else { N = N * d + D * f; D = D * d; }
        }
    }
}

// (a) terms: grid (ceil(A / (ARGS_THREADS * ARGS_BATCH)), k)
__global__ __launch_bounds__(ARGS_THREADS) void k_args_terms(uint32_t* __restrict__ accum, const uint32_t* __restrict__ code,
                                                            const uint32_t* __restrict__ data, const ArgTerm* __restrict__ terms,
                                                            const ArgCols* __restrict__ cols, BetaPows bp, uint32_t n, uint32_t A,
                                                            unsigned long long* __restrict__ bad) {
    const uint32_t c = blockIdx.y;
    const ArgCols cc = cols[c];
    const uint32_t base = blockIdx.x * (ARGS_THREADS * ARGS_BATCH) + threadIdx.x;
    Fp4 D[ARGS_BATCH], Pre[ARGS_BATCH], N[ARGS_BATCH];
    Fp4 run = Fp4::one();
#pragma unroll
    for (uint32_t j = 0; j < ARGS_BATCH; j++) {
        row_fraction(code, data, terms, cc, bp, n, A, base + j * ARGS_THREADS, c, bad, D[j], N[j]);
        Pre[j] = run;                  // product of the batch's D before row j
        run = run * D[j];
    }
    Fp4 inv = fp4_inv(run);            // 1 / prod_j D_j (0 if some D_j vanished: that row is reported, the accum refused)
#pragma unroll
    for (uint32_t jj = 0; jj < ARGS_BATCH; jj++) {
        const uint32_t j = ARGS_BATCH - 1 - jj;
        const uint32_t r = base + j * ARGS_THREADS;
        const Fp4 t = N[j] * (inv * Pre[j]);
        inv = inv * D[j];
        if (r < A)
#pragma unroll
            for (int e = 0; e < 4; e++) accum[(size_t)(4 * c + e) * n + r] = t.c[e].v;
    }
}

// (b) batched inclusive scan over the first A words of every plane: plane = blockIdx.y, planes n words apart
__device__ __forceinline__ uint32_t block_scan_1024(uint32_t v, uint32_t (*buf)[1024]) {
    const uint32_t t = threadIdx.x;
    buf[0][t] = v;
    __syncthreads();
    int cur = 0;
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        uint32_t x = buf[cur][t];
        if (t >= d) x = add_mod(x, buf[cur][t - d]);
        buf[cur ^ 1][t] = x;
        cur ^= 1;
        __syncthreads();
    }
    return buf[cur][t];
}
__global__ __launch_bounds__(1024) void k_args_scan_chunks(uint32_t* accum, uint32_t n, uint32_t A, uint32_t* totals, uint32_t chunks) {
    __shared__ uint32_t buf[2][1024];
    uint32_t* col = accum + (size_t)blockIdx.y * n;
    const uint32_t i = blockIdx.x * 1024 + threadIdx.x;
    const uint32_t v = block_scan_1024(i < A ? col[i] : 0, buf);
    if (i < A) col[i] = v;
    if (threadIdx.x == 1023) totals[(size_t)blockIdx.y * chunks + blockIdx.x] = v;
}
// one workgroup per plane over its chunk totals; last[plane] = the plane's grand total S[A-1]
__global__ __launch_bounds__(1024) void k_args_scan_totals(uint32_t* totals, uint32_t chunks, uint32_t* last) {
    __shared__ uint32_t buf[2][1024];
    __shared__ uint32_t carry_s;
    uint32_t* col = totals + (size_t)blockIdx.y * chunks;
    const uint32_t t = threadIdx.x;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < chunks; base += 1024) {
        const uint32_t i = base + t;
        const uint32_t v = add_mod(block_scan_1024(i < chunks ? col[i] : 0, buf), carry_s);
        if (i < chunks) col[i] = v;
        __syncthreads();
        if (t == 1023) carry_s = v;
        __syncthreads();
    }
    if (t == 0) last[blockIdx.y] = carry_s;
}
__global__ __launch_bounds__(1024) void k_args_scan_carry(uint32_t* accum, uint32_t n, uint32_t A, const uint32_t* totals, uint32_t chunks) {
    const uint32_t i = blockIdx.x * 1024 + threadIdx.x;
    if (blockIdx.x == 0 || i >= A) return;
    uint32_t* col = accum + (size_t)blockIdx.y * n;
    col[i] = add_mod(col[i], totals[(size_t)blockIdx.y * chunks + blockIdx.x - 1]);
}

// (c) blinding rows [A, n) of every plane
__global__ void k_args_blind(uint32_t* accum, uint32_t n, uint32_t A, NoiseKey nk) {
    const uint32_t r = A + blockIdx.x * blockDim.x + threadIdx.x, col = blockIdx.y;
    if (r >= n) return;
    accum[(size_t)col * n + r] = noise_cell(nk, GROUP_ACCUM, col, r);
}

// Version 2: term word 7 bit 0 = "multiplicity derived by the library" (zkh_derive_multiplicities).  A derived term is (a) of sign -1,
// (b) with a data-group multiplicity column (c) that no tuple and no other term's multiplicity names, and (d) every other term of its
// tag is a lookup of sign +1.  Version 1 leaves word 7 unread.
// Version 3 adds bit 1 and its fields (validate_sorted, which has checked the word before this runs).
const char* validate_derived(const uint32_t* a, uint32_t n_terms) {
    auto term = [&](uint32_t i) { return a + ARGS_HEADER + (size_t)TERM_WORDS * i; };
    for (uint32_t i = 0; i < n_terms; i++) {
        const uint32_t* t = term(i);
        ZKH_REQUIRE(a[1] == 3 || t[7] <= 1, "set_arguments: term %u: word 7 is %u (bit 0: derived multiplicity; the other bits are reserved)", i, t[7]);
        if (!(t[7] & 1)) continue;
        ZKH_REQUIRE(t[1] == 1, "set_arguments: term %u: a derived multiplicity needs sign -1 (the table side of a lookup)", i);
        ZKH_REQUIRE(t[3] == GROUP_DATA, "set_arguments: term %u: a derived multiplicity must be a data-group column", i);
        for (uint32_t j = 0; j < n_terms; j++) {
            const uint32_t* u = term(j);
            ZKH_REQUIRE(j == i || !(u[3] == GROUP_DATA && u[4] == t[4]), "set_arguments: term %u: its derived multiplicity column (data %u) is "
                        "also the multiplicity of term %u", i, t[4], j);
            for (uint32_t e = 0; e < u[6]; e++)
                ZKH_REQUIRE(!(u[8 + 2 * e] == GROUP_DATA && u[9 + 2 * e] == t[4]), "set_arguments: term %u: its derived multiplicity column "
                            "(data %u) is read by the tuple of term %u", i, t[4], j);
            ZKH_REQUIRE(u[5] != t[5] || (u[7] & 1) || u[1] == 0, "set_arguments: term %u: term %u of its tag %u has sign -1 and is not derived "
                        "(the lookups of a derived tag have sign +1)", i, j, t[5]);
        }
    }
    return nullptr;
}

// Version 3: term word 7 bit 1 = "this term D is a sorted copy derived by the library" (zkh_derive_sorted, sort.hip) of its source term
// S (bits 16..31), by nkeys (bits 4..6) tuple positions (2 bits each from bit 8, most significant key first).  (a) D has sign -1 and no
// derived multiplicity, S is another term of sign +1 without a flag and the source of no other copy; (b) the same tag, tuple width and
// selector, both multiplicities the constant 1; (c) D's tuple columns are pairwise distinct data columns that no other tuple and no
// multiplicity names; (d) 1..3 key positions, distinct and below the width; (e) no derived multiplicity in D's tag.
const char* validate_sorted(const uint32_t* a, uint32_t n_terms) {
    auto term = [&](uint32_t i) { return a + ARGS_HEADER + (size_t)TERM_WORDS * i; };
    constexpr uint32_t MAX_SORT_KEYS = 3;
    for (uint32_t i = 0; i < n_terms; i++) {
        const uint32_t* t = term(i);
        const uint32_t f = t[7], nkeys = (f >> 4) & 7, s = f >> 16, w = t[6];
        bool reserved = (f & 0x8c) || (!(f & 2) && f > 1);
        for (uint32_t j = nkeys; j < 4; j++) reserved |= ((f >> (8 + 2 * j)) & 3) != 0;
        ZKH_REQUIRE(!reserved, "set_arguments: term %u: word 7 is %#x (bit 0: derived multiplicity; bit 1: sorted copy, with its keys in "
                    "bits 4..15 and its source term in bits 16..31; the other bits are reserved)", i, f);
        if (!(f & 2)) continue;
        ZKH_REQUIRE(t[1] == 1, "set_arguments: term %u: a sorted copy needs sign -1 (the permuted side of a multiset equality)", i);
        ZKH_REQUIRE(!(f & 1), "set_arguments: term %u: a sorted copy cannot also have a derived multiplicity", i);
        ZKH_REQUIRE(s != i && s < n_terms, "set_arguments: term %u: its source term %u is not another term of the arguments", i, s);
        const uint32_t* u = term(s);
        ZKH_REQUIRE(u[1] == 0, "set_arguments: term %u: its source term %u needs sign +1", i, s);
        ZKH_REQUIRE(u[7] == 0, "set_arguments: term %u: its source term %u is itself derived or a sorted copy", i, s);
        for (uint32_t j = 0; j < n_terms; j++)
            ZKH_REQUIRE(j == i || !(term(j)[7] & 2) || term(j)[7] >> 16 != s, "set_arguments: term %u: its source term %u is also the source of "
                        "term %u", i, s, j);
        ZKH_REQUIRE(u[5] == t[5] && u[6] == w && u[2] == t[2], "set_arguments: term %u: its source term %u has another tag, tuple width or selector", i, s);
        ZKH_REQUIRE(t[3] == NONE && u[3] == NONE, "set_arguments: term %u: a sorted copy and its source term %u have the constant multiplicity 1", i, s);
        for (uint32_t e = 0; e < w; e++) {
            const uint32_t g = t[8 + 2 * e], col = t[9 + 2 * e];
            ZKH_REQUIRE(g == GROUP_DATA, "set_arguments: term %u: tuple column (%u, %u) of a sorted copy must be a data-group column", i, g, col);
            for (uint32_t e2 = 0; e2 < e; e2++)
                ZKH_REQUIRE(t[9 + 2 * e2] != col, "set_arguments: term %u: its sorted column (data %u) appears twice in its tuple", i, col);
            for (uint32_t j = 0; j < n_terms; j++) {
                const uint32_t* x = term(j);
                for (uint32_t e2 = 0; j != i && e2 < x[6]; e2++)
                    ZKH_REQUIRE(!(x[8 + 2 * e2] == GROUP_DATA && x[9 + 2 * e2] == col), "set_arguments: term %u: its sorted column (data %u) is "
                                "read by the tuple of term %u", i, col, j);
                ZKH_REQUIRE(!(x[3] == GROUP_DATA && x[4] == col), "set_arguments: term %u: its sorted column (data %u) is the multiplicity of "
                            "term %u", i, col, j);
            }
        }
        const uint32_t kmax = w < MAX_SORT_KEYS ? w : MAX_SORT_KEYS;
        ZKH_REQUIRE(nkeys >= 1 && nkeys <= kmax, "set_arguments: term %u: %u sort keys (1..%u: at most %u, and no more than the tuple width %u)", i,
                    nkeys, kmax, MAX_SORT_KEYS, w);
        for (uint32_t j = 0; j < nkeys; j++) {
            const uint32_t pos = (f >> (8 + 2 * j)) & 3;
            bool ok = pos < w;
            for (uint32_t j2 = 0; j2 < j; j2++) ok &= ((f >> (8 + 2 * j2)) & 3) != pos;
            ZKH_REQUIRE(ok, "set_arguments: term %u: its sort key positions must be distinct and below the tuple width %u", i, w);
        }
        for (uint32_t j = 0; j < n_terms; j++)
            ZKH_REQUIRE(!((term(j)[7] & 1) && term(j)[5] == t[5]), "set_arguments: term %u: term %u of its tag %u has a derived multiplicity", i, j, t[5]);
    }
    return nullptr;
}

const char* validate_args(const zkh_circuit* c, const uint32_t* a, size_t words) {
    ZKH_REQUIRE(words >= ARGS_HEADER && a[0] == ARGS_MAGIC && a[1] >= 1 && a[1] <= 3, "set_arguments: not a ZKA1 (version 1) argument blob");
    const uint32_t k = a[2], alpha = a[3], beta = a[4], n_terms = a[5];
    ZKH_REQUIRE(words == ARGS_HEADER + (size_t)TERM_WORDS * n_terms, "set_arguments: %zu words for %u terms", words, n_terms);
    ZKH_REQUIRE(k >= 1 && 4ull * k == c->group_size[GROUP_ACCUM], "set_arguments: %u accum Fp4 columns, the circuit's accum group is %u wide",
                k, c->group_size[GROUP_ACCUM]);
    const uint32_t mix = c->global_size[GLOBAL_MIX];
    ZKH_REQUIRE((uint64_t)alpha + 4 <= mix && (uint64_t)beta + 4 <= mix, "set_arguments: alpha / beta at mix words %u / %u, the circuit has %u",
                alpha, beta, mix);
    std::vector<uint32_t> per_col(k, 0);
    uint32_t prev = 0;
    for (uint32_t i = 0; i < n_terms; i++) {
        const uint32_t* t = a + ARGS_HEADER + (size_t)TERM_WORDS * i;
        const uint32_t col = t[0], neg = t[1], sel = t[2], mg = t[3], mc = t[4], tag = t[5], w = t[6];
        ZKH_REQUIRE(col < k && col >= prev, "set_arguments: term %u: accum column %u (columns 0..%u, terms sorted by column)", i, col, k - 1);
        prev = col;
        ZKH_REQUIRE(++per_col[col] <= MAX_TERMS, "set_arguments: accum column %u has more than %u terms (the degree bound)", col, MAX_TERMS);
        ZKH_REQUIRE(neg <= 1 && tag < P, "set_arguments: term %u: sign word %u / tag %u", i, neg, tag);
        ZKH_REQUIRE(sel == NONE || sel < c->group_size[GROUP_CODE], "set_arguments: term %u: selector %u is not a code column", i, sel);
        ZKH_REQUIRE(mg == NONE || ((mg == GROUP_CODE || mg == GROUP_DATA) && mc < c->group_size[mg]),
                    "set_arguments: term %u: multiplicity column (%u, %u) is not a code or data column", i, mg, mc);
        ZKH_REQUIRE(w >= 1 && w <= MAX_TUPLE, "set_arguments: term %u: tuple width %u (1..%u)", i, w, MAX_TUPLE);
        for (uint32_t e = 0; e < w; e++) {
            const uint32_t g = t[8 + 2 * e], cc = t[9 + 2 * e];
            ZKH_REQUIRE((g == GROUP_CODE || g == GROUP_DATA) && cc < c->group_size[g], "set_arguments: term %u: tuple column (%u, %u) is not a "
                        "code or data column", i, g, cc);
        }
    }
    for (uint32_t col = 0; col < k; col++) ZKH_REQUIRE(per_col[col] >= 1, "set_arguments: accum column %u has no terms", col);
    if (a[1] == 3) ZKH_TRY(validate_sorted(a, n_terms));
    return a[1] >= 2 ? validate_derived(a, n_terms) : nullptr;
}

}  // namespace

extern "C" const char* zkh_circuit_set_arguments(zkh_circuit* c, const uint32_t* blob, size_t words) {
    ZKH_REQUIRE(c && (blob || !words), "set_arguments: null argument");
    if (!words) { c->args.clear(); return nullptr; }
    ZKH_TRY(validate_args(c, blob, words));
    c->args.assign(blob, blob + words);
    return nullptr;
}

extern "C" int zkh_circuit_has_arguments(const zkh_circuit* c) { return c && !c->args.empty(); }

extern "C" const char* zkh_accumulate(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const uint32_t* noise_key,
                                      const zkh_buf* code, const zkh_buf* data, const uint32_t* mix_global, zkh_buf* accum) {
    ZKH_REQUIRE(ctx && c && code && data && accum && mix_global, "accumulate: null argument");
    ZKH_REQUIRE(!c->args.empty(), "accumulate: the circuit has no arguments (zkh_circuit_set_arguments)");
    ZKH_REQUIRE(po2 >= 1 && po2 <= 24, "accumulate: po2 %zu out of range", po2);
    const size_t n = (size_t)1 << po2;
    ZKH_REQUIRE(zk_cycles < n, "accumulate: zk_cycles %zu leaves no active row at po2 %zu", zk_cycles, po2);
    const uint32_t* a = c->args.data();
    const uint32_t k = a[2], n_terms = a[5], A = (uint32_t)(n - zk_cycles);
    ZKH_REQUIRE(code->len == (size_t)c->group_size[GROUP_CODE] * n && data->len == (size_t)c->group_size[GROUP_DATA] * n &&
                accum->len == (size_t)4 * k * n, "accumulate: buffer shape mismatch");
    NoiseKey nk;
    ZKH_TRY(resolve_noise_key(noise_key, &nk));
    bind_thread(ctx);

    // the terms in device form: alpha - tag, beta's powers, columns resolved
    const Fp4 alpha(Fp::raw(mix_global[a[3]]), Fp::raw(mix_global[a[3] + 1]), Fp::raw(mix_global[a[3] + 2]), Fp::raw(mix_global[a[3] + 3]));
    const Fp4 beta(Fp::raw(mix_global[a[4]]), Fp::raw(mix_global[a[4] + 1]), Fp::raw(mix_global[a[4] + 2]), Fp::raw(mix_global[a[4] + 3]));
    BetaPows bp;
    Fp4 pw = beta;
    for (uint32_t e = 0; e < MAX_TUPLE; e++, pw = pw * beta)
        for (int i = 0; i < 4; i++) bp.b[e][i] = pw.c[i].v;
    std::vector<ArgTerm> terms(n_terms);
    std::vector<ArgCols> cols(k, ArgCols{0, 0});
    for (uint32_t i = 0; i < n_terms; i++) {
        const uint32_t* t = a + ARGS_HEADER + (size_t)TERM_WORDS * i;
        ArgTerm& d = terms[i];
        const Fp4 am = alpha - Fp4(fp_encode(t[5]));
        for (int e = 0; e < 4; e++) d.am[e] = am.c[e].v;
        d.w = t[6]; d.neg = t[1]; d.sel = t[2]; d.mg = t[3]; d.mc = t[4];
        for (uint32_t e = 0; e < MAX_TUPLE; e++) { d.tg[e] = e < d.w ? t[8 + 2 * e] : GROUP_DATA; d.tc[e] = e < d.w ? t[9 + 2 * e] : 0; }
        if (cols[t[0]].count == 0) cols[t[0]].begin = i;
        cols[t[0]].count++;
    }
    static_assert(sizeof(ArgTerm) % 4 == 0 && sizeof(ArgCols) % 4 == 0, "word records");
    std::vector<uint32_t> table(terms.size() * (sizeof(ArgTerm) / 4) + cols.size() * (sizeof(ArgCols) / 4));
    memcpy(table.data(), terms.data(), terms.size() * sizeof(ArgTerm));
    memcpy(table.data() + terms.size() * (sizeof(ArgTerm) / 4), cols.data(), cols.size() * sizeof(ArgCols));
    Tmp dtab, status, totals;
    ZKH_TRY(zkh_copy_from(ctx, "args_terms", table.data(), table.size(), dtab.out()));
    const uint32_t planes = 4 * k, chunks = (A + 1023) / 1024;
    ZKH_TRY(new_buf(ctx, 2 + planes, false, status.out()));          // [0, 2): first vanishing denominator (u64 key); then the plane totals
    ZKH_TRY(new_buf(ctx, (size_t)planes * chunks, false, totals.out()));
    ZKH_HIP(hipMemsetAsync(status->ptr(), 0xff, 8, ctx->stream));
    unsigned long long* bad = (unsigned long long*)status->ptr();
    const ArgTerm* d_terms = (const ArgTerm*)dtab->ptr();
    const ArgCols* d_cols = (const ArgCols*)(dtab->ptr() + terms.size() * (sizeof(ArgTerm) / 4));
    {
        // per term and row: w tuple loads + selector + multiplicity in, 16 bytes (the Fp4 term) out per column and row
        double in_words = 0;
        for (const ArgTerm& t : terms) in_words += t.w + (t.sel != NONE) + (t.mg != NONE);
        ProfScope prof(ctx, "args_terms", 4.0 * in_words * A + 16.0 * k * A);
        const unsigned bx = (unsigned)((A + ARGS_THREADS * ARGS_BATCH - 1) / (ARGS_THREADS * ARGS_BATCH));
        k_args_terms<<<dim3(bx, k), ARGS_THREADS, 0, ctx->stream>>>(accum->ptr(), code->ptr(), data->ptr(), d_terms, d_cols, bp, (uint32_t)n, A, bad);
        ZKH_TRY(last_launch_error("args_terms"));
    }
    {
        ProfScope prof(ctx, "args_scan", 4.0 * 4 * planes * (double)A);
        k_args_scan_chunks<<<dim3(chunks, planes), 1024, 0, ctx->stream>>>(accum->ptr(), (uint32_t)n, A, totals->ptr(), chunks);
        k_args_scan_totals<<<dim3(1, planes), 1024, 0, ctx->stream>>>(totals->ptr(), chunks, status->ptr() + 2);
        k_args_scan_carry<<<dim3(chunks, planes), 1024, 0, ctx->stream>>>(accum->ptr(), (uint32_t)n, A, totals->ptr(), chunks);
        ZKH_TRY(last_launch_error("args_scan"));
    }
    if (n > A) {
        ProfScope prof(ctx, "args_blind", 4.0 * planes * (double)(n - A));
        k_args_blind<<<dim3((unsigned)((n - A + 255) / 256), planes), 256, 0, ctx->stream>>>(accum->ptr(), (uint32_t)n, A, nk);
        ZKH_TRY(last_launch_error("args_blind"));
    }
    std::vector<uint32_t> st(2 + planes);
    ZKH_TRY(zkh_read(ctx, status, st.data(), 0, st.size()));
    unsigned long long key;
    memcpy(&key, st.data(), 8);
    const char* refusal = nullptr;
    if (key != ~0ull) {
        const uint32_t row = (uint32_t)(key >> 32), col = ((uint32_t)key) >> 2, term = key & 3;
        refusal = make_err("accumulate: a denominator vanishes at row %u, accum column %u (Fp columns %u..%u), term %u of the column: "
                           "the witness is refused", row, col, 4 * col, 4 * col + 3, term);
    } else {
        Fp4 tot = Fp4::zero();
        for (uint32_t col = 0; col < k; col++)
            tot += Fp4(Fp::raw(st[2 + 4 * col]), Fp::raw(st[3 + 4 * col]), Fp::raw(st[4 + 4 * col]), Fp::raw(st[5 + 4 * col]));
        if (!(tot == Fp4::zero()))
            refusal = make_err("accumulate: the bus does not balance: total (%u, %u, %u, %u) over the %u accum columns, not zero: the witness "
                               "is refused", fp_decode(tot.c[0]), fp_decode(tot.c[1]), fp_decode(tot.c[2]), fp_decode(tot.c[3]), k);
    }
    if (refusal) {                                       // no accum: the refused trace is not left behind for a seal
        (void)hipMemsetAsync(accum->ptr(), 0, accum->len * 4, ctx->stream);
        (void)hipStreamSynchronize(ctx->stream);
        return refusal;
    }
    return nullptr;
}

// ---- derived multiplicities (ZKA1 version 2; DESIGN.md §2 ARGUMENTS) ----
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
// the witness before (c): `data` is left unchanged.
namespace {

constexpr unsigned long long SLOT_EMPTY = ~0ull;
constexpr uint32_t DERIVE_THREADS = 256;
constexpr uint32_t LDS_KEYS = 4096;              // u64 counters per workgroup in the LDS path: 32 KiB
constexpr uint32_t COUNT_BLOCKS = 1024;          // workgroups of the count (4 per CU); each loops over every lookup term

struct KeyTerm {                                 // a derived or lookup term as the derive kernels read it
    uint32_t w, tag, sel, mg, mc;                // tuple width; tag (canonical); selector code column or NONE; multiplicity or NONE
    uint32_t tg[MAX_TUPLE], tc[MAX_TUPLE];
};
struct Key { uint32_t v[MAX_TUPLE]; };

__device__ __forceinline__ uint32_t cell(const uint32_t* code, const uint32_t* data, uint32_t g, uint32_t c, uint32_t n, uint32_t r) {
    return group_ptr(code, data, g)[(size_t)c * n + r] % P;
}
__device__ __forceinline__ Key read_key(const uint32_t* code, const uint32_t* data, const KeyTerm& t, uint32_t n, uint32_t r) {
    Key k;
#pragma unroll
    for (uint32_t e = 0; e < MAX_TUPLE; e++) k.v[e] = e < t.w ? cell(code, data, t.tg[e], t.tc[e], n, r) : 0;
    return k;
}
__device__ __forceinline__ uint32_t key_hash(uint32_t tag, const Key& k) {
    uint64_t h = (tag + 1) * 0x9e3779b97f4a7c15ull;
#pragma unroll
    for (uint32_t e = 0; e < MAX_TUPLE; e++) {
        h = (h ^ k.v[e]) * 0xff51afd7ed558ccdull;
        h ^= h >> 32;
    }
    return (uint32_t)h;
}
// does the entry in a slot have the key (tag, k)?  Its key is re-read from the trace.
__device__ __forceinline__ bool slot_has_key(const uint32_t* code, const uint32_t* data, const KeyTerm* terms, unsigned long long entry,
                                             uint32_t tag, const Key& k, uint32_t n) {
    const KeyTerm& o = terms[entry >> 32];
    if (o.tag != tag) return false;
    const Key ok = read_key(code, data, o, n, (uint32_t)entry);
    bool eq = true;
#pragma unroll
    for (uint32_t e = 0; e < MAX_TUPLE; e++) eq &= ok.v[e] == k.v[e];
    return eq;
}
// the slot of key (tag, k), or NONE if it has no entry (the table always has empty slots: the probe ends)
__device__ __forceinline__ uint32_t find_slot(const uint32_t* code, const uint32_t* data, const KeyTerm* terms, const unsigned long long* slots,
                                              uint32_t mask, uint32_t tag, const Key& k, uint32_t n) {
    for (uint32_t s = key_hash(tag, k) & mask;; s = (s + 1) & mask) {
        const unsigned long long cur = slots[s];
        if (cur == SLOT_EMPTY) return NONE;
        if (slot_has_key(code, data, terms, cur, tag, k, n)) return s;
    }
}
// weight of a term's row as a canonical residue: sel * m (absent = 1)
__device__ __forceinline__ uint32_t row_weight(const uint32_t* code, const uint32_t* data, const KeyTerm& t, uint32_t n, uint32_t r) {
    uint32_t w = R1;                             // Montgomery words from here on
    if (t.sel != NONE) w = cell(code, data, GROUP_CODE, t.sel, n, r);
    if (t.mg != NONE) w = mul_mod(w, cell(code, data, t.mg, t.mc, n, r));
    return fp_decode(Fp::raw(w));
}

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
        if (t.sel != NONE) {
            const uint32_t s = cell(code, data, GROUP_CODE, t.sel, n, r);
            if (s == 0) continue;
            if (s != R1) { atomicMin((unsigned long long*)(status + 2), ((unsigned long long)r << 32) | ti); continue; }
        }
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
    if (t.sel == NONE || cell(code, data, GROUP_CODE, t.sel, n, r) != 0) {
        const uint32_t s = find_slot(code, data, terms, slots, mask, t.tag, read_key(code, data, t, n, r), n);
        if (s != NONE && slots[s] == (((unsigned long long)ti << 32) | r)) out = fp_encode((uint32_t)(cnt[sid[s]] % P)).v;
    }
    data[(size_t)t.mc * n + r] = out;            // m_D is read by no term (set_arguments): no lane of this grid reads it
}

}  // namespace

extern "C" int zkh_circuit_derives_multiplicities(const zkh_circuit* c) {
    if (!c || c->args.size() < ARGS_HEADER || c->args[1] < 2) return 0;
    for (uint32_t i = 0; i < c->args[5]; i++)
        if (c->args[ARGS_HEADER + (size_t)TERM_WORDS * i + 7] & 1) return 1;
    return 0;
}

extern "C" const char* zkh_derive_multiplicities(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code,
                                                 zkh_buf* data) {
    ZKH_REQUIRE(ctx && c && data, "derive_multiplicities: null argument");
    ZKH_REQUIRE(code, "derive_multiplicities: the raw code trace is required (the keys and selectors of the terms read it)");
    ZKH_REQUIRE(zkh_circuit_derives_multiplicities(c), "derive_multiplicities: the circuit's arguments derive no multiplicity (ZKA1 version 2)");
    ZKH_REQUIRE(po2 >= 1 && po2 <= 24, "derive_multiplicities: po2 %zu out of range", po2);
    const size_t n = (size_t)1 << po2;
    ZKH_REQUIRE(zk_cycles < n, "derive_multiplicities: zk_cycles %zu leaves no active row at po2 %zu", zk_cycles, po2);
    ZKH_REQUIRE(code->len == (size_t)c->group_size[GROUP_CODE] * n && data->len == (size_t)c->group_size[GROUP_DATA] * n,
                "derive_multiplicities: buffer shape mismatch");
    const uint32_t* a = c->args.data();
    const uint32_t n_terms = a[5], A = (uint32_t)(n - zk_cycles);
    std::vector<KeyTerm> terms(n_terms);
    std::vector<uint32_t> derived, lookups, tags;
    for (uint32_t i = 0; i < n_terms; i++) {
        const uint32_t* t = a + ARGS_HEADER + (size_t)TERM_WORDS * i;
        KeyTerm& d = terms[i];
        d.w = t[6]; d.tag = t[5]; d.sel = t[2]; d.mg = t[3]; d.mc = t[4];
        for (uint32_t e = 0; e < MAX_TUPLE; e++) { d.tg[e] = e < d.w ? t[8 + 2 * e] : GROUP_DATA; d.tc[e] = e < d.w ? t[9 + 2 * e] : 0; }
        if (t[7] & 1) {
            derived.push_back(i);
            if (std::find(tags.begin(), tags.end(), t[5]) == tags.end()) tags.push_back(t[5]);
        }
    }
    for (uint32_t i = 0; i < n_terms; i++)
        if (!(a[ARGS_HEADER + (size_t)TERM_WORDS * i + 7] & 1) && std::find(tags.begin(), tags.end(), terms[i].tag) != tags.end()) lookups.push_back(i);
    // counters: at most n_lookups * A adds of < 2^31 each
    ZKH_REQUIRE((uint64_t)lookups.size() * A < (1ull << 33), "derive_multiplicities: %zu lookup terms x %u rows could overflow a counter",
                lookups.size(), A);
    uint64_t slots_n = 64;
    while (slots_n < 2ull * derived.size() * A) slots_n <<= 1;
    ZKH_REQUIRE(slots_n <= (1ull << 31), "derive_multiplicities: %zu table terms x %u rows do not fit one table", derived.size(), A);
    const uint32_t mask = (uint32_t)(slots_n - 1);
    bind_thread(ctx);

    static_assert(sizeof(KeyTerm) % 4 == 0, "word records");
    std::vector<uint32_t> table(terms.size() * (sizeof(KeyTerm) / 4) + derived.size() + lookups.size());
    memcpy(table.data(), terms.data(), terms.size() * sizeof(KeyTerm));
    uint32_t* lists = table.data() + terms.size() * (sizeof(KeyTerm) / 4);
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
    const uint32_t* d_derived = dtab->ptr() + terms.size() * (sizeof(KeyTerm) / 4);
    const uint32_t* d_lookups = d_derived + derived.size();
    unsigned long long* d_slots = (unsigned long long*)slots->ptr();
    double key_words = 0;                                             // tuple + selector words per row of the derived terms
    for (uint32_t i : derived) key_words += terms[i].w + (terms[i].sel != NONE);
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
        uint32_t w;
        ZKH_TRY(zkh_read(ctx, code, &w, (size_t)terms[term].sel * n + row, 1));
        return make_err("derive_multiplicities: table term %u (tag %u) has selector %u at row %u, not 0 or 1: the witness is refused", term,
                        terms[term].tag, fp_decode(Fp::raw(w % P)), row);
    }
    const uint32_t U = st[4];
    ZKH_TRY(new_buf(ctx, 2 * (size_t)std::max<uint32_t>(U, 1), true, cnt.out()));
    unsigned long long* d_cnt = (unsigned long long*)cnt->ptr();
    {
        double in_words = 0;                                          // weight + tuple words per lookup row, the key re-reads not counted
        for (uint32_t i : lookups) in_words += terms[i].w + (terms[i].sel != NONE) + (terms[i].mg != NONE);
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
        const KeyTerm& t = terms[term];
        uint32_t v[MAX_TUPLE] = {0, 0, 0, 0};
        for (uint32_t e = 0; e < t.w; e++) {
            ZKH_TRY(zkh_read(ctx, t.tg[e] == GROUP_CODE ? code : data, v + e, (size_t)t.tc[e] * n + row, 1));
            v[e] = fp_decode(Fp::raw(v[e] % P));
        }
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
