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
//   (b) an inclusive prefix sum over the A active rows of all 4k Fp planes in one set of launches (circuit.hip's
//       prefix_sum_planes), which also leaves every plane's total;
//   (c) the blinding rows (noise_cell(GROUP_ACCUM, column, row), as k_syn_accum_store writes them).
// The host then reads back the totals and the first vanishing denominator (one sync) and refuses the witness if either is wrong:
// the accum is zeroed and an error names the row and column, or the bus total.
//
// THE OPEN BUS (zkh_accumulate_open; a ZKA1 version-8 blob with an OPEN record): the same pass with the challenge alpha ‖ beta given by the
// caller (the seal states it in `out`, where the constraints read it) and the total RETURNED instead of compared with zero: the terms of
// the open tag are answered by another seal.  One body, `accumulate`, serves both calls.
#include "arguments.h"

using namespace zkh;

namespace {

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
    uint32_t neg;                   // sign
    TermCols c;
};
struct ArgCols { uint32_t begin, count; };
struct BetaPows { uint32_t b[MAX_TUPLE][4]; };      // beta^1 .. beta^4

__device__ __forceinline__ bool fp4_is_zero(const Fp4& x) { return (x.c[0].v | x.c[1].v | x.c[2].v | x.c[3].v) == 0; }

// N / D of one row: the column's terms folded as N / D + f / d = (N d + f D) / (D d); rows past A give 0 / 1.  Every cell is read as
// its residue (cell(): raw words >= P are legal, and neither -f nor a product takes one).  Fixed trip counts
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
                if (e < t.c.w) {
                    const Fp v = Fp::raw(cell(code, data, t.c.tg[e], t.c.tc[e], n, r));
                    const Fp4 b(Fp::raw(bp.b[e][0]), Fp::raw(bp.b[e][1]), Fp::raw(bp.b[e][2]), Fp::raw(bp.b[e][3]));
                    d = d - b * v;
                }
            }
            Fp f = Fp::one();
            if (t.c.sel != NONE) f = Fp::raw(cell(code, data, GROUP_CODE, t.c.sel, n, r));
            if (t.c.mg != NONE) f = f * Fp::raw(cell(code, data, t.c.mg, t.c.mc, n, r));
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

// (c) blinding rows [A, n) of every plane
__global__ void k_args_blind(uint32_t* accum, uint32_t n, uint32_t A, NoiseKey nk) {
    const uint32_t r = A + blockIdx.x * blockDim.x + threadIdx.x, col = blockIdx.y;
    if (r >= n) return;
    accum[(size_t)col * n + r] = noise_cell(nk, GROUP_ACCUM, col, r);
}

// both calls: alpha, beta = the two challenges as 4 Montgomery words each; total = NULL: the bus must close on zero (zkh_accumulate), else
// the 4 Montgomery words of sum_c S_c[A-1] are returned there (zkh_accumulate_open)
const char* accumulate(const char* who, zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const uint32_t* noise_key, const zkh_buf* code,
                       const zkh_buf* data, const uint32_t* alpha_words, const uint32_t* beta_words, zkh_buf* accum, uint32_t* total) {
    size_t n;
    uint32_t A;
    ZKH_TRY(trace_rows(who, c, po2, zk_cycles, code, data, accum, &n, &A));
    const Arguments& a = *c->args;
    const uint32_t k = a.k, n_terms = (uint32_t)a.terms.size();
    NoiseKey nk;
    ZKH_TRY(resolve_noise_key(noise_key, &nk));
    bind_thread(ctx);

    // the terms in device form: alpha - tag, beta's powers, columns resolved
    auto challenge = [](const uint32_t* w) { return Fp4(Fp::raw(w[0]), Fp::raw(w[1]), Fp::raw(w[2]), Fp::raw(w[3])); };
    const Fp4 alpha = challenge(alpha_words), beta = challenge(beta_words);
    BetaPows bp;
    Fp4 pw = beta;
    for (uint32_t e = 0; e < MAX_TUPLE; e++, pw = pw * beta)
        for (int i = 0; i < 4; i++) bp.b[e][i] = pw.c[i].v;
    std::vector<ArgTerm> terms(n_terms);
    std::vector<ArgCols> cols(k, ArgCols{0, 0});
    for (uint32_t i = 0; i < n_terms; i++) {
        const Term& t = a.terms[i];
        ArgTerm& d = terms[i];
        const Fp4 am = alpha - Fp4(fp_encode(t.tag));
        for (int e = 0; e < 4; e++) d.am[e] = am.c[e].v;
        d.neg = t.neg;
        d.c = term_cols(t);
        if (cols[t.col].count == 0) cols[t.col].begin = i;
        cols[t.col].count++;
    }
    static_assert(sizeof(ArgTerm) % 4 == 0 && sizeof(ArgCols) % 4 == 0, "word records");
    std::vector<uint32_t> table(terms.size() * (sizeof(ArgTerm) / 4) + cols.size() * (sizeof(ArgCols) / 4));
    memcpy(table.data(), terms.data(), terms.size() * sizeof(ArgTerm));
    memcpy(table.data() + terms.size() * (sizeof(ArgTerm) / 4), cols.data(), cols.size() * sizeof(ArgCols));
    Tmp dtab, status;
    ZKH_TRY(zkh_copy_from(ctx, "args_terms", table.data(), table.size(), dtab.out()));
    const uint32_t planes = 4 * k;
    ZKH_TRY(new_buf(ctx, 2 + planes, false, status.out()));          // [0, 2): first vanishing denominator (u64 key); then the plane totals
    ZKH_HIP(hipMemsetAsync(status->ptr(), 0xff, 8, ctx->stream));
    unsigned long long* bad = (unsigned long long*)status->ptr();
    const ArgTerm* d_terms = (const ArgTerm*)dtab->ptr();
    const ArgCols* d_cols = (const ArgCols*)(dtab->ptr() + terms.size() * (sizeof(ArgTerm) / 4));
    {
        // per term and row: w tuple loads + selector + multiplicity in, 16 bytes (the Fp4 term) out per column and row
        double in_words = 0;
        for (const Term& t : a.terms) in_words += entry_words(t);
        ProfScope prof(ctx, "args_terms", 4.0 * in_words * A + 16.0 * k * A);
        const unsigned bx = (unsigned)((A + ARGS_THREADS * ARGS_BATCH - 1) / (ARGS_THREADS * ARGS_BATCH));
        k_args_terms<<<dim3(bx, k), ARGS_THREADS, 0, ctx->stream>>>(accum->ptr(), code->ptr(), data->ptr(), d_terms, d_cols, bp, (uint32_t)n, A, bad);
        ZKH_TRY(last_launch_error("args_terms"));
    }
    {
        ProfScope prof(ctx, "args_scan", 4.0 * 4 * planes * (double)A);
        ZKH_TRY(prefix_sum_planes(ctx, "args_scan", accum->ptr(), planes, n, A, status->ptr() + 2));
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
        refusal = make_err("%s: a denominator vanishes at row %u, accum column %u (Fp columns %u..%u), term %u of the column: "
                           "the witness is refused", who, row, col, 4 * col, 4 * col + 3, term);
    } else {
        Fp4 tot = Fp4::zero();
        for (uint32_t col = 0; col < k; col++)
            tot += Fp4(Fp::raw(st[2 + 4 * col]), Fp::raw(st[3 + 4 * col]), Fp::raw(st[4 + 4 * col]), Fp::raw(st[5 + 4 * col]));
        if (total)
            for (int e = 0; e < 4; e++) total[e] = tot.c[e].v % P;
        else if (!(tot == Fp4::zero()))
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

}  // namespace

extern "C" const char* zkh_accumulate(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const uint32_t* noise_key,
                                      const zkh_buf* code, const zkh_buf* data, const uint32_t* mix_global, zkh_buf* accum) {
    ZKH_REQUIRE(ctx && c && code && data && accum && mix_global, "accumulate: null argument");
    ZKH_REQUIRE(c->args, "accumulate: the circuit has no arguments (zkh_circuit_set_arguments)");
    ZKH_REQUIRE(!c->args->is_open(), "accumulate: the arguments are an open bus (ZKA1 version 8): its total is not zero but a word of `out` (zkh_accumulate_open)");
    return accumulate("accumulate", ctx, c, po2, zk_cycles, noise_key, code, data, mix_global + c->args->alpha, mix_global + c->args->beta, accum, nullptr);
}

extern "C" const char* zkh_accumulate_open(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const uint32_t* noise_key, const zkh_buf* code,
                                           const zkh_buf* data, const uint32_t* challenge, zkh_buf* accum, uint32_t total[4]) {
    ZKH_REQUIRE(ctx && c && code && data && accum && challenge && total, "accumulate_open: null argument");
    ZKH_REQUIRE(c->args, "accumulate_open: the circuit has no arguments (zkh_circuit_set_arguments)");
    ZKH_REQUIRE(c->args->is_open(), "accumulate_open: the arguments are a closed bus (no OPEN record): its total must be zero (zkh_accumulate)");
    for (int e = 0; e < 8; e++) ZKH_REQUIRE(challenge[e] < P, "accumulate_open: challenge word %d is not a reduced element", e);
    return accumulate("accumulate_open", ctx, c, po2, zk_cycles, noise_key, code, data, challenge, challenge + 4, accum, total);
}
