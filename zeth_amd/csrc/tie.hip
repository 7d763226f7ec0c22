// tie.hip — THE TABLE'S FINGERPRINT (zkh_table_fingerprint; host twin: zeth_amd/circuits/logup.py table_fingerprint; DESIGN.md §2 "THE TIE"):
//
//   F = sum_{i < D} 1 / (alpha - (tag + beta a_i + beta^2 in_i + beta^3 out_i))        (Fp4, tag = TIE_TAG = 2)
//
// over the D rows (a_i, in_i, out_i) of a page table where a ZKU1 proof holds it (zku1.h: three words a row, the address an integer, in
// and out Montgomery words).  It is what the open total of a tied paging segment's seal (SYN-LOOKUP-tied: + p_on (p_addr, p_in, p_out))
// must be, and minus what the totals of the P2-PAGE-tied parts of its page-out add up to.  A rank that holds the proof and not the
// segment's trace learns from it what the parts must sum to, and the prover refuses a proof whose table is not the segment's before a
// part is sealed on it (prover.seal_tied).
//
// Two launches, no atomics, one read-back:
//   k_tie_rows  : a lane owns TIE_BATCH rows, interleaved by the block width so that a wave reads consecutive rows.  The rows'
//                 denominators are inverted with ONE fp4_inv (prefix products and back-substitution, as accumulate.hip's k_args_terms
//                 batches) and summed in the lane; the workgroup reduces the lanes' sums and the lowest row whose denominator vanishes
//                 in LDS and writes one record of 5 words: the partial sum, that row (NONE: none).
//   k_tie_total : ONE workgroup sums the workgroups' records the same way into the call's record, which the host reads back.
// Field sums are exact, so the result is the same bit for bit whatever the order.  A row past D is 0 / 1: it adds nothing.
#include "arguments.h"
#include "zku1.h"

using namespace zkh;

namespace {

constexpr uint32_t TIE_THREADS = 256, TIE_BATCH = 4, TIE_TAG = 2;
constexpr uint32_t TIE_RECORD = 5;                  // a partial sum (4 Montgomery words) and the lowest vanishing row
struct TieChallenge { uint32_t am[4]; uint32_t b[3][4]; };     // alpha - tag; beta, beta^2, beta^3

// the workgroup's reduction: the lanes' (sum, bad) -> lane 0's, in LDS; every lane must call it
__device__ __forceinline__ void tie_reduce(Fp4& sum, uint32_t& bad, uint32_t (&s)[4][TIE_THREADS], uint32_t (&low)[TIE_THREADS]) {
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (int e = 0; e < 4; e++) s[e][t] = sum.c[e].v;
    low[t] = bad;
    __syncthreads();
    for (uint32_t w = TIE_THREADS / 2; w; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int e = 0; e < 4; e++) s[e][t] = add_mod(s[e][t], s[e][t + w]);
            low[t] = low[t] < low[t + w] ? low[t] : low[t + w];
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < 4; e++) sum.c[e] = Fp::raw(s[e][0]);
    bad = low[0];
}

// grid ceil(D / (TIE_THREADS * TIE_BATCH)); `table` = the first of the 3 D words; D < 2^31 (the host checks that they lie in the buffer)
__global__ __launch_bounds__(TIE_THREADS) void k_tie_rows(const uint32_t* __restrict__ table, uint32_t D, TieChallenge ch, uint32_t* __restrict__ partial) {
    __shared__ uint32_t s[4][TIE_THREADS];
    __shared__ uint32_t low[TIE_THREADS];
    const uint32_t base = blockIdx.x * (TIE_THREADS * TIE_BATCH) + threadIdx.x;
    const Fp4 am(Fp::raw(ch.am[0]), Fp::raw(ch.am[1]), Fp::raw(ch.am[2]), Fp::raw(ch.am[3]));
    Fp4 den[TIE_BATCH], pre[TIE_BATCH];
    Fp4 run = Fp4::one();
    uint32_t bad = NONE;
#pragma unroll
    for (uint32_t j = 0; j < TIE_BATCH; j++) {
        const uint32_t r = base + j * TIE_THREADS;                          // < 2^31 + 2^10: no wrap
        Fp4 d = Fp4::one();
        if (r < D) {
            const uint32_t* row = table_row(table, r);
            const Fp v[3] = {fp_encode(row[ROW_ADDR]), Fp::raw(row[ROW_IN] % P), Fp::raw(row[ROW_OUT] % P)};
            d = am;
#pragma unroll
            for (int e = 0; e < 3; e++) d = d - Fp4(Fp::raw(ch.b[e][0]), Fp::raw(ch.b[e][1]), Fp::raw(ch.b[e][2]), Fp::raw(ch.b[e][3])) * v[e];
            if ((d.c[0].v | d.c[1].v | d.c[2].v | d.c[3].v) == 0 && bad == NONE) bad = r;      // rows ascend with j: the lane's lowest
        }
        den[j] = d;
        pre[j] = run;                                                       // the product of the batch's denominators before row j
        run = run * d;
    }
    Fp4 inv = fp4_inv(run);                                                 // 0 if a denominator vanished: that row is reported, the sum refused
    Fp4 sum = Fp4::zero();
#pragma unroll
    for (uint32_t jj = 0; jj < TIE_BATCH; jj++) {
        const uint32_t j = TIE_BATCH - 1 - jj;
        if (base + j * TIE_THREADS < D) sum += inv * pre[j];
        inv = inv * den[j];
    }
    tie_reduce(sum, bad, s, low);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int e = 0; e < 4; e++) partial[(size_t)TIE_RECORD * blockIdx.x + e] = sum.c[e].v;
        partial[(size_t)TIE_RECORD * blockIdx.x + 4] = bad;
    }
}

// ONE workgroup: the `blocks` records of k_tie_rows -> record[5]
__global__ __launch_bounds__(TIE_THREADS) void k_tie_total(const uint32_t* __restrict__ partial, uint32_t blocks, uint32_t* __restrict__ record) {
    __shared__ uint32_t s[4][TIE_THREADS];
    __shared__ uint32_t low[TIE_THREADS];
    Fp4 sum = Fp4::zero();
    uint32_t bad = NONE;
    for (uint32_t i = threadIdx.x; i < blocks; i += TIE_THREADS) {
        const uint32_t* p = partial + (size_t)TIE_RECORD * i;
        sum += Fp4(Fp::raw(p[0]), Fp::raw(p[1]), Fp::raw(p[2]), Fp::raw(p[3]));
        bad = p[4] < bad ? p[4] : bad;
    }
    tie_reduce(sum, bad, s, low);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int e = 0; e < 4; e++) record[e] = sum.c[e].v;
        record[4] = bad;
    }
}

}  // namespace

extern "C" const char* zkh_table_fingerprint(zkh_ctx* ctx, const zkh_buf* table, size_t table_at, size_t D, const uint32_t* challenge, uint32_t total[4]) {
    ZKH_REQUIRE(ctx && table && challenge && total, "table_fingerprint: null argument");
    ZKH_REQUIRE(D < ((size_t)1 << 31) && table_at <= table->len && (size_t)PROOF_ROW * D <= table->len - table_at,
                "table_fingerprint: a table of %zu rows at word %zu does not lie in a buffer of %zu words", D, table_at, table->len);
    for (int e = 0; e < 8; e++) ZKH_REQUIRE(challenge[e] < P, "table_fingerprint: challenge word %d is not a reduced element", e);
    for (int e = 0; e < 4; e++) total[e] = 0;
    if (!D) return nullptr;
    bind_thread(ctx);
    auto word4 = [](const uint32_t* w) { return Fp4(Fp::raw(w[0]), Fp::raw(w[1]), Fp::raw(w[2]), Fp::raw(w[3])); };
    const Fp4 alpha = word4(challenge), beta = word4(challenge + 4), am = alpha - Fp4(fp_encode(TIE_TAG));
    TieChallenge ch;
    Fp4 pw = beta;
    for (int e = 0; e < 3; e++, pw = pw * beta)
        for (int i = 0; i < 4; i++) ch.b[e][i] = pw.c[i].v;
    for (int i = 0; i < 4; i++) ch.am[i] = am.c[i].v;
    const uint32_t blocks = (uint32_t)((D + TIE_THREADS * TIE_BATCH - 1) / (TIE_THREADS * TIE_BATCH));
    Tmp partial;
    ZKH_TRY(new_buf(ctx, (size_t)TIE_RECORD * (blocks + 1), false, partial.out()));       // the workgroups' records, then the call's
    uint32_t* record = partial->ptr() + (size_t)TIE_RECORD * blocks;
    {
        ProfScope prof(ctx, "tie_rows", 4.0 * PROOF_ROW * (double)D + 4.0 * TIE_RECORD * blocks);
        k_tie_rows<<<blocks, TIE_THREADS, 0, ctx->stream>>>(table->ptr() + table_at, (uint32_t)D, ch, partial->ptr());
        ZKH_TRY(last_launch_error("tie_rows"));
    }
    {
        ProfScope prof(ctx, "tie_total", 4.0 * TIE_RECORD * (blocks + 1));
        k_tie_total<<<1, TIE_THREADS, 0, ctx->stream>>>(partial->ptr(), blocks, record);
        ZKH_TRY(last_launch_error("tie_total"));
    }
    uint32_t r[TIE_RECORD];
    ZKH_TRY(zkh_read(ctx, partial, r, (size_t)TIE_RECORD * blocks, TIE_RECORD));
    ZKH_REQUIRE(r[4] == NONE, "table_fingerprint: the denominator of row %u vanishes under this challenge: the table is refused", r[4]);
    memcpy(total, r, 16);
    return nullptr;
}
