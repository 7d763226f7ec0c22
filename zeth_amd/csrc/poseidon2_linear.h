// poseidon2_linear.h — the 21 partial rounds of poseidon2.h as ONE affine map applied through int8 matrix products.
// Included by poseidon2.h (which lays out everything this file builds on); include that, not this.
//
// Cells 1..23 never meet an s-box.  With z_r the s-box output of partial round r, the s-box inputs are
//   u_0 = x_0,   u_r = alpha_r . x[1..23] + sum_{j<r} beta_rj z_j + kappa_r,
// and the state after round 21 is  x' = Gamma x[1..23] + Delta z + kappa'.  All of alpha, beta, Gamma, Delta, kappa are
// constants of (diag, round constants): the builder pushes symbolic unit vectors through the literal round.
//
// A constant matrix applied to 64 states at once is an int8 GEMM over byte digits (v_mfma_i32_32x32x32_i8 on gfx950):
//   state word w, |w| < 2^31:  w ^ 0x00808080 has four SIGNED bytes s_b with  w = sum_b s_b 2^(8b) + 0x808080;
//   constant c in (-P/2, P/2):  four balanced digits in [-128, 127];
//   matrix row (o, i), column (c, b) = digit_i(M[o,c] 2^(8b) mod P), so that  sum_i 2^(8i) r_(o,i) = sum_c M[o,c] w_c  (mod P)
// once 0x808080 sum_c M[o,c] is folded into the constant column (the K position after cell 23 holds the byte 1).
// |r| < 2^21, so lo = r_0 + (r_1 << 8) and hi = r_2 + (r_3 << 8) are 32-bit words and  lo R + hi (2^16 R)  is one signed
// 64-bit sum, reduced once.  Every scale of poseidon2.h's chain is a field factor of a row or a column and sits in the
// digits: the entry scale R^-2800 (columns of x), z_0's scale (u_0 is the raw entry word, its s-box output a known power),
// the exit scale sigma (rows of Gamma, Delta), F64_OFF (constant column), the partial rounds' constants (kappa) and the
// constants of the full round that follows (kappa' = sigma (kappa' + rc): that round's s-boxes add a zero row).
// The beta terms stay on the VALU: they are the serial chain.
//
// Table (uint32 words): A fragments of the first product (alpha: 3 row tiles x 3 k-steps), of the second (Gamma | Delta:
// 3 row tiles x 6 k-steps), each 64 lanes x 16 bytes in the order the kernel walks them; beta (triangular, centred, times R);
// three scalars; the eight full rounds' constant rows with the fifth zeroed.
#pragma once
#if !defined(ZKH_POSEIDON2_H_PARTS)
#error "include poseidon2.h"
#endif

namespace zkh {

constexpr int LIN_ALPHA = PARTIAL - 1;                   // rows u_1 .. u_20
constexpr int LIN_POS = 24;                              // K positions (words) per operand block: 23 cells + the constant; 21 z + 3 unused
constexpr int LIN_KS = 3;                                // k-steps per operand block (8 words = 32 bytes each)
constexpr int LIN_TILES = 3;                             // row tiles (8 outputs x 4 digits each) of either product
constexpr int LIN_FRAG = 256;                            // words per A fragment
constexpr int LIN_A1 = 0, LIN_A2 = LIN_A1 + LIN_TILES * LIN_KS * LIN_FRAG, LIN_BETA = LIN_A2 + LIN_TILES * 2 * LIN_KS * LIN_FRAG,
              LIN_BETA_WORDS = LIN_ALPHA * (LIN_ALPHA + 1) / 2, LIN_SCALARS = LIN_BETA + LIN_BETA_WORDS, LIN_RCF = LIN_SCALARS + 4,
              LIN_WORDS = LIN_RCF + 2 * HALF_FULL * CELLS;
constexpr uint32_t LIN_XOR = 0x00808080u;                // makes bytes 0..2 of a word signed; the word is then sum s_b 2^(8b) + LIN_XOR
constexpr int64_t LIN_DOMAIN = (int64_t)P << 31;         // smont_reduce: |t| < P 2^31

// row of a tile that holds digit i of the tile's output o (o < 8): what one half-wave swap of an accumulator pair gathers
ZKH_HD int lin_row(int o, int i) { return 8 * (o >> 1) + 4 * (o & 1) + i; }
// word and byte of the table that hold the digit at (row, k) of product `second` (row < 96; k < 96 or 192): lane l of a
// fragment holds bytes k = 16 (l >> 5) + 0..15 of row l & 31
ZKH_HD int lin_digit_at(int second, int row, int k, int* byte) {
    const int ks = second ? 2 * LIN_KS : LIN_KS, frag = (row >> 5) * ks + (k >> 5), kk = k & 31, lane = (row & 31) + 32 * (kk >> 4);
    *byte = kk & 3;
    return (second ? LIN_A2 : LIN_A1) + (frag * 64 + lane) * 4 + ((kk & 15) >> 2);
}
ZKH_HD int lin_digit(const uint32_t* t, int second, int row, int k) {
    int b;
    const uint32_t w = t[lin_digit_at(second, row, k, &b)];
    return (int)(int8_t)(w >> (8 * b));
}
ZKH_HD int lin_beta_at(int r, int j) { return LIN_BETA + (r - 1) * r / 2 + j; }         // 1 <= r <= 20, j < r

// x^7 / R^6 of a signed operand |u| <= P + 64, in (-P, P)
ZKH_HD int32_t lin_sbox(int32_t u) {
    const int32_t x2 = smont(u, u), x3 = smont(x2, u), x4 = smont(x2, x2);
    return smont(x3, x4);
}
ZKH_HD int64_t mul_i64_k(int32_t a, int32_t b_uniform) {
#if defined(__HIP_DEVICE_COMPILE__)
    int64_t d; uint64_t carry;
    asm("v_mad_i64_i32 %0, %1, %2, %3, 0" : "=v"(d), "=s"(carry) : "v"(a), "s"(b_uniform));
    return d;
#else
    return (int64_t)a * b_uniform;
#endif
}
// the four digit sums of one output -> lo R + hi 2^16 R  (c0 = R, c1 = centred 2^16 R)
ZKH_HD int64_t lin_recombine(int32_t r0, int32_t r1, int32_t r2, int32_t r3, int32_t c0, int32_t c1) {
    const int32_t lo = (int32_t)((uint32_t)r0 + ((uint32_t)r1 << 8)), hi = (int32_t)((uint32_t)r2 + ((uint32_t)r3 << 8));
    return mad_i64_k(lo, c0, mul_i64_k(hi, c1));
}
// The serial chain.  A signed 64-bit sum takes four
// products z beta (|z| < P, |beta| <= (P-1)/2: 2 P^2 < 2^63) on top of a folded sum (< 2^59.1), and is folded (hi R + lo) before
// the fifth; it is folded before the reduction when it holds two or more (one product on a folded sum stays inside P 2^31).
// The builder checks exactly this schedule against the table's own beta.
ZKH_HD bool lin_fold_before(int n) { return n == 4; }
ZKH_HD bool lin_fold_last(int n) { return n >= 2; }
struct LinStats { int64_t acc = 0, lo = 0, t = 0, out = 0; };      // largest |digit sum|, |lo| or |hi|, |reduced sum|, |output word|
// row r of beta (r words), requested: the wait is wherever its first word is read (poseidon2.h's p2_request_here keeps the request here)
ZKH_HD void lin_beta_row(int r, uint32_t (&beta)[LIN_ALPHA], const uint32_t* __restrict__ lin) {
#pragma unroll
    for (int j = 0; j < LIN_ALPHA; j++)
        if (j < r) beta[j] = lin[lin_beta_at(r, j)];
    p2_request_here();
}
// round r >= 1: z[r] from row alpha_r's recombined sum t and z[0..r).  beta[r % 3] holds row r.  Rows 1..3 are requested ahead of the
// chain (lin_beta_first); round r >= 3 requests row r + 1 behind its first product, into the buffer row r - 2 has left.  Where, and why:
//   - scalar loads return out of order, so every wait for one is a wait for all of them: a request ahead of the first read of row r
//     would be waited for together with row r, at once;
//   - the products of round r + 1 that do not read z[r] issue under round r's reduction and s-box, so row r + 1 is first read right
//     behind round r's last product: a request there would be waited for at once as well.
// Between the two lie round r's other r - 1 products.
ZKH_HD void lin_beta_first(uint32_t (&beta)[3][LIN_ALPHA], const uint32_t* __restrict__ lin) {
    lin_beta_row(1, beta[1], lin); lin_beta_row(2, beta[2], lin); lin_beta_row(3, beta[0], lin);
}
ZKH_HD void lin_chain_round(int r, int64_t t, int32_t (&z)[PARTIAL], uint32_t (&beta)[3][LIN_ALPHA], const uint32_t* __restrict__ lin, LinStats* st) {
    int64_t acc = t;
    int n = 0;
#pragma unroll
    for (int j = 0; j < PARTIAL - 1; j++)
        if (j < r) {
            if (lin_fold_before(n)) { acc = fold_acc_s(acc); n = 0; }
            acc = mad_i64_k(z[j], (int32_t)beta[r % 3][j], acc);
            n++;
            if (j == 0 && r >= 3 && r < LIN_ALPHA) lin_beta_row(r + 1, beta[(r + 1) % 3], lin);
        }
    if (lin_fold_last(n)) acc = fold_acc_s(acc);
#if !defined(__HIP_DEVICE_COMPILE__)
    if (st) { const int64_t a = acc < 0 ? -acc : acc; if (a > st->t) st->t = a; }
#endif
    (void)st;
    z[r] = lin_sbox(smont_reduce(acc));
}

#if defined(__HIP_DEVICE_COMPILE__)
typedef int lin_v4 __attribute__((ext_vector_type(4)));
typedef int lin_v16 __attribute__((ext_vector_type(16)));
// a's upper half-wave <-> b's lower half-wave: afterwards a = [a.lo, b.lo], b = [a.hi, b.hi]
__device__ __forceinline__ void lin_swap(uint32_t& a, uint32_t& b) {
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0]; b = r[1];
}
// B operands of both column tiles (permutations 0..31 and 32..63 of the wave) from each lane's own words (eight per k-step): after the swaps
// v[8 ks + j] is register j of tile 0's k-step ks and v[8 ks + 4 + j] register j of tile 1's
template <int NPOS>
__device__ __forceinline__ void lin_operands(uint32_t (&v)[NPOS]) {
#pragma unroll
    for (int ks = 0; ks < NPOS / 8; ks++)
#pragma unroll
        for (int j = 0; j < 4; j++) lin_swap(v[8 * ks + j], v[8 * ks + 4 + j]);
}
template <int NPOS>
__device__ __forceinline__ lin_v4 lin_b(const uint32_t (&v)[NPOS], int ks, int tile) {
    lin_v4 b;
    b[0] = (int)v[8 * ks + 4 * tile]; b[1] = (int)v[8 * ks + 4 * tile + 1]; b[2] = (int)v[8 * ks + 4 * tile + 2]; b[3] = (int)v[8 * ks + 4 * tile + 3];
    return b;
}
// A fragment f of the table, this lane's 16 bytes.  The address is (uniform base of f's group of four) + (lane's 32-bit offset) +
// (immediate below 4 KiB): one VGPR for all 27 fragments.  Left to itself the compiler keeps a 64-bit per-lane pointer for every
// 4 KiB of the table; the opaque scalar offset keeps the base in scalar registers (the pointer itself stays a global one).
__device__ __forceinline__ lin_v4 lin_frag(const uint32_t* __restrict__ lin, int f, uint32_t lane16) {
    uint32_t group = (uint32_t)(f & ~3) * LIN_FRAG * 4;
    asm("" : "+s"(group));
    return *(const lin_v4*)((const char*)lin + group + (uint32_t)(f & 3) * LIN_FRAG * 4 + lane16);
}
// After two column tiles' products every lane gathers rows of its OWN permutation: the swap of accumulator register 4 g + i of the
// pair brings digit sum i of the tile's outputs 2 g (first) and 2 g + 1 (second).  Returns both recombined sums.
__device__ __forceinline__ void lin_gather2(int64_t& t0, int64_t& t1, const lin_v16& c0, const lin_v16& c1, int g, int32_t k0, int32_t k1) {
    uint32_t a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { a[i] = (uint32_t)c0[4 * g + i]; b[i] = (uint32_t)c1[4 * g + i]; lin_swap(a[i], b[i]); }
    t0 = lin_recombine((int32_t)a[0], (int32_t)a[1], (int32_t)a[2], (int32_t)a[3], k0, k1);
    t1 = lin_recombine((int32_t)b[0], (int32_t)b[1], (int32_t)b[2], (int32_t)b[3], k0, k1);
}
#endif

// The partial rounds.  In: s as the fourth full round leaves it (nearly centred words at the entry scale, + F64_OFF).  Out: every
// cell as the signed s-box operand of the fifth full round, |.| < P (that round adds no constants: the row of lin + LIN_RCF that
// would be its own is zero, and poseidon2_mix_core does not load it).
// On the device a whole wave must arrive here together.  The host form is the model of it: same digits, same bytes, same
// recombination and chain, the tile products as plain int32 loops.
ZKH_HD void poseidon2_partial_linear(uint32_t (&s)[CELLS], const uint32_t* __restrict__ lin, LinStats* st = nullptr) {
    const int32_t c0 = (int32_t)lin[LIN_SCALARS], c1 = (int32_t)lin[LIN_SCALARS + 1];
    const int32_t u0 = (int32_t)(s[0] + lin[LIN_SCALARS + 2]);
    uint32_t vx[LIN_POS], vz[LIN_POS];
#pragma unroll
    for (int q = 0; q < CELLS - 1; q++) vx[q] = s[q + 1] ^ LIN_XOR;
    vx[CELLS - 1] = 1u;
    int32_t z[PARTIAL];
    uint32_t beta[3][LIN_ALPHA];                           // rows of beta in flight (lin_chain_round)
#if defined(__HIP_DEVICE_COMPILE__)
    // Table data is requested ahead of its use, in source order (hash.hip is built without the machine scheduler): the A fragments
    // are double-buffered, the next one requested before the products of the current one issue, and the first fragment of a row
    // tile before the work that precedes it (the operand swaps, the previous tile's eight chain rounds); beta as lin_chain_round says.
    const uint32_t lane16 = __lane_id() * 16;              // (recomputed here: threadIdx.x would be one more register live across the kernel)
    lin_v4 next = lin_frag(lin, LIN_A1 / LIN_FRAG, lane16);
    lin_beta_first(beta, lin);
    z[0] = lin_sbox(u0);
    // each row tile of alpha right before the eight rounds it feeds: eight sums live at a time, not twenty
    lin_operands(vx);
#pragma unroll
    for (int T = 0; T < LIN_TILES; T++) {
        lin_v16 a0 = {0}, a1 = {0};
#pragma unroll
        for (int ks = 0; ks < LIN_KS; ks++) {
            const lin_v4 a = next;
            next = lin_frag(lin, LIN_A1 / LIN_FRAG + T * LIN_KS + ks + 1, lane16);  // after the last of alpha: Gamma | Delta's first (LIN_A2 follows LIN_A1)
            a0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, lin_b(vx, ks, 0), a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, lin_b(vx, ks, 1), a1, 0, 0, 0);
        }
        int64_t t[8];
#pragma unroll
        for (int g = 0; g < 4; g++)
            if (8 * T + 2 * g < LIN_ALPHA) lin_gather2(t[2 * g], t[2 * g + 1], a0, a1, g, c0, c1);
#pragma unroll
        for (int o = 0; o < 8; o++)
            if (8 * T + o < LIN_ALPHA) lin_chain_round(8 * T + o + 1, t[o], z, beta, lin, nullptr);
    }
#pragma unroll
    for (int q = 0; q < LIN_POS; q++) vz[q] = q < PARTIAL ? (uint32_t)z[q] ^ LIN_XOR : 0u;
    lin_operands(vz);
#pragma unroll
    for (int T = 0; T < LIN_TILES; T++) {
        lin_v16 a0 = {0}, a1 = {0};
#pragma unroll
        for (int ks = 0; ks < 2 * LIN_KS; ks++) {
            const lin_v4 a = next;
            if (ks + 1 < 2 * LIN_KS) next = lin_frag(lin, LIN_A2 / LIN_FRAG + T * 2 * LIN_KS + ks + 1, lane16);
            a0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, ks < LIN_KS ? lin_b(vx, ks, 0) : lin_b(vz, ks - LIN_KS, 0), a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, ks < LIN_KS ? lin_b(vx, ks, 1) : lin_b(vz, ks - LIN_KS, 1), a1, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; g++) {
            int64_t t0, t1;
            lin_gather2(t0, t1, a0, a1, g, c0, c1);
            s[8 * T + 2 * g] = (uint32_t)smont_reduce(t0); s[8 * T + 2 * g + 1] = (uint32_t)smont_reduce(t1);
            // the next tile's first fragment: behind the first gather, which has freed eight accumulator registers (both operand
            // blocks, both accumulators and the outputs so far are live here: the kernel's register peak)
            if (g == 0 && T + 1 < LIN_TILES) next = lin_frag(lin, LIN_A2 / LIN_FRAG + (T + 1) * 2 * LIN_KS, lane16);
        }
    }
    (void)st;
#else
    z[0] = lin_sbox(u0);
    lin_beta_first(beta, lin);
    auto track = [](int64_t& m, int64_t v) { if (v < 0) v = -v; if (v > m) m = v; };
    auto byte_of = [](const uint32_t (&v)[LIN_POS], int k) { return (int32_t)(int8_t)(v[k >> 2] >> (8 * (k & 3))); };
    auto output = [&](int second, int o, int64_t* lo_hi_track) {
        int32_t r[4];
        for (int i = 0; i < 4; i++) {
            const int row = 32 * (o >> 3) + lin_row(o & 7, i);
            int32_t acc = 0;
            for (int k = 0; k < 4 * LIN_POS; k++) acc += lin_digit(lin, second, row, k) * byte_of(vx, k);
            if (second) for (int k = 0; k < 4 * LIN_POS; k++) acc += lin_digit(lin, second, row, 4 * LIN_POS + k) * byte_of(vz, k);
            r[i] = acc;
            if (st) track(st->acc, acc);
        }
        if (st) { track(*lo_hi_track, (int64_t)r[0] + 256 * (int64_t)r[1]); track(*lo_hi_track, (int64_t)r[2] + 256 * (int64_t)r[3]); }
        return lin_recombine(r[0], r[1], r[2], r[3], c0, c1);
    };
    int64_t scratch = 0;
    int64_t* lh = st ? &st->lo : &scratch;
    for (int o = 0; o < LIN_ALPHA; o++) lin_chain_round(o + 1, output(0, o, lh), z, beta, lin, st);
    for (int q = 0; q < LIN_POS; q++) vz[q] = q < PARTIAL ? (uint32_t)z[q] ^ LIN_XOR : 0u;
    for (int o = 0; o < CELLS; o++) {
        const int64_t tt = output(1, o, lh);
        s[o] = (uint32_t)smont_reduce(tt);
        if (st) { track(st->t, tt); track(st->out, (int64_t)(int32_t)s[o]); }
    }
#endif
}

// ---- host: the table ----
// exact worst cases of a table, from its own digits (bytes in [-128, 127], |z| < P)
struct LinBounds { int64_t acc, lo, t, out; };
inline bool poseidon2_linear_bounds(const uint32_t* lin, LinBounds* out) {
    LinBounds b = {0, 0, 0, 0};
    bool ok = true;
    const int64_t c0 = (int32_t)lin[LIN_SCALARS], c1 = (int32_t)lin[LIN_SCALARS + 1], ac1 = c1 < 0 ? -c1 : c1;
    auto row_t = [&](int second, int o) {                 // worst |lo c0 + hi c1| of output o
        int64_t r[4];
        for (int i = 0; i < 4; i++) {
            r[i] = 0;
            for (int k = 0; k < (second ? 8 : 4) * LIN_POS; k++) { const int d = lin_digit(lin, second, 32 * (o >> 3) + lin_row(o & 7, i), k); r[i] += 128 * (d < 0 ? -d : d); }
            if (r[i] > b.acc) b.acc = r[i];
        }
        const int64_t lo = r[0] + 256 * r[1], hi = r[2] + 256 * r[3];
        if (lo > b.lo) b.lo = lo;
        if (hi > b.lo) b.lo = hi;
        if (lo >= (1ll << 31) || hi >= (1ll << 31)) ok = false;
        return lo * c0 + hi * ac1;                            // < 2^31 2^28 + 2^31 2^30: no wrap
    };
    auto folded = [](int64_t a) { return ((a >> 32) + 1) * (int64_t)R1 + (1ll << 32); };
    for (int r = 1; r < PARTIAL; r++) {
        int64_t acc = row_t(0, r - 1);
        int n = 0;
        for (int j = 0; j < r; j++) {
            if (lin_fold_before(n)) { acc = folded(acc); n = 0; }
            const int64_t be = (int32_t)lin[lin_beta_at(r, j)], prod = (int64_t)(P - 1) * (be < 0 ? -be : be);
            if (prod > INT64_MAX - acc) return false;         // the sum would wrap
            acc += prod; n++;
        }
        if (lin_fold_last(n)) acc = folded(acc);
        if (acc > b.t) b.t = acc;
    }
    for (int o = 0; o < CELLS; o++) { const int64_t t = row_t(1, o); if (t > b.t) b.t = t; }
    b.out = ((b.t + LIN_DOMAIN) >> 32) + 1;                   // |smont_reduce(t)| <= (|t| + 2^31 P) / 2^32
    if (out) *out = b;
    return ok && b.acc < (1 << 21) && b.t < LIN_DOMAIN && b.out < (int64_t)P;
}
// ptab: poseidon2_partial_table's table for the same constants.  Returns false (and leaves a table that must not be used) if the
// second half's scale chain does not end at R, if x_0 survives the first round, or if a bound fails.
inline bool poseidon2_linear_table(uint32_t* t, const uint32_t* ptab, const uint32_t* rc_canonical, const uint32_t* diag_canonical, LinBounds* bounds = nullptr) {
    constexpr int NV = CELLS + PARTIAL + 1, ZV = CELLS, KV = CELLS + PARTIAL;     // variables: x_0..x_23, z_0..z_20, 1
    auto addm = [](uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + b) % P); };
    static thread_local uint32_t form[CELLS][NV], alpha[PARTIAL][NV];
    for (int i = 0; i < CELLS; i++) for (int v = 0; v < NV; v++) form[i][v] = i == v;
    for (int r = 0; r < PARTIAL; r++) {
        for (int v = 0; v < NV; v++) alpha[r][v] = form[0][v];
        alpha[r][KV] = addm(alpha[r][KV], rc_canonical[(HALF_FULL + r) * CELLS] % P);
        for (int v = 0; v < NV; v++) form[0][v] = v == ZV + r;
        uint32_t sum[NV];
        for (int v = 0; v < NV; v++) { sum[v] = 0; for (int i = 0; i < CELLS; i++) sum[v] = addm(sum[v], form[i][v]); }
        for (int i = 0; i < CELLS; i++) for (int v = 0; v < NV; v++) form[i][v] = addm(sum[v], p2_mulm(diag_canonical[i] % P, form[i][v]));
    }
    bool ok = true;
    for (int r = 1; r < PARTIAL; r++) ok = ok && alpha[r][0] == 0;
    for (int i = 0; i < CELLS; i++) ok = ok && form[i][0] == 0;
    // scales, as plain residues: a word is scale * value
    const uint32_t rinv = p2_powm(R1, P - 2), lam_inv = p2_powm(R1, 2800), lam = p2_powm(rinv, 2800), sigma = p2_exit_scale();
    uint32_t chain = sigma;
    for (int f = 0; f < HALF_FULL; f++) chain = p2_full_round_scale(chain);
    ok = ok && chain == R1;
    uint32_t zeta_inv[PARTIAL];
    zeta_inv[0] = p2_powm(p2_mulm(p2_powm(lam, 7), p2_powm(rinv, 6)), P - 2);          // z_0 = u_0^7 / R^6 with u_0 at the entry scale
    for (int j = 1; j < PARTIAL; j++) zeta_inv[j] = rinv;                               // u_r at R: z_r at R^7 / R^6
    const uint32_t off_x = (uint32_t)(((uint64_t)LIN_XOR + P - F64_OFF % P) % P);       // register word = sum s_b 2^(8b) + LIN_XOR = w + F64_OFF
    const uint32_t off_z = LIN_XOR;
    for (int i = 0; i < LIN_WORDS; i++) t[i] = 0;
    auto put = [&](int second, int row, int k, int digit) {
        int b;
        const int w = lin_digit_at(second, row, k, &b);
        t[w] = (t[w] & ~(0xffu << (8 * b))) | ((uint32_t)(uint8_t)(int8_t)digit << (8 * b));
    };
    auto digits = [&](int second, int o, int k, uint32_t m) {                          // m: plain residue, the factor of the byte at k
        int32_t c = center(m);
        for (int i = 0; i < 4; i++) {
            const int32_t d = ((c + 128) & 255) - 128;
            c = (c - d) >> 8;
            put(second, 32 * (o >> 3) + lin_row(o & 7, i), k, d);
        }
        ok = ok && c == 0;
    };
    auto entry = [&](int second, int o, int pos, uint32_t m) { for (int b = 0; b < 4; b++) digits(second, o, 4 * pos + b, p2_mulm(m, 1u << (8 * b))); };
    for (int r = 1; r < PARTIAL; r++) {                                                  // word u_r = R u_r
        uint32_t k = p2_mulm(R1, alpha[r][KV]);
        for (int c = 1; c < CELLS; c++) {
            const uint32_t m = p2_mulm(p2_mulm(R1, alpha[r][c]), lam_inv);
            entry(0, r - 1, c - 1, m);
            k = addm(k, p2_mulm(off_x, m));
        }
        for (int j = 0; j < r; j++) {
            const uint32_t m = p2_mulm(p2_mulm(R1, alpha[r][ZV + j]), zeta_inv[j]);
            t[lin_beta_at(r, j)] = (uint32_t)center(p2_mulm(m, R1));                  // meets smont_reduce: times R
            // z_j enters as its word, no bytes: no offset
        }
        digits(0, r - 1, 4 * (CELLS - 1), k);
    }
    for (int o = 0; o < CELLS; o++) {                                                    // word = sigma (x'_o + rc_o of the fifth full round)
        uint32_t k = p2_mulm(sigma, addm(form[o][KV], rc_canonical[(HALF_FULL + PARTIAL) * CELLS + o] % P));
        for (int c = 1; c < CELLS; c++) {
            const uint32_t m = p2_mulm(p2_mulm(sigma, form[o][c]), lam_inv);
            entry(1, o, c - 1, m);
            k = addm(k, p2_mulm(off_x, m));
        }
        for (int j = 0; j < PARTIAL; j++) {
            const uint32_t m = p2_mulm(p2_mulm(sigma, form[o][ZV + j]), zeta_inv[j]);
            entry(1, o, LIN_POS + j, m);
            k = addm(k, p2_mulm(off_z, m));
        }
        digits(1, o, 4 * (CELLS - 1), k);
    }
    t[LIN_SCALARS] = R1;
    t[LIN_SCALARS + 1] = (uint32_t)center(p2_mulm(1u << 16, R1));
    t[LIN_SCALARS + 2] = (uint32_t)center(p2_mulm(lam, rc_canonical[HALF_FULL * CELLS] % P)) - F64_OFF;     // u_0 = s_0 + this
    for (int i = 0; i < 2 * HALF_FULL * CELLS; i++) t[LIN_RCF + i] = i / CELLS == HALF_FULL ? 0u : ptab[P2_TAB_FULL + i];
    return poseidon2_linear_bounds(t, bounds) && ok;
}

}  // namespace zkh
