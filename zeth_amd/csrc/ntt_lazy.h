// ntt_lazy.h — the lazy signed forward (DIT) butterflies of the register-radix NTT passes (ntt.hip), host + gfx950 device.
//
// Values are SIGNED representatives in (-P, P).  Two consecutive layers b, b + 1 on the four elements
//   x0 = v[k], x1 = v[k + 2^b], x2 = v[k + 2^(b+1)], x3 = v[k + 2^(b+1) + 2^b]
// are done with ONE Montgomery reduction per output:
//   s+ = sext(x0) + wa x1              s- = sext(x0) - wa x1              (64-bit, NOT reduced)
//   u2 = red(sext(x2) + wa x3)         u3 = red(sext(x2) - wa x3)
//   y0 = red(s+ + Wb u2)   y2 = red(s+ - Wb u2)   y1 = red(s- + Wb' u3)   y3 = red(s- - Wb' u3)
// wa is the PLAIN residue of the layer-b twiddle, Wb / Wb' = wb 2^32 mod P the MONTGOMERY words of the two layer-(b+1)
// twiddles, so that the reduced u re-enters the unreduced sum at its scale: every output is (two-layer result) / 2^32,
// one factor R^-1 per PAIR of layers.  24 instructions per block (2 sign extensions, 8 v_mad_i64_i32, 6 reductions of
// v_mul_lo + v_mad_i64_i32) against 32 for two single layers.
// Bounds, |x| <= P on entry and twiddles CENTRED (|w| <= (P-1)/2; with words in [0, P) the sums reach 1.42 P):
//   |u| <= (P + P^2/2) / 2^32 + P/2 = 0.734 P;   |y| <= (P + P^2/2 + 0.734 P^2/2) / 2^32 + P/2 = 0.906 P < 2^31;
//   largest reduced sum 0.813 P 2^31 < P 2^31 (smont_reduce's domain);  a single layer alone gives |y| <= 0.734 P.
// tests/cpp/ntt_lazy_bounds.cpp drives exactly this header with edge-valued operands and whole columns.
#pragma once
#include "fp.h"

// host bound tests define this to see every sum that enters a reduction
#ifndef ZKH_LAZY_SUM
#define ZKH_LAZY_SUM(t) ((void)0)
#endif

namespace zkh {

constexpr int LAZY_TAB_LOG = 12;                      // per-layer tables up to w_{2^12} (= LDS_TW_LOG)
constexpr uint32_t LAZY_TAB_MONT = 1u << LAZY_TAB_LOG;  // word offset of the Montgomery half of the lazy table
constexpr uint32_t LAZY_TAB_WORDS = 2u << LAZY_TAB_LOG;

// The lazy table from layer_fwd (Montgomery words, [2^(j-1) + e] = w_j^e): [0, 4096) centred plain residues (even layer of a
// pair, single layers), [4096, 8192) centred Montgomery words (odd layer of a pair); two's-complement words.  One table, so
// that both halves are reached from one address register (the second by an immediate offset).
inline void lazy_layer_table(uint32_t* out, const uint32_t* layer_fwd) {
    for (uint32_t i = 0; i < LAZY_TAB_MONT; i++) {
        out[i] = (uint32_t)center(mont_reduce((uint64_t)layer_fwd[i]));       // word / R: the plain residue
        out[LAZY_TAB_MONT + i] = (uint32_t)center(layer_fwd[i]);
    }
}

// acc + a*w; UNIFORM: w is wave-uniform and stays in an SGPR (as a "v" operand it would cost a v_mov per product)
template <bool UNIFORM>
ZKH_HD int64_t lazy_mad(int32_t a, int32_t w, int64_t acc) {
    if constexpr (UNIFORM) return mad_i64_k(a, w, acc);
    else return mad_i64(a, w, acc);
}
ZKH_HD int32_t lazy_reduce(int64_t t) {
    ZKH_LAZY_SUM(t);
    return smont_reduce(t);
}

// one layer: (x + w y) / R, (x - w y) / R;  w plain, centred
template <bool UNIFORM>
ZKH_HD void lazy_single(uint32_t& v0, uint32_t& v1, int32_t w) {
    const int64_t x = (int64_t)(int32_t)v0;
    const int32_t y = (int32_t)v1, nw = -w;
    v0 = (uint32_t)lazy_reduce(lazy_mad<UNIFORM>(y, w, x));
    v1 = (uint32_t)lazy_reduce(lazy_mad<UNIFORM>(y, nw, x));
}

// two layers (see the head of this file);  wa plain, wb0 / wb1 Montgomery, all centred
template <bool UNIFORM>
ZKH_HD void lazy_pair(uint32_t& v0, uint32_t& v1, uint32_t& v2, uint32_t& v3, int32_t wa, int32_t wb0, int32_t wb1) {
    const int32_t nwa = -wa, nwb0 = -wb0, nwb1 = -wb1;
    const int64_t x0 = (int64_t)(int32_t)v0, x2 = (int64_t)(int32_t)v2;
    const int32_t x1 = (int32_t)v1, x3 = (int32_t)v3;
    const int32_t u2 = lazy_reduce(lazy_mad<UNIFORM>(x3, wa, x2));
    const int32_t u3 = lazy_reduce(lazy_mad<UNIFORM>(x3, nwa, x2));
    const int64_t sp = lazy_mad<UNIFORM>(x1, wa, x0), sm = lazy_mad<UNIFORM>(x1, nwa, x0);
    v0 = (uint32_t)lazy_reduce(lazy_mad<UNIFORM>(u2, wb0, sp));
    v2 = (uint32_t)lazy_reduce(lazy_mad<UNIFORM>(u2, nwb0, sp));
    v1 = (uint32_t)lazy_reduce(lazy_mad<UNIFORM>(u3, wb1, sm));
    v3 = (uint32_t)lazy_reduce(lazy_mad<UNIFORM>(u3, nwb1, sm));
}

// number of reductions (factors R^-1) on every path through layers [first_b, LOGR) of one round, LOGR even
ZKH_HD uint32_t lazy_reductions(uint32_t logr, uint32_t first_b) {
    const uint32_t live = first_b < logr ? logr - first_b : 0;
    return (live + 1) / 2;
}

// Layers [first_b, LOGR) of one register round on v[2^LOGR] (LOGR even): pairs (b, b + 1) from the even b up, one single layer in
// front when first_b is odd.  Layer b of the round is layer J_LO + b of the transform; its twiddle for element index k is
// w^(base_low + (k mod 2^b) << (J_LO - 1)).  BASE0: base_low = 0 and J_LO = 1, every twiddle is wave-uniform, the first is 1.
template <int LOGR, bool BASE0, int J_LO>
ZKH_HD void lazy_layers(uint32_t (&v)[1 << LOGR], const uint32_t* __restrict__ ltab, const uint32_t base_low, const int first_b) {
    static_assert(LOGR % 2 == 0, "lazy rounds hold an even number of layers");
    constexpr int N = 1 << LOGR;
#pragma unroll
    for (int b = 0; b < LOGR; b += 2) {
        const uint32_t* twa = ltab + (1u << (J_LO + b - 1));
        const uint32_t* twb = ltab + LAZY_TAB_MONT + (1u << (J_LO + b));
        if (b >= first_b) {
#pragma unroll
            for (int kk = 0; kk < (1 << b); kk++) {
                const uint32_t e = base_low + ((uint32_t)kk << (J_LO - 1));
                const int32_t wa = (BASE0 && kk == 0) ? 1 : (int32_t)twa[e];
                const int32_t wb0 = (BASE0 && kk == 0) ? (int32_t)R1 : (int32_t)twb[e];
                const int32_t wb1 = (int32_t)twb[e + ((1u << b) << (J_LO - 1))];
#pragma unroll
                for (int hi = 0; hi < (N >> (b + 2)); hi++) {
                    const int k = (hi << (b + 2)) | kk;
                    lazy_pair<BASE0>(v[k], v[k + (1 << b)], v[k + (2 << b)], v[k + (3 << b)], wa, wb0, wb1);
                }
            }
        } else if (b + 1 >= first_b) {                  // odd first_b: layer b + 1 alone
            const uint32_t* tw1 = ltab + (1u << (J_LO + b));
#pragma unroll
            for (int kk = 0; kk < (2 << b); kk++) {
                const int32_t w = (BASE0 && kk == 0) ? 1 : (int32_t)tw1[base_low + ((uint32_t)kk << (J_LO - 1))];
#pragma unroll
                for (int hi = 0; hi < (N >> (b + 2)); hi++) {
                    const int k = (hi << (b + 2)) | kk;
                    lazy_single<BASE0>(v[k], v[k + (2 << b)], w);
                }
            }
        }
    }
}

}  // namespace zkh
