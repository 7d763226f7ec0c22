// ntt_plan.h — which kernels a transform of ntt.hip runs, decided once and on the host alone (no HIP types: tests/cpp/ntt_plan_test.cpp
// compiles this header with g++ and walks every size, direction and expansion; tests/golden/ntt_plan.json pins the result).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "ntt_lazy.h"

namespace zkh {

struct Pass { uint32_t L, R; };
// Cut log_n index bits into HBM passes of <= 12 bits.  The lowest pass works on contiguous runs (cheapest), the
// strided passes above it are kept <= 10 bits so a 2^R x 16-word tile stays <= 64 KiB.
inline std::vector<Pass> plan_passes(uint32_t log_n) {
    std::vector<Pass> v;
    if (log_n <= 12) { v.push_back({0, log_n}); return v; }
    if (log_n < 18) {                       // two balanced LDS passes
        const uint32_t low = (log_n + 1) / 2;
        v.push_back({0, low});
        v.push_back({low, log_n - low});
        return v;
    }
    // >= 2^18: the contiguous 4096-word register-radix pass, then strided passes.  2^8 and 2^10 rows have
    // register-radix kernels; what is left over (1..4 bits at 2^21, 2^23 .. 2^26: po2 19, 21 .. 24) goes to a last streaming pass in
    // registers (k_ntt_top) instead of a 9..12-layer LDS sweep.
    const uint32_t rem = log_n - 12;
    v.push_back({0, 12});
    if (rem == 8 || rem == 10 || rem <= 7) v.push_back({12, rem});
    else if (rem == 9) { v.push_back({12, 8}); v.push_back({20, 1}); }
    else if (rem == 11 || rem == 12) { v.push_back({12, 8}); v.push_back({20, rem - 8}); }     // the top pass streams 1..4 bits at the same cost: the cheaper strided pass below it
    else { v.push_back({12, 10}); v.push_back({22, rem - 10}); }
    return v;
}

// profiler record = "<Hal op>:<kernel>", so both the op totals and the per-kernel (per-pass) times can be read off
enum class NttKernel { pass, low12, high8, high10, top };
constexpr const char* NTT_KERNEL_SCOPE[] = {":k_ntt_pass", ":k_ntt_low12", ":k_ntt_high8", ":k_ntt_high10", ":k_ntt_top"};

struct PassPlan {
    NttKernel kernel;
    uint32_t L, R;                      // index bits [L, L + R)
    uint32_t log_t;                     // tile width 2^log_t consecutive low indices (k_ntt_top has no tile: 0)
    uint32_t expand_bits, first_layer;  // forward first pass only (else 0, 1)
    bool twiddle, scale, zk_shift;      // inter-pass twiddle; n^-1 and 3^bitrev(i): last inverse pass only
    uint32_t grid_x, block, lds_bytes;  // the launch: grid y is the column count, lds_bytes the dynamic LDS
};
struct NttPlan {
    std::vector<PassPlan> passes;       // in execution order
    bool lazy;                          // forward register-radix pair (low12 + high<8|10>): see radix_layers<..., LAZY>
    uint32_t lazy_reds;                 // lazy reductions on a path through both passes
};

inline NttPlan plan_transform(uint32_t log_n, bool inverse, uint32_t expand_bits, bool zk) {
    const std::vector<Pass> passes = plan_passes(log_n);
    const size_t npass = passes.size();
    NttPlan plan{};
    // forward transforms whose two passes are both register-radix kernels (2^20 and 2^22: what po2-18/20 seals
    // expand into) run the lazy signed butterflies; the constant R^(layers run) rides on the four-step twiddle
    // (letting the lazy pair also run under a third pass - 2^21 / 2^23 / 2^24 - is bit-exact and was measured flat twice; the
    // per-shape twiddle matrix, 32-byte tiles and the column-fast grid were measured slower: profiles/README.md, r03_ntt_matrix.txt,
    // r03_ntt_ab*.jsonl.  None of those variants is in the library any more.)
    plan.lazy = !inverse && npass == 2 && passes[0].R == 12 && (passes[1].R == 8 || passes[1].R == 10) && expand_bits <= 4;
    // reductions on a path: the low pass's rounds of 4 layers (the first without its expand_bits skipped ones), the strided
    // pass's rounds of 4 + 4 (+ 2) layers, one per pair of layers and one per single layer
    plan.lazy_reds = plan.lazy ? lazy_reductions(4, expand_bits) + 2 * lazy_reductions(4, 0) + lazy_reductions(passes[1].R, 0) : 0;
    for (size_t pi = 0; pi < npass; pi++) {
        // inverse: high bits first; forward: low bits first
        const Pass ps = inverse ? passes[npass - 1 - pi] : passes[pi];
        const bool first = pi == 0, last = pi + 1 == npass;
        PassPlan p{};
        p.L = ps.L; p.R = ps.R;
        p.expand_bits = (!inverse && first) ? expand_bits : 0;
        // the first pass skips the layers it owns; what expand_bits asks beyond them it accounts for in its load (k_ntt_pass: pad_mask)
        p.first_layer = (!inverse && first) ? std::min(expand_bits, ps.R) + 1 : 1;
        p.twiddle = ps.L != 0;
        p.scale = inverse && last;
        p.zk_shift = inverse && last && zk;
        p.block = 256;
        if (ps.L == 0 && ps.R == 12 && p.expand_bits <= 4) {
            p.kernel = NttKernel::low12;                    // one workgroup = 4096 contiguous words, static LDS
            p.grid_x = 1u << (log_n - 12);
        } else if (ps.L >= 4 && (ps.R == 8 || ps.R == 10)) {
            // the register-radix strided kernels: 16-word runs, one lane per (16 rows, column).  (A strided pass is never the last
            // inverse one, so these kernels carry neither n^-1 nor the zk shift.)
            p.kernel = ps.R == 8 ? NttKernel::high8 : NttKernel::high10;
            p.log_t = 4;
            p.grid_x = 1u << (log_n - ps.R - 4);
            p.block = 1u << ps.R;
            p.lds_bytes = 4u << (ps.R + 4);
        } else if (ps.L >= 12 && ps.R <= 4) {
            // what is left above the strided pass: always the last bits, never the first forward or the last inverse pass
            p.kernel = NttKernel::top;
            p.grid_x = 1u << (ps.L - 10);                   // 256 lanes x 4 low indices per workgroup
        } else {
            // the generic kernel takes as wide a run as a 4096-element tile allows: on a strided pass runs of 2^(12 - R) consecutive
            // words, 16 at the least (a 1..3-bit top pass then streams 2..8 KiB runs; with 16-word runs it moved 64 elements per
            // workgroup: 0.6 TB/s).  R <= 12 at L = 0 and R <= 10 above it: the tile stays <= 64 KiB.
            p.kernel = NttKernel::pass;
            p.log_t = std::min(ps.L, std::max<uint32_t>(4, 12 - ps.R));
            p.grid_x = 1u << (log_n - ps.R - p.log_t);
            p.lds_bytes = 4u << (ps.R + p.log_t);
        }
        plan.passes.push_back(p);
    }
    return plan;
}

}  // namespace zkh
