// Host-side check of the paired lazy NTT butterflies (zeth_amd/csrc/ntt_lazy.h: the header the kernels compile) against
// plain 64-bit modular arithmetic.  Three things are asserted everywhere: every output is congruent to the radix-2 layers
// it replaces (times R^-reductions), every output is in (-P, P), and every sum that enters a reduction is below P 2^31 in
// magnitude (smont_reduce's domain).  Operands: all combinations of the edge values +-P, +-(P-1), +-(P-1)/2, 0, +-1 with
// the extreme centred twiddles, random ones, and whole columns (4096 contiguous words as k_ntt_low12 walks them, 1024 / 256
// rows as k_ntt_high<10 | 8> does) through ALL lazy rounds with the kernels' real table, so that the bounds are tested as
// iterated.  Build: g++ -O2 -std=c++17 -I zeth_amd/csrc tests/cpp/ntt_lazy_bounds.cpp -o <out>;  exit code 0 = all hold.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static uint64_t g_max_sum = 0;          // largest |sum| seen by a reduction
static long g_sums = 0;
static inline void note_sum(int64_t t) {
    const uint64_t a = t < 0 ? (uint64_t)0 - (uint64_t)t : (uint64_t)t;
    if (a > g_max_sum) g_max_sum = a;
    g_sums++;
}
#define ZKH_LAZY_SUM(t) note_sum(t)
#include "ntt_lazy.h"

using namespace zkh;

static const uint64_t SUM_LIMIT = (uint64_t)P << 31;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next64() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                           z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static uint32_t modp(int64_t x) { const int64_t r = x % (int64_t)P; return (uint32_t)(r < 0 ? r + (int64_t)P : r); }
static uint32_t mulp(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)a * b % P); }
static uint32_t addp(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + b) % P); }
static uint32_t subp(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + P - b) % P); }
static uint32_t powp(uint32_t a, uint64_t e) { uint32_t r = 1; for (; e; e >>= 1, a = mulp(a, a)) if (e & 1) r = mulp(r, a); return r; }

static uint32_t RINV;                   // 2^-32 mod P
static int32_t g_max_out = 0;
static long g_blocks = 0, g_columns = 0;

static bool in_range(uint32_t word, const char* what) {
    const int32_t y = (int32_t)word;
    const int32_t a = y < 0 ? -y : y;
    if (y == INT32_MIN || a >= (int32_t)P) { fprintf(stderr, "%s: output %d outside (-P, P)\n", what, y); return false; }
    if (a > g_max_out) g_max_out = a;
    return true;
}
static bool sums_ok(const char* what) {
    if (g_max_sum >= SUM_LIMIT) { fprintf(stderr, "%s: a reduced sum reached %.4f P 2^31\n", what, (double)g_max_sum / (double)SUM_LIMIT); return false; }
    return true;
}

// one fused block against two radix-2 layers; wa plain, wb0 / wb1 Montgomery words (all signed)
static bool check_pair(const int32_t x[4], int32_t wa, int32_t wb0, int32_t wb1) {
    uint32_t v[4] = {(uint32_t)x[0], (uint32_t)x[1], (uint32_t)x[2], (uint32_t)x[3]};
    lazy_pair<false>(v[0], v[1], v[2], v[3], wa, wb0, wb1);
    const uint32_t pa = modp(wa), pb0 = mulp(modp(wb0), RINV), pb1 = mulp(modp(wb1), RINV);
    const uint32_t c[4] = {modp(x[0]), modp(x[1]), modp(x[2]), modp(x[3])};
    const uint32_t a0 = addp(c[0], mulp(pa, c[1])), a1 = subp(c[0], mulp(pa, c[1]));
    const uint32_t a2 = addp(c[2], mulp(pa, c[3])), a3 = subp(c[2], mulp(pa, c[3]));
    const uint32_t z[4] = {addp(a0, mulp(pb0, a2)), addp(a1, mulp(pb1, a3)), subp(a0, mulp(pb0, a2)), subp(a1, mulp(pb1, a3))};
    g_blocks++;
    for (int i = 0; i < 4; i++) {
        if (!in_range(v[i], "lazy_pair")) return false;
        if (modp((int32_t)v[i]) != mulp(z[i], RINV)) {
            fprintf(stderr, "lazy_pair: output %d not congruent (x = %d %d %d %d, wa %d, wb %d %d)\n", i, x[0], x[1], x[2], x[3], wa, wb0, wb1);
            return false;
        }
    }
    return sums_ok("lazy_pair");
}
static bool check_single(int32_t x, int32_t y, int32_t w) {
    uint32_t v0 = (uint32_t)x, v1 = (uint32_t)y;
    lazy_single<false>(v0, v1, w);
    const uint32_t t = mulp(modp(w), modp(y));
    if (!in_range(v0, "lazy_single") || !in_range(v1, "lazy_single")) return false;
    if (modp((int32_t)v0) != mulp(addp(modp(x), t), RINV) || modp((int32_t)v1) != mulp(subp(modp(x), t), RINV)) {
        fprintf(stderr, "lazy_single: not congruent (x %d, y %d, w %d)\n", x, y, w);
        return false;
    }
    return sums_ok("lazy_single");
}

// ---- whole columns ----
static std::vector<uint32_t> g_layer_plain;     // [2^(j-1) + e] = w_j^e as plain residues, j <= 12: the reference's twiddles
static std::vector<uint32_t> g_ltab;            // the kernels' lazy table

// plain DIT layers first..last (1-based) on a (canonical plain residues), in place
static void ref_layers(std::vector<uint32_t>& a, int first, int last) {
    for (int j = first; j <= last; j++) {
        const size_t h = (size_t)1 << (j - 1);
        for (size_t i = 0; i < a.size(); i++) {
            if (i & h) continue;
            const uint32_t w = g_layer_plain[h + (i & (h - 1))];
            const uint32_t x = a[i], y = mulp(a[i + h], w);
            a[i] = addp(x, y); a[i + h] = subp(x, y);
        }
    }
}
static bool compare_column(const std::vector<uint32_t>& got, const std::vector<uint32_t>& want, uint32_t reductions, const char* what) {
    const uint32_t scale = powp(RINV, reductions);
    for (size_t i = 0; i < got.size(); i++) {
        if (!in_range(got[i], what)) return false;
        if (modp((int32_t)got[i]) != mulp(want[i], scale)) { fprintf(stderr, "%s: element %zu not congruent\n", what, i); return false; }
    }
    g_columns++;
    return sums_ok(what);
}
// k_ntt_low12<false, true>: 4096 contiguous words, the first expand_bits layers skipped on a replicated input
static bool low12_column(const std::vector<uint32_t>& in, int eb, const char* what) {
    std::vector<uint32_t> col(4096), ref(4096);
    for (int i = 0; i < 4096; i++) { col[i] = in[i >> eb]; ref[i] = modp((int32_t)in[i >> eb]); }
    ref_layers(ref, eb + 1, 12);
    uint32_t v[16];
    const uint32_t* ltab = g_ltab.data();
    for (uint32_t tid = 0; tid < 256; tid++) {
        for (int k = 0; k < 16; k++) v[k] = col[tid * 16 + k];
        lazy_layers<4, true, 1>(v, ltab, 0, eb);
        for (int k = 0; k < 16; k++) col[tid * 16 + k] = v[k];
    }
    for (uint32_t tid = 0; tid < 256; tid++) {
        const uint32_t hi = tid >> 4, low = tid & 15;
        for (int k = 0; k < 16; k++) v[k] = col[hi * 256 + k * 16 + low];
        lazy_layers<4, false, 5>(v, ltab, low, 0);
        for (int k = 0; k < 16; k++) col[hi * 256 + k * 16 + low] = v[k];
    }
    for (uint32_t tid = 0; tid < 256; tid++) {
        for (int k = 0; k < 16; k++) v[k] = col[k * 256 + tid];
        lazy_layers<4, false, 9>(v, ltab, tid, 0);
        for (int k = 0; k < 16; k++) col[k * 256 + tid] = v[k];
    }
    return compare_column(col, ref, lazy_reductions(4, (uint32_t)eb) + 2 * lazy_reductions(4, 0), what);
}
// the rounds of k_ntt_high<10, false, true> on the 1024 rows of one tile column (signed words in, as the pre-twiddle leaves them)
static bool high10_column(const std::vector<uint32_t>& in, const char* what) {
    std::vector<uint32_t> col(in), ref(1024);
    for (int i = 0; i < 1024; i++) ref[i] = modp((int32_t)in[i]);
    ref_layers(ref, 1, 10);
    const uint32_t* ltab = g_ltab.data();
    for (uint32_t g = 0; g < 64; g++)
        for (int i = 0; i < 4; i++) {
            uint32_t u[4];
            const uint32_t m0 = (g * 4 + i) * 4;
            for (int k = 0; k < 4; k++) u[k] = col[m0 + k];
            lazy_layers<2, true, 1>(u, ltab, 0, 0);
            for (int k = 0; k < 4; k++) col[m0 + k] = u[k];
        }
    uint32_t v[16];
    for (uint32_t g = 0; g < 64; g++) {
        const uint32_t hi = g >> 2, low = g & 3;
        for (int k = 0; k < 16; k++) v[k] = col[hi * 64 + k * 4 + low];
        lazy_layers<4, false, 3>(v, ltab, low, 0);
        for (int k = 0; k < 16; k++) col[hi * 64 + k * 4 + low] = v[k];
    }
    for (uint32_t g = 0; g < 64; g++) {
        for (int k = 0; k < 16; k++) v[k] = col[k * 64 + g];
        lazy_layers<4, false, 7>(v, ltab, g, 0);
        for (int k = 0; k < 16; k++) col[k * 64 + g] = v[k];
    }
    return compare_column(col, ref, lazy_reductions(10, 0), what);
}
static bool high8_column(const std::vector<uint32_t>& in, const char* what) {
    std::vector<uint32_t> col(in), ref(256);
    for (int i = 0; i < 256; i++) ref[i] = modp((int32_t)in[i]);
    ref_layers(ref, 1, 8);
    const uint32_t* ltab = g_ltab.data();
    uint32_t v[16];
    for (uint32_t g = 0; g < 16; g++) {
        for (int k = 0; k < 16; k++) v[k] = col[g * 16 + k];
        lazy_layers<4, true, 1>(v, ltab, 0, 0);
        for (int k = 0; k < 16; k++) col[g * 16 + k] = v[k];
    }
    for (uint32_t g = 0; g < 16; g++) {
        for (int k = 0; k < 16; k++) v[k] = col[k * 16 + g];
        lazy_layers<4, false, 5>(v, ltab, g, 0);
        for (int k = 0; k < 16; k++) col[k * 16 + g] = v[k];
    }
    return compare_column(col, ref, lazy_reductions(8, 0), what);
}

int main(int argc, char** argv) {
    const long random_blocks = argc > 1 ? atol(argv[1]) : 400000;
    RINV = powp(R1, P - 2);
    const int32_t SP = (int32_t)P, H = (int32_t)((P - 1) / 2);
    const int32_t xs[] = {SP, -SP, SP - 1, -(SP - 1), H, -H, 0, 1, -1};
    const int32_t ws[] = {H, -H, 0, 1, -1};                  // centred twiddles: (P+-1)/2, 0, 1, P-1
    // the table as the library builds it (hal.hip: powers of w_j = 137^(2^(27-j)) in Montgomery form -> lazy_layer_table)
    {
        std::vector<uint32_t> lf(LAZY_TAB_MONT, R1);
        g_layer_plain.assign(LAZY_TAB_MONT, 1);
        for (int j = 1; j <= LAZY_TAB_LOG; j++) {
            const uint32_t wj = powp(137, 1ull << (27 - j));
            uint32_t w = 1;
            for (size_t e = 0; e < ((size_t)1 << (j - 1)); e++, w = mulp(w, wj)) {
                g_layer_plain[((size_t)1 << (j - 1)) + e] = w;
                lf[((size_t)1 << (j - 1)) + e] = fp_encode(w).v;
            }
        }
        g_ltab.resize(LAZY_TAB_WORDS);
        lazy_layer_table(g_ltab.data(), lf.data());
        for (uint32_t i = 0; i < LAZY_TAB_MONT; i++) {          // centred, and the residues they claim to be
            const int32_t a = (int32_t)g_ltab[i], b = (int32_t)g_ltab[LAZY_TAB_MONT + i];
            if (a > H || a < -H || b > H || b < -H) { fprintf(stderr, "table entry %u is not centred\n", i); return 1; }
            if (modp(a) != g_layer_plain[i] || mulp(modp(b), RINV) != g_layer_plain[i]) { fprintf(stderr, "table entry %u is wrong\n", i); return 1; }
        }
    }
    // 1. every combination of edge operands with the extreme twiddles
    for (int32_t x0 : xs) for (int32_t x1 : xs) for (int32_t x2 : xs) for (int32_t x3 : xs)
        for (int32_t wa : ws) for (int32_t wb0 : ws) for (int32_t wb1 : ws) {
            const int32_t x[4] = {x0, x1, x2, x3};
            if (!check_pair(x, wa, wb0, wb1)) return 1;
        }
    for (int32_t x : xs) for (int32_t y : xs) for (int32_t w : ws) if (!check_single(x, y, w)) return 1;
    // 2. random and mixed operands, random / edge / real twiddles
    auto rnd_x = [&](int mode) -> int32_t {
        if (mode == 0) return xs[next64() % 9];
        return (int32_t)(next64() % (2ull * P + 1)) - SP;                   // [-P, P]
    };
    auto rnd_w = [&](int mode, bool mont) -> int32_t {
        if (mode == 0) return ws[next64() % 5];
        if (mode == 1) return (int32_t)g_ltab[(mont ? LAZY_TAB_MONT : 0) + next64() % LAZY_TAB_MONT];
        return (int32_t)(next64() % P) - H;                                 // [-H, H]
    };
    for (long t = 0; t < random_blocks; t++) {
        const int xm = (int)(t % 2), wm = (int)((t / 2) % 3);
        const int32_t x[4] = {rnd_x(xm), rnd_x(xm), rnd_x(xm), rnd_x(xm)};
        if (!check_pair(x, rnd_w(wm, false), rnd_w(wm, true), rnd_w(wm, true))) return 1;
        if (!check_single(rnd_x(xm), rnd_x(xm), rnd_w(wm, false))) return 1;
    }
    const uint64_t block_max_sum = g_max_sum;
    const int32_t block_max_out = g_max_out;
    // 3. whole columns through all lazy rounds with the real table
    {
        std::vector<std::vector<uint32_t>> cols;                            // canonical words, as the low pass reads them
        cols.push_back(std::vector<uint32_t>(4096, P - 1));
        cols.push_back(std::vector<uint32_t>(4096, (P - 1) / 2));
        cols.push_back(std::vector<uint32_t>(4096, (P + 1) / 2));
        cols.push_back(std::vector<uint32_t>(4096, 0));
        cols.push_back(std::vector<uint32_t>(4096, 1));
        { std::vector<uint32_t> c(4096); for (int i = 0; i < 4096; i++) c[i] = (i & 1) ? P - 1 : 0; cols.push_back(c); }
        { std::vector<uint32_t> c(4096); for (int i = 0; i < 4096; i++) c[i] = (i & 1) ? 0 : P - 1; cols.push_back(c); }
        { std::vector<uint32_t> c(4096); for (int i = 0; i < 4096; i++) c[i] = (i % 3) ? P - 1 : 1; cols.push_back(c); }
        for (int r = 0; r < 24; r++) { std::vector<uint32_t> c(4096); for (auto& w : c) w = (uint32_t)(next64() % P); cols.push_back(c); }
        for (int r = 0; r < 8; r++) { std::vector<uint32_t> c(4096); for (auto& w : c) w = (next64() & 1) ? P - 1 : (uint32_t)((P - 1) / 2 + (next64() & 1)); cols.push_back(c); }
        for (const auto& c : cols)
            for (int eb = 0; eb <= 4; eb++)
                if (!low12_column(c, eb, "low12 column")) return 1;
        // the strided pass reads signed words in [-P, P]
        for (size_t ci = 0; ci < cols.size(); ci++)
            for (int sgn = 0; sgn < 3; sgn++) {
                std::vector<uint32_t> s(1024);
                for (int i = 0; i < 1024; i++) {
                    const int32_t a = (int32_t)cols[ci][i] + (cols[ci][i] == P - 1 ? 1 : 0);        // P-1 -> P: the closed end of the range
                    s[i] = (uint32_t)(sgn == 0 ? a : sgn == 1 ? -a : ((next64() & 1) ? a : -a));
                }
                if (!high10_column(s, "high10 column")) return 1;
                s.resize(256);
                if (!high8_column(s, "high8 column")) return 1;
            }
    }
    printf("lazy NTT pairs == radix-2 layers on %ld blocks and %ld columns; max |output| %.4f P (blocks %.4f P), "
           "max reduced sum %.4f P 2^31 (blocks %.4f) over %ld reductions\n", g_blocks, g_columns, (double)g_max_out / P,
           (double)block_max_out / P, (double)g_max_sum / (double)SUM_LIMIT, (double)block_max_sum / (double)SUM_LIMIT, g_sums);
    return 0;
}
