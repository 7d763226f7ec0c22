// Host-side check of the partial rounds as one affine map through int8 digit products (zeth_amd/csrc/poseidon2_linear.h):
// the host model (same table, same bytes, same recombination and chain as the device path; the tile product as int32 loops)
// against the literal 21 partial rounds written here with plain modular arithmetic, and the whole permutation through it
// against poseidon2_mix, the literal 29 rounds and the published known-answer vector.  Shipped tables.  The largest digit
// sum, recombined word, reduced sum and output are printed and held against the builder's exact bounds; a table with one
// digit (or one beta word) altered is refused by the bound check or caught by the comparison.
// Build: g++ -O2 -std=c++17 -I zeth_amd/csrc -I include tests/cpp/poseidon2_linear.cpp -o <out>;  exit code 0 = all hold.
#include "poseidon2.h"
#include "zkh_poseidon2_consts.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace zkh;

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t next64() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                           z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static uint32_t mulp(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)a * b % P); }
static uint32_t addp(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + b) % P); }
static uint32_t pow7(uint32_t x) { const uint32_t x2 = mulp(x, x), x4 = mulp(x2, x2); return mulp(mulp(x4, x2), x); }
static uint32_t residue(int64_t v) { return (uint32_t)((v % (int64_t)P + P) % P); }

static void lit_m_ext(uint32_t* x) {
    static const uint32_t M4[4][4] = {{5, 7, 1, 3}, {4, 6, 1, 1}, {1, 3, 5, 7}, {1, 1, 4, 6}};
    uint32_t y[CELLS], col[4] = {0, 0, 0, 0};
    for (int b = 0; b < CELLS; b += 4)
        for (int r = 0; r < 4; r++) {
            uint32_t acc = 0;
            for (int c = 0; c < 4; c++) acc = addp(acc, mulp(M4[r][c], x[b + c]));
            y[b + r] = acc; col[r] = addp(col[r], acc);
        }
    for (int i = 0; i < CELLS; i++) x[i] = addp(y[i], col[i % 4]);
}
static void lit_partial(uint32_t* x, const uint32_t* rc, const uint32_t* diag) {
    for (int r = 0; r < PARTIAL; r++) {
        x[0] = pow7(addp(x[0], rc[(HALF_FULL + r) * CELLS] % P));
        uint32_t s = 0;
        for (int i = 0; i < CELLS; i++) s = addp(s, x[i]);
        for (int i = 0; i < CELLS; i++) x[i] = addp(s, mulp(diag[i] % P, x[i]));
    }
}
static void literal(uint32_t* x, const uint32_t* rc, const uint32_t* diag) {
    lit_m_ext(x);
    for (int r = 0; r < HALF_FULL; r++) {
        for (int i = 0; i < CELLS; i++) x[i] = pow7(addp(x[i], rc[r * CELLS + i] % P));
        lit_m_ext(x);
    }
    lit_partial(x, rc, diag);
    for (int r = HALF_FULL + PARTIAL; r < ROUNDS_TOTAL; r++) {
        for (int i = 0; i < CELLS; i++) x[i] = pow7(addp(x[i], rc[r * CELLS + i] % P));
        lit_m_ext(x);
    }
}

static const uint32_t* RC = ZKH_P2_ROUND_CONSTANTS;
static const uint32_t* DIAG = ZKH_P2_M_INT_DIAG;
static long checked = 0;

// The model on register words as the fourth full round leaves them (word = entry-scale value + F64_OFF; cells 1..23 may be ANY
// 32-bit word, cell 0 is nearly centred) against the literal partial rounds: out word = sigma (x' + the fifth round's constant).
// Returns 0 = equal, 1 = differs, 2 = equal but a tracked magnitude exceeds its bound.
static int run_partial(const uint32_t* words, const uint32_t* lin, const LinBounds& b, LinStats* st, bool quiet = false) {
    const uint32_t lam_inv = p2_powm(R1, 2800), sigma = p2_exit_scale();
    uint32_t x[CELLS], s[CELLS];
    for (int i = 0; i < CELLS; i++) { s[i] = words[i]; x[i] = mulp(residue((int64_t)(int32_t)words[i] - (int64_t)F64_OFF), lam_inv); }
    lit_partial(x, RC, DIAG);
    LinStats one;
    poseidon2_partial_linear(s, lin, &one);
    checked++;
    for (int i = 0; i < CELLS; i++) {
        const uint32_t want = mulp(sigma, addp(x[i], RC[(HALF_FULL + PARTIAL) * CELLS + i] % P));
        if (residue((int32_t)s[i]) != want) {
            if (!quiet) fprintf(stderr, "MISMATCH partial rounds, cell %d: got %d want %u\n", i, (int32_t)s[i], want);
            return 1;
        }
    }
    if (one.acc > st->acc) st->acc = one.acc;
    if (one.lo > st->lo) st->lo = one.lo;
    if (one.t > st->t) st->t = one.t;
    if (one.out > st->out) st->out = one.out;
    if (one.acc > b.acc || one.lo > b.lo || one.t > b.t || one.out > b.out) {
        if (!quiet) fprintf(stderr, "a magnitude exceeds the builder's bound: acc %lld/%lld lo %lld/%lld t %lld/%lld out %lld/%lld\n", (long long)one.acc, (long long)b.acc,
                            (long long)one.lo, (long long)b.lo, (long long)one.t, (long long)b.t, (long long)one.out, (long long)b.out);
        return 2;
    }
    return 0;
}
// the whole permutation through the model: every kept-cell form the two kernels use, against poseidon2_mix and the literal rounds
static bool run_whole(const uint32_t* plain, const uint32_t* rcs, const uint32_t* tab, const uint32_t* lin) {
    uint32_t want[CELLS], mix[CELLS], in[CELLS], s[CELLS];
    for (int i = 0; i < CELLS; i++) { want[i] = plain[i] % P; in[i] = mix[i] = fp_encode(plain[i]).v; }
    literal(want, RC, DIAG);
    poseidon2_mix(mix, rcs, tab);
    checked++;
    for (int i = 0; i < CELLS; i++) s[i] = in[i];
    poseidon2_mix_raw_linear<0, CELLS>(s, tab, lin);
    for (int i = 0; i < CELLS; i++)
        if (p2_finish(s[i]) != mix[i] || fp_decode(Fp::raw(mix[i])) != want[i]) { fprintf(stderr, "MISMATCH whole permutation, cell %d\n", i); return false; }
    for (int last = 0; last < 2; last++) {
        for (int i = 0; i < CELLS; i++) s[i] = in[i];
        poseidon2_mix_sponge_linear(s, tab, lin, last);
        for (int i = 0; i < OUT; i++)
            if (p2_finish(s[RATE + i]) != mix[last ? i : RATE + i]) { fprintf(stderr, "MISMATCH sponge block (last %d), cell %d\n", last, i); return false; }
    }
    uint32_t z[CELLS];
    for (int i = 0; i < CELLS; i++) { z[i] = i < RATE ? in[i] : 0u; s[i] = i < RATE ? in[i] : 0xdeadbeefu; }
    poseidon2_mix(z, rcs, tab);
    poseidon2_mix_raw_linear<0, OUT, RATE>(s, tab, lin);
    for (int i = 0; i < OUT; i++) if (p2_finish(s[i]) != z[i]) { fprintf(stderr, "MISMATCH zero-capacity entry, cell %d\n", i); return false; }
    return true;
}

int main(int argc, char** argv) {
    const long random_cases = argc > 1 ? atol(argv[1]) : 2000;
    std::vector<uint32_t> rcs(ROUNDS_TOTAL * CELLS), tab(P2_TAB_WORDS), lin(LIN_WORDS);
    for (int i = 0; i < ROUNDS_TOTAL * CELLS; i++) rcs[i] = fp_encode(RC[i]).v - P;
    if (!poseidon2_partial_table(tab.data(), RC, DIAG)) { fprintf(stderr, "partial table refused\n"); return 1; }
    LinBounds b;
    if (!poseidon2_linear_table(lin.data(), tab.data(), RC, DIAG, &b)) { fprintf(stderr, "the shipped constants' linear table is refused\n"); return 1; }
    printf("bounds from the table's digits: digit sum %lld (< 2^21 = %d), lo/hi %lld, reduced sum %lld (< P 2^31 = %lld), output %lld (< P)\n",
           (long long)b.acc, 1 << 21, (long long)b.lo, (long long)b.t, (long long)LIN_DOMAIN, (long long)b.out);
    LinStats st;
    uint32_t w[CELLS];
    auto centred = [] { return (uint32_t)((int64_t)(next64() % (P + 129)) - (int64_t)(P / 2 + 64)) + F64_OFF; };   // what a full round leaves
    // cells 1..23 at fixed signed words: +-(P-1), +-(P-1)/2, and words whose bytes are all 0x00, 0x7f, 0x80 or 0xff
    const uint32_t fixed[] = {P - 1, (uint32_t)-(int32_t)(P - 1), (P - 1) / 2, (uint32_t)-(int32_t)((P - 1) / 2), 0x00000000u, 0x7f7f7f7fu, 0x80808080u, 0xffffffffu,
                              0x7fffffffu, 0x80000000u, 0x807f807fu, 0x7f80ff00u};
    for (uint32_t f : fixed)
        for (int c0 = 0; c0 < 4; c0++) {
            for (int i = 1; i < CELLS; i++) w[i] = f;
            w[0] = c0 == 0 ? F64_OFF + (P / 2 + 64) : c0 == 1 ? F64_OFF - (P / 2 + 64) : c0 == 2 ? F64_OFF : centred();
            if (run_partial(w, lin.data(), b, &st)) return 1;
        }
    for (long k = 0; k < random_cases; k++) {
        for (int i = 0; i < CELLS; i++) w[i] = k % 3 == 0 ? (uint32_t)next64() : k % 3 == 1 ? centred() : fixed[next64() % 12];
        w[0] = centred();
        if (run_partial(w, lin.data(), b, &st)) return 1;
    }
    printf("largest seen: digit sum %lld, lo/hi %lld, reduced sum %lld, output %lld\n", (long long)st.acc, (long long)st.lo, (long long)st.t, (long long)st.out);
    // the whole permutation: known-answer vector, edge states, random states
    {
        static const uint32_t kat[CELLS] = {0x2ed3e23d, 0x12921fb0, 0x0e659e79, 0x61d81dc9, 0x32bae33b, 0x62486ae3, 0x1e681b60, 0x24b91325,
                                            0x2a2ef5b9, 0x50e8593e, 0x5bc818ec, 0x10691997, 0x35a14520, 0x2ba6a3c5, 0x279d47ec, 0x55014e81,
                                            0x5953a67f, 0x2f403111, 0x6b8828ff, 0x1801301f, 0x2749207a, 0x3dc9cf21, 0x3c985ba2, 0x57a99864};
        uint32_t s[CELLS];
        for (int i = 0; i < CELLS; i++) s[i] = fp_encode((uint32_t)i).v;
        poseidon2_mix_raw_linear<0, CELLS>(s, tab.data(), lin.data());
        for (int i = 0; i < CELLS; i++)
            if (fp_decode(Fp::raw(p2_finish(s[i]))) != kat[i]) { fprintf(stderr, "known-answer vector: cell %d differs\n", i); return 1; }
    }
    const uint32_t edge[] = {0u, 1u, P - 1, (P - 1) / 2, (P + 1) / 2, P - 2, 2u, R1, P - R1};
    for (long k = 0; k < 9 + random_cases; k++) {
        for (int i = 0; i < CELLS; i++) w[i] = k < 9 ? edge[k] : k % 2 ? (uint32_t)(next64() % P) : edge[next64() % 9];
        if (!run_whole(w, rcs.data(), tab.data(), lin.data())) return 1;
    }
    // one digit altered, at every 97th byte of the fragments (zero padding included), and every 7th beta word: refused or caught
    // (a digit meets one byte of one word, and that byte may be zero: three random states, caught by any of them)
    long altered = 0, refused = 0;
    uint32_t w3[3][CELLS];
    for (auto& ws : w3) for (int i = 0; i < CELLS; i++) ws[i] = i ? (uint32_t)next64() : centred();
    auto caught = [&](const uint32_t* bad) {
        LinStats s2;
        for (auto& ws : w3) if (run_partial(ws, bad, b, &s2, true) != 0) return true;
        return false;
    };
    for (int at = 0; at < 4 * LIN_BETA; at += 97) {
        std::vector<uint32_t> bad(lin);
        bad[at >> 2] ^= 0x01u << (8 * (at & 3));
        LinBounds bb;
        const bool ok = poseidon2_linear_bounds(bad.data(), &bb);
        altered++;
        if (!ok) { refused++; continue; }
        // a digit of an unused K position (the three after z_20) or an unused row meets a zero byte or is not read: find out which
        int second = at >> 2 >= LIN_A2, frag = ((at >> 2) - (second ? LIN_A2 : LIN_A1)) / LIN_FRAG, lane = ((at >> 2) % LIN_FRAG) / 4, byte = at & 15;
        const int ks = second ? 2 * LIN_KS : LIN_KS, row = 32 * (frag / ks) + (lane & 31), k = 32 * (frag % ks) + 16 * (lane >> 5) + byte;
        const bool row_used = second ? true : row < 4 * LIN_ALPHA + 0 && 8 * (row >> 5) + 2 * ((row & 31) >> 3) + (((row & 31) >> 2) & 1) < LIN_ALPHA;
        const bool k_used = (k < 4 * CELLS - 4) || k == 4 * CELLS - 4 || (second && k >= 4 * LIN_POS && k < 4 * LIN_POS + 4 * PARTIAL);
        if (!(row_used && k_used)) continue;
        if (!caught(bad.data())) { fprintf(stderr, "a table with the digit at byte %d altered passes\n", at); return 1; }
    }
    for (int at = 0; at < LIN_BETA_WORDS; at += 7) {
        std::vector<uint32_t> bad(lin);
        bad[LIN_BETA + at] ^= 1u;
        altered++;
        if (!caught(bad.data())) { fprintf(stderr, "a table with beta word %d altered passes\n", at); return 1; }
    }
    {   // a digit row pushed past 2^21 is refused by the bound check itself
        std::vector<uint32_t> bad(lin);
        for (int k = 0; k < 8 * LIN_POS; k++) { int bt; const int wd = lin_digit_at(1, 0, k, &bt); bad[wd] = (bad[wd] & ~(0xffu << (8 * bt))) | (0x80u << (8 * bt)); }
        if (poseidon2_linear_bounds(bad.data(), nullptr)) { fprintf(stderr, "a row of 192 digits -128 is not refused\n"); return 1; }
    }
    if (st.acc > b.acc || st.lo > b.lo || st.t > b.t || st.out > b.out) return 1;
    printf("poseidon2 linear partial rounds == literal rounds and poseidon2_mix on %ld cases; %ld altered tables refused (%ld by the bounds) or caught\n",
           checked, altered, refused);
    return 0;
}
