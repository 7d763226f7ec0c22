// Host-side check of the forms of the Poseidon2 permutation that the Merkle kernels call (zeth_amd/csrc/poseidon2.h):
// the kept-cell ranges of the peeled last round, the zero-capacity entry, the sponge that carries its capacity as a signed
// word, and the exit scale that makes p2_finish a subtract and a canonicalisation.  Everything is compared with a literal
// 29-round permutation written here with plain 64-bit modular arithmetic, on the edge set and constant fills of
// poseidon2_bounds.cpp plus random mixtures.  Also: the last partial group's update sum against its P 2^31 bound at
// all-extreme operands, and the forward scale chain of the table.
// Build: g++ -O2 -std=c++17 -I zeth_amd/csrc -I include tests/cpp/poseidon2_callers.cpp -o <out>;  exit code 0 = all hold.
#include "poseidon2.h"
#include "zkh_poseidon2_consts.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace zkh;

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static uint64_t next64() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                           z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static uint32_t mulp(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)a * b % P); }
static uint32_t addp(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + b) % P); }
static uint32_t pow7(uint32_t x) { const uint32_t x2 = mulp(x, x), x4 = mulp(x2, x2); return mulp(mulp(x4, x2), x); }

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
// plain residues in, plain residues out
static void literal(uint32_t* x, const uint32_t* rc, const uint32_t* diag) {
    lit_m_ext(x);
    int round = 0;
    for (int r = 0; r < HALF_FULL; r++, round++) {
        for (int i = 0; i < CELLS; i++) x[i] = pow7(addp(x[i], rc[round * CELLS + i] % P));
        lit_m_ext(x);
    }
    for (int r = 0; r < PARTIAL; r++, round++) {
        x[0] = pow7(addp(x[0], rc[round * CELLS] % P));
        uint32_t s = 0;
        for (int i = 0; i < CELLS; i++) s = addp(s, x[i]);
        for (int i = 0; i < CELLS; i++) x[i] = addp(s, mulp(diag[i] % P, x[i]));
    }
    for (int r = 0; r < HALF_FULL; r++, round++) {
        for (int i = 0; i < CELLS; i++) x[i] = pow7(addp(x[i], rc[round * CELLS + i] % P));
        lit_m_ext(x);
    }
}

struct Tables {
    std::vector<uint32_t> rcs, tab;
    bool chain_ok;
    Tables(const uint32_t* rc, const uint32_t* diag) : rcs(ROUNDS_TOTAL * CELLS), tab(P2_TAB_WORDS) {
        for (int i = 0; i < ROUNDS_TOTAL * CELLS; i++) rcs[i] = fp_encode(rc[i]).v - P;
        chain_ok = poseidon2_partial_table(tab.data(), rc, diag);
    }
};

static bool fail(const char* what, const char* form, int cell, uint32_t got, uint32_t want) {
    fprintf(stderr, "MISMATCH (%s) %s cell %d: got %u (plain %u) want %u\n", what, form, cell, got, got < P ? fp_decode(Fp::raw(got)) : 0u, want);
    return false;
}
// finished word == the literal cell, and canonical
static bool same(uint32_t got, uint32_t want_plain) { return got < P && fp_decode(Fp::raw(got)) == want_plain; }
// a raw kept cell is (nearly centred signed word) + F64_OFF
static bool centred(uint32_t raw) {
    const int32_t r = (int32_t)p2_signed(raw);
    return r <= (int32_t)(P / 2 + 64) && r >= -(int32_t)(P / 2 + 64);
}

static long checked = 0;
// every kept-cell instance, then p2_finish, against the literal permutation on the kept cells
static bool run_forms(const char* what, const uint32_t* state_plain, const uint32_t* rc, const uint32_t* diag, const Tables& t) {
    uint32_t want[CELLS], in[CELLS], s[CELLS];
    for (int i = 0; i < CELLS; i++) { want[i] = state_plain[i] % P; in[i] = fp_encode(state_plain[i]).v; }
    literal(want, rc, diag);
    const uint32_t *rcs = t.rcs.data(), *tab = t.tab.data();
    checked++;
    for (int i = 0; i < CELLS; i++) s[i] = in[i];
    poseidon2_mix_raw<0, OUT>(s, rcs, tab);
    for (int i = 0; i < OUT; i++) if (!centred(s[i]) || !same(p2_finish(s[i]), want[i])) return fail(what, "raw<0, 8>", i, p2_finish(s[i]), want[i]);
    for (int i = 0; i < CELLS; i++) s[i] = in[i];
    poseidon2_mix_raw<RATE, OUT>(s, rcs, tab);
    for (int i = RATE; i < CELLS; i++) if (!centred(s[i]) || !same(p2_finish(s[i]), want[i])) return fail(what, "raw<16, 8>", i, p2_finish(s[i]), want[i]);
    for (int i = 0; i < CELLS; i++) s[i] = in[i];
    poseidon2_mix_raw<0, CELLS>(s, rcs, tab);
    for (int i = 0; i < CELLS; i++) if (!centred(s[i]) || !same(p2_finish(s[i]), want[i])) return fail(what, "raw<0, 24>", i, p2_finish(s[i]), want[i]);
    for (int i = 0; i < CELLS; i++) s[i] = in[i];
    poseidon2_mix(s, rcs, tab);
    for (int i = 0; i < CELLS; i++) if (!same(s[i], want[i])) return fail(what, "poseidon2_mix", i, s[i], want[i]);
    // the sponge block: capacity or digest, both in s[16..24)
    for (int i = 0; i < CELLS; i++) s[i] = in[i];
    poseidon2_mix_sponge(s, rcs, tab, false);
    for (int i = 0; i < OUT; i++) if (!centred(s[RATE + i]) || !same(p2_finish(s[RATE + i]), want[RATE + i])) return fail(what, "sponge interior", RATE + i, p2_finish(s[RATE + i]), want[RATE + i]);
    for (int i = 0; i < CELLS; i++) s[i] = in[i];
    poseidon2_mix_sponge(s, rcs, tab, true);
    for (int i = 0; i < OUT; i++) if (!centred(s[RATE + i]) || !same(p2_finish(s[RATE + i]), want[i])) return fail(what, "sponge last", i, p2_finish(s[RATE + i]), want[i]);
    // the zero-capacity entry (hash_fold): cells 16..23 are not read, so leave rubbish there
    uint32_t wz[CELLS];
    for (int i = 0; i < CELLS; i++) { wz[i] = i < RATE ? state_plain[i] % P : 0u; s[i] = i < RATE ? in[i] : 0xdeadbeefu; }
    literal(wz, rc, diag);
    poseidon2_mix_raw<0, OUT, RATE>(s, rcs, tab);
    for (int i = 0; i < OUT; i++) if (!centred(s[i]) || !same(p2_finish(s[i]), wz[i])) return fail(what, "raw<0, 8, live 16>", i, p2_finish(s[i]), wz[i]);
    return true;
}
// a sponge of `blocks` rate blocks whose capacity stays signed from block to block (k_hash_rows) against the literal sponge
static bool run_sponge(const char* what, const uint32_t* data_plain, int blocks, const uint32_t* rc, const uint32_t* diag, const Tables& t) {
    uint32_t lit[CELLS] = {0}, s[CELLS] = {0};
    for (int b = 0; b < blocks; b++) {
        for (int i = 0; i < RATE; i++) { lit[i] = data_plain[b * RATE + i] % P; s[i] = fp_encode(data_plain[b * RATE + i]).v; }
        literal(lit, rc, diag);
        poseidon2_mix_sponge(s, t.rcs.data(), t.tab.data(), b + 1 == blocks);
        for (int i = RATE; i < CELLS; i++) {
            if (!centred(s[i])) return fail(what, "sponge capacity range", i, s[i], 0);
            s[i] = p2_signed(s[i]);
        }
    }
    checked++;
    for (int i = 0; i < OUT; i++) {
        const uint32_t got = canon((int32_t)s[RATE + i]);
        if (!same(got, lit[i])) return fail(what, "three-block sponge digest", i, got, lit[i]);
    }
    return true;
}
// The last group's cell update sums  center(mu S2) R1 + (mu d) S1c + (mu d^2) S0c + (mu d^3) s  with every operand at its
// extreme and every sign aligned: the magnitude must stay below P 2^31 (smont_reduce's domain), for every cell's rows.
static bool update_bound(const char* what, const uint32_t* tab) {
    const uint64_t half = (P - 1) / 2, lim = (uint64_t)P << 31;
    auto mag = [](uint32_t w) { const int64_t v = (int32_t)w; return (uint64_t)(v < 0 ? -v : v); };
    for (int i = 1; i < CELLS; i++) {
        const uint64_t r1 = mag(tab[P2_TAB_EXIT + i]), r2 = mag(tab[P2_TAB_EXIT + CELLS + i]), r3 = mag(tab[P2_TAB_EXIT + 2 * CELLS + i]);
        if (r1 > half || r2 > half || r3 > half) { fprintf(stderr, "%s: exit row of cell %d is not centred\n", what, i); return false; }
        const uint64_t sum = half * R1 + r1 * half + r2 * half + r3 * (uint64_t)(P - 1);      // < 2^62: no wrap
        if (sum >= lim) { fprintf(stderr, "%s: update sum of cell %d reaches %llu >= P 2^31\n", what, i, (unsigned long long)sum); return false; }
    }
    // the exact reduction at the extreme rows a table could hold at all (all four terms of one sign)
    const int64_t worst = (int64_t)(half * R1 + 2 * half * half + half * (uint64_t)(P - 1));
    for (int64_t t : {worst, -worst}) {
        const int32_t r = smont_reduce(t);
        if (r <= -(int32_t)P || r >= (int32_t)P) { fprintf(stderr, "%s: smont_reduce out of range at the extreme sum\n", what); return false; }
        const uint32_t rc = canon(r), tc = (uint32_t)((t % (int64_t)P + P) % P);
        if (mulp(rc, R1) != tc) { fprintf(stderr, "%s: smont_reduce value at the extreme sum\n", what); return false; }
    }
    return true;
}
// sigma (the table's word for the last group's S2 product) through four full rounds' scale map lambda^7 / R^7, recomputed here
static bool chain(const char* what, const Tables& t) {
    const uint32_t rinv = p2_powm(R1, P - 2);
    uint32_t lam = t.tab[P2_TAB_KAPPA + 2];
    for (int f = 0; f < HALF_FULL; f++) {
        uint32_t l7 = 1, r7 = 1;
        for (int k = 0; k < 7; k++) { l7 = mulp(l7, lam); r7 = mulp(r7, rinv); }
        lam = mulp(l7, r7);
    }
    if (lam != R1 || !t.chain_ok) { fprintf(stderr, "%s: forward scale chain ends at %u, not R = %u (table says %d)\n", what, lam, R1, (int)t.chain_ok); return false; }
    return true;
}

int main(int argc, char** argv) {
    const long random_cases = argc > 1 ? atol(argv[1]) : 20000;
    std::vector<uint32_t> rc(ROUNDS_TOTAL * CELLS), diag(CELLS), st(CELLS), data(3 * RATE);
    const uint32_t edge[] = {0u, 1u, P - 1, (P - 1) / 2, (P + 1) / 2, P - 2, 2u, R1, P - R1};
    const int n_edge = sizeof edge / sizeof edge[0];
    // every combination of constant fills from the edge set, with edge and random states
    for (int a = 0; a < n_edge; a++)
        for (int b = 0; b < n_edge; b++) {
            for (auto& v : rc) v = edge[a];
            for (auto& v : diag) v = edge[b];
            const Tables t(rc.data(), diag.data());
            if (!chain("edge fills", t) || !update_bound("edge fills", t.tab.data())) return 1;
            for (int c = 0; c < n_edge; c++) {
                for (auto& v : st) v = edge[c];
                if (!run_forms("edge fills", st.data(), rc.data(), diag.data(), t)) return 1;
                for (auto& v : data) v = edge[c];
                if (!run_sponge("edge fills", data.data(), 3, rc.data(), diag.data(), t)) return 1;
                for (auto& v : st) v = (uint32_t)(next64() % P);
                if (!run_forms("edge constants, random state", st.data(), rc.data(), diag.data(), t)) return 1;
                for (auto& v : data) v = (uint32_t)(next64() % P);
                if (!run_sponge("edge constants, random data", data.data(), 3, rc.data(), diag.data(), t)) return 1;
            }
        }
    // per-word mixtures of edge values and random values
    for (long k = 0; k < random_cases; k++) {
        const int mode = (int)(k % 4);
        for (auto& v : rc) v = (mode & 1) ? edge[next64() % n_edge] : (uint32_t)(next64() % P);
        for (auto& v : diag) v = (mode & 2) ? edge[next64() % n_edge] : (uint32_t)(next64() % P);
        for (auto& v : st) v = (k % 3 == 0) ? edge[next64() % n_edge] : (uint32_t)(next64() % P);
        for (auto& v : data) v = (k % 3 == 1) ? edge[next64() % n_edge] : (uint32_t)(next64() % P);
        const Tables t(rc.data(), diag.data());
        if (!chain("mixtures", t) || !update_bound("mixtures", t.tab.data())) return 1;
        if (!run_forms("mixtures", st.data(), rc.data(), diag.data(), t)) return 1;
        if (!run_sponge("mixtures", data.data(), 3, rc.data(), diag.data(), t)) return 1;
    }
    {   // the shipped tables: chain, update bound, every form and sponges of 1..3 blocks on edge and random data
        const Tables t(ZKH_P2_ROUND_CONSTANTS, ZKH_P2_M_INT_DIAG);
        if (!chain("shipped tables", t) || !update_bound("shipped tables", t.tab.data())) return 1;
        for (int c = 0; c < n_edge + 200; c++) {
            for (auto& v : st) v = c < n_edge ? edge[c] : (uint32_t)(next64() % P);
            for (auto& v : data) v = c < n_edge ? edge[c] : (uint32_t)(next64() % P);
            if (c == n_edge) for (size_t i = 0; i < data.size(); i++) data[i] = st[i % CELLS] = (i & 1) ? (P + 1) / 2 : (P - 1) / 2;
            if (!run_forms("shipped tables", st.data(), ZKH_P2_ROUND_CONSTANTS, ZKH_P2_M_INT_DIAG, t)) return 1;
            for (int blocks = 1; blocks <= 3; blocks++)
                if (!run_sponge("shipped tables", data.data(), blocks, ZKH_P2_ROUND_CONSTANTS, ZKH_P2_M_INT_DIAG, t)) return 1;
        }
    }
    printf("poseidon2 caller forms == literal permutation and sponge on %ld cases; update bound and scale chain hold\n", checked);
    return 0;
}
