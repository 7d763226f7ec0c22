// Host-side walk of the NTT plan (zeth_amd/csrc/ntt_plan.h: the header run_transform consumes) over every case a caller can reach:
// log_n 0..26, forward with every expand_bits 0..log_n, inverse with and without the zk shift (432 cases).  One line per case,
// "<key>\t<passes> | lazy<0|1>", in the format of tests/golden/ntt_plan.json (tests/test_ntt_plan.py compares them); and, whatever
// the fixture says, what every kernel needs of the pass it is given is asserted here: exit code 1 at the first violation.
// Build: g++ -O2 -std=c++17 -I zeth_amd/csrc tests/cpp/ntt_plan_test.cpp -o <out>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "ntt_plan.h"

using namespace zkh;

static std::string g_case;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "%s: violated: %s\n", g_case.c_str(), #cond); exit(1); } \
    } while (0)

static const char* short_name(NttKernel k) { return NTT_KERNEL_SCOPE[(int)k] + 7; }      // ":k_ntt_low12" -> "low12"

static void walk(uint32_t log_n, bool inverse, uint32_t expand_bits, bool zk) {
    char key[64];
    if (inverse) snprintf(key, sizeof key, "inv %u %s", log_n, zk ? "zk" : "plain");
    else snprintf(key, sizeof key, "fwd %u %u", log_n, expand_bits);
    g_case = key;
    const NttPlan plan = plan_transform(log_n, inverse, expand_bits, zk);
    const size_t npass = plan.passes.size();
    CHECK(npass >= 1 && npass <= 3);
    std::string line;
    uint32_t next = inverse ? log_n : 0;            // the passes tile [0, log_n): forward from bit 0 up, inverse from bit log_n down
    bool reg_radix = true;
    for (size_t pi = 0; pi < npass; pi++) {
        const PassPlan& p = plan.passes[pi];
        const bool first = pi == 0, last = pi + 1 == npass;
        if (inverse) { CHECK(p.L + p.R == next); next = p.L; }
        else { CHECK(p.L == next); next = p.L + p.R; }
        CHECK(p.lds_bytes <= 65536 && ((uint64_t)4 << (p.R + p.log_t)) <= 65536);
        CHECK(p.log_t <= p.L);
        CHECK(p.grid_x >= 1 && p.block >= 64 && p.block <= 1024);
        CHECK(p.twiddle == (p.L != 0));
        CHECK(p.scale == (inverse && last) && p.zk_shift == (inverse && last && zk));
        CHECK(p.expand_bits == ((!inverse && first) ? expand_bits : 0u));
        CHECK(p.first_layer == ((!inverse && first) ? std::min(expand_bits, p.R) + 1 : 1u));
        switch (p.kernel) {
        case NttKernel::low12:
            CHECK(p.L == 0 && p.R == 12 && p.expand_bits <= 4 && p.log_t == 0);
            CHECK(p.block == 256 && p.lds_bytes == 0 && ((uint64_t)p.grid_x << 12) == ((uint64_t)1 << log_n));
            break;
        case NttKernel::high8:
        case NttKernel::high10:
            CHECK(p.L >= 4 && p.log_t == 4 && p.R == (p.kernel == NttKernel::high8 ? 8u : 10u) && !p.scale && !p.zk_shift);
            CHECK(p.expand_bits == 0 && p.first_layer == 1);
            CHECK(p.L <= 14);                       // the kernel's 32-bit tile offsets: 2^(R + L + 2) <= 2^26 bytes
            CHECK(p.block == (1u << p.R) && p.lds_bytes == (4u << (p.R + 4)) && ((uint64_t)p.grid_x << (p.R + 4)) == ((uint64_t)1 << log_n));
            break;
        case NttKernel::top:
            CHECK(p.L >= 12 && p.L + p.R == log_n && (p.R == 1 || p.R == 3 || p.R == 4));
            CHECK(p.twiddle && p.expand_bits == 0 && p.first_layer == 1 && !p.scale && !p.zk_shift);
            CHECK(p.block == 256 && p.lds_bytes == 0 && p.log_t == 0 && ((uint64_t)p.grid_x << 10) == ((uint64_t)1 << p.L));
            break;
        case NttKernel::pass:
            CHECK(p.R <= 12 && p.block == 256 && p.lds_bytes == (4u << (p.R + p.log_t)));
            CHECK(((uint64_t)p.grid_x << (p.R + p.log_t)) == ((uint64_t)1 << log_n));
            break;
        }
        reg_radix = reg_radix && (p.kernel == NttKernel::low12 || p.kernel == NttKernel::high8 || p.kernel == NttKernel::high10);
        char buf[160];
        snprintf(buf, sizeof buf, "%s%s L%u R%u t%u f%u g%u b%u lds%u", pi ? "; " : "", short_name(p.kernel), p.L, p.R, p.log_t,
                 p.first_layer, p.grid_x, p.block, p.lds_bytes);
        line += buf;
    }
    CHECK(next == (inverse ? 0u : log_n));
    if (plan.lazy) {
        CHECK(!inverse && npass == 2 && reg_radix && expand_bits <= 4);
        CHECK(plan.lazy_reds == lazy_reductions(4, expand_bits) + 2 * lazy_reductions(4, 0) + lazy_reductions(plan.passes[1].R, 0));
    } else {
        CHECK(plan.lazy_reds == 0);
    }
    printf("%s\t%s | lazy%d\n", key, line.c_str(), plan.lazy ? 1 : 0);
}

int main() {
    for (uint32_t log_n = 0; log_n <= 26; log_n++) {
        for (uint32_t expand_bits = 0; expand_bits <= log_n; expand_bits++) walk(log_n, false, expand_bits, false);
        for (int zk = 0; zk < 2; zk++) walk(log_n, true, 0, zk != 0);
    }
    return 0;
}
