// ubench_sort.hip — an outside yardstick for the library's hand-written sort (zeth_amd/csrc/sort.hip, zkh_derive_sorted):
// rocprim::radix_sort_pairs on N = 2^LOG_N (u64 key, u32 value) pairs, the keys with KEY_BITS live bits (SYN-LOOKUP-sorted packs
// (addr, time) into 40), once over all 64 key bits and once told the live range [0, KEY_BITS).  Standalone: the library itself
// includes nothing of rocPRIM.  One JSON line per variant: the average time of REPS sorts (events on the null stream).
//   hipcc --offload-arch=gfx950 -O3 tools/ubench_sort.hip -o tools/ubench_sort && tools/ubench_sort [log_n] [key_bits] [reps]
#include <hip/hip_runtime.h>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                                   \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
    } while (0)

int main(int argc, char** argv) {
    const unsigned log_n = argc > 1 ? atoi(argv[1]) : 20, key_bits = argc > 2 ? atoi(argv[2]) : 40;
    const int reps = argc > 3 ? atoi(argv[3]) : 20;
    if (log_n < 8 || log_n > 26 || key_bits < 1 || key_bits > 64 || reps < 1) { fprintf(stderr, "usage: ubench_sort [log_n 8..26] [key_bits 1..64] [reps]\n"); return 2; }
    const size_t n = (size_t)1 << log_n;
    std::vector<uint64_t> keys(n);
    std::vector<uint32_t> vals(n);
    uint64_t s = 0x9e3779b97f4a7c15ull;
    for (size_t i = 0; i < n; i++) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;                     // xorshift64
        keys[i] = key_bits == 64 ? s : s & ((1ull << key_bits) - 1);
        vals[i] = (uint32_t)i;
    }
    uint64_t *k_in, *k_out;
    uint32_t *v_in, *v_out;
    CHECK(hipMalloc(&k_in, 8 * n)); CHECK(hipMalloc(&k_out, 8 * n)); CHECK(hipMalloc(&v_in, 4 * n)); CHECK(hipMalloc(&v_out, 4 * n));
    CHECK(hipMemcpy(k_in, keys.data(), 8 * n, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(v_in, vals.data(), 4 * n, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const unsigned ends[2] = {64, key_bits};
    for (unsigned end : ends) {
        size_t tmp_bytes = 0;
        CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, k_in, k_out, v_in, v_out, n, 0, end));
        void* tmp;
        CHECK(hipMalloc(&tmp, tmp_bytes));
        CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, k_in, k_out, v_in, v_out, n, 0, end));      // warm-up
        CHECK(hipDeviceSynchronize());
        CHECK(hipEventRecord(e0));
        for (int r = 0; r < reps; r++) CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, k_in, k_out, v_in, v_out, n, 0, end));
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        std::vector<uint64_t> out(n);
        CHECK(hipMemcpy(out.data(), k_out, 8 * n, hipMemcpyDeviceToHost));
        size_t unsorted = 0;
        for (size_t i = 1; i < n; i++) unsorted += out[i - 1] > out[i];
        printf("{\"bench\": \"rocprim_radix_sort_pairs\", \"pairs\": %zu, \"key_bits\": %u, \"sorted_bits\": %u, \"ms\": %.4f, \"tmp_MiB\": %.1f, "
               "\"unsorted\": %zu}\n", n, key_bits, end, ms / reps, tmp_bytes / 1048576.0, unsorted);
        CHECK(hipFree(tmp));
    }
    return 0;
}
