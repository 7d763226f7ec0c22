// scan.h — the workgroup-wide inclusive scan every kernel of the library uses: one value per thread, THREADS lanes, log2(THREADS)
// double-buffered steps through LDS.
#pragma once
#include "common.h"

namespace zkh {

struct AddMod { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return add_mod(a, b); } };   // Fp words
struct AddWrap { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };          // counters

// Returns add(v_0, ..., v_t) for thread t of a workgroup of THREADS threads.  `buf` is the caller's __shared__ [2][THREADS]; every
// thread of the workgroup calls.  The scan ends on a barrier and a thread reads back only its own element, so the same buffer can
// carry the next scan at once.
template <uint32_t THREADS, typename Add>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t (*buf)[THREADS], Add add) {
    const uint32_t t = threadIdx.x;
    buf[0][t] = v;
    __syncthreads();
    int cur = 0;
    for (uint32_t d = 1; d < THREADS; d <<= 1) {
        uint32_t x = buf[cur][t];
        if (t >= d) x = add(x, buf[cur][t - d]);
        buf[cur ^ 1][t] = x;
        cur ^= 1;
        __syncthreads();
    }
    return buf[cur][t];
}

}  // namespace zkh
