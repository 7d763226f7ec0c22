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

// THE HEADS STAGE of a compaction over m items, item t on lane threadIdx.x of its workgroup (t >= m: `head` is 0): local[t] = the heads
// among the items of t's workgroup up to t, sums[blockIdx.x] = the workgroup's heads.  The counter scan (sort.h scan_counters) turns `sums`
// into the heads of the workgroups before each one; then head_rank, given the same `sums`, is the rank of the head at item t.
template <uint32_t THREADS>
__device__ __forceinline__ void scan_heads(uint32_t head, uint32_t t, uint32_t m, uint32_t (*buf)[THREADS], uint32_t* __restrict__ local, uint32_t* __restrict__ sums) {
    const uint32_t incl = block_scan<THREADS>(head, buf, AddWrap());
    if (t < m) local[t] = incl;
    if (threadIdx.x == THREADS - 1) sums[blockIdx.x] = incl;
}
__device__ __forceinline__ uint32_t head_rank(const uint32_t* __restrict__ local, const uint32_t* __restrict__ sums, uint32_t t) { return local[t] + sums[blockIdx.x] - 1; }

}  // namespace zkh
