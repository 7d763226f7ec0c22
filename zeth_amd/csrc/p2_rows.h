// p2_rows.h — the Poseidon2 permutation as TRACE ROWS (zeth_amd/circuits/p2_join.py block_rows): what the witness generators of
// P2-JOIN (circuit.hip k_p2join_*) and P2-PAGE (page_circuit.hip k_page_*) share.  A block is 31 rows: the input, the state before
// each of the 29 rounds with the cubes of that round, the output.  The rounds themselves are literal (the trace needs every
// intermediate state).  Each generator keeps its round loop written out: as one shared function it compiled k_p2join_blocks to
// other instructions than the ones that were measured.
#pragma once
#include "common.h"
#include "poseidon2.h"

namespace zkh {

constexpr uint32_t PJ_T = 24, PJ_HALF = 4, PJ_RP = 21, PJ_ROUNDS = 29, PJ_BLOCK = 31;
__device__ __forceinline__ bool pj_is_full(uint32_t rnd) { return rnd < PJ_HALF || rnd >= PJ_HALF + PJ_RP; }
static __device__ void pj_m_ext(uint32_t (&c)[PJ_T]) {
    uint32_t sums[4] = {0, 0, 0, 0};
    for (uint32_t b = 0; b < PJ_T; b += 4) {
        m4(c[b], c[b + 1], c[b + 2], c[b + 3]);
        for (uint32_t i = 0; i < 4; i++) sums[i] = add_mod(sums[i], c[b + i]);
    }
    for (uint32_t k = 0; k < PJ_T; k++) c[k] = add_mod(c[k], sums[k & 3]);
}

// circuit.hip: the SHIPPED round constants and diagonal as Montgomery words on the device, rc[24 * 29] then diag[24]: the `tab` of both generators
const char* p2_rows_tables(zkh_ctx* ctx, Tmp& tab);
// page_circuit.hip: k_page_tail over the rows [first_row, n) of the `wd` columns of a data group: zero while active, blinding noise
// after.  What the generators of P2-PAGE and of P2-TREE (page_tree.hip) share for the rows past their last block.
const char* page_tail_rows(zkh_ctx* ctx, zkh_buf* data, uint32_t wd, size_t n, uint32_t A, uint32_t first_row, const NoiseKey& nk);

}  // namespace zkh
