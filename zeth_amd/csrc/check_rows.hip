// check_rows.hip — zkh_check_rows: a witness checked against the circuit's own constraints on the device, row by row (DESIGN.md §2
// CHECK ROWS; the definition's host twin: zeth_amd/circuits/check.py reference_check_rows).  Every constraint of the step list is
// evaluated exactly on every row r of the TRACE domain (n = 2^po2 rows, not the 4n evaluation domain): no mix, no probability.
//   * a tap (g, col, back) reads row (r - back) mod n; a cell and a global word are read as their residues (raw % P);
//   * value steps compute in Fp, and in Fp4 (fp.h) downstream of a ConstExt;
//   * mix steps carry F, the lowest failing and_eqz step (its index in the ZKC1 step list) or NONE:
//       F(true) = NONE,  F(and_eqz(x, v)) = min(F(x), v != 0 ? this step : NONE),
//       F(and_cond(x, cond, inner)) = min(F(x), cond != 0 ? F(inner) : NONE),   an Fp4 is non-zero when any component is.
// Row r fails when F(ret) != NONE.  The program is the one zkh_circuit_load builds for the step interpreter of circuit.hip (same
// instructions, same slots, same LDS limit); an and_eqz instruction carries its step index in its `c` word, which that interpreter
// does not read.
#include "arguments.h"

using namespace zkh;

namespace {

constexpr uint32_t CHECK_THREADS = 128;      // the lanes the loader's LDS test (zkh_circuit::interp_ok) assumes
constexpr uint32_t INSN_WORDS = 6;

struct CheckRowsArgs {
    const uint32_t* groups[3];       // raw accum, code, data traces (W x n)
    const uint32_t* globals;         // out then mix, reduced below P
    uint32_t mix_at;                 // where mix starts in `globals`
    uint32_t n, row_lo, row_hi;
    unsigned long long* lowest;      // min over the window of row << 32 | F(ret); all ones = no row failed
    uint32_t* failing;               // rows of the window that fail
    uint32_t* per_row;               // null, or n words: F(ret) of every row of the window
    uint32_t probe_step;             // VALUE launches: the and_eqz step whose operand is written to `value` (4 Montgomery words)
    uint32_t* value;
};

// The lowest key of the wave into *status: only a wave that holds one reduces (the branch is wave-uniform) and issues one 64-bit
// atomicMin (the BadRow pattern of arguments.h with a key that differs in both halves from lane to lane).
__device__ __forceinline__ void report_lowest_key(unsigned long long* status, unsigned long long key) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off, 64);
        key = o < key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) atomicMin(status, key);
}

// One lane per trace row.  LDS: fp slots [slot][lane], then the 16-byte slots as four planes [slot][component][lane], so that every
// access is one word per lane at stride 1 (no bank conflict); a mix slot uses plane 0 alone.
// VALUE = false: the pass over [row_lo, row_hi).  VALUE = true: one workgroup on the row row_lo; the lane of that row writes the
// operand of the and_eqz step `probe_step`.
template <bool VALUE>
__global__ __launch_bounds__(CHECK_THREADS) void k_check_rows(CheckRowsArgs a, const uint32_t* __restrict__ prog, uint32_t n_insn,
                                                              const uint32_t* __restrict__ taps, uint32_t n_fp_slots, uint32_t ret_slot) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* fps = lds;                                              // [n_fp_slots][THREADS]
    uint32_t* wide = lds + (size_t)n_fp_slots * CHECK_THREADS;        // [n_wide_slots][4][THREADS]
    const uint32_t t = threadIdx.x;
    const uint32_t idx = a.row_lo + blockIdx.x * CHECK_THREADS + t;
    const bool in_window = idx < a.row_hi;
    const uint32_t row = in_window ? idx : a.row_hi - 1;              // lanes past the window stay in step on its last row (no store)
    const uint32_t mask = a.n - 1;
    auto fp_operand = [&](uint32_t kind, uint32_t x) -> uint32_t {
        switch (kind) {
        case OPK_FP: return fps[x * CHECK_THREADS + t];
        case OPK_TAP: {
            const uint32_t g = taps[3 * x], off = taps[3 * x + 1], back = taps[3 * x + 2];
            return a.groups[g][(size_t)off * a.n + ((row - back) & mask)] % P; }
        case OPK_CONST: return x;
        default: return a.globals[(x >> 16 ? a.mix_at : 0) + (x & 0xffffu)];
        }
    };
    auto load_ext = [&](uint32_t slot) -> Fp4 {
        const uint32_t* p = wide + (size_t)slot * 4 * CHECK_THREADS + t;
        return Fp4(Fp::raw(p[0]), Fp::raw(p[CHECK_THREADS]), Fp::raw(p[2 * CHECK_THREADS]), Fp::raw(p[3 * CHECK_THREADS]));
    };
    auto store_ext = [&](uint32_t slot, const Fp4& v) {
        uint32_t* p = wide + (size_t)slot * 4 * CHECK_THREADS + t;
        p[0] = v.c[0].v; p[CHECK_THREADS] = v.c[1].v; p[2 * CHECK_THREADS] = v.c[2].v; p[3 * CHECK_THREADS] = v.c[3].v;
    };
    auto ext_operand = [&](uint32_t kind, uint32_t x) -> Fp4 {
        if (kind == OPK_EXT) return load_ext(x);
        return Fp4(Fp::raw(fp_operand(kind, x)));
    };
    auto nonzero = [&](uint32_t kind, uint32_t x) -> bool {
        if (kind != OPK_EXT) return fp_operand(kind, x) != 0;
        const Fp4 v = load_ext(x);
        return (v.c[0].v | v.c[1].v | v.c[2].v | v.c[3].v) != 0;
    };
    auto mix = [&](uint32_t slot) -> uint32_t& { return wide[(size_t)slot * 4 * CHECK_THREADS + t]; };
    for (uint32_t pc = 0; pc < n_insn; pc++) {
        const uint32_t* in = prog + pc * INSN_WORDS;
        const uint32_t opw = in[0], dst = in[1], x = in[2], y = in[3], z = in[4], w = in[5];
        const uint32_t op = opw & 0xffu, ka = (opw >> 8) & 7u, kb = (opw >> 11) & 7u;
        const bool dst_ext = (opw >> 14) & 1u;
        switch (op) {
        case OP_CONST_EXT: store_ext(dst, Fp4(Fp::raw(x), Fp::raw(y), Fp::raw(z), Fp::raw(w))); break;
        case OP_ADD: case OP_SUB: case OP_MUL:
            if (dst_ext) {
                const Fp4 l = ext_operand(ka, x), r = ext_operand(kb, y);
                store_ext(dst, op == OP_ADD ? l + r : (op == OP_SUB ? l - r : l * r));
            } else {
                const uint32_t l = fp_operand(ka, x), r = fp_operand(kb, y);
                fps[dst * CHECK_THREADS + t] = op == OP_ADD ? add_mod(l, r) : (op == OP_SUB ? sub_mod(l, r) : mul_mod(l, r));
            }
            break;
        case OP_TRUE: mix(dst) = NONE; break;
        case OP_AND_EQZ: {   // z = this step's index in the ZKC1 step list
            if (VALUE && z == a.probe_step && t == 0) {
                const Fp4 v = ext_operand(kb, y);
                for (int i = 0; i < 4; i++) a.value[i] = v.c[i].v;
            }
            const uint32_t here = nonzero(kb, y) ? z : NONE, before = mix(x);
            mix(dst) = before < here ? before : here;
            break; }
        case OP_AND_COND: {  // z = the inner chain's slot
            const uint32_t inner = nonzero(kb, y) ? mix(z) : NONE, before = mix(x);
            mix(dst) = before < inner ? before : inner;
            break; }
        }
    }
    if (VALUE) return;
    const uint32_t f = in_window ? mix(ret_slot) : NONE;
    if (a.per_row && in_window) a.per_row[row] = f;
    const unsigned long long failed = __ballot(f != NONE);
    if (failed != 0) {
        report_lowest_key(a.lowest, f != NONE ? ((unsigned long long)row << 32) | f : ~0ull);
        if ((t & 63) == 0) atomicAdd(a.failing, (uint32_t)__popcll(failed));
    }
}

template <bool VALUE>
const char* launch(zkh_ctx* ctx, const zkh_circuit* c, const CheckRowsArgs& a, size_t lds) {
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)k_check_rows<VALUE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return make_err("check_rows: %zu bytes of LDS for the interpreter: %s", lds, hipGetErrorString(e));
    }
    const size_t rows = (size_t)a.row_hi - a.row_lo;
    k_check_rows<VALUE><<<(unsigned)((rows + CHECK_THREADS - 1) / CHECK_THREADS), CHECK_THREADS, lds, ctx->stream>>>(
        a, c->d_prog, (uint32_t)c->prog.size(), c->d_taps, c->n_fp_slots, c->ret_slot);
    return last_launch_error("check_rows");
}

}  // namespace

extern "C" const char* zkh_check_rows(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, const zkh_buf* const* groups, size_t n_groups,
                                      const uint32_t* out_global, const uint32_t* mix_global, size_t row_lo, size_t row_hi,
                                      zkh_buf* per_row, zkh_check_rows_result* result) {
    ZKH_REQUIRE(ctx && c && groups && result, "check_rows: null argument");
    ZKH_REQUIRE(c->ctx == ctx && c->d_prog, "check_rows: circuit was not loaded on this context");
    ZKH_REQUIRE(n_groups == 3, "check_rows: expected 3 register groups (accum, code, data), got %zu", n_groups);
    ZKH_REQUIRE(po2 >= 1 && po2 <= 24, "check_rows: po2 %zu out of range (1..24)", po2);
    const size_t n = (size_t)1 << po2;
    for (int g = 0; g < 3; g++) {
        ZKH_REQUIRE(groups[g], "check_rows: group %d is null", g);
        ZKH_REQUIRE(groups[g]->len == (size_t)c->group_size[g] * n, "check_rows: group %d has %zu words, expected %zu", g, groups[g]->len,
                    (size_t)c->group_size[g] * n);
    }
    ZKH_REQUIRE((out_global || !c->global_size[GLOBAL_OUT]) && (mix_global || !c->global_size[GLOBAL_MIX]), "check_rows: the globals (out, mix) are required");
    ZKH_REQUIRE(row_lo < row_hi && row_hi <= n, "check_rows: window [%zu, %zu) is empty or outside [0, %zu]", row_lo, row_hi, n);
    ZKH_REQUIRE(!per_row || per_row->len == n, "check_rows: the per-row buffer has %zu words, expected %zu", per_row ? per_row->len : 0, n);
    if (!c->interp_ok)
        return make_err("check_rows: the step list has more live values than the interpreter's LDS holds");
    bind_thread(ctx);
    const size_t lds = ((size_t)c->n_fp_slots * 4 + (size_t)c->n_mix_slots * 16) * CHECK_THREADS;

    const uint32_t n_out = c->global_size[GLOBAL_OUT], n_mix = c->global_size[GLOBAL_MIX];
    std::vector<uint32_t> gl(n_out + n_mix + 1, 0);
    for (uint32_t i = 0; i < n_out; i++) gl[i] = out_global[i] % P;
    for (uint32_t i = 0; i < n_mix; i++) gl[n_out + i] = mix_global[i] % P;
    Tmp dgl, status;
    ZKH_TRY(zkh_copy_from(ctx, "check_rows_globals", gl.data(), gl.size(), dgl.out()));
    ZKH_TRY(new_buf(ctx, 8, false, status.out()));           // [0, 2): lowest key; [2]: failing rows; [4, 8): the failing step's value
    ZKH_HIP(hipMemsetAsync(status->ptr(), 0xff, 8, ctx->stream));
    ZKH_HIP(hipMemsetAsync(status->ptr() + 2, 0, 24, ctx->stream));

    CheckRowsArgs a{};
    for (int g = 0; g < 3; g++) a.groups[g] = groups[g]->ptr();
    a.globals = dgl->ptr();
    a.mix_at = n_out;
    a.n = (uint32_t)n; a.row_lo = (uint32_t)row_lo; a.row_hi = (uint32_t)row_hi;
    a.lowest = (unsigned long long*)status->ptr();
    a.failing = status->ptr() + 2;
    a.per_row = per_row ? per_row->ptr() : nullptr;
    a.probe_step = NONE;
    a.value = status->ptr() + 4;
    {
        size_t total_w = 0;
        for (int g = 0; g < 3; g++) total_w += c->group_size[g];
        ProfScope prof(ctx, "check_rows", 4.0 * total_w * (double)(row_hi - row_lo) + (per_row ? 4.0 * (double)(row_hi - row_lo) : 0.0));
        ZKH_TRY(launch<false>(ctx, c, a, lds));
    }
    uint32_t st[8];
    ZKH_TRY(zkh_read(ctx, status, st, 0, 3));
    result->row = -1; result->step = NONE; result->failing_rows = 0;
    for (int i = 0; i < 4; i++) result->value[i] = 0;
    if ((st[0] & st[1]) == NONE) return nullptr;
    result->row = st[1]; result->step = st[0]; result->failing_rows = st[2];
    a.row_lo = st[1]; a.row_hi = st[1] + 1; a.probe_step = st[0]; a.per_row = nullptr;
    ZKH_TRY(launch<true>(ctx, c, a, lds));
    ZKH_TRY(zkh_read(ctx, status, st + 4, 4, 4));
    for (int i = 0; i < 4; i++) result->value[i] = fp_decode(Fp::raw(st[4 + i]));
    return nullptr;
}
