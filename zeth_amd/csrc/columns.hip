// columns.hip — derived-column records (ZKA1 version 4; zeth_amd/circuits/logup.py `reference_columns`; DESIGN.md §2 ARGUMENTS): data
// columns that are a row-wise function of other columns, filled on the device.
//
// x(c, r) = the canonical value of the raw Montgomery word of column c at row r (raw words >= P are legal).  Over the active rows r < A:
//   LIMBS  dst_j[r] = Montgomery((x(src, r) >> jL) & (2^L - 1)), j < nl; refused when x >= 2^(L nl).
//   ORDER  row 0: zeros.  r >= 1, one key:  d = k0[r] - k0[r-1];
//                         two keys: e = [k0[r] == k0[r-1]], d = e ? k1[r] - k1[r-1] : k0[r] - k0[r-1] - 1, the flag column = Montgomery(e);
//          the limb columns hold d as LIMBS holds x; refused when d < 0 ("not ordered") or d >= 2^(L nl).
// Rows [A, n) are never touched.
//
// Two passes of one kernel over all records at once (grid.y = the record), four consecutive rows per lane: sources are read and
// destinations written as one 16-byte access per lane and column (columns start 16-byte aligned: c * n words, n a multiple of 4), the
// last rows below A (A is odd in general) and traces of fewer than 4 rows one word at a time.  An ORDER lane also reads the row before
// its four.  The check pass reads the sources only and reduces the first bad (record, row): one 64-bit atomicMin per wave that found
// one.  The host reads that word back; only a witness that passed is written (the write pass), so a refusal leaves `data` unchanged.
// Sources are never destinations (set_arguments), so the passes of one call see the same sources and no lane reads what another writes.
#include "arguments.h"

using namespace zkh;

namespace {

constexpr uint32_t COL_THREADS = 256, COL_ROWS = 4;      // rows per lane: one dwordx4 per column

// rows [r0, r0 + cnt) of a column as canonical values; vec: a full, aligned quad
__device__ __forceinline__ void load_rows(const uint32_t* __restrict__ col, uint32_t r0, uint32_t cnt, bool vec, uint32_t v[COL_ROWS]) {
    if (vec) {
        const uint4 q = *reinterpret_cast<const uint4*>(col + r0);
        v[0] = canonical(q.x); v[1] = canonical(q.y); v[2] = canonical(q.z); v[3] = canonical(q.w);
    } else {
#pragma unroll
        for (uint32_t j = 0; j < COL_ROWS; j++) v[j] = j < cnt ? canonical(col[r0 + j]) : 0;
    }
}
__device__ __forceinline__ void store_rows(uint32_t* __restrict__ col, uint32_t r0, uint32_t cnt, bool vec, const uint32_t v[COL_ROWS]) {
    if (vec) {
        *reinterpret_cast<uint4*>(col + r0) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (uint32_t j = 0; j < COL_ROWS; j++)
            if (j < cnt) col[r0 + j] = v[j];
    }
}

// grid (ceil(A / (COL_THREADS * COL_ROWS)), records).  kWrite = false: the check pass (status = the lowest bad record << 32 | row);
// kWrite = true: the write pass over a witness that passed.  The record's words are read through the uniform pointer (scalar loads).
template <bool kWrite>
__global__ __launch_bounds__(COL_THREADS) void k_columns(const uint32_t* __restrict__ code, uint32_t* data, const Record* __restrict__ recs,
                                                         uint32_t n, uint32_t A, unsigned long long* __restrict__ status) {
    const Record* __restrict__ rec = recs + blockIdx.y;
    const uint32_t r0 = (blockIdx.x * COL_THREADS + threadIdx.x) * COL_ROWS;
    const uint32_t cnt = r0 >= A ? 0 : A - r0 < COL_ROWS ? A - r0 : COL_ROWS;
    const bool vec = cnt == COL_ROWS && (n & 3) == 0;
    const uint32_t L = rec->L, nl = rec->nl, bits = L * nl;
    const bool order = rec->kind == KIND_ORDER, two = rec->n_src == 2;
    uint32_t flag[COL_ROWS] = {0, 0, 0, 0};
    long long d[COL_ROWS] = {0, 0, 0, 0};
    if (cnt) {
        const uint32_t* k0p = group_ptr(code, data, rec->sg[0]) + (size_t)rec->sc[0] * n;
        uint32_t k0[COL_ROWS];
        load_rows(k0p, r0, cnt, vec, k0);
        if (!order) {
#pragma unroll
            for (uint32_t j = 0; j < COL_ROWS; j++) d[j] = k0[j];
        } else {
            uint32_t p0 = r0 ? canonical(k0p[r0 - 1]) : 0;
            if (!two) {
#pragma unroll
                for (uint32_t j = 0; j < COL_ROWS; j++) { d[j] = r0 + j ? (long long)k0[j] - p0 : 0; p0 = k0[j]; }
            } else {
                const uint32_t* k1p = group_ptr(code, data, rec->sg[1]) + (size_t)rec->sc[1] * n;
                uint32_t k1[COL_ROWS];
                load_rows(k1p, r0, cnt, vec, k1);
                uint32_t p1 = r0 ? canonical(k1p[r0 - 1]) : 0;
#pragma unroll
                for (uint32_t j = 0; j < COL_ROWS; j++) {
                    const bool e = r0 + j && k0[j] == p0;
                    flag[j] = e ? R1 : 0;
                    d[j] = !(r0 + j) ? 0 : e ? (long long)k1[j] - p1 : (long long)k0[j] - p0 - 1;
                    p0 = k0[j]; p1 = k1[j];
                }
            }
        }
    }
    if (!kWrite) {
        uint32_t bad = NONE;                             // this lane's first row that is refused
#pragma unroll
        for (uint32_t j = COL_ROWS; j-- > 0;)
            if (j < cnt && (d[j] < 0 || (d[j] >> bits) != 0)) bad = r0 + j;
        report_bad_row(status, blockIdx.y, bad);
        return;
    }
    if (!cnt) return;
    uint32_t e0 = 0;
    if (order && two) {
        store_rows(data + (size_t)rec->dst[0] * n, r0, cnt, vec, flag);
        e0 = 1;
    }
    const uint32_t mask = (uint32_t)((1ull << L) - 1);
    for (uint32_t j = 0; j < nl; j++) {
        uint32_t v[COL_ROWS];
#pragma unroll
        for (uint32_t i = 0; i < COL_ROWS; i++) v[i] = fp_encode((uint32_t)((unsigned long long)d[i] >> (j * L)) & mask).v;
        store_rows(data + (size_t)rec->dst[e0 + j] * n, r0, cnt, vec, v);
    }
}

}  // namespace

extern "C" const char* zkh_derive_columns(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data) {
    ZKH_REQUIRE(ctx && c && data, "derive_columns: null argument");
    ZKH_REQUIRE(code, "derive_columns: the raw code trace is required (the code-group source columns of the records read it)");
    ZKH_REQUIRE(zkh_circuit_derives_columns(c), "derive_columns: the circuit's arguments hold no derived-column record (ZKA1 version 4)");
    size_t n;
    uint32_t A;
    ZKH_TRY(trace_rows("derive_columns", c, po2, zk_cycles, code, data, nullptr, &n, &A));
    const std::vector<Record>& recs = c->args->records;
    ZKH_REQUIRE(recs.size() <= 65535, "derive_columns: %zu records in one blob (at most 65535)", recs.size());
    bind_thread(ctx);
    static_assert(sizeof(Record) % 4 == 0, "word records");
    Tmp drecs;
    BadRow bad;
    ZKH_TRY(zkh_copy_from(ctx, "column_records", (const uint32_t*)recs.data(), recs.size() * (sizeof(Record) / 4), drecs.out()));
    ZKH_TRY(bad.init(ctx));
    double src_words = 0, dst_words = 0;                 // per row: the sources of every record, its destinations
    for (const Record& r : recs) { src_words += r.n_src; dst_words += r.n_dst; }
    const dim3 grid((unsigned)((A + COL_THREADS * COL_ROWS - 1) / (COL_THREADS * COL_ROWS)), (unsigned)recs.size());
    const Record* d_recs = (const Record*)drecs->ptr();
    {
        ProfScope prof(ctx, "columns_check", 4.0 * src_words * A);
        k_columns<false><<<grid, COL_THREADS, 0, ctx->stream>>>(code->ptr(), data->ptr(), d_recs, (uint32_t)n, A, bad.ptr());
        ZKH_TRY(last_launch_error("columns_check"));
    }
    ZKH_TRY(bad.read(ctx));
    if (bad.found) {
        const uint32_t i = bad.hi, row = bad.lo;
        const Record& r = recs[i];
        long long k[2] = {0, 0}, p[2] = {0, 0};
        for (uint32_t s = 0; s < r.n_src; s++) {
            ZKH_TRY(read_cell(ctx, code, data, r.sg[s], r.sc[s], n, row, &k[s]));
            if (r.kind == KIND_ORDER) ZKH_TRY(read_cell(ctx, code, data, r.sg[s], r.sc[s], n, row - 1, &p[s]));   // row 0 is never refused
        }
        if (r.kind == KIND_LIMBS)
            return make_err("derive_columns: record %u at row %u: the value %lld does not fit %u limbs of %u bits: the witness is refused", i, row, k[0], r.nl, r.L);
        const long long d = r.n_src == 1 ? k[0] - p[0] : k[0] == p[0] ? k[1] - p[1] : k[0] - p[0] - 1;
        if (d < 0) return make_err("derive_columns: record %u at row %u: not ordered (difference %lld): the witness is refused", i, row, d);
        return make_err("derive_columns: record %u at row %u: the difference %lld does not fit %u limbs of %u bits: the witness is refused", i, row, d, r.nl, r.L);
    }
    {
        ProfScope prof(ctx, "columns_write", 4.0 * (src_words + dst_words) * A);
        k_columns<true><<<grid, COL_THREADS, 0, ctx->stream>>>(code->ptr(), data->ptr(), d_recs, (uint32_t)n, A, bad.ptr());
        ZKH_TRY(last_launch_error("columns_write"));
    }
    return nullptr;
}
