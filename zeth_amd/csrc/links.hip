// links.hip — LINK records (ZKA1 version 5; zeth_amd/circuits/logup.py `reference_links`; DESIGN.md §2 ARGUMENTS): every memory access
// gets the previous access to its own address, on the device; and (version 6) a load is checked to return the last store.
//
// x(c, r) = the canonical value of the raw Montgomery word of column c at row r (raw words >= P are legal).  A row r < A is an ACCESS
// of a record when its selector is 1 (no selector: every active row).  For an access r with key K = x(key, r), r' = the greatest
// access below r with key K:
//   linked[r] = Montgomery([r' exists]);   last[r] = Montgomery([no access above r has key K]);
//   prev_j[r] = the raw word of carried column c_j at r' (a copy), 0 when r is not linked;
//   limb_j[r] = Montgomery(limb j of d = x(c_0, r) - x(c_0, r') - 1), 0 when r is not linked; refused when d < 0 ("clock not increasing")
//               or d >= 2^(L nl).
// Active rows that are no access get zeros in every destination; rows [A, n) are never touched.
//
// THE READ RULE (a record with READS, ZKA1 version 6): a load returns the last store.  With w(r) = x(write flag, r) on an access r:
// w(r) not 0 / 1 is refused; a store (w = 1) is free; a load (w = 0) is refused unless, for every carried column j = 1 .. nc - 1 (the
// clock c_0 is exempt), x(c_j, r) = x(c_j, r') when r is linked and x(c_j, r) = 0 when it is not (memory starts zeroed).  Residues
// mod P are compared: a raw word P is a zero.  The rule adds no destination.  On one row the order is write flag, clock, read rule
// (lowest j first), and the lowest (record, row) over all of these is the one refusal reported.
//
// sort_rows (sort.h; the passes and kernels of sort.hip) sorts every record's accesses by key, stably: position j of the sorted order
// holds (packed key, row), equal keys in row order, so the previous access of the row at j is the row at j - 1 when the keys are equal,
// and it is the last one when the key at j + 1 differs.  Then two passes of one kernel over all records at once (grid.y = the record),
// one lane per sorted position: the neighbours' keys and rows are coalesced loads, the carried cells at row(j - 1) and the clock at row(j)
// random ones (with READS the check pass also reads the write flag at row(j) and, for a load, the value cells at row(j) and row(j - 1):
// random 4-byte reads like the clock's).  The check pass reads only and reduces the first bad (record, row): one 64-bit atomicMin per
// wave that found one.  The host reads that word back; only a witness that passed is written (the write pass: the destinations at row(j), 4-byte scattered
// stores, and zeros on the active rows that are no access, coalesced), so a refusal leaves `data` unchanged.  Sources are never
// destinations (set_arguments), so both passes see the same sources and no lane reads what another writes.  Selectors are refused by
// the sort's key pass, over all records, before any clock is read.
//
// PAGING (a PAGES record, ZKA1 version 7; `reference_links(..., image)`): the memory of ONE record, the paged one (READS, nc = 2: a clock and
// one value), starts from an image of W raw Montgomery words, image[a] the word of address a = x(key, r); a >= W is refused ("address A
// outside the image of W words").  An UNLINKED access r of the paged record takes the image as its previous access: prev_1[r] = the raw word
// image[a] (a copy), prev_0[r] = 0 (clock 0 is the image's), the limbs those of d = x(clock, r) - 0 - 1; "clock 0 is the image's" refuses a
// clock 0, the range refusal a d that does not fit, and an unlinked load must return image[a] (residues) where it had to return 0.  linked
// and last keep their meaning; linked accesses and the other records are untouched.  On one row the order is write flag, address, clock, read
// rule.  THE PAGE TABLE: a_0 < .. < a_{D-1} the distinct addresses of the record's accesses; on the active rows i < D p_on = Montgomery(1),
// p_addr = the raw key word of a_i's first access, p_in = the raw word image[a_i], p_out / p_time = the raw value / clock word of a_i's last
// access, alimb_j = limb j of a_i (refused, under the PAGES record's index, when a_i >= 2^(L ng)), gap_j = limb j of a_i - a_{i-1} - 1 (zeros
// on row 0); active rows [D, A) get zeros in all destinations, rows [A, n) are never touched.  Writing the table back into the image,
// the page-out, has a file of its own.
//
// The paged passes reuse the one sort, and they are the same kernel (k_links<.., kPaged>: one body for the link semantics and the read rule;
// the plain passes compile the paging out).  Position t of the paged record is a HEAD when the packed key at t - 1 differs (the first access
// of its address) and a TAIL when the one at t + 1 does: neighbouring packed keys, coalesced.  An inclusive scan of the head flags over the m
// sorted positions gives every position its page index + 1: k_page_heads is the heads stage (scan.h scan_heads), the sort's counter scan
// (sort.h scan_counters, ONE workgroup, so none waits for another) leaves the carries and D, head_rank is the index.  The paged check pass adds the image reads and
// the new refusals to the same wave minimum and the same atomicMin; the paged write pass also fills the table — head lanes p_on, p_addr,
// p_in, alimb and gap (the previous address re-read from the trace at rows[t - 1]: packed keys drop bits and are no addresses), tail lanes
// p_out and p_time, lanes D <= t < A zeros (coalesced).  No atomic but that min: the result is a function of the traces and the image.
//
// PAGING FROM A PAGE TABLE (zkh_derive_links_paged_table; `reference_links(..., table=, image_words=)`): the image's words reach the derive as
// the rows (a_i, in_i, out_i) of a ZKU1 table, where it lies in a device buffer (rows of 3 words from word `table_at`; a_i an integer, in_i
// the raw word that stands for image[a_i]), in place of the W words.  Only an unlinked access of the paged record uses the image's word, and
// it is a head: the page scan has run before the check pass, so head_rank gives its page i, and image[a] is table[3 i + 1] once table[3 i]
// is a: one indexed read and one comparison per head, no search, no W-word buffer.  This is the third mode of k_links' paging parameter
// (PAGED_TABLE); the plain and the image passes are the instantiations they were.  Three refusals are its own, under the PAGES record's index:
// a head whose page the table does not have ("the page table has D rows"), a head whose row of the table holds another address, both
// tested on the row after "outside the image" and before the clock; and, when no row is refused, a table of more rows than the trace pages,
// which the host reads off the scan's total (it comes back in the check pass's one read-back).  The table is only read.
//
// PORTS (a LINK record with JOINS, ZKA1 version 9; `reference_links`' merged order): a memory is a run of k <= 8 consecutive records, the head
// and the records that join it, and its accesses are the (row, port) whose record's selector is 1, in that order.  sort_rows sorts a MEMORY's
// accesses as one run (sort.h: one lane per virtual row v = row k + port, the masks per memory), so position t holds (packed key, v) in (key,
// row, port) order and the neighbours t - 1 and t + 1 still give linked, head and tail.  k_links<.., kPorts> runs over memories (grid.y): the
// lane's record is links[first + v % k] and its row v / k, the previous access's record and row those of the neighbour's v; sources and
// destinations are the lane's own port's, the previous cells the neighbour's port's.  The record's fields are then per lane, not uniform:
// only this instantiation pays for that, a blob without a joiner runs the instantiations it always ran.  The refused (record, row) is the
// port's own record's, a 64-bit minimum per wave.  The page scan, head_rank and k_page_of run over the memory's run.
//
// WIDE (ZKA1 version 10; logup.py states it once): the paged memory holds V = 2 value words per address, the paged LINK carries nc = 3.
// The image is FLAT, V W raw words, word j of address a at image[V a + j] (a length that is no multiple of V is refused before any launch;
// W counts addresses).  An unlinked access takes prev_{1+j} = image[V a + j] and prev_0 = 0, an unlinked load must return both words
// (residues; the host names the lowest j first).  The head lane of page i writes p_in_j, the tail lane p_out_j from its own record's value
// columns; the PAGES record's destinations are p_on, p_addr, p_in_0 .., p_out_0 .., p_time, alimb_*, gap_* (arguments.h pg_out, pg_time,
// pg_limbs).  V is k_links' compile-time kV, in image and table mode, with and without ports; a blob with V = 1 launches the
// instantiations it always launched.  IMAGE MODE: the two words of an address are adjacent and 8-byte aligned (the image's first word is:
// checked before the launch), so they are ONE 64-bit load.  TABLE MODE: the table is the FLAT one, V rows (V a + j, in_j, out_j) per page,
// i major: the head of page i reads rows V i + j (`table_at` is arbitrary: 4-byte loads) and checks each row's address against V a + j; D'
// pages of the trace must meet V D' rows, and the three table refusals name the flat row.
//
// FLAT (ZKA1 version 11; logup.py states it once): a PAGES record with V = 2 may have two more destinations, p_flat_0 and p_flat_1
// (Pages::flat, behind every field the existing kernels read).  The head lane of page i stores fp_encode(2 addr + j) there, next to
// p_in_j: canonical, from the decoded address (p_addr stays the raw key word), and 2 addr + 1 < 2^30 because the check pass has refused
// an address the limbs do not hold.  The rows below the table zero the two columns with the rest.  kFlat is a compile-time parameter of
// the four wide WRITE instantiations (image and table mode, with and without ports): a blob without flats launches what it launched, and
// the check passes do not know it.  No launch and no profile scope is added.
#include <algorithm>
#include <cstdio>
#include <functional>

#include "scan.h"
#include "sort.h"

using namespace zkh;

namespace {

constexpr uint32_t LINK_THREADS = 256;

// ---- paging ----
constexpr uint32_t PG_TOTAL = 0;                        // word 0 of the carry buffer: D, the pages; the workgroups' carries follow from word 1

// what the paged passes of k_links read on top of the plain ones'; the plain passes get a zeroed one and read none of it
enum : int { PAGED_NO = 0, PAGED_IMAGE = 1, PAGED_TABLE = 2 };      // k_links' kPaged: no PAGES record; the image as W words; the image as a page table
struct Paging {
    const Pages* pg;                                    // the PAGES record
    uint32_t paged;                                     // the place among the LINK records of the record it pages
    const uint32_t* image;                              // PAGED_TABLE: the table's rows of 3 words (address, in, out); kV = 2: the flat image, the flat table
    uint32_t W;                                         // the image's addresses (kV = 1: its words)
    uint32_t rows;                                      // PAGED_TABLE: the table's (flat) rows
    const uint32_t *local, *sums;                       // the page scan: k_page_heads' local indices; D and the workgroups' carries
};
// what the ported passes of k_links (kPorts) read on top: the memories, the items a run can hold (sort.h SortedRows::cap) and the number of
// LINK records, under which the PAGES record's own refusal is reported; the other passes get a zeroed one and read none of it
struct Ports {
    const Memory* runs;
    uint32_t cap, records;
};

// grid ceil(m_max / LINK_THREADS) over the sorted positions of the paged record (its place p among the LINK records; with ports: the paged
// memory's place among the memories, and A the items a run can hold): the heads stage
__global__ __launch_bounds__(LINK_THREADS) void k_page_heads(const uint32_t* __restrict__ status, const unsigned long long* __restrict__ keys, uint32_t p, uint32_t A,
                                                             uint32_t* __restrict__ local, uint32_t* __restrict__ sums) {
    __shared__ uint32_t buf[2][LINK_THREADS];
    const uint32_t m = status[ST_HEAD + ST_WORDS * p + ST_M];
    const uint32_t t = blockIdx.x * LINK_THREADS + threadIdx.x;
    const size_t base = (size_t)p * A;
    const uint32_t head = t < m && (t == 0 || keys[base + t - 1] != keys[base + t]);
    scan_heads<LINK_THREADS>(head, t, m, buf, local, sums + 1);
}

// grid (ceil(A / LINK_THREADS), records).  kWrite = false: the check pass (bad = the lowest bad record << 32 | row, the record by its place
// among the LINK records; the PAGES record's own refusal under the place `records`: it comes after every LINK); kWrite = true: the write
// pass over a witness that passed.  kReads: the check pass of a blob in which a record has READS; the flag is uniform per record, so the
// branch is scalar, and which rule a row broke the host finds out by reading its few cells back.  kPaged: the blob has a PAGES record, and
// `pages` says whether blockIdx.y is the record it pages (uniform: a scalar branch); without kPaged `pages` is the constant false, `word`
// the constant 0, and nothing of `pa` is read.  kPaged = PAGED_TABLE: the image's word of a head is its row's of the page table, and a head that the
// table does not list is refused.  The record's words are read through the uniform pointer (scalar loads): nothing is indexed
// in registers.
// kPorts (the blob has a LINK that joins): grid (ceil(cap / LINK_THREADS), memories), blockIdx.y the memory and `pages` whether it is the
// paged one; the item's source id v gives the lane its own record, links[first + v % k], and its row v / k, the neighbour's v the record and
// row of the previous access (`prec`, prow): the record's words are per-lane loads here, and nowhere else.
// kV (the paged instantiations): the value words per address of the paged memory, 1 or 2 (this file's header, WIDE).
// kFlat (the write passes with kV = 2): the PAGES record has the flat-address destinations (this file's header, FLAT).
template <bool kWrite, bool kReads, int kPaged, bool kPorts = false, int kV = 1, bool kFlat = false>
__global__ __launch_bounds__(LINK_THREADS) void k_links(const uint32_t* __restrict__ code, uint32_t* data, const Link* __restrict__ links,
                                                        const uint32_t* __restrict__ status, const unsigned long long* __restrict__ keys,
                                                        const uint32_t* __restrict__ rows, uint32_t n, uint32_t A, unsigned long long* __restrict__ bad,
                                                        const Paging pa, const Ports po) {
    const uint32_t p = blockIdx.y;
    const Link* const first = links + (kPorts ? po.runs[p].first : p);      // kPorts: the memory's head, port 0
    const uint32_t k = kPorts ? po.runs[p].k : 1;
    const Link* __restrict__ rec = first;                                    // the lane's record; kPorts: its own port's, once its item is read
    const Link* __restrict__ prec = first;                                   // the record of the access before it: kPorts: the neighbour's port's
    const bool pages = kPaged != PAGED_NO && p == pa.paged;
    const uint32_t m = status[ST_HEAD + ST_WORDS * p + ST_M];                 // the record's accesses: m <= A (kPorts: the memory's, m <= k A)
    const uint32_t t = blockIdx.x * LINK_THREADS + threadIdx.x;             // a sorted position (t < m) and, in the write pass, a row (t < A)
    const size_t base = (size_t)p * (kPorts ? po.cap : A);
    const bool access = t < m;
    uint32_t row = 0, prow = 0;
    bool linked = false, last = false;
    if (access) {
        const unsigned long long key = keys[base + t];
        row = rows[base + t];
        if (t) {
            linked = keys[base + t - 1] == key;
            prow = rows[base + t - 1];                    // linked: the previous access; a head of the paged record: the last access of the address below
        }
        last = t + 1 >= m || keys[base + t + 1] != key;
        if constexpr (kPorts) {                           // the source ids are virtual rows v = row k + port
            const uint32_t v = row, pv = prow;
            row = v / k;
            rec = first + (v - row * k);
            prow = pv / k;
            prec = first + (pv - prow * k);
        }
    }
    const bool from_image = pages && access && !linked;  // an unlinked access of the paged record: the image is its previous access, at clock 0
    long long d = 0;
    if (linked || from_image) {
        const uint32_t* clock = group_ptr(code, data, rec->cg[0]) + (size_t)rec->cc[0] * n;
        const uint32_t* pclock = kPorts ? group_ptr(code, data, prec->cg[0]) + (size_t)prec->cc[0] * n : clock;
        d = (long long)canonical(clock[row]) - (linked ? canonical(pclock[prow]) : 0) - 1;      // clock 0 is the image's: d = -1 refuses it
    }
    uint32_t addr = 0, word = 0;                          // the paged record's access: its address and, in range, the image's word
    [[maybe_unused]] uint32_t word1 = 0;                  // kV = 2: the image's second word of the address
    bool inside = true;
    if (pages && access) {
        addr = canonical(group_ptr(code, data, rec->kg)[(size_t)rec->kc * n + row]);
        inside = addr < pa.W;
        if constexpr (kPaged == PAGED_TABLE && kV == 2) {
            if (inside && !linked) {                      // a head: the flat rows 2 page, 2 page + 1 must hold the flat addresses 2 addr, 2 addr + 1
                const size_t at = (size_t)2 * head_rank(pa.local, pa.sums + 1, t);
                inside = at + 1 < pa.rows && pa.image[3 * at] == 2 * addr && pa.image[3 * at + 3] == 2 * addr + 1;      // addr < W <= 2^31: no wrap
                if (at < pa.rows) word = pa.image[3 * at + 1];
                if (at + 1 < pa.rows) word1 = pa.image[3 * at + 4];
            }
        } else if constexpr (kPaged == PAGED_TABLE) {
            if (inside && !linked) {                      // a head: row `page` of the table must be its address's; not listed: refused as `inside` is
                const uint32_t page = head_rank(pa.local, pa.sums + 1, t);
                inside = page < pa.rows && pa.image[(size_t)3 * page] == addr;
                if (page < pa.rows) word = pa.image[(size_t)3 * page + 1];
            }
        } else if constexpr (kV == 2) {
            if (inside) {                                 // the two words of an address: adjacent, 8-byte aligned, one 64-bit load
                const uint2 both = *(const uint2*)(pa.image + (size_t)2 * addr);
                word = both.x; word1 = both.y;
            }
        } else if (inside) word = pa.image[addr];
    }
    const uint32_t L = rec->L, nl = rec->nl;
    if (!kWrite) {
        uint32_t mine = (linked || from_image) && (d < 0 || (d >> (L * nl)) != 0) ? row : NONE;
        if (!inside) mine = row;
        if constexpr (kReads) {
            if ((rec->flags & LINK_READS) && access) {
                const uint32_t w = cell(code, data, rec->wg, rec->wc, n, row);
                bool ok = w == 0 || w == R1;
                if (w == 0) {                             // a load: every value column equals the previous access's; without one 0, or the image's word
                    const uint32_t nc = rec->nc;
                    for (uint32_t j = 1; j < nc; j++) {
                        const uint32_t* col = group_ptr(code, data, rec->cg[j]) + (size_t)rec->cc[j] * n;
                        const uint32_t* pcol = kPorts ? group_ptr(code, data, prec->cg[j]) + (size_t)prec->cc[j] * n : col;
                        if constexpr (kV == 2) ok &= col[row] % P == (linked ? pcol[prow] % P : (j == 1 ? word : word1) % P);
                        else ok &= col[row] % P == (linked ? pcol[prow] % P : word % P);
                    }
                }
                if (!ok) mine = row;
            }
        }
        if constexpr (kPorts) {                           // the record is the lane's own port's: the wave's minimum over (record, row), 64 bits
            unsigned long long worst = mine == NONE ? ~0ull : ((unsigned long long)(rec - links) << 32) | mine;
            if (__ballot(mine != NONE) != 0) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const unsigned long long o = __shfl_xor(worst, off, 64);
                    worst = o < worst ? o : worst;
                }
                if ((threadIdx.x & 63) == 0) atomicMin(bad, worst);
            }
        } else
        // report_bad_row (arguments.h) written out: through the helper this kernel's argument loads are scheduled otherwise
        if (__ballot(mine != NONE) != 0) {                // wave-uniform: only a wave that found one reduces and writes
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t o = __shfl_xor(mine, off, 64);
                mine = o < mine ? o : mine;
            }
            if ((threadIdx.x & 63) == 0) atomicMin(bad, ((unsigned long long)p << 32) | mine);
        }
        if (pages) report_bad_row(bad, kPorts ? po.records : gridDim.y, access && (addr >> (pa.pg->L * pa.pg->ng)) != 0 ? row : NONE);     // an address the limbs do not hold
        if constexpr (kPaged == PAGED_TABLE || (kPorts && kPaged != PAGED_NO))    // the trace's pages ride back with the refused row (BadRow's third word): one lane, no read-back of its own
            if (pages && t == 0) ((uint32_t*)bad)[2] = pa.sums[PG_TOTAL];
        return;
    }
    const uint32_t nc = rec->nc, n_dst = rec->n_dst;
    if constexpr (kPorts) {                               // lane t is also the virtual row t: port t % k at row t / k, zeroed where it is no access
        const uint32_t zrow = t / k;
        const Link* __restrict__ z = first + (t - zrow * k);
        if (zrow < A && z->sel != NONE && sel_class(code, z->sel, n, zrow) != 1)
            for (uint32_t e = 0; e < z->n_dst; e++) data[(size_t)z->dst[e] * n + zrow] = 0;
    } else
    if (rec->sel != NONE && t < A && sel_class(code, rec->sel, n, t) != 1)
        for (uint32_t e = 0; e < n_dst; e++) data[(size_t)rec->dst[e] * n + t] = 0;
    if (pages) {                                          // the page table
        const Pages* __restrict__ pg = pa.pg;
        const uint32_t D = pa.sums[PG_TOTAL];
        if (t >= D && t < A)                              // the rows below the table, coalesced
            for (uint32_t e = 0; e < pg->n_dst; e++) data[(size_t)pg->dst[e] * n + t] = 0;
        if constexpr (kFlat)
            if (t >= D && t < A) {
                data[(size_t)pg->flat[0] * n + t] = 0;
                data[(size_t)pg->flat[1] * n + t] = 0;
            }
        if (access && (!linked || last)) {                // (with ports the host has refused a trace of more than A pages: i < A)
            const uint32_t i = head_rank(pa.local, pa.sums + 1, t);            // the page of t's address: the heads up to t, less one
            const uint32_t Lp = pg->L, ng = pg->ng, maskp = (1u << Lp) - 1;
            if (!linked) {                                // the head: the first access of the address
                const uint32_t* keycol = group_ptr(code, data, rec->kg) + (size_t)rec->kc * n;
                data[(size_t)pg->dst[PG_ON] * n + i] = R1;
                data[(size_t)pg->dst[PG_ADDR] * n + i] = keycol[row];
                data[(size_t)pg->dst[PG_IN] * n + i] = word;
                if constexpr (kV == 2) data[(size_t)pg->dst[PG_IN + 1] * n + i] = word1;
                if constexpr (kFlat) {                    // the flat addresses of the page's two words: 2 addr + 1 < 2^30 < P
                    data[(size_t)pg->flat[0] * n + i] = fp_encode(2 * addr).v;
                    data[(size_t)pg->flat[1] * n + i] = fp_encode(2 * addr + 1).v;
                }
                const uint32_t* pkeycol = kPorts ? group_ptr(code, data, prec->kg) + (size_t)prec->kc * n : keycol;
                const uint32_t gap = t ? addr - canonical(pkeycol[prow]) - 1 : 0;
                for (uint32_t j = 0; j < ng; j++) {
                    data[(size_t)pg->dst[pg_limbs(kV) + j] * n + i] = fp_encode((addr >> (j * Lp)) & maskp).v;
                    data[(size_t)pg->dst[pg_limbs(kV) + ng + j] * n + i] = fp_encode((gap >> (j * Lp)) & maskp).v;
                }
            }
            if (last) {                                   // the tail: the last access of the address
                data[(size_t)pg->dst[pg_out(kV)] * n + i] = group_ptr(code, data, rec->cg[1])[(size_t)rec->cc[1] * n + row];
                if constexpr (kV == 2) data[(size_t)pg->dst[pg_out(kV) + 1] * n + i] = group_ptr(code, data, rec->cg[2])[(size_t)rec->cc[2] * n + row];
                data[(size_t)pg->dst[pg_time(kV)] * n + i] = group_ptr(code, data, rec->cg[0])[(size_t)rec->cc[0] * n + row];
            }
        }
    }
    if (!access) return;
    data[(size_t)rec->dst[0] * n + row] = linked ? R1 : 0;
    data[(size_t)rec->dst[1] * n + row] = last ? R1 : 0;
    for (uint32_t j = 0; j < nc; j++)                     // the previous access's cells; an unlinked access: 0, and the image's word for the paged value
        if constexpr (kV == 2) data[(size_t)rec->dst[2 + j] * n + row] = linked ? group_ptr(code, data, prec->cg[j])[(size_t)prec->cc[j] * n + prow] : j == 1 ? word : j == 2 ? word1 : 0;
        else data[(size_t)rec->dst[2 + j] * n + row] = linked ? group_ptr(code, data, prec->cg[j])[(size_t)prec->cc[j] * n + prow] : j == 1 ? word : 0;
    const uint32_t mask = (1u << L) - 1;                  // L <= 16
    for (uint32_t j = 0; j < nl; j++)
        data[(size_t)rec->dst[2 + nc + j] * n + row] = fp_encode((uint32_t)((unsigned long long)d >> (j * L)) & mask).v;
}

// Which rule the refused access `row` of the LINK record r = links[place] broke, as the reference names it (pages: r is a port of the paged memory,
// and `image` its image): the access and its previous one are found on the host as the reference finds them, from the keys and the selectors of
// the memory's ports (`mem`: r's memory, one record unless a LINK joins) on rows [0, row], walking back in (row, port) order.
// With a page table (mem.table) the image's word is the row's of the table: `page_of` gives the page of the refused row, and two words of
// that row are read; the table is never read back.
const char* refusal(zkh_ctx* ctx, const zkh_buf* code, const zkh_buf* data, size_t n, const std::vector<Link>& links, const Memory& ports, uint32_t place, uint32_t row,
                    bool pages, const PagedFrom& mem, uint32_t pages_index, const std::function<const char*(uint32_t*)>& page_of, uint32_t V = 1) {
    const Link& r = links[place];
    const uint32_t port = place - ports.first;
    std::vector<std::vector<uint32_t>> key(ports.k, std::vector<uint32_t>(row + 1)), sel(ports.k, std::vector<uint32_t>(row + 1, R1));
    for (uint32_t q = 0; q < ports.k; q++) {
        const Link& x = links[ports.first + q];
        ZKH_TRY(zkh_read(ctx, x.kg == GROUP_CODE ? code : data, key[q].data(), (size_t)x.kc * n, row + 1));
        if (x.sel != NONE) ZKH_TRY(zkh_read(ctx, code, sel[q].data(), (size_t)x.sel * n, row + 1));
    }
    uint32_t prow = row, pport = port;                    // (prow, pport) == (row, port): no earlier access has its key (unlinked)
    for (uint32_t at = row + 1; at-- > 0 && prow == row && pport == port;)
        for (uint32_t q = at == row ? port : ports.k; q-- > 0;)
            if (sel[q][at] % P == R1 && key[q][at] % P == key[port][row] % P) { prow = at; pport = q; break; }
    const bool linked = prow != row || pport != port;
    const Link& pr = links[ports.first + pport];          // the record of the previous access
    char there[48];                                       // where it lies: "row R", and "of record Q" when that is not r
    if (pport != port) snprintf(there, sizeof there, "row %u of record %u", prow, pr.index);
    else snprintf(there, sizeof there, "row %u", prow);
    if (r.flags & LINK_READS) {
        uint32_t w;
        ZKH_TRY(read_cell(ctx, code, data, r.wg, r.wc, n, row, &w));
        if (w > 1) return make_err("derive_links: record %u at row %u: write flag %u, not 0 or 1: the witness is refused", r.index, row, w);
    }
    const uint32_t addr = canonical(key[port][row]);
    uint32_t words[MAX_PAGE_WORDS] = {};                  // paged: the image's words at the address (V of them, flat: V addr + j), canonical
    if (pages) {
        const uint32_t W = (uint32_t)((mem.table ? mem.image_words : mem.image->len) / V);      // in addresses
        if (addr >= W) return make_err("derive_links: record %u at row %u: address %u outside the image of %u words: the witness is refused", r.index, row, addr, W);
        if (!mem.table) {
            ZKH_TRY(zkh_read(ctx, mem.image, words, (size_t)V * addr, V));
        } else if (!linked) {                             // the head's page, then its rows of the (flat) table: their addresses, their in words; the lowest j first
            uint32_t page, listed;
            ZKH_TRY(page_of(&page));
            for (uint32_t j = 0; j < V; j++) {
                const size_t at = (size_t)V * page + j;
                if (at >= mem.D)
                    return make_err("derive_links: record %u at row %u: address %u is page %u of the trace, but the page table has %zu rows: the witness is refused",
                                    pages_index, row, addr, page, mem.D);
                ZKH_TRY(zkh_read(ctx, mem.table, &listed, mem.table_at + 3 * at, 1));
                if (listed != V * addr + j)
                    return make_err("derive_links: record %u at row %u: address %u is page %u of the trace, but row %zu of the page table holds address %u: the witness "
                                    "is refused", pages_index, row, addr, page, at, listed);
                ZKH_TRY(zkh_read(ctx, mem.table, &words[j], mem.table_at + 3 * at + 1, 1));
            }
        }
        for (uint32_t j = 0; j < V; j++) words[j] = canonical(words[j]);
    }
    if (linked || pages) {
        long long now, before = 0;
        ZKH_TRY(read_cell(ctx, code, data, r.cg[0], r.cc[0], n, row, &now));
        if (linked) ZKH_TRY(read_cell(ctx, code, data, pr.cg[0], pr.cc[0], n, prow, &before));
        if (!linked && now == 0) return make_err("derive_links: record %u at row %u: clock 0 is the image's: the witness is refused", r.index, row);
        const long long d = now - before - 1;
        if (d < 0)
            return make_err("derive_links: record %u at row %u: clock not increasing (%lld after %lld at %s): the witness is refused", r.index, row, now, before, there);
        if ((d >> (r.L * r.nl)) != 0 && linked)
            return make_err("derive_links: record %u at row %u: the clock difference %lld (after %s) does not fit %u limbs of %u bits: the witness is refused",
                            r.index, row, d, there, r.nl, r.L);
        if ((d >> (r.L * r.nl)) != 0)
            return make_err("derive_links: record %u at row %u: the clock difference %lld (after the image) does not fit %u limbs of %u bits: the witness is refused",
                            r.index, row, d, r.nl, r.L);
    }
    for (uint32_t j = 1; (r.flags & LINK_READS) && j < r.nc; j++) {     // a load (the write flag is 0, or something above was named)
        uint32_t now, before = pages && j <= V ? words[j - 1] : 0;
        ZKH_TRY(read_cell(ctx, code, data, r.cg[j], r.cc[j], n, row, &now));
        if (linked) ZKH_TRY(read_cell(ctx, code, data, pr.cg[j], pr.cc[j], n, prow, &before));
        if (now == before) continue;
        if (linked)
            return make_err("derive_links: record %u at row %u: a load of carried column %u returns %u, but %u was last stored (%s): the witness is refused",
                            r.index, row, j, now, before, there);
        if (pages)
            return make_err("derive_links: record %u at row %u: a load of carried column %u returns %u, but the image holds %u at its address %u: the witness is "
                            "refused", r.index, row, j, now, before, addr);
        return make_err("derive_links: record %u at row %u: a load of carried column %u returns %u, but its address was never accessed: the value must be 0: "
                        "the witness is refused", r.index, row, j, now);
    }
    return make_err("derive_links: record %u at row %u was refused, but the host finds no rule it breaks", r.index, row);
}

// grid ceil(A / LINK_THREADS), k_page_heads' geometry (with ports: p the paged memory, A the items a run can hold, `row` the virtual row) (head_rank reads the workgroup's carry): the page of the access `row` of the paged
// record, for the host's message about a refused row.  A row is at one sorted position: one writer.
__global__ __launch_bounds__(LINK_THREADS) void k_page_of(const uint32_t* __restrict__ status, const uint32_t* __restrict__ rows, uint32_t p, uint32_t A, uint32_t row,
                                                          const uint32_t* __restrict__ local, const uint32_t* __restrict__ sums, uint32_t* __restrict__ page) {
    const uint32_t m = status[ST_HEAD + ST_WORDS * p + ST_M];
    const uint32_t t = blockIdx.x * LINK_THREADS + threadIdx.x;
    if (t < m && rows[(size_t)p * A + t] == row) *page = head_rank(local, sums + 1, t);
}

}  // namespace

// zkh_derive_links (no image), zkh_derive_links_paged (mem.image) and zkh_derive_links_paged_table (mem.table): one sort, the check pass, one
// read-back, the write pass.  With a PAGES record both passes are k_links' paged ones and the page scan runs between the sort and the check.
const char* zkh::derive_links_from(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data, const PagedFrom& mem) {
    ZKH_REQUIRE(ctx && c && data, "derive_links: null argument");
    ZKH_REQUIRE(code, "derive_links: the raw code trace is required (the selectors and code-group source columns of the records read it)");
    ZKH_REQUIRE(zkh_circuit_derives_links(c), "derive_links: the circuit's arguments hold no LINK record (ZKA1 version 5)");
    const bool paging = !c->args->pages.empty();
    const bool tabled = paging && mem.table;            // the image's words come as a page table
    const zkh_buf* image = mem.image;
    ZKH_REQUIRE(image || tabled || !paging, "derive_links: the arguments page memory: an image is required (zkh_derive_all_paged)");
    if (tabled) {
        ZKH_REQUIRE(mem.table_at <= mem.table->len && mem.D <= (mem.table->len - mem.table_at) / 3,
                    "derive_links: a table of %zu rows of 3 words at word %zu does not fit a buffer of %zu words", mem.D, mem.table_at, mem.table->len);
        ZKH_REQUIRE(mem.image_words >= 1 && mem.image_words <= 0xffffffffull, "derive_links: an image of %zu words (1 .. 2^32 - 1)", mem.image_words);
    }
    size_t n;
    uint32_t A;
    ZKH_TRY(trace_rows("derive_links", c, po2, zk_cycles, code, data, nullptr, &n, &A));
    const std::vector<Link>& links = c->args->links;
    const uint32_t nr = (uint32_t)links.size();
    ZKH_REQUIRE(nr <= 65535, "derive_links: %u LINK records in one blob (at most 65535)", nr);
    ZKH_REQUIRE(!paging || tabled || image->len <= 0xffffffffull, "derive_links: an image of %zu words (at most 2^32 - 1)", paging && !tabled ? image->len : 0);
    const uint32_t V = paging ? c->args->pages[0].V : 1;    // the value words per address: the image and the table are flat
    const size_t flat_words = !paging ? 0 : tabled ? mem.image_words : image->len;
    ZKH_REQUIRE(flat_words % V == 0, "derive_links: an image of %zu words is not a whole number of addresses of %u value words", flat_words, V);
    ZKH_REQUIRE(V == 1 || tabled || ((uintptr_t)image->ptr() & 7) == 0, "derive_links: the image of a memory of two value words per address begins at an odd word of its "
                "buffer (the two words of an address are one 64-bit load)");
    const int paged = paging ? c->args->paged_link() : -1;
    ZKH_REQUIRE(!paging || paged >= 0, "derive_links: the PAGES record names no LINK record");    // set_arguments has refused such a blob
    const bool ported = c->args->ports();               // a LINK joins: the passes run over memories, one sort run per memory
    const std::vector<Memory> mems = c->args->memories();
    std::vector<uint32_t> mem_of(nr);                   // the memory of every LINK record
    for (uint32_t g = 0; g < mems.size(); g++)
        for (uint32_t q = 0; q < mems[g].k; q++) mem_of[mems[g].first + q] = g;
    std::vector<SortPair> pairs(nr, SortPair{});
    for (uint32_t p = 0; p < nr; p++) {                 // the accesses of a record sorted by their key alone: the sort is stable
        pairs[p].d_term = links[p].index; pairs[p].nkeys = 1; pairs[p].sel = links[p].sel;
        for (uint32_t f = 0; f < MAX_SORT_KEYS; f++) { pairs[p].kg[f] = links[p].kg; pairs[p].kc[f] = links[p].kc; }
        for (uint32_t e = 0; e < MAX_TUPLE; e++) pairs[p].sg[e] = GROUP_DATA;
    }
    bind_thread(ctx);
    SortedRows sorted;
    ZKH_TRY(sort_rows(ctx, code, data, n, A, pairs, &sorted, ported ? &mems : nullptr));
    if (sorted.bad_selector) {
        const Link& r = links[sorted.bad_pair];
        uint32_t sel;
        ZKH_TRY(read_cell(ctx, code, data, GROUP_CODE, r.sel, n, sorted.bad_row, &sel));
        return make_err("derive_links: record %u at row %u: selector %u, not 0 or 1: the witness is refused", r.index, sorted.bad_row, sel);
    }
    ZKH_REQUIRE(!sorted.wide, "derive_links: a packed key of more than 64 bits from one 31-bit field");
    static_assert(sizeof(Link) % 4 == 0 && sizeof(Pages) % 4 == 0, "word records");
    Tmp drecs, dpages, local, sums;
    BadRow bad;
    ZKH_TRY(zkh_copy_from(ctx, "link_records", (const uint32_t*)links.data(), links.size() * (sizeof(Link) / 4), drecs.out()));
    ZKH_TRY(bad.init(ctx));
    double carried = 0, dsts = 0;
    for (const Link& r : links) { carried += r.nc; dsts += r.n_dst; }
    const uint32_t span = ported ? sorted.cap : A;      // the sorted positions of a run; with ports a memory's, at most k A
    const uint32_t nb = (span + LINK_THREADS - 1) / LINK_THREADS, ny = ported ? (uint32_t)mems.size() : nr;
    const uint32_t paged_run = paging ? (ported ? mem_of[paged] : (uint32_t)paged) : 0;     // the paged record's run of the sort
    const Ports po = ported ? Ports{(const Memory*)sorted.runs->ptr(), sorted.cap, nr} : Ports{};
    const bool reads = c->args->reads != 0;             // a record has READS: the check pass with the read rule, over all records
    Paging pa{};
    if (paging) {                                       // every sorted position of the paged record gets its page: a two-level scan of the head flags
        const Pages& g = c->args->pages[0];
        ZKH_TRY(zkh_copy_from(ctx, "pages_record", (const uint32_t*)&g, sizeof(Pages) / 4, dpages.out()));
        ZKH_TRY(new_buf(ctx, span, false, local.out()));
        ZKH_TRY(new_buf(ctx, 1 + (size_t)nb, false, sums.out()));
        pa = tabled ? Paging{(const Pages*)dpages->ptr(), paged_run, mem.table->ptr() + mem.table_at, (uint32_t)(mem.image_words / V),
                             (uint32_t)std::min<size_t>(mem.D, 0xffffffffu), local->ptr(), sums->ptr()}       // a trace pages at most A rows: more never match
                    : Paging{(const Pages*)dpages->ptr(), paged_run, image->ptr(), (uint32_t)(image->len / V), 0, local->ptr(), sums->ptr()};
        ProfScope prof(ctx, "pages_scan", 12.0 * span + 8.0 * nb);            // the keys of every position, its index, the workgroups' totals twice
        k_page_heads<<<nb, LINK_THREADS, 0, ctx->stream>>>(sorted.status->ptr(), sorted.keys(), paged_run, span, local->ptr(), sums->ptr());
        ZKH_TRY(last_launch_error("pages_heads"));
        scan_counters(ctx, sums->ptr() + 1, 1, nb, sums->ptr() + PG_TOTAL, 0);      // the totals become the workgroups' carries, their sum D
        ZKH_TRY(last_launch_error("pages_carry"));
    }
    auto pass = [&](auto* kernel) {
        kernel<<<dim3(nb, ny), LINK_THREADS, 0, ctx->stream>>>(code->ptr(), data->ptr(), (const Link*)drecs->ptr(), sorted.status->ptr(), sorted.keys(), sorted.rows(),
                                                              (uint32_t)n, A, bad.ptr(), pa, po);
    };
    {
        double cells = 0;                                 // with READS: the write flag and, at most, the value cells at both rows
        for (const Link& r : links) cells += r.flags & LINK_READS ? 1 + 2 * (r.nc - 1) : 0;
        ProfScope prof(ctx, "links_check", (20.0 * nr + 4.0 * cells + (paging ? 4.0 + 4.0 * V : 0.0)) * A);   // key and row of every item; the clock at both rows; paged: the key and the image's words
        if (V == 2 && ported) pass(tabled ? k_links<false, true, PAGED_TABLE, true, 2> : k_links<false, true, PAGED_IMAGE, true, 2>);
        else if (V == 2) pass(tabled ? k_links<false, true, PAGED_TABLE, false, 2> : k_links<false, true, PAGED_IMAGE, false, 2>);
        else if (ported) pass(tabled ? k_links<false, true, PAGED_TABLE, true> : paging ? k_links<false, true, PAGED_IMAGE, true> : k_links<false, true, PAGED_NO, true>);
        else pass(tabled ? k_links<false, true, PAGED_TABLE> : paging ? k_links<false, true, PAGED_IMAGE> : reads ? k_links<false, true, PAGED_NO> : k_links<false, false, PAGED_NO>);
        ZKH_TRY(last_launch_error("links_check"));
    }
    ZKH_TRY(bad.read(ctx));
    if (bad.found && bad.hi >= nr) {                    // the PAGES record's own refusal: an address that its limbs do not hold
        const Pages& g = c->args->pages[0];
        uint32_t a = 0;
        const Memory& ports = mems[mem_of[paged]];      // the row's first port (the lowest (row, port)) whose access has such an address
        for (uint32_t q = 0; q < ports.k; q++) {
            const Link& x = links[ports.first + q];
            uint32_t on = 1;
            if (x.sel != NONE) ZKH_TRY(read_cell(ctx, code, data, GROUP_CODE, x.sel, n, bad.lo, &on));
            ZKH_TRY(read_cell(ctx, code, data, x.kg, x.kc, n, bad.lo, &a));
            if (on == 1 && (a >> (g.L * g.ng)) != 0) break;
        }
        return make_err("derive_links: record %u at row %u: address %u does not fit %u limbs of %u bits: the witness is refused", g.index, bad.lo, a, g.ng, g.L);
    }
    if (bad.found) {
        const auto page_of = [&](uint32_t* page) -> const char* {      // the refused head's page: one more launch, on a refusal only
            Tmp at;
            ZKH_TRY(new_buf(ctx, 1, true, at.out()));
            const Memory& ports = mems[mem_of[paged]];  // the refused access's source id: its virtual row
            k_page_of<<<nb, LINK_THREADS, 0, ctx->stream>>>(sorted.status->ptr(), sorted.rows(), paged_run, span, bad.lo * ports.k + (bad.hi - ports.first), pa.local, pa.sums,
                                                            at->ptr());
            ZKH_TRY(last_launch_error("links_page_of"));
            return zkh_read(ctx, at, page, 0, 1);
        };
        return refusal(ctx, code, data, n, links, mems[mem_of[bad.hi]], bad.hi, bad.lo, paging && mem_of[bad.hi] == mem_of[paged], mem, paging ? c->args->pages[0].index : 0,
                       page_of, V);
    }
    // with ports a memory has up to k A accesses, and their distinct addresses may be more than the A rows its page table has
    ZKH_REQUIRE(!(ported && paging) || bad.extra <= A, "derive_links: record %u: the trace pages %u addresses, but the page table has the %u active rows: the witness is refused",
                c->args->pages[0].index, bad.extra, A);
    if (tabled) {                                       // no row is refused: every head is listed, so the table has at least the trace's pages
        const uint32_t D = bad.extra;                   // the scan's total, which the check pass sent back with its verdict
        ZKH_REQUIRE((size_t)V * D == mem.D, "derive_links: record %u: the trace pages %u addresses, but the page table has %zu rows: the witness is refused",
                    c->args->pages[0].index, D, mem.D);                 // the flat table: V rows per page
    }
    {
        const bool flat = paging && c->args->pages[0].F != 0;   // set_arguments has refused flats with V = 1
        ProfScope prof(ctx, "links_write", (20.0 * nr + 4.0 * carried + 4.0 * dsts + (paging ? 12.0 + 4.0 * (c->args->pages[0].n_dst + c->args->pages[0].F) : 0.0)) * A);
        if (V == 2 && flat && ported) pass(tabled ? k_links<true, false, PAGED_TABLE, true, 2, true> : k_links<true, false, PAGED_IMAGE, true, 2, true>);
        else if (V == 2 && flat) pass(tabled ? k_links<true, false, PAGED_TABLE, false, 2, true> : k_links<true, false, PAGED_IMAGE, false, 2, true>);
        else if (V == 2 && ported) pass(tabled ? k_links<true, false, PAGED_TABLE, true, 2> : k_links<true, false, PAGED_IMAGE, true, 2>);
        else if (V == 2) pass(tabled ? k_links<true, false, PAGED_TABLE, false, 2> : k_links<true, false, PAGED_IMAGE, false, 2>);
        else if (ported) pass(tabled ? k_links<true, false, PAGED_TABLE, true> : paging ? k_links<true, false, PAGED_IMAGE, true> : k_links<true, false, PAGED_NO, true>);
        else pass(tabled ? k_links<true, false, PAGED_TABLE> : paging ? k_links<true, false, PAGED_IMAGE> : k_links<true, false, PAGED_NO>);
        ZKH_TRY(last_launch_error("links_write"));
    }
    // the temporaries go back to the pool on return: the stream orders their next use after these launches
    return nullptr;
}

extern "C" const char* zkh_derive_links(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data) {
    return derive_links_from(ctx, c, po2, zk_cycles, code, data, PagedFrom{});
}

extern "C" const char* zkh_derive_links_paged(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data,
                                              const zkh_buf* image) {
    return derive_links_from(ctx, c, po2, zk_cycles, code, data, PagedFrom{image});
}

extern "C" const char* zkh_derive_links_paged_table(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data,
                                                    const zkh_buf* table, size_t table_at, size_t D, size_t image_words) {
    ZKH_REQUIRE(table || !zkh_circuit_pages(c), "derive_links: the arguments page memory: a page table is required (zkh_derive_all_paged_table)");
    return derive_links_from(ctx, c, po2, zk_cycles, code, data, PagedFrom{nullptr, table, table_at, D, image_words});
}
