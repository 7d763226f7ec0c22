// arguments.h — lookup and permutation arguments as data (ZKA1 blob; zeth_amd/circuits/logup.py; DESIGN.md §2 ARGUMENTS): the decoded
// form every consumer reads, and what the consumers share.  arguments.hip owns the blob format and the rules a blob must keep;
// accumulate.hip (zkh_accumulate), multiplicities.hip (zkh_derive_multiplicities), sort.hip (zkh_derive_sorted), columns.hip
// (zkh_derive_columns), links.hip (zkh_derive_links, zkh_derive_links_paged, zkh_derive_links_paged_table) and page_out.hip (zkh_page_out, zkh_page_out_tree,
// zkh_page_out_proof) read zkh_circuit::args and never see a blob word.
//
// WHO WRITES A DATA COLUMN (the module docstring of logup.py says the same; check_owned in arguments.hip keeps it).  A data column has at
// most one writer, and a derive reads only what the stages before it have finished writing.  The writers: a sorted copy (its tuple
// columns), a LIMBS / ORDER record and a LINK record (their destinations), a derived multiplicity (its column); every other column is
// the host's.  The stages run one after the other, each over the whole trace: sorted -> columns -> links -> multiplicities (STAGES in
// arguments.hip is that order in code, and zkh_derive_all runs it; no caller spells it out).  Of the
// columns a derive writes, the sort reads none; a LIMBS / ORDER record reads a sorted copy's columns and no record's destination
// (records never chain); a LINK reads none; the multiplicities count lookup tuples, and those read every derived column freely.
// Nothing reads a derived multiplicity.  A term's multiplicity is the host's column or a derived one, and of a LINK's destinations
// linked and last (only they) may be the multiplicity of a term that is not derived.  The PAGES record (version 7) is one more writer of
// the links stage: it reads what the LINK it pages reads, writes the page table, and of its destinations p_on may be such a multiplicity
// (version 10, two value words per address: p_in_1 and p_out_1 are destinations like the others; still only p_on.  Version 11: so are the
// flat-address destinations p_flat_0, p_flat_1: one writer, no record reads them, none is a multiplicity; terms may read them).
//
// THE READ RULE (a LINK record with READS, ZKA1 version 6; links.hip's header has it in full): the write flag is one more source of the
// record, the host's column.  On an access it must be 0 or 1; a load (0) returns, in every carried column but the clock, what the
// previous access to its address left, or 0 where there is none.  Residues mod P are compared.  The rule adds no destination.
//
// A derive that refuses a witness leaves `data` unchanged: its check pass reduces the lowest bad (record, row) into a BadRow, the host
// reads that back, and only then does anything write.
#pragma once
#include <algorithm>
#include <vector>

#include "circuit.h"

namespace zkh {

constexpr uint32_t ARGS_MAGIC = 0x5a4b4131u;        // 'ZKA1'
constexpr uint32_t ARGS_HEADER = 8, TERM_WORDS = 16;
constexpr uint32_t MAX_TUPLE = 4, MAX_TERMS = 3, MAX_SORT_KEYS = 3, NONE = 0xffffffffu;
constexpr uint32_t RECORD_WORDS = 16, KIND_LIMBS = 1, KIND_ORDER = 2, MAX_LIMBS = 8;
constexpr uint32_t KIND_LINK = 3, LINK_WORDS = 32, MAX_CARRIED = 3, MAX_LINK_LIMBS = 4, MAX_LINK_DSTS = 2 + MAX_CARRIED + MAX_LINK_LIMBS;
constexpr uint32_t LINK_READS = 1;                  // LINK word 5, bit 0 (version 6): the record carries the read rule
constexpr uint32_t KIND_PAGES = 4, PAGES_WORDS = 32, MAX_PAGE_LIMBS = 4, MAX_PAGE_WORDS = 2;   // a PAGES record (version 7); V, its value words per address (version 10)
constexpr uint32_t MAX_PAGE_DSTS = 3 + 2 * MAX_PAGE_WORDS + 2 * MAX_PAGE_LIMBS;
constexpr uint32_t MAX_PAGE_FLATS = 2;              // F, the flat-address destinations of a PAGES record (version 11: 0 or 2, in words 6, 7; word 5 holds F)
constexpr uint32_t PAGES_BIT = 0x10000;             // header word 7, bit 16 (version 7): the blob has a PAGES record
constexpr uint32_t OPEN_BIT = 0x20000;              // header word 7, bit 17 (version 8): the blob has an OPEN record
constexpr uint32_t KIND_OPEN = 5, OPEN_WORDS = 16;  // the OPEN record (version 8): the bus closes on `out` words, not on zero
constexpr uint32_t LINK_JOINS = 2;                  // LINK word 5, bit 1 (version 9): the record joins the memory of the head that word 31 names
constexpr uint32_t MAX_PORTS = 8;                   // the records of one memory, the head included
constexpr uint32_t PORTS_BIT = 0x40000;             // header word 7, bit 18 (version 9): a LINK record joins
constexpr uint32_t WIDE_BIT = 0x80000;              // header word 7, bit 19 (version 10): the PAGES record pages two value words per address
constexpr uint32_t FLAT_BIT = 0x100000;             // header word 7, bit 20 (version 11): the PAGES record has the two flat-address destinations
constexpr uint32_t MAX_ORDER_BITS = 29;             // logup.MAX_ORDER_BITS: a negative difference stays out of the limbs' range

// logup.Term as the blob gives it: the fields are the blob's words, checked by the rules of arguments.hip before a circuit keeps them
struct Term {
    uint32_t col, neg;                      // accum Fp4 column; sign (0: +1, 1: -1)
    uint32_t sel, mg, mc;                   // selector code column or NONE; multiplicity group (NONE = the constant 1) and column
    uint32_t tag, w;                        // tag (canonical); tuple width
    uint32_t tg[MAX_TUPLE], tc[MAX_TUPLE];  // the tuple's (group, column), the first w
    uint32_t flags;                         // the flag word as the blob's version reads it (0 = no flag; version 1: always 0)
    bool reserved;                          // ... and it sets a bit that this version reserves
    bool derive;                            // the multiplicity is derived by the library
    bool sorted;                            // this term is the sorted copy of the term sorted_from (logup.Term.sorted_from is not None),
    uint32_t sorted_from, nkeys, key[4];    // by the tuple positions key[0 .. nkeys), most significant first (the rules bound nkeys)
};
// logup.Record, a derived-column record (version 4), as the blob gives it; the kernels of columns.hip read it in this form
struct Record {
    uint32_t kind, L, nl, n_src;            // KIND_LIMBS / KIND_ORDER; limb bits; limb count; sources (the rules bound them all)
    uint32_t sg[2], sc[2];                  // the sources' (group, column), the first n_src
    uint32_t dst[MAX_LIMBS];                // destination data columns: (ORDER with two keys: the flag,) then the nl limbs
    uint32_t n_dst, reserved;               // destinations in use; a word the format reserves was not 0
};
// logup.Link, a LINK record (version 5; version 6: the read rule), as the blob gives it; the kernels of links.hip read it in this form
struct Link {
    uint32_t index;                         // its index among all records of the blob (LINK records follow the LIMBS / ORDER ones)
    uint32_t L, nl, nc, sel;                // limb bits; limb count; carried columns; selector code column or NONE
    uint32_t kg, kc;                        // the key's (group, column)
    uint32_t cg[MAX_CARRIED], cc[MAX_CARRIED];      // the carried columns, the first nc; c_0 is the clock
    uint32_t dst[MAX_LINK_DSTS];            // destination data columns: linked, last, prev_0 .. prev_{nc-1}, limb_0 .. limb_{nl-1}
    uint32_t n_dst, reserved;               // destinations in use; a word the format reserves was not 0
    uint32_t flags, wg, wc;                 // version 6: word 5 (bit 0 = READS, LINK_READS; version 9: bit 1 = JOINS) and words 14, 15, the write flag's (group, column)
};
// A memory (version 9, PORTS): a run of k consecutive LINK records, the head at place `first` among the LINK records and the records that join
// it; port q is the record at first + q.  A LINK that nothing joins is a memory of one port.
struct Memory { uint32_t first, k; };
// logup.Pages, the PAGES record (version 7), as the blob gives it; the paged kernels of links.hip and the page-out of page_out.hip read it in this form
struct Pages {
    uint32_t index;                         // its index among all records of the blob (it comes last)
    uint32_t L, ng, link;                   // limb bits; limbs of an address and of a gap; the blob record index of the LINK it pages
    uint32_t dst[MAX_PAGE_DSTS];            // destination data columns: p_on, p_addr, p_in_0 .., p_out_0 .., p_time, alimb_0 .., gap_0 ..
    uint32_t n_dst, reserved;               // destinations in use; a word the format reserves was not 0
    uint32_t V, word4;                      // the value words per address (version 10: word 4 holds V - 1; 1 before), clamped to 1..2; word 4 as the blob has it
    // behind every field an earlier kernel reads, so that none of their offsets moves:
    uint32_t F, word5;                      // the flat-address destinations in use (version 11: word 5 holds F; 0 before), 0 or 2; word 5 as the blob has it
    uint32_t flat[MAX_PAGE_FLATS];          // p_flat_0, p_flat_1: the data columns that take 2 a_i + j (links.hip kFlat)
};
// logup.Open, the OPEN record (version 8), as the blob gives it: the terms of `tag` are answered by another seal, the challenges and the
// bus total are words of `out` (accumulate.hip zkh_accumulate_open; bus.hip skips the tag's keys)
struct Open {
    uint32_t index;                         // its index among all records of the blob (it comes last)
    uint32_t tag, alpha, beta, total;       // the open tag; the `out` word offsets of alpha, beta and the total (4 words each)
    uint32_t out_words, reserved;           // the circuit's `out` words; a word the format reserves was not 0
};
enum { PG_ON = 0, PG_ADDR = 1, PG_IN = 2, PG_OUT = 3, PG_TIME = 4, PG_LIMBS = 5 };      // the places of Pages::dst of a record with V = 1
// ... and with V value words per address: p_in_j at PG_IN + j, p_out_j at pg_out(V) + j, then p_time and the limbs
constexpr uint32_t pg_out(uint32_t V) { return PG_IN + V; }
constexpr uint32_t pg_time(uint32_t V) { return PG_IN + 2 * V; }
constexpr uint32_t pg_limbs(uint32_t V) { return PG_IN + 2 * V + 1; }
static_assert(pg_out(1) == PG_OUT && pg_time(1) == PG_TIME && pg_limbs(1) == PG_LIMBS, "one value word: the places they always were");
// logup.Arguments
struct Arguments {
    uint32_t version, k, alpha, beta;       // blob version; accum Fp4 columns; mix word offsets of the two challenges (OPEN: `out` offsets)
    std::vector<Term> terms;
    std::vector<Record> records;            // the LIMBS / ORDER records: their index here is their index in the blob
    std::vector<Link> links;                // the LINK records
    std::vector<uint32_t> heads;            // per LINK record (version 9): the blob record index of the head it joins (word 31), NONE: it joins none
    uint32_t late_record = NONE, late_after = 0;    // a LIMBS / ORDER record that follows a LINK record, and that LINK record (refused)
    uint32_t reads = 0;                     // the LINK records with READS (version 6: header word 7)
    std::vector<Pages> pages;               // the PAGES record (version 7; the rules allow one)
    uint32_t after_pages = NONE;            // a record that follows the first PAGES record (refused)
    bool second_pages = false;              // ... and it is a PAGES record itself
    std::vector<Open> open;                 // the OPEN record (version 8; the rules allow one, the last record)
    uint32_t after_open = NONE;             // a record that follows the first OPEN record (refused)
    bool second_open = false;               // ... and it is an OPEN record itself
    bool is_open() const { return !open.empty(); }
    bool open_tag(uint32_t tag) const { return !open.empty() && open[0].tag == tag; }
    bool ports() const { return std::any_of(heads.begin(), heads.end(), [](uint32_t h) { return h != NONE; }); }
    std::vector<Memory> memories() const {  // the LINK records as memories, in blob order (the rules have made every joiner follow its head's run)
        std::vector<Memory> m;
        for (uint32_t p = 0; p < links.size(); p++) {
            if (heads[p] == NONE || m.empty()) m.push_back(Memory{p, 1});
            else m.back().k++;
        }
        return m;
    }
    uint32_t page_words() const { return pages.empty() ? 0 : pages[0].V; }     // V of the paged memory, 0: none
    uint32_t page_flats() const { return pages.empty() ? 0 : pages[0].F; }     // F of the PAGES record: 2 with flat-address destinations, else 0
    int paged_link() const {                // the place among `links` of the LINK that the PAGES record names, -1: none (or no such LINK)
        for (size_t p = 0; !pages.empty() && p < links.size(); p++)
            if (links[p].index == pages[0].link) return (int)p;
        return -1;
    }
};

// a term's columns as the kernels read them; unused tuple slots name (data, 0)
struct TermCols {
    uint32_t w, sel, mg, mc;                // tuple width; selector code column or NONE; multiplicity group (NONE = 1) and column
    uint32_t tg[MAX_TUPLE], tc[MAX_TUPLE];
};
inline TermCols term_cols(const Term& t) {
    TermCols d{t.w, t.sel, t.mg, t.mc, {}, {}};
    for (uint32_t e = 0; e < MAX_TUPLE; e++) { d.tg[e] = e < t.w ? t.tg[e] : GROUP_DATA; d.tc[e] = e < t.w ? t.tc[e] : 0; }
    return d;
}
// the words a term reads per row for its weight and tuple (selector, multiplicity, tuple columns): the ProfScope byte counts of its consumers
inline uint32_t entry_words(const Term& t) { return t.w + (t.sel != NONE) + (t.mg != NONE); }

// what the entry points over a trace share: po2 in 1..24, an active row left, the data (and, if given, code and accum) buffers of the
// circuit's widths at 2^po2 rows.  `who` prefixes the messages.  *n = rows, *A = active rows.
const char* trace_rows(const char* who, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* data,
                       const zkh_buf* accum, size_t* n, uint32_t* A);

// Where the links stage of a paging circuit takes the memory image from: the image's W words (zkh_derive_links_paged), or the rows (address,
// in, out) of a ZKU1 page table from word table_at of `table`, D rows over an image of image_words words (zkh_derive_links_paged_table); both
// NULL: no image, and a circuit with a PAGES record is refused.  Without a PAGES record none of it is looked at.
struct PagedFrom {
    const zkh_buf* image = nullptr;
    const zkh_buf* table = nullptr;
    size_t table_at = 0, D = 0, image_words = 0;
};
// the links stage (links.hip): what zkh_derive_links and its paged variants call, and the stage table of arguments.hip
const char* derive_links_from(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data, const PagedFrom& mem);

// the canonical value of a raw trace word (raw words >= P are legal)
__host__ __device__ __forceinline__ uint32_t canonical(uint32_t raw) { return fp_decode(Fp::raw(raw % P)); }
// the canonical value of the cell (g, c) at `row` of an n-row trace, read back for an error message (T: uint32_t, or wider to subtract)
template <typename T>
const char* read_cell(zkh_ctx* ctx, const zkh_buf* code, const zkh_buf* data, uint32_t g, uint32_t c, size_t n, uint32_t row, T* v) {
    uint32_t w;
    ZKH_TRY(zkh_read(ctx, g == GROUP_CODE ? code : data, &w, (size_t)c * n + row, 1));
    *v = canonical(w);
    return nullptr;
}

// The lowest (hi, lo) that a check pass refused, hi << 32 | lo on the device: two words, all ones = none.  A third word, `extra`, comes
// back with them for a check pass that has one more thing to tell (zkh_page_out: the last row of its table); it starts as all ones too.
struct BadRow {
    Tmp buf;
    bool found = false;
    uint32_t hi = 0, lo = 0, extra = NONE;
    const char* init(zkh_ctx* ctx) {
        ZKH_TRY(new_buf(ctx, 4, false, buf.out()));             // three words in use
        ZKH_HIP(hipMemsetAsync(buf->ptr(), 0xff, 12, ctx->stream));
        return nullptr;
    }
    unsigned long long* ptr() const { return (unsigned long long*)buf->ptr(); }
    uint32_t* extra_ptr() const { return buf->ptr() + 2; }
    const char* read(zkh_ctx* ctx) {                    // after the check pass: found, and then (hi, lo); extra
        uint32_t st[3];
        ZKH_TRY(zkh_read(ctx, buf, st, 0, 3));
        lo = st[0]; hi = st[1]; extra = st[2];
        found = (lo & hi) != NONE;
        return nullptr;
    }
};
// ... and its device side: this lane's refused row (NONE = none) of `record`.  Only a wave that found one reduces (the branch is
// wave-uniform) and issues one 64-bit atomicMin.
__device__ __forceinline__ void report_bad_row(unsigned long long* status, uint32_t record, uint32_t bad) {
    if (__ballot(bad != NONE) != 0) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = __shfl_xor(bad, off, 64);
            bad = o < bad ? o : bad;
        }
        if ((threadIdx.x & 63) == 0) atomicMin(status, ((unsigned long long)record << 32) | bad);
    }
}

__device__ __forceinline__ const uint32_t* group_ptr(const uint32_t* code, const uint32_t* data, uint32_t g) { return g == GROUP_CODE ? code : data; }
// a trace cell as its residue below P (a Montgomery word): cells are compared mod P
__device__ __forceinline__ uint32_t cell(const uint32_t* code, const uint32_t* data, uint32_t g, uint32_t c, uint32_t n, uint32_t r) {
    return group_ptr(code, data, g)[(size_t)c * n + r] % P;
}
// 0 / 1 / 2 = selector 0 / 1 / anything else (NONE = the constant 1)
__device__ __forceinline__ uint32_t sel_class(const uint32_t* code, uint32_t sel, uint32_t n, uint32_t r) {
    if (sel == NONE) return 1;
    const uint32_t s = code[(size_t)sel * n + r] % P;
    return s == 0 ? 0 : s == R1 ? 1 : 2;
}

}  // namespace zkh
