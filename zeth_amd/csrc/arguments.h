// arguments.h — lookup and permutation arguments as data (ZKA1 blob; zeth_amd/circuits/logup.py; DESIGN.md §2 ARGUMENTS): the decoded
// form every consumer reads, and what the consumers share.  arguments.hip owns the blob format and the rules a blob must keep;
// accumulate.hip (zkh_accumulate), multiplicities.hip (zkh_derive_multiplicities), sort.hip (zkh_derive_sorted), columns.hip
// (zkh_derive_columns) and links.hip (zkh_derive_links) read zkh_circuit::args and never see a blob word.
#pragma once
#include <vector>

#include "circuit.h"

namespace zkh {

constexpr uint32_t ARGS_MAGIC = 0x5a4b4131u;        // 'ZKA1'
constexpr uint32_t ARGS_HEADER = 8, TERM_WORDS = 16;
constexpr uint32_t MAX_TUPLE = 4, MAX_TERMS = 3, MAX_SORT_KEYS = 3, NONE = 0xffffffffu;
constexpr uint32_t RECORD_WORDS = 16, KIND_LIMBS = 1, KIND_ORDER = 2, MAX_LIMBS = 8;
constexpr uint32_t KIND_LINK = 3, LINK_WORDS = 32, MAX_CARRIED = 3, MAX_LINK_LIMBS = 4, MAX_LINK_DSTS = 2 + MAX_CARRIED + MAX_LINK_LIMBS;
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
// logup.Link, a LINK record (version 5), as the blob gives it; the kernels of links.hip read it in this form
struct Link {
    uint32_t index;                         // its index among all records of the blob (LINK records follow the LIMBS / ORDER ones)
    uint32_t L, nl, nc, sel;                // limb bits; limb count; carried columns; selector code column or NONE
    uint32_t kg, kc;                        // the key's (group, column)
    uint32_t cg[MAX_CARRIED], cc[MAX_CARRIED];      // the carried columns, the first nc; c_0 is the clock
    uint32_t dst[MAX_LINK_DSTS];            // destination data columns: linked, last, prev_0 .. prev_{nc-1}, limb_0 .. limb_{nl-1}
    uint32_t n_dst, reserved;               // destinations in use; a word the format reserves was not 0
};
// logup.Arguments
struct Arguments {
    uint32_t version, k, alpha, beta;       // blob version; accum Fp4 columns; mix word offsets of the two challenges
    std::vector<Term> terms;
    std::vector<Record> records;            // the LIMBS / ORDER records: their index here is their index in the blob
    std::vector<Link> links;                // the LINK records
    uint32_t late_record = NONE, late_after = 0;    // a LIMBS / ORDER record that follows a LINK record, and that LINK record (refused)
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

// what the entry points over a trace share: po2 in 1..24, an active row left, the code / data (and, if given, accum) buffers of the
// circuit's widths at 2^po2 rows.  `who` prefixes the messages.  *n = rows, *A = active rows.
const char* trace_rows(const char* who, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* data,
                       const zkh_buf* accum, size_t* n, uint32_t* A);

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
