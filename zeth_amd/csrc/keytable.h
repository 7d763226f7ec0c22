// keytable.h — the keyed open-addressing table over a trace that multiplicities.hip (zkh_derive_multiplicities) and bus.hip
// (zkh_check_bus) share: the key of a term at a row, its hash, and the probe.
//
// The key of a term at row r is (tag, v_0 .. v_3) as field elements, the tuple zero-padded to 4 (words compared mod P): the denominator
// alpha - (tag + beta v_0 + beta^2 v_1 + ...) of the accumulate, so a width-1 tuple (x) and a width-2 tuple (x, 0) are one key.
// A slot holds no key, only a packed entry (term << 32 | row) of it, all ones = empty: the key is re-read from the trace through the
// entry.  An entry never changes its key once it is in a slot, so whoever reads a slot, however stale, reads the slot's one key.
// The table is a power of two with empty slots left (its owner keeps it at most half full): a linear probe ends.
#pragma once
#include "arguments.h"

namespace zkh {

constexpr unsigned long long SLOT_EMPTY = ~0ull;

struct KeyTerm {                                 // a term as the keyed kernels read it
    uint32_t tag;                                // canonical
    TermCols c;
};
struct Key { uint32_t v[MAX_TUPLE]; };
static_assert(sizeof(KeyTerm) % 4 == 0, "word records");
constexpr size_t KEY_TERM_WORDS = sizeof(KeyTerm) / 4;
// the circuit's terms in that form, by blob index, as words for the upload, with room for `extra` words that the caller appends
inline std::vector<uint32_t> key_term_table(const std::vector<Term>& a, size_t extra) {
    std::vector<uint32_t> table(a.size() * KEY_TERM_WORDS + extra);
    for (size_t i = 0; i < a.size(); i++) {
        const KeyTerm t{a[i].tag, term_cols(a[i])};
        memcpy(table.data() + i * KEY_TERM_WORDS, &t, sizeof t);
    }
    return table;
}

__device__ __forceinline__ Key read_key(const uint32_t* code, const uint32_t* data, const KeyTerm& t, uint32_t n, uint32_t r) {
    Key k;
#pragma unroll
    for (uint32_t e = 0; e < MAX_TUPLE; e++) k.v[e] = e < t.c.w ? cell(code, data, t.c.tg[e], t.c.tc[e], n, r) : 0;
    return k;
}
__device__ __forceinline__ uint32_t key_hash(uint32_t tag, const Key& k) {
    uint64_t h = (tag + 1) * 0x9e3779b97f4a7c15ull;
#pragma unroll
    for (uint32_t e = 0; e < MAX_TUPLE; e++) {
        h = (h ^ k.v[e]) * 0xff51afd7ed558ccdull;
        h ^= h >> 32;
    }
    return (uint32_t)h;
}
// does the entry in a slot have the key (tag, k)?  Its key is re-read from the trace.
__device__ __forceinline__ bool slot_has_key(const uint32_t* code, const uint32_t* data, const KeyTerm* terms, unsigned long long entry,
                                             uint32_t tag, const Key& k, uint32_t n) {
    const KeyTerm& o = terms[entry >> 32];
    if (o.tag != tag) return false;
    const Key ok = read_key(code, data, o, n, (uint32_t)entry);
    bool eq = true;
#pragma unroll
    for (uint32_t e = 0; e < MAX_TUPLE; e++) eq &= ok.v[e] == k.v[e];
    return eq;
}
// the slot of key (tag, k), or NONE if it has no entry (the table always has empty slots: the probe ends)
__device__ __forceinline__ uint32_t find_slot(const uint32_t* code, const uint32_t* data, const KeyTerm* terms, const unsigned long long* slots,
                                              uint32_t mask, uint32_t tag, const Key& k, uint32_t n) {
    for (uint32_t s = key_hash(tag, k) & mask;; s = (s + 1) & mask) {
        const unsigned long long cur = slots[s];
        if (cur == SLOT_EMPTY) return NONE;
        if (slot_has_key(code, data, terms, cur, tag, k, n)) return s;
    }
}
// weight of a term's row as a canonical residue: sel * m (absent = 1)
__device__ __forceinline__ uint32_t row_weight(const uint32_t* code, const uint32_t* data, const KeyTerm& t, uint32_t n, uint32_t r) {
    uint32_t w = R1;                             // Montgomery words from here on
    if (t.c.sel != NONE) w = cell(code, data, GROUP_CODE, t.c.sel, n, r);
    if (t.c.mg != NONE) w = mul_mod(w, cell(code, data, t.c.mg, t.c.mc, n, r));
    return fp_decode(Fp::raw(w));
}

}  // namespace zkh
