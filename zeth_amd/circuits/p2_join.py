"""P2-JOIN: the join circuit of the succinct-receipt tree — Poseidon2 INSIDE the AIR.

Upstream's recursion circuit (risc0-circuit-recursion 4.0.2, un-vendored: /root/reference/Cargo.lock:5305; BASELINE.json
config 5: "lift/join recursion to a single succinct receipt") verifies two child seals in-circuit; its dominant workload is
the Poseidon2 permutation evaluated as trace rows (Merkle paths and the Fiat-Shamir sponge of the child proofs).  That
Zirgen-generated circuit cannot be obtained offline.  P2-JOIN keeps the part that can be stated from public material: it
CONSTRAINS   parent = Poseidon2-hash_pair(claim_left, claim_right)   with the permutation unrolled over trace rows, so a
join tree is a Merkle tree of claims that a verifier follows from the root receipt's `out` alone (zeth_amd/host.py
SuccinctReceipt) — and fills the rest of the segment with further permutations of the same kind (inputs bound to the
parent and to public sibling words in the code group: the shape of Merkle-path verification), ~8.4 k permutations at po2 18.
It does NOT verify the child seals (declared).  The permutation, its tables and hash_pair are the ones every Merkle tree of
the prover uses (risc0-zkp src/core/hash/poseidon2/mod.rs; pinned here by the published known-answer vector,
tests/golden/poseidon2_kat.json).

Trace (A = n - zk_cycles active rows, K = A // 31 blocks of 31 rows; row k of a block):
  k = 0      S = the permutation's input (block 0: left ‖ right ‖ 0^8; block p >= 1: parent ‖ sib_p ‖ 0^8)
  k = 1..4   S = state before full round k-1 (k = 1: M_ext of the input),  Q_j = (S_j + rc_j)^3
  k = 5..25  partial rounds 0..20: Q_0 = (S_0 + rc_0)^3
  k = 26..29 full rounds 4..7;   k = 30: S = the output state
  data (48 columns): S[24], Q[24].   x^7 = Q^2 (S + rc): every constraint has degree <= 3 (+ its selector).
  code (43 columns, a function of (po2, zk_cycles)): 0 active 1 first 2 body (accum argument)  3 in0  4 inp  5 lin
      6 fullr 7 partr (this row performs a full / partial round)  8 lf 9 lp (this row follows a full / partial round)
      10 bind0 (row 30)  11..34 the round constants of this row's round  35..42 sib_p on the input rows of blocks p >= 1
  accum: one Fp4 running product of (mix + data column 0) — SYN-AIR's argument and kernel.
Globals: out = parent (8) ‖ left (8) ‖ right (8);  mix = 4 words.
"""
from __future__ import annotations

import functools

import numpy as np

from .desc import GLOBAL_OUT, GROUP_CODE, GROUP_DATA, P, CircuitBuilder
# the permutation's shape and tables, and the constraint text P2-PAGE and P2-TREE share with this circuit: p2_blocks.py
from .p2_blocks import (BLOCK_ROWS, DIAG, HALF, M4, NBETA, R, RC, RINV, ROUNDS, RP, T, emit_rounds, gated, round_kind, running_product, sanity,  # noqa: F401
                        shipped_tables)

KIND_P2_JOIN = 3
WC, WD, WA, OUT_WORDS = 43, 48, 4, 24
C_IN0, C_INP, C_LIN, C_FULLR, C_PARTR, C_LF, C_LP, C_BIND0, C_RC, C_SIB = 3, 4, 5, 6, 7, 8, 9, 10, 11, 35


def m_ext(s):
    out = [0] * T
    for c in range(0, T, 4):
        for i in range(4):
            out[c + i] = sum(M4[i][j] * s[c + j] for j in range(4)) % P
    sums = [sum(out[c + i] for c in range(0, T, 4)) % P for i in range(4)]
    return [(out[k] + sums[k % 4]) % P for k in range(T)]


def block_rows(inp):
    """One permutation as trace rows over canonical residues: [(S[24], Q[24])] for k = 0..30.  The plain-Python statement
    of what the witness generators (oracle/p2join.c, circuit.hip k_p2join_*) must produce; rows[30][0] is the output."""
    rows = [([x % P for x in inp], [0] * T)]
    s = m_ext(rows[0][0])
    for rnd in range(ROUNDS):
        rc = RC[rnd * T:(rnd + 1) * T]
        if HALF <= rnd < HALF + RP:
            q = [pow((s[0] + rc[0]) % P, 3, P)] + [0] * (T - 1)
            rows.append((s, q))
            x7 = q[0] * q[0] % P * ((s[0] + rc[0]) % P) % P
            tot = (x7 + sum(s[1:])) % P
            s = [(tot + DIAG[0] * x7) % P] + [(tot + DIAG[i] * s[i]) % P for i in range(1, T)]
        else:
            q = [pow((s[i] + rc[i]) % P, 3, P) for i in range(T)]
            rows.append((s, q))
            s = m_ext([q[i] * q[i] % P * ((s[i] + rc[i]) % P) % P for i in range(T)])
    rows.append((s, [0] * T))
    return rows


def permute(state):
    return block_rows(state)[-1][0]


def hash_pair_words(left, right):
    """`hash_pair` on raw Montgomery words (what Merkle nodes and claims are): 8 + 8 words -> 8 words."""
    st = [int(w) * RINV % P for w in list(left) + list(right)] + [0] * 8
    return [v * R % P for v in permute(st)[:8]]


@functools.lru_cache(maxsize=None)
def build_p2_join() -> np.ndarray:
    b = CircuitBuilder((WA, WC, WD), (OUT_WORDS, WA), kind=KIND_P2_JOIN)
    code = lambda c, back=0: b.get(GROUP_CODE, c, back)
    S = lambda j, back=0: b.get(GROUP_DATA, j, back)
    out = lambda i: b.get_global(GLOBAL_OUT, i)
    b.const(1)
    active, first, body = code(0), code(1), code(2)
    cst = {v: b.const(v) for v in (2, 3, 4, 5, 6, 7)}

    chain = b.true()
    # inputs
    chain = gated(b, chain, code(C_IN0), [b.sub(S(i), out(8 + i)) for i in range(16)] + [S(16 + i) for i in range(8)])
    chain = gated(b, chain, code(C_INP), [b.sub(S(i), out(i)) for i in range(8)] + [b.sub(S(8 + i), code(C_SIB + i)) for i in range(8)]
                  + [S(16 + i) for i in range(8)])
    # the cubes of this row's round, and the links: this row's state from the previous row
    chain = emit_rounds(b, chain, code, S, cst, ((0, T),), (C_LIN, C_FULLR, C_PARTR, C_LF, C_LP, C_RC), diag_first=False)
    # block 0's output is the parent claim
    chain = gated(b, chain, code(C_BIND0), [b.sub(S(i), out(i)) for i in range(8)])
    # accum: one Fp4 running product of (mix + data column 0), SYN-AIR's argument; selector sanity (ungated)
    chain = running_product(b, chain, first, body, S(0))
    return b.finish(sanity(b, chain, active, first, body))


def p2_join_circuit() -> np.ndarray:
    return build_p2_join().copy()


if __name__ == "__main__":      # python -m zeth_amd.circuits.p2_join out.desc   (blob for non-Python hosts, e.g. examples/seal_segments)
    import sys
    blob = p2_join_circuit()
    np.asarray(blob, dtype="<u4").tofile(sys.argv[1])
    print(f"{sys.argv[1]}: {blob.size} words")
