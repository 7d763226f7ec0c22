"""What the circuits built from Poseidon2 BLOCKS share: P2-JOIN (p2_join.py), P2-PAGE (p2_page.py), P2-PAGE-ordered
(p2_page_ordered.py) and P2-TREE (p2_tree.py).  A block is 31 trace rows, one permutation laid out round by round (p2_join.py's
docstring has the row roles).  Here: the permutation's shape and shipped tables; the pieces of constraint text the builders emit
(`gated`, the family log, the `rounds` family, the Fp4 running product, the selector sanity); and the pieces of the host twins
(Montgomery words, the tree's height, the round columns of a code group, the gap-bit columns).

A description numbers its steps in emission order, and constants, globals and taps are emitted once, where they are first asked for.
So a piece emits exactly what the builders emitted before they shared it, in the same order: tests/test_page_blobs.py pins every blob.
NOT shared: the two `order` families (p2_page_ordered._order over (live, addr), p2_tree's over (leaf, id)).  They state the same gap
decomposition but emit its constraints in different orders, and either order taken over would change the other's blob.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from .desc import GLOBAL_MIX, GROUP_ACCUM, P

T, HALF, RP = 24, 4, 21
ROUNDS = 2 * HALF + RP
BLOCK_ROWS = ROUNDS + 2                     # input row, 29 round rows, output row
M4 = ((5, 7, 1, 3), (4, 6, 1, 1), (1, 3, 5, 7), (1, 1, 4, 6))
NBETA = P - 11
R = (1 << 32) % P
RINV = pow(R, -1, P)
GAP_BITS = 29                               # the bits a gap between two addresses (P2-PAGE-ordered) or two ids (P2-TREE) is decomposed into


def shipped_tables():
    """(rc[24 * 29], diag[24]) canonical residues: circuits/poseidon2_consts.py, generated in the same run as
    include/zkh_poseidon2_consts.h (tests/test_abi_and_host.py compares the two word for word)."""
    from . import poseidon2_consts as pc
    return list(pc.ROUND_CONSTANTS), list(pc.M_INT_DIAG)


RC, DIAG = shipped_tables()


def round_kind(k: int) -> str:
    """what row k of a block DOES: 'in', 'full', 'partial' or 'out'"""
    if k == 0:
        return "in"
    if k <= HALF or HALF + RP < k <= ROUNDS:
        return "full"
    if k <= HALF + RP:
        return "partial"
    return "out"


# ------------------------------------------------------------------------------------------------ constraint text
def gated(b, chain, sel, constraints):
    """`chain` and, where the selector `sel` is set, every one of `constraints` = 0"""
    inner = b.true()
    for c in constraints:
        inner = b.and_eqz(inner, c)
    return b.and_cond(chain, sel, inner)


def family_log(b):
    """-> (families, family): family(name, start) logs the steps [start, len(b.steps)) of the builder as the family `name`"""
    families: List[Tuple[str, int, int]] = []
    return families, lambda name, start: families.append((name, start, len(b.steps)))


def family_of(families, step: int) -> str:
    """the name of the family of `families` that holds a step of the description"""
    for name, lo, hi in families:
        if lo <= step < hi:
            return name
    raise ValueError(f"step {step} is outside the description")


def emit_rounds(b, chain, code, dat, cst, sides, cols, input_rows=None, diag_first=True):
    """The `rounds` family, emitted onto `chain`: the round constraints of one permutation on every (S, Q) pair of `sides` (data
    column offsets), and the capacity cells S[16 .. 24) zero where the selector `input_rows()` (built after the round constraints, as
    the builders always did) is set.  cols = the code columns (lin, fullr, partr, lf, lp, rc); cst = the constants 2 .. 7 as handles.
    diag_first: the diagonal's constants are emitted before the first side (P2-PAGE, P2-TREE); else where the partial round's link
    first needs them (P2-JOIN, which also states its capacity cells with its inputs: no input_rows)."""
    c_lin, c_fullr, c_partr, c_lf, c_lp, c_rc = cols

    def times(c, x):
        return x if c == 1 else b.mul(cst[c], x)

    def lin_m_ext(x):                                  # the 24 x 24 external matrix as expressions over 24 values
        y = []
        for blk in range(0, T, 4):
            for i in range(4):
                e = times(M4[i][0], x[blk])
                for j in range(1, 4):
                    e = b.add(e, times(M4[i][j], x[blk + j]))
                y.append(e)
        tot = []
        for i in range(4):
            e = y[i]
            for blk in range(4, T, 4):
                e = b.add(e, y[blk + i])
            tot.append(e)
        return [b.add(y[k], tot[k % 4]) for k in range(T)]

    if diag_first:
        for d in DIAG:
            b.const(d)
    cube = lambda x: b.mul(b.mul(x, x), x)
    cap = []
    for s0, q0 in sides:
        S = lambda j, back=0, s0=s0: dat(s0 + j, back)
        Q = lambda j, back=0, q0=q0: dat(q0 + j, back)
        u = [b.add(S(j), code(c_rc + j)) for j in range(T)]
        chain = gated(b, chain, code(c_fullr), [b.sub(Q(j), cube(u[j])) for j in range(T)])
        chain = gated(b, chain, code(c_partr), [b.sub(Q(0), cube(u[0]))])
        prev = [S(j, 1) for j in range(T)]
        chain = gated(b, chain, code(c_lin), [b.sub(S(k), e) for k, e in enumerate(lin_m_ext(prev))])
        x7 = [b.mul(b.mul(Q(j, 1), Q(j, 1)), b.add(S(j, 1), code(c_rc + j, 1))) for j in range(T)]
        chain = gated(b, chain, code(c_lf), [b.sub(S(k), e) for k, e in enumerate(lin_m_ext(x7))])
        tot = x7[0]
        for j in range(1, T):
            tot = b.add(tot, prev[j])
        diag = [b.const(d) for d in DIAG]              # handles of constants: emitted once
        chain = gated(b, chain, code(c_lp), [b.sub(S(0), b.add(tot, b.mul(diag[0], x7[0])))]
                      + [b.sub(S(j), b.add(tot, b.mul(diag[j], prev[j]))) for j in range(1, T)])
        cap += [S(16 + i) for i in range(8)]
    return gated(b, chain, input_rows(), cap) if input_rows else chain


def running_product(b, chain, first, body, col0):
    """The accum family of P2-JOIN and P2-PAGE: one Fp4 running product of (mix + col0) over the four accum columns, SYN-AIR's
    argument and kernel."""
    acc = lambda c, back=0: b.get(GROUP_ACCUM, c, back)
    nbeta = b.const(NBETA)
    m = [b.get_global(GLOBAL_MIX, i) for i in range(4)]
    term = [b.add(m[0], col0), m[1], m[2], m[3]]
    chain = gated(b, chain, first, [b.sub(acc(i), term[i]) for i in range(4)])
    pa = [acc(i, 1) for i in range(4)]
    mm = lambda i, j: b.mul(pa[i], term[j])
    pr = [b.add(mm(0, 0), b.mul(nbeta, b.add(b.add(mm(1, 3), mm(2, 2)), mm(3, 1)))),
          b.add(b.add(mm(0, 1), mm(1, 0)), b.mul(nbeta, b.add(mm(2, 3), mm(3, 2)))),
          b.add(b.add(b.add(mm(0, 2), mm(1, 1)), mm(2, 0)), b.mul(nbeta, mm(3, 3))),
          b.add(b.add(mm(0, 3), mm(1, 2)), b.add(mm(2, 1), mm(3, 0)))]
    return gated(b, chain, body, [b.sub(acc(i), pr[i]) for i in range(4)])


def sanity(b, chain, active, first, body):
    """the selector sanity (ungated): active and first are boolean, body = active - first"""
    one = b.const(1)
    chain = b.and_eqz(chain, b.mul(active, b.sub(one, active)))
    chain = b.and_eqz(chain, b.mul(first, b.sub(one, first)))
    return b.and_eqz(chain, b.sub(b.sub(active, first), body))


# ------------------------------------------------------------------------------------------------ host twins
def enc(x: int) -> int:
    """the Montgomery word of the integer x"""
    return x % P * R % P


def decode(word: int) -> int:
    """the integer a Montgomery word of the trace (out[16], out[17]) stands for"""
    return int(word) % P * RINV % P


def tree_height(image_words: int) -> int:
    """h = log2 L of an image of W words, L the smallest power of two >= ceil(W / 8)"""
    L = 1
    while 8 * L < image_words:
        L <<= 1
    return L.bit_length() - 1


def reference_round_code(wc: int, po2: int, zk_cycles: int, blocks: int, cols) -> np.ndarray:
    """A code group of `wc` columns, (wc, 2^po2) Montgomery words, with what every block circuit's has: active, first, body in columns
    0 .. 2, and on the rows of the first `blocks` blocks the round columns cols = (lin, fullr, partr, lf, lp, rc)."""
    c_lin, c_fullr, c_partr, c_lf, c_lp, c_rc = cols
    n = 1 << po2
    A = n - zk_cycles
    code = np.zeros((wc, n), dtype=np.uint32)
    code[0, :A] = R
    code[1, 0] = R
    code[2, 1:A] = R
    for k in range(1, BLOCK_ROWS):
        rows = slice(k, BLOCK_ROWS * blocks, BLOCK_ROWS)
        kind = round_kind(k)
        if k == 1:
            code[c_lin, rows] = R
        if kind == "full":
            code[c_fullr, rows] = R
            for j in range(T):
                code[c_rc + j, rows] = enc(RC[(k - 1) * T + j])
        if kind == "partial":
            code[c_partr, rows] = R
            code[c_rc, rows] = enc(RC[(k - 1) * T])
        if k >= 2:
            code[c_lf if round_kind(k - 1) == "full" else c_lp, rows] = R
    return code


def gap_columns(g: int):
    """(gbit, gacc) on the rows k = 1 .. 29 of a block: bit k - 1 of the gap g, and g mod 2^k"""
    return [R * ((g >> k) & 1) for k in range(GAP_BITS)], [enc(g % (2 << k)) for k in range(GAP_BITS)]
