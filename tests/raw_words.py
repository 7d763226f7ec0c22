"""Raw words >= P, for the tests that hold the trace path to one rule (imported the way args_gpu is): a trace cell is read as its residue,
raw % P, so the result on a trace T' equals the result on T = T' % P.  `raise_words` makes T' from T; `assert_raised` is what every test
says about the traces it actually uploads, so that none passes on reduced input.

2^32 = 2 P + 268435454: a residue w has the words w and w + P, and w + 2 P as well when w < 2^32 - 2 P.  The words a test plants by hand
where its witness allows (`plant`): P and 2 P (zero), R1 + P (Montgomery one), and 0xFFFFFFFF, which is the word just below 2^32 - 2 P
raised by 2 P."""
import numpy as np

P = 2013265921
R1 = (1 << 32) % P                              # Montgomery one
TOP = (1 << 32) - 2 * P - 1                     # the largest word that w + 2 P fits: TOP + 2 P = 0xFFFFFFFF
EDGES = (0, 0, R1, TOP)                         # the residues `plant` writes, in this order: raised to P, 2 P, R1 + P, 0xFFFFFFFF
EDGE_WORDS = (P, 2 * P, R1 + P, 0xFFFFFFFF)


def plant(a, rng, rows=None):
    """a copy of `a` ((columns, n), or one column) with the residues EDGES written at distinct random places (of `rows`, if given): for
    a test whose witness does not care what those cells hold.  raise_words then raises exactly these to EDGE_WORDS."""
    out = np.array(a, dtype=np.uint32)
    v = out.reshape(-1, out.shape[-1])
    rows = np.arange(v.shape[1]) if rows is None else np.asarray(rows)
    at = rng.choice(v.shape[0] * rows.size, len(EDGES), replace=False)
    for k, w in zip(at, EDGES):
        v[k // rows.size, rows[k % rows.size]] = w
    return out


def raise_words(a, rng, share, rows=None):
    """a copy of `a` ((columns, n), or one column of n words) in which a `share` of the words, of the rows `rows` if given, becomes
    w + P, and about half of those below 2^32 - 2 P become w + 2 P.  Planted by hand wherever `a` holds the residue among the words in
    reach: the first two zeros become P and 2 P, the first R1 becomes R1 + P, the first TOP becomes 0xFFFFFFFF.  The residues are those
    of `a`; at least a fifth of the words in reach are >= P and some are >= 2 P (asserted)."""
    a = np.asarray(a, dtype=np.uint32)
    v = a.reshape(-1, a.shape[-1]).astype(np.uint64)
    rows = np.arange(v.shape[1]) if rows is None else np.asarray(rows)
    sub = v[:, rows]
    add = np.where((rng.random(sub.shape) < share) & (sub < (1 << 32) - P), P, 0).astype(np.uint64)
    add[(add != 0) & (sub < (1 << 32) - 2 * P) & (rng.random(sub.shape) < 0.5)] = 2 * P
    flat, fadd = sub.reshape(-1), add.reshape(-1)
    zeros, ones, tops = np.flatnonzero(flat == 0), np.flatnonzero(flat == R1), np.flatnonzero(flat == TOP)
    for at, by in ((zeros[:1], P), (zeros[1:2], 2 * P), (ones[:1], P), (tops[:1], 2 * P)):
        fadd[at] = by
    v[:, rows] = sub + add
    out = v.astype(np.uint32).reshape(a.shape)
    assert_raised(out, a, rows)
    return out


def assert_raised(raised, reduced, rows=None):
    """`raised` holds the residues of `reduced` (all words), and of its words on `rows` (default: all) at least a fifth are >= P and some
    are >= 2 P"""
    raised, reduced = np.asarray(raised, dtype=np.uint32), np.asarray(reduced, dtype=np.uint32)
    assert raised.shape == reduced.shape and np.array_equal(raised % P, reduced % P)
    sub = raised.reshape(-1, raised.shape[-1])
    sub = sub if rows is None else sub[:, rows]
    assert 5 * int((sub >= P).sum()) >= sub.size and (sub >= 2 * P).any(), (int((sub >= P).sum()), sub.size)


def planted(raised):
    """the EDGE_WORDS that `raised` holds"""
    return {w for w in EDGE_WORDS if (np.asarray(raised) == np.uint32(w)).any()}
