"""What the page-out circuits (P2-JOIN, P2-PAGE, P2-PAGE-ordered, P2-TREE) must keep while the code they share moves: every blob word
for word (sha256 of its little-endian uint32 words), the step ranges of the constraint families, the names the tests and
tools/microbench.py import from the four modules, and prover.link_page_parts, the one linking loop behind verify_page_out_chain,
verify_page_ordered_chain and link_page_tree_chain, on hand-made parts: one exact message per cause under each public prefix.  No seal
and no device."""
import hashlib
import re

import numpy as np
import pytest

from zeth_amd import prover
from zeth_amd.circuits import p2_join, p2_page, p2_page_ordered, p2_tree
from zeth_amd.hal import HalError

BLOBS = {
    "p2_join": (p2_join.p2_join_circuit, 6374, "40955f0229165830ab61d7d368f52c0dbf8a8ab7e66a866a869eb21a372ea5a3"),
    "p2_page": (p2_page.p2_page_circuit, 13303, "770fdd0363d8f334464e41de454daf7677713243a0f952a82a3660f0949c0f8e"),
    "p2_page_ordered": (p2_page_ordered.p2_page_ordered_circuit, 13658, "82803e2fc8f034a577afe37345533fa84d793f857f280f9406a77ac361265e3f"),
    "p2_tree": (p2_tree.p2_tree_circuit, 22948, "57f977c3714737455985935b324f213b7d8d13c6bdaa644cc3a34483a8d8c2c2"),
    "p2_tree_arguments": (p2_tree.arguments, 296, "3783fef077c41a4f2d9d604d9b0d7f9203669582ab0dbe97cd821d075c791060"),
}

PAGE_HEAD = [("rounds", 13, 1847), ("leaf_in", 1876, 2111), ("node_in", 2111, 2266), ("carry", 2266, 2307), ("top_out", 2307, 2328), ("roots", 2328, 2400)]
FAMILIES = {
    "p2_page": (p2_page, PAGE_HEAD + [("accum", 2400, 2465), ("sanity", 2465, 2474)]),
    "p2_page_ordered": (p2_page_ordered, PAGE_HEAD + [("order", 2400, 2465), ("accum", 2465, 2530), ("sanity", 2530, 2539)]),
    "p2_tree": (p2_tree, [("rounds", 12, 1845), ("in_row", 1856, 1933), ("carry", 1933, 1968), ("order", 1968, 2016), ("root", 2016, 2069), ("bus", 2069, 4382),
                          ("sanity", 4382, 4391)]),
}

# every name a test or tools/microbench.py takes from the four modules
IMPORTED = {
    p2_join: "P R RINV WC WD block_rows hash_pair_words p2_join_circuit permute round_kind",
    p2_page: "BLOCK_ROWS D_ADDR D_B D_CUR D_E D_SN D_W_IN D_W_OUT FAMILIES KIND_P2_PAGE MAX_H WA WC WD constraint_degrees family_of p2_page_circuit parts "
             "reference_page_code reference_page_part reference_page_trace slots tree_height",
    p2_page_ordered: "C_GSEL D_GACC D_GBIT D_LIVE D_LO FAMILIES GAP_BITS KIND_P2_PAGE_ORDERED MAX_H WA WC WD decode family_of p2_page_ordered_circuit "
                     "reference_ordered_code reference_ordered_part",
    p2_tree: "C_GEND C_GPOW C_IN_ROW C_LAST C_LAST_TOP C_OUT_ROW D_DL D_DR D_GACC D_GBIT D_ID D_IDL D_IDR D_LEAF D_LO D_SN D_SO D_UP FAMILIES GAP_BITS "
             "KIND_P2_TREE MIX_WORDS WA WC WD arguments block_slots decode family_of p2_tree_circuit parts reference_tree_code reference_tree_part",
}


@pytest.mark.parametrize("name", sorted(BLOBS))
def test_blob_is_word_for_word(name):
    build, words, digest = BLOBS[name]
    blob = np.asarray(build())
    assert blob.size == words
    assert hashlib.sha256(blob.astype("<u4").tobytes()).hexdigest() == digest


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_family_ranges(name):
    module, want = FAMILIES[name]
    for family, lo, hi in want:                        # family_of builds the description, which fills FAMILIES
        assert module.family_of(lo) == family == module.family_of(hi - 1)
    assert [tuple(f) for f in module.FAMILIES] == want


def test_imported_names_resolve():
    for module, names in IMPORTED.items():
        missing = [n for n in names.split() if not hasattr(module, n)]
        assert not missing, f"{module.__name__}: {missing}"
    assert p2_page_ordered.decode(p2_join.R) == p2_tree.decode(p2_join.R) == 1
    assert p2_page.tree_height(9) == 1 and p2_page.tree_height(65) == 4


# ---------------------------------------------------------------------------------------------------- the linking loop
H = 5                                                   # the tree height the P2-TREE kind is told
ROOT = [np.arange(8, dtype=np.uint32) + 0x100 * i for i in range(5)]
FMT = [" ".join(f"{int(w):08x}" for w in r) for r in ROOT]
# per public prefix: whether its parts carry lo and hi, the lo part 0 must have and the words after "not ", the bound of the last hi
KINDS = {
    "verify_page_out_chain": dict(lo0=None),
    "verify_page_ordered_chain": dict(lo0=0, first_lo=(0, "0: addresses below it are not covered")),
    "verify_page_tree_chain": dict(lo0=16, first_lo=(16, "2^4 = 16, the id of the first pair of leaves of a tree of height 5"),
                                   last_hi=(32, "2^5 = 32: a pair block outside a tree of height 5")),
}
ORDERED = [who for who, k in KINDS.items() if k["lo0"] is not None]


def _chain(who, bounds=None):
    """three good parts ROOT[0] -> ROOT[3]; the ordered kinds with the lo / hi runs `bounds` (default: three ids from the kind's lo)"""
    lo0 = KINDS[who]["lo0"]
    roots = [(ROOT[p], ROOT[p + 1]) for p in range(3)]
    if lo0 is None:
        return roots
    bounds = bounds or [(lo0, lo0 + 3), (lo0 + 3, lo0 + 4), (lo0 + 4, lo0 + 9)]
    return [r + b for r, b in zip(roots, bounds)]


def _link(who, parts, root_before=None):
    kind = {k: v for k, v in KINDS[who].items() if k != "lo0"}
    return prover.link_page_parts(who, parts, root_before, **kind)


def _refused(who, parts, message, root_before=None):
    with pytest.raises(HalError, match="^" + re.escape(f"{who}: {message}") + "$"):
        _link(who, parts, root_before)


@pytest.mark.parametrize("who", sorted(KINDS))
def test_link_good_chain(who):
    got = _link(who, _chain(who), ROOT[0])
    assert np.array_equal(got[0], ROOT[0]) and np.array_equal(got[1], ROOT[3])
    assert len(got) == (2 if KINDS[who]["lo0"] is None else 3)
    if KINDS[who]["lo0"] is not None:
        assert got[2] == KINDS[who]["lo0"] + 9
    assert np.array_equal(_link(who, iter(_chain(who)))[1], ROOT[3]), "parts may be an iterator, and root_before is optional"


@pytest.mark.parametrize("who", sorted(KINDS))
def test_link_refuses_roots(who):
    _refused(who, [], "no receipt (a page-out of no rows still has one part)")
    _refused(who, _chain(who), f"part 0 opens root {FMT[0]}, not root_before {FMT[4]}", root_before=ROOT[4])
    parts = _chain(who)
    parts[2] = (ROOT[4],) + parts[2][1:]
    _refused(who, parts, f"part 2 opens root {FMT[4]}, but part 1 left root {FMT[2]}")


@pytest.mark.parametrize("who", ORDERED)
def test_link_refuses_bounds(who):
    lo0, big = KINDS[who]["lo0"], (1 << 29) + 1
    _refused(who, _chain(who, [(lo0, lo0 + 3), (lo0 + 3, big), (big, big)]), f"part 1: hi {big} is above 2^29, the bound the order check is sound for")
    _refused(who, _chain(who, [(lo0, lo0 + 3), (big, lo0 + 4), (lo0 + 4, lo0 + 9)]), f"part 1: lo {big} is above 2^29, the bound the order check is sound for")
    _link(who, _chain(who, [(lo0, lo0 + 1), (lo0 + 1, lo0 + 1), (lo0 + 1, lo0 + 2)]))       # a part without a live update: hi = lo
    _refused(who, _chain(who, [(lo0 + 1, lo0 + 3), (lo0 + 3, lo0 + 4), (lo0 + 4, lo0 + 9)]), f"part 0 starts at lo {lo0 + 1}, not {KINDS[who]['first_lo'][1]}")
    _refused(who, _chain(who, [(lo0, lo0 + 3), (lo0 + 2, lo0 + 4), (lo0 + 4, lo0 + 9)]), f"part 1 starts at lo {lo0 + 2}, but part 0 left hi {lo0 + 3}")
    # the first cause in the order the public functions report them: a bound, the first lo, the first root, a link
    _refused(who, _chain(who, [(lo0 + 1, lo0 + 3), (lo0 + 2, big), (big, big)]), f"part 1: hi {big} is above 2^29, the bound the order check is sound for",
             root_before=ROOT[4])
    _refused(who, _chain(who, [(lo0 + 1, lo0 + 3), (lo0 + 2, lo0 + 4), (lo0 + 4, lo0 + 9)]), f"part 0 starts at lo {lo0 + 1}, not {KINDS[who]['first_lo'][1]}",
             root_before=ROOT[4])


def test_link_refuses_a_last_hi_outside_the_tree():
    who = "verify_page_tree_chain"
    _link(who, _chain(who, [(16, 19), (19, 20), (20, 32)]))
    _refused(who, _chain(who, [(16, 19), (19, 20), (20, 33)]), "the last part leaves hi 33, above 2^5 = 32: a pair block outside a tree of height 5")
    # ... and through the public function, which decodes the out words and is told h
    enc = lambda x: x * p2_join.R % p2_join.P
    outs = [np.concatenate([a, b, [enc(lo), enc(hi)]]).astype(np.uint32) for a, b, lo, hi in _chain(who, [(16, 19), (19, 20), (20, 33)])]
    with pytest.raises(HalError, match=re.escape("verify_page_tree_chain: the last part leaves hi 33, above 2^5 = 32: a pair block outside a tree of height 5")):
        prover.link_page_tree_chain(outs, H)
    outs[2][17] = enc(32)
    before, after, hi = prover.link_page_tree_chain(outs, H, ROOT[0])
    assert np.array_equal(before, ROOT[0]) and np.array_equal(after, ROOT[3]) and hi == 32
