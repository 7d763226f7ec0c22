"""The two lane-per-permutation Merkle kernels against the oracle, at the shapes where their sponge takes another path:
k_hash_rows (interior blocks keep a signed capacity, the last block keeps the digest; full blocks and a tail block share one
call site of the permutation) and k_hash_fold (zero-capacity entry).  Random words and the fills that put every cell at an
extreme of its representation at once."""
import numpy as np
import pytest

from conftest import rand_fp

pytestmark = pytest.mark.gpu
P = 2013265921
ROWS = (1, 63, 64, 65, 257)
COLS = (0, 1, 15, 16, 17, 32, 33, 48)          # empty, tail only, one block, block + tail, two blocks, ..., three blocks
PARENTS = (1, 2, 255, 256, 257)
FILLS = ("random", "all P-1", "all 0", "alternating (P+-1)/2")


def fill(kind, n, rng):
    if kind == "random":
        return rand_fp(rng, n)
    if kind == "all P-1":
        return np.full(n, P - 1, dtype=np.uint32)
    if kind == "all 0":
        return np.zeros(n, dtype=np.uint32)
    a = np.full(n, (P - 1) // 2, dtype=np.uint32)
    a[1::2] = (P + 1) // 2
    return a


@pytest.mark.parametrize("rows", ROWS)
def test_hash_rows_equals_oracle(hal, oracle, rows):
    rng = np.random.default_rng(1100 + rows)
    for cols in COLS:
        for kind in FILLS:
            mat = fill(kind, rows * cols, rng)
            m = hal.copy_from("m", mat) if cols else hal.alloc("m", 0)
            out = hal.alloc_digest("leaves", rows)
            hal.hash_rows(out, m)
            want = np.zeros(rows * 8, dtype=np.uint32)
            oracle.zko_hash_rows(want, rows, np.ascontiguousarray(mat) if cols else np.zeros(1, np.uint32), rows * cols)
            got = out.to_vec()
            assert got.max() < P, (rows, cols, kind)
            assert np.array_equal(got, want), (rows, cols, kind)


@pytest.mark.parametrize("parents", PARENTS)
def test_hash_fold_equals_oracle(hal, oracle, parents):
    """hal.hash_fold always runs the lane-per-parent kernel: parents [p, 2p) from children [2p, 4p)."""
    rng = np.random.default_rng(1200 + parents)
    for kind in FILLS:
        nodes = np.zeros(4 * parents * 8, dtype=np.uint32)
        nodes[2 * parents * 8:] = fill(kind, 2 * parents * 8, rng)
        io = hal.copy_from("nodes", nodes)
        hal.hash_fold(io, 2 * parents, parents)
        want = nodes.copy()
        oracle.zko_hash_fold(want, 2 * parents, parents)
        got = io.to_vec()
        assert got.max() < P, (parents, kind)
        assert np.array_equal(got, want), (parents, kind)
