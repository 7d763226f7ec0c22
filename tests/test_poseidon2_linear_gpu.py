"""The partial rounds of k_hash_rows and k_hash_fold as int8 matrix products (zeth_amd/csrc/poseidon2_linear.h) on the device:
the tile product alone through the library's test hook (this pins the A / B / C lane maps of v_mfma_i32_32x32x32_i8 and both
directions of the half-wave swap with exact, asymmetric integers), then the two kernels against the oracle at the shapes
where the wave-wide path can go wrong: the half-wave boundary, partial waves (lanes past the end stay in the wave and only
their store is predicated), several waves and blocks, empty / tail-only / multi-block sponges."""
import ctypes as C

import numpy as np
import pytest

from conftest import rand_fp
from test_poseidon2_callers_gpu import FILLS, fill

pytestmark = pytest.mark.gpu
P = 2013265921
ROWS = (1, 31, 32, 33, 63, 64, 65, 96, 257)
COLS = (0, 1, 16, 17, 48, 208)
PARENTS = (1, 31, 32, 33, 64, 65, 257)


def test_tile_product_lane_maps_and_swaps(hal):
    """One wave, one 32 x 32 x 32 product per half-wave of columns.  A is a permutation-like matrix with distinct entries (row r
    has its one entry at k = 5 r + 3 mod 32, a bijection, with a value that names the row) plus a dense asymmetric part; B is
    different in every lane and every byte.  The hook returns, per lane, lo = r_0 + (r_1 << 8) and hi = r_2 + (r_3 << 8) of the
    eight outputs of the lane's OWN column, whose rows a half-wave swap of the two tiles' accumulators gathers."""
    from zeth_amd import hal as H
    lib = H.load_library()
    fn = lib.zkh_test_lin_tile
    fn.restype, fn.argtypes = C.c_void_p, [C.c_void_p] * 4
    rng = np.random.default_rng(77)
    a = rng.integers(-3, 4, size=(32, 32)).astype(np.int8)
    for r in range(32):
        a[r, (5 * r + 3) % 32] = np.int8(r * 7 - 110)                     # distinct, both signs
    b = rng.integers(-128, 128, size=(64, 32)).astype(np.int8)           # column l = lane l's own 32 bytes
    b[:, 0] = np.arange(64, dtype=np.int64).astype(np.int8) - 30         # names the lane
    da = hal.copy_from("a", a.view(np.uint32).reshape(-1))
    db = hal.copy_from("b", b.view(np.uint32).reshape(-1))
    out = hal.alloc("out", 2048, zero=True)
    H._check(fn(hal.ctx, da.h, db.h, out.h))
    got = out.to_vec().view(np.int32).reshape(64, 32)
    c = a.astype(np.int64) @ b.astype(np.int64).T                         # c[row, lane]
    for lane in range(64):
        for o in range(8):
            rows = [8 * (o >> 1) + 4 * (o & 1) + i for i in range(4)]    # lin_row(o, i)
            lo = c[rows[0], lane] + (c[rows[1], lane] << 8)
            hi = c[rows[2], lane] + (c[rows[3], lane] << 8)
            assert (got[lane, 4 * o], got[lane, 4 * o + 1]) == (lo, hi), (lane, o)


@pytest.mark.parametrize("rows", ROWS)
def test_hash_rows_equals_oracle(hal, oracle, rows):
    rng = np.random.default_rng(2100 + rows)
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
    rng = np.random.default_rng(2200 + parents)
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


def test_merkle_build_and_three_openings_equal_oracle(hal, oracle):
    """2^10 leaves of 17 columns: the tree, and the openings (leaf digest and the sibling at every layer) at three positions."""
    rows, cols = 1 << 10, 17
    mat = rand_fp(np.random.default_rng(2300), rows * cols)
    nodes = hal.alloc_digest("nodes", 2 * rows)
    hal.merkle_build(nodes, hal.copy_from("m", mat), rows)
    got = nodes.to_vec().reshape(2 * rows, 8)
    want = np.zeros(2 * rows * 8, dtype=np.uint32)
    leaves = np.zeros(rows * 8, dtype=np.uint32)
    oracle.zko_hash_rows(leaves, rows, mat, rows * cols)
    want[rows * 8:] = leaves
    size = rows
    while size > 1:
        oracle.zko_hash_fold(want, size, size // 2)
        size //= 2
    want = want.reshape(2 * rows, 8)
    for pos in (0, 613, rows - 1):
        node = rows + pos
        assert np.array_equal(got[node], want[node]), pos
        while node > 1:
            assert np.array_equal(got[node ^ 1], want[node ^ 1]), (pos, node)
            node >>= 1
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[1:], want[1:])
