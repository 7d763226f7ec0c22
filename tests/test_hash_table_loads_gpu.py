"""k_hash_rows and k_hash_fold request their table data (A fragments, beta rows, full-round constant rows) ahead of its use and
address a leaf as (the workgroup's first row) + (a 32-bit lane offset): bit-exact against the oracle at the shapes where that
can go wrong.  Rows at the workgroup borders (255, 256, 511, 513: the last workgroup's clamped lanes re-hash its last row, and
anything held per workgroup must be right in every one); columns that are tail-only (15), two full blocks (32) and two full
blocks plus a tail (33), so that a request made in one block of the sponge is read in the next; and two different matrices
hashed back to back on one context, so that nothing requested for the first leaks into the second.  Fills as the callers' test."""
import numpy as np
import pytest

from test_poseidon2_callers_gpu import FILLS, fill

pytestmark = pytest.mark.gpu
P = 2013265921
ROWS = (255, 256, 511, 513)
COLS = (15, 32, 33)


def want_rows(oracle, mat, rows, cols):
    want = np.zeros(rows * 8, dtype=np.uint32)
    oracle.zko_hash_rows(want, rows, np.ascontiguousarray(mat), rows * cols)
    return want


@pytest.mark.parametrize("rows", ROWS)
def test_hash_rows_at_workgroup_borders_equals_oracle(hal, oracle, rows):
    rng = np.random.default_rng(3300 + rows)
    for cols in COLS:
        for kind in FILLS:
            mat = fill(kind, rows * cols, rng)
            out = hal.alloc_digest("leaves", rows)
            hal.hash_rows(out, hal.copy_from("m", mat))
            got = out.to_vec()
            assert got.max() < P, (rows, cols, kind)
            assert np.array_equal(got, want_rows(oracle, mat, rows, cols)), (rows, cols, kind)


@pytest.mark.parametrize("parents", ROWS)
def test_hash_fold_at_workgroup_borders_equals_oracle(hal, oracle, parents):
    rng = np.random.default_rng(3400 + parents)
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


def test_two_matrices_back_to_back_on_one_context(hal, oracle):
    """Different shapes and different words, both launches queued before either result is read; then the first again."""
    rng = np.random.default_rng(3500)
    shapes = ((513, 33), (255, 15))
    mats = [fill(kind, r * c, rng) for kind, (r, c) in zip(("random", "alternating (P+-1)/2"), shapes)]
    dev = [hal.copy_from(f"m{i}", m) for i, m in enumerate(mats)]
    outs = [hal.alloc_digest(f"leaves{i}", r) for i, (r, _) in enumerate(shapes)]
    again = hal.alloc_digest("again", shapes[0][0])
    hal.hash_rows(outs[0], dev[0])
    hal.hash_rows(outs[1], dev[1])
    hal.hash_rows(again, dev[0])
    want = [want_rows(oracle, m, r, c) for m, (r, c) in zip(mats, shapes)]
    assert not np.array_equal(want[0][:8], want[1][:8])
    assert np.array_equal(outs[0].to_vec(), want[0])
    assert np.array_equal(outs[1].to_vec(), want[1])
    assert np.array_equal(again.to_vec(), want[0])
