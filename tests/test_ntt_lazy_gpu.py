"""The lazy forward NTT (pairs of layers with one reduction per pair: zeth_amd/csrc/ntt_lazy.h) on the shapes that run it,
2^18 -> 2^20 and 2^20 -> 2^22, and on odd expand_bits (a single layer in front of the pairs), with columns whose intermediates
sit at the edges of the signed representation.  Word for word against the CPU oracle AND against the non-lazy kernels: the
transform of twice the size with one more expand bit (2^21 / 2^23: canonical butterflies + k_ntt_top) evaluates the same
polynomial on a domain whose even points are this one's."""
import numpy as np
import pytest

from conftest import P, rand_fp

pytestmark = pytest.mark.gpu


def edge_columns(n_in, seed):
    rng = np.random.default_rng(seed)
    i = np.arange(n_in)
    return [np.full(n_in, P - 1, np.uint32), np.full(n_in, (P - 1) // 2, np.uint32), np.full(n_in, (P + 1) // 2, np.uint32),
            np.where(i % 2 == 0, 0, P - 1).astype(np.uint32), np.where(i % 2 == 0, P - 1, 0).astype(np.uint32),
            rand_fp(rng, n_in)]


def first_mismatch(a, b):
    bad = np.flatnonzero(a != b)
    return None if bad.size == 0 else f"{bad.size} mismatches, first at {bad[:5]}: {a[bad[:5]]} vs {b[bad[:5]]}"


@pytest.mark.parametrize("log_n,bits", [(20, 2), (22, 2), (20, 1), (20, 3), (22, 3)])
def test_lazy_expand_ntt_edge_columns(hal, oracle, log_n, bits):
    n_out = 1 << log_n
    n_in = n_out >> bits
    cols = edge_columns(n_in, log_n * 10 + bits)
    count = len(cols)
    x = np.concatenate(cols)
    src = hal.copy_from("in", x)
    out = hal.alloc_elem("out", count * n_out)
    hal.batch_expand_into_evaluate_ntt(out, src, count, bits)
    got = out.to_vec()
    # the non-lazy kernels: twice the domain, every second point
    wide = hal.alloc_elem("wide", count * 2 * n_out)
    hal.batch_expand_into_evaluate_ntt(wide, src, count, bits + 1)
    ref = wide.to_vec().reshape(count, 2 * n_out)[:, ::2].reshape(-1)
    assert got.max() < P
    assert first_mismatch(got, ref) is None, "lazy vs non-lazy kernels: " + first_mismatch(got, ref)
    want = np.zeros(count * n_out, dtype=np.uint32)
    oracle.zko_batch_expand_into_evaluate_ntt(want, want.size, x, x.size, count, bits)
    assert first_mismatch(got, want) is None, "lazy vs oracle: " + first_mismatch(got, want)
