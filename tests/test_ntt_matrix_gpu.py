"""The transforms of zeth_amd/csrc/ntt.hip over every size, expansion and entry point a `Hal` caller may use, word for word against
the CPU oracle: every `expand_bits` in 0..log_n up to 2^17 and the path switches above it (the generic first pass above 4 bits,
expansion wider than the first pass, replication), every inverse entry point at every log_n in 0..17, edge-valued columns through
each inverse kernel class up to 2^24, the column-count limit, bit reversal around its kernel switch, and the refusals.  One test
ties the conventions (bit-reversed coefficients, n^-1, the coset 3<w>) to the definition by direct summation in plain integers,
which shares no butterfly with either implementation."""
import numpy as np
import pytest

from conftest import P, rand_fp
from test_fuzz_gpu import spicy
from zeth_amd.hal import HalError

pytestmark = pytest.mark.gpu


def mismatch(got, want):
    """None, or the report of test_hal_parity_gpu.eq: count, first indices, both values."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.shape != want.shape:
        return f"shape {got.shape} vs {want.shape}"
    if np.array_equal(got, want):
        return None
    bad = np.flatnonzero(got != want)
    return f"{bad.size} mismatches, first at {bad[:5]}: {got[bad[:5]]} vs {want[bad[:5]]}"


def eq(got, want, what=""):
    m = mismatch(got, want)
    assert m is None, f"{what}: {m}" if what else m


def forward_columns(rng, n_in, edge=True):
    cols = [rand_fp(rng, n_in)] + ([np.full(n_in, P - 1, np.uint32)] if edge else []) + [spicy(rng, n_in)]
    return np.concatenate(cols), len(cols)


def forward_case(hal, oracle, rng, log_n, bits, edge=True):
    """None if the device's expansion by `bits` into 2^log_n equals the oracle's, else what differs (a refusal included)."""
    n_out = 1 << log_n
    x, count = forward_columns(rng, n_out >> bits, edge)
    want = np.zeros(count * n_out, dtype=np.uint32)
    oracle.zko_batch_expand_into_evaluate_ntt(want, want.size, x, x.size, count, bits)
    out = hal.alloc_elem("out", count * n_out)
    try:
        hal.batch_expand_into_evaluate_ntt(out, hal.copy_from("in", x), count, bits)
    except HalError as e:
        return f"refused: {e}"
    return mismatch(out.to_vec(), want)


# ---- 1. forward, small sizes, exhaustive ----
@pytest.mark.parametrize("log_n", range(18))
def test_forward_every_expand_bits(hal, oracle, log_n):
    """Every expand_bits in 0..log_n (log_n included: replication), three columns: uniform, all P-1, runs of 0 and P-1."""
    rng = np.random.default_rng(4100 + log_n)
    failed = {}
    for bits in range(log_n + 1):
        m = forward_case(hal, oracle, rng, log_n, bits)
        if m:
            failed[bits] = m
    assert not failed, f"log_n {log_n}: expand_bits {sorted(failed)} differ from the oracle: " + "; ".join(
        f"expand_bits {b}: {m}" for b, m in failed.items())


# ---- 2. forward, large sizes: where run_transform switches path ----
@pytest.mark.parametrize("log_n,bits", [
    (18, 5), (18, 12), (18, 13), (18, 18),      # generic first pass; last skip inside it; first skip beyond it; replication
    (20, 4), (20, 5),                           # last lazy, first non-lazy
    (20, 13),                                   # skip beyond the first pass
    (21, 5),                                    # generic -> high8 -> top<1>
    (22, 0), (22, 5)])                          # lazy with no expansion; non-lazy
def test_forward_path_switches(hal, oracle, log_n, bits):
    m = forward_case(hal, oracle, np.random.default_rng(4200 + 32 * log_n + bits), log_n, bits, edge=False)
    assert m is None, f"log_n {log_n} expand_bits {bits}: {m}"


# ---- 2b. the kernels launched are the planned ones ----
PLAN_CASES = ([("fwd", log_n, bits) for log_n, bits in ((16, 0), (18, 2), (18, 5), (20, 2), (21, 0), (22, 5))] +
              [("inv", log_n, zk) for log_n in (13, 16, 18, 20, 21, 22) for zk in ("plain", "zk")])


@pytest.mark.parametrize("direction,log_n,arg", PLAN_CASES)
def test_launches_match_the_plan(hal, direction, log_n, arg):
    """One column, profiler on: the scopes the call records are the kernel sequence tests/golden/ntt_plan.json holds for the case
    (the smallest size of each sequence), one launch each — a pass that moved to another kernel would still compute the same words."""
    from test_ntt_plan import kernels_of, load_golden
    n = 1 << log_n
    if direction == "fwd":
        op = "batch_expand_into_evaluate_ntt"
        out, src = hal.alloc_elem("out", n), hal.copy_from("in", np.zeros(n >> arg, np.uint32))
        call = lambda: hal.batch_expand_into_evaluate_ntt(out, src, 1, arg)
    else:
        op = "batch_interpolate_ntt_zk_shift" if arg == "zk" else "batch_interpolate_ntt"
        io = hal.copy_from("io", np.zeros(n, np.uint32))
        call = (lambda: hal.batch_interpolate_ntt_zk_shift(io, 1)) if arg == "zk" else (lambda: hal.batch_interpolate_ntt(io, 1))
    want = {}
    for k in kernels_of(load_golden()[f"{direction} {log_n} {arg}"]):
        want[f"{op}:k_ntt_{k}"] = want.get(f"{op}:k_ntt_{k}", 0) + 1
    hal.prof_enable(True)
    try:
        hal.prof_reset()
        call()
        hal.sync()
        got = {r["name"]: r["calls"] for r in hal.prof_get() if r["calls"]}
    finally:
        hal.prof_enable(False)
    assert got == want


# ---- 3. inverse, every entry point ----
SENTINEL = 0xDEADBEEF       # not a field element: a word of `out` that a transform left behind shows


@pytest.mark.parametrize("log_n", range(18))
def test_inverse_every_entry_point(hal, oracle, log_n):
    rng = np.random.default_rng(4300 + log_n)
    n, count = 1 << log_n, 3
    x = np.concatenate([rand_fp(rng, n), spicy(rng, n), np.full(n, P - 1, np.uint32)])
    want = x.copy()
    oracle.zko_batch_interpolate_ntt(want, want.size, count)
    want_zk = want.copy()
    oracle.zko_zk_shift(want_zk, want_zk.size, count)

    buf = hal.copy_from("io", x)
    hal.batch_interpolate_ntt(buf, count)
    eq(buf.to_vec(), want, "batch_interpolate_ntt")
    hal.zk_shift(buf, count)
    eq(buf.to_vec(), want_zk, "zk_shift")
    buf = hal.copy_from("io", x)
    hal.batch_interpolate_ntt_zk_shift(buf, count)
    eq(buf.to_vec(), want_zk, "batch_interpolate_ntt_zk_shift")
    src = hal.copy_from("in", x)
    for zk, w in ((False, want), (True, want_zk)):
        out = hal.copy_from("out", np.full(x.size, SENTINEL, np.uint32))
        hal.batch_interpolate_ntt_from(out, src, count, zk)
        eq(out.to_vec(), w, f"batch_interpolate_ntt_from(zk_shift={zk})")
        eq(src.to_vec(), x, f"batch_interpolate_ntt_from(zk_shift={zk}) source")
    # round trip: coefficients, then their evaluations on the same domain
    coeffs = hal.copy_from("out", np.full(x.size, SENTINEL, np.uint32))
    hal.batch_interpolate_ntt_from(coeffs, src, count, False)
    back = hal.copy_from("back", np.full(x.size, SENTINEL, np.uint32))
    hal.batch_expand_into_evaluate_ntt(back, coeffs, count, 0)
    eq(back.to_vec(), x, "interpolate_from then evaluate")


# ---- 4. inverse, edge-valued columns, one size per kernel class ----
def edge_column(name, n, rng):
    if name == "random":
        return rand_fp(rng, n)
    x = np.zeros(n, np.uint32)
    if name == "p-1":
        x[:] = P - 1
    elif name == "(p-1)/2":
        x[:] = (P - 1) // 2
    elif name == "(p+1)/2":
        x[:] = (P + 1) // 2
    elif name == "alt0":
        x[1::2] = P - 1
    elif name == "alt1":
        x[0::2] = P - 1
    else:
        x[{"first": 0, "last": n - 1}[name]] = P - 1
    return x


ALL_EDGE = ("p-1", "(p-1)/2", "(p+1)/2", "alt0", "alt1", "first", "last", "random")
# 2^23 and 2^24: the oracle transforms one column per thread and its time is the test's, so these keep the columns the test's time allows
EDGE_COLUMNS = {23: ("alt0", "alt1", "random"), 24: ("alt1", "random")}


@pytest.mark.parametrize("log_n", [12,            # low12 alone
                                   13, 17,        # two generic passes
                                   18,            # low12 + generic
                                   19, 20,        # high8
                                   21,            # top<1>
                                   22,            # high10
                                   23,            # top<3>
                                   24])           # top<4>
def test_inverse_edge_columns(hal, oracle, log_n):
    """The inverse butterfly multiplies the lazy difference x - y + P in (0, 2P): columns that put x - y at both ends of its range
    (0 against P-1 in both phases, constants whose differences vanish, a single non-zero word) through every inverse kernel."""
    rng = np.random.default_rng(4400 + log_n)
    n = 1 << log_n
    names = EDGE_COLUMNS.get(log_n, ALL_EDGE)
    count = len(names)
    x = np.concatenate([edge_column(name, n, rng) for name in names])

    def by_column(got, want):
        if np.array_equal(got, want):
            return []
        return [f"column '{name}': {m}" for c, name in enumerate(names) if (m := mismatch(got[c * n:(c + 1) * n], want[c * n:(c + 1) * n]))]

    want = x.copy()
    oracle.zko_batch_interpolate_ntt(want, want.size, count)
    buf = hal.copy_from("io", x)
    hal.batch_interpolate_ntt(buf, count)
    bad = by_column(buf.to_vec(), want)
    assert not bad, "batch_interpolate_ntt: " + "; ".join(bad)
    oracle.zko_zk_shift(want, want.size, count)
    buf.write(x)
    hal.batch_interpolate_ntt_zk_shift(buf, count)
    bad = by_column(buf.to_vec(), want)
    assert not bad, "batch_interpolate_ntt_zk_shift: " + "; ".join(bad)


# ---- 5. the definition, independent of the oracle's algorithm ----
def bitrev(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2) if bits else 0


def powers(base, n):
    """[base^0 .. base^(n-1)] mod P as uint64"""
    out = np.empty(n, np.uint64)
    acc = 1
    for k in range(n):
        out[k] = acc
        acc = acc * base % P
    return out


def dft(values, root_powers, chunk=256):
    """out[j] = sum_k values[k] * root^(j k) mod P for j < order, term by term; root_powers = powers(root, order), root^order = 1"""
    order, n = len(root_powers), len(values)
    out = np.empty(order, np.uint64)
    k = np.arange(n, dtype=np.uint64)
    for j0 in range(0, order, chunk):
        j = np.arange(j0, min(order, j0 + chunk), dtype=np.uint64)[:, None]
        terms = root_powers[(j * k[None, :]) % np.uint64(order)] * values[None, :] % np.uint64(P)      # each product < P^2 < 2^62
        out[j0:j0 + len(j)] = terms.sum(axis=1) % np.uint64(P)                                          # n P < 2^43
    return out


@pytest.mark.parametrize("log_in", [0, 1, 2, 3, 4, 5, 6, 11])
@pytest.mark.parametrize("bits", [1, 2])
def test_definition_by_direct_summation(hal, oracle, log_in, bits):
    """interpolate (+ zk shift) then expand == the evaluations, on <w_out> (on the coset 3<w_out>), of the one polynomial of degree
    below n that takes the input values on <w_n>: coefficients c_k = n^-1 sum_i v_i w_n^(-i k) and values sum_k c_k x^k, both summed
    term by term in integers mod P.  The coefficients are also compared: bit-reversed order, scaled by n^-1, times 3^k when shifted."""
    rng = np.random.default_rng(4500 + 8 * log_in + bits)
    n, log_out = 1 << log_in, log_in + bits
    n_out = 1 << log_out
    enc = lambda a: np.array([oracle.zko_fp_encode(int(v)) for v in a], np.uint32)
    dec = lambda a: np.array([oracle.zko_fp_decode(int(v)) for v in a], np.uint64)
    w_out = int(oracle.zko_fp_decode(oracle.zko_rou_fwd(log_out)))
    w_n = int(oracle.zko_fp_decode(oracle.zko_rou_fwd(log_in)))
    assert pow(w_out, n_out, P) == 1 and (n_out == 1 or pow(w_out, n_out // 2, P) == P - 1), "w_out is not a primitive 2^log_out-th root"
    assert w_n == pow(w_out, 1 << bits, P), "the smaller domain is not the subgroup of the larger one"
    values = rng.integers(0, P, size=n, dtype=np.uint64)
    values[rng.integers(0, n)] = P - 1
    if n > 2:
        values[rng.integers(0, n)] = 0
    # the polynomial, by the definition
    coeffs = dft(values, powers(pow(w_n, P - 2, P), n)) * np.uint64(pow(n, P - 2, P)) % np.uint64(P)
    rev = np.array([bitrev(i, log_in) for i in range(n)])
    for zk in (False, True):
        c = coeffs * powers(3, n) % np.uint64(P) if zk else coeffs          # p(3 x) has coefficients 3^k c_k
        want = dft(c, powers(w_out, n_out))
        buf = hal.copy_from("io", enc(values))
        (hal.batch_interpolate_ntt_zk_shift if zk else hal.batch_interpolate_ntt)(buf, 1)
        eq(dec(buf.to_vec()), c[rev], f"coefficients (zk_shift={zk})")
        out = hal.copy_from("out", np.full(n_out, SENTINEL, np.uint32))
        hal.batch_expand_into_evaluate_ntt(out, buf, 1, bits)
        eq(dec(out.to_vec()), want, f"evaluations (zk_shift={zk})")


# ---- 6. column count, bit reversal, refusals ----
@pytest.mark.parametrize("log_n", [1, 3])
def test_column_count_limit(hal, oracle, log_n):
    """65535 columns (the grid's y limit) are transformed; 65536 are refused by the transforms and leave their output alone."""
    rng = np.random.default_rng(4600 + log_n)
    n, count = 1 << log_n, 65535
    x = spicy(rng, n * count)
    want = x.copy()
    oracle.zko_batch_interpolate_ntt(want, want.size, count)
    buf = hal.copy_from("io", x)
    hal.batch_interpolate_ntt(buf, count)
    eq(buf.to_vec(), want, "batch_interpolate_ntt")
    big = np.zeros(2 * x.size, np.uint32)
    oracle.zko_batch_expand_into_evaluate_ntt(big, big.size, want, want.size, count, 1)
    out = hal.alloc_elem("out", big.size)
    hal.batch_expand_into_evaluate_ntt(out, buf, count, 1)
    eq(out.to_vec(), big, "batch_expand_into_evaluate_ntt")
    oracle.zko_batch_bit_reverse(want, want.size, count)
    hal.batch_bit_reverse(buf, count)
    eq(buf.to_vec(), want, "batch_bit_reverse")

    count = 65536
    x = rand_fp(rng, n * count)
    io = hal.copy_from("io", x)
    for name, call in (("batch_interpolate_ntt", lambda: hal.batch_interpolate_ntt(io, count)),
                       ("batch_interpolate_ntt_zk_shift", lambda: hal.batch_interpolate_ntt_zk_shift(io, count))):
        with pytest.raises(HalError, match=f"{name}: too many columns"):
            call()
        eq(io.to_vec(), x, f"{name} after its refusal")
    filled = np.full(2 * x.size, SENTINEL, np.uint32)
    out = hal.copy_from("out", filled[:x.size])
    with pytest.raises(HalError, match="batch_interpolate_ntt_from: too many columns"):
        hal.batch_interpolate_ntt_from(out, io, count, True)
    eq(out.to_vec(), filled[:x.size], "batch_interpolate_ntt_from after its refusal")
    out = hal.copy_from("out", filled)
    with pytest.raises(HalError, match="batch_expand_into_evaluate_ntt: too many columns"):
        hal.batch_expand_into_evaluate_ntt(out, io, count, 1)
    eq(out.to_vec(), filled, "batch_expand_into_evaluate_ntt after its refusal")
    # bit reversal has no such limit: above 65535 columns it goes through k_bit_reverse_small
    want = x.copy()
    oracle.zko_batch_bit_reverse(want, want.size, count)
    hal.batch_bit_reverse(io, count)
    eq(io.to_vec(), want, "batch_bit_reverse of 65536 columns")


def test_bit_reverse_65536_long_columns(hal, oracle):
    """2^11 words is the shortest column that k_bit_reverse_tiled takes: with 65536 of them the column count alone must send the
    call to k_bit_reverse_small.  (Bit reversal moves words and never reads them as field elements: the index is the data.)"""
    log_n, count = 11, 65536
    x = np.arange(count << log_n, dtype=np.uint32)
    want = x.copy()
    oracle.zko_batch_bit_reverse(want, want.size, count)
    buf = hal.copy_from("io", x)
    hal.batch_bit_reverse(buf, count)
    eq(buf.to_vec(), want)


@pytest.mark.parametrize("log_n", [0, 10, 11, 12, 13, 14])
def test_bit_reverse_around_the_tiled_kernel(hal, oracle, log_n):
    """2^10 is the last size of k_bit_reverse_small, 2^11 the first of k_bit_reverse_tiled (one tile, its own partner), 2^12..2^14 its
    middle widths 2..4 where tiles swap in pairs."""
    rng = np.random.default_rng(4700 + log_n)
    count = 3
    x = rand_fp(rng, count << log_n)
    want = x.copy()
    oracle.zko_batch_bit_reverse(want, want.size, count)
    buf = hal.copy_from("io", x)
    hal.batch_bit_reverse(buf, count)
    eq(buf.to_vec(), want)
    hal.batch_bit_reverse(buf, count)      # involution
    eq(buf.to_vec(), x, "applied twice")


def refusal_cases(hal):
    """(what is wrong, entry point's name, words of io, words of src, count, call(io, src, count)): `io` is the buffer the call would
    write, `src` the input of the out-of-place calls"""
    interp = [("batch_interpolate_ntt", lambda io, src, count: hal.batch_interpolate_ntt(io, count)),
              ("batch_interpolate_ntt_zk_shift", lambda io, src, count: hal.batch_interpolate_ntt_zk_shift(io, count)),
              ("batch_interpolate_ntt_from", lambda io, src, count: hal.batch_interpolate_ntt_from(io, src, count, True)),
              ("batch_interpolate_ntt_from", lambda io, src, count: hal.batch_interpolate_ntt_from(io, src, count, False)),
              ("zk_shift", lambda io, src, count: hal.zk_shift(io, count)),
              ("batch_bit_reverse", lambda io, src, count: hal.batch_bit_reverse(io, count))]
    cases = []
    for name, call in interp:
        # (out words, in words, count)
        cases += [("not a power of two", name, 24, 24, 2, call),           # columns of 12
                  ("not a power of two", name, 3, 3, 1, call),
                  ("not a multiple of count", name, 16, 16, 3, call),
                  ("count 0", name, 16, 16, 0, call)]
    name = "batch_expand_into_evaluate_ntt"
    expand = lambda bits: (lambda io, src, count: hal.batch_expand_into_evaluate_ntt(io, src, count, bits))
    cases += [("not a power of two", name, 24, 12, 2, expand(1)),          # 6 -> 12
              ("not a multiple of count", name, 16, 8, 3, expand(1)),
              ("input not a multiple of count", name, 16, 7, 2, expand(1)),
              ("count 0", name, 16, 8, 0, expand(1)),
              ("ratio 2 with expand_bits 2", name, 32, 16, 2, expand(2)),
              ("ratio 2 with expand_bits 0", name, 32, 16, 2, expand(0)),
              ("ratio 1 with expand_bits 1", name, 16, 16, 1, expand(1)),
              ("input longer than output", name, 16, 32, 1, expand(1)),
              ("expand_bits above log_n", name, 4, 1, 1, expand(3)),
              ("expand_bits 64", name, 4, 4, 1, expand(64))]
    name = "batch_interpolate_ntt_from"
    for zk in (False, True):
        call = lambda io, src, count, zk=zk: hal.batch_interpolate_ntt_from(io, src, count, zk)
        cases += [("output shorter than input", name, 16, 32, 2, call), ("output longer than input", name, 32, 16, 2, call)]
    return cases


def test_refusals(hal):
    """Every malformed shape raises HalError naming the entry point, and the buffer the call would have written is as it was."""
    rng = np.random.default_rng(4800)
    accepted, wrong = [], []
    for what, name, n_io, n_src, count, call in refusal_cases(hal):
        x = rand_fp(rng, n_io)
        io, src = hal.copy_from("io", x), hal.copy_from("src", rand_fp(rng, n_src))
        try:
            call(io, src, count)
            accepted.append(f"{name} ({what})")
        except HalError as e:
            if f"{name}:" not in str(e):
                wrong.append(f"{name} ({what}): message does not name the entry point: {e}")
        m = mismatch(io.to_vec(), x)
        if m:
            wrong.append(f"{name} ({what}): the output buffer changed: {m}")
    assert not accepted, "accepted instead of refused: " + "; ".join(accepted)
    assert not wrong, "; ".join(wrong)
