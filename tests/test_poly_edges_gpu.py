"""The polynomial-side ops of csrc/poly.hip at the edges of their REAL geometry, bit-exact against the CPU oracle.

  A  batch_evaluate_any / _bitrev over runs of equal `which[]` of every length around the run-leadership limits (EV_MAXP = 5
     points per block, a back-scan of EV_SCAN = 255 entries), up to one run of 4000 entries
  B  evaluation at x = 0, 1, (P-1, P-1, P-1, P-1) of random / all-(P-1) / all-zero columns, natural and bit-reversed; the
     300-coefficient cases also against Horner in Python integers over Fp[x] / (x^4 + 11)
  C  prefix_products and combos_divide at the scan-block edges: a level-0 block is 256 lanes x 8 = 2048 ExtElems, a level-1 block
     2048 x 256 = 2^19, so the third scan level does work only from 2^19 + 1 on
  D  combos_divide_all on every branch: the partial-fraction path with 0 ... 8 points per combo and structured points, the
     round-by-round fallback (more than 8 points, a repeated point)

The expected values come from the oracle's sequential loops (zko_batch_evaluate_any, zko_prefix_products, zko_poly_divide)."""
import numpy as np
import pytest

import hal_only_prover as hop
from conftest import P, rand_fp

pytestmark = pytest.mark.gpu

ONE = hop.enc(1)                    # the Montgomery word of 1
EV_CH = 256 * 64                    # coefficients per block of k_eval_partial
BL0, BL1 = 2048, 1 << 19            # ExtElems per level-0 / level-1 scan block


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
        raise AssertionError(f"{bad.size} mismatches, first at {bad[:5]}: {a.reshape(-1)[bad[:5]]} vs {b.reshape(-1)[bad[:5]]}")


# ---------------------------------------------------------------------------------------------------------------------
# A. evaluation runs
# ---------------------------------------------------------------------------------------------------------------------
RUNS = [5, 6, 255, 256, 257, 259, 260, 261, 300, 600]


def which_of_runs(lengths, main=1, others=(0, 2)):
    """Runs of column `main` of the given lengths, in that order, separated by singletons and short runs of the other columns."""
    seps = [[others[0]], [others[1], others[1]], [others[0], others[1], others[0]], [others[1]], [others[0], others[0], others[0], others[1]]]
    which = []
    for i, run in enumerate(lengths):
        which += [main] * run
        if i + 1 < len(lengths):
            which += seps[i % len(seps)]
    return np.array(which, dtype=np.uint32)


def run_offsets(which):
    """-> (offset of every entry inside its run of equal which[], length of that run)"""
    n = which.size
    starts = np.flatnonzero(np.concatenate([[True], which[1:] != which[:-1]]))
    lens = np.diff(np.concatenate([starts, [n]]))
    run_id = np.repeat(np.arange(starts.size), lens)
    return np.arange(n) - starts[run_id], lens[run_id]


def check_evaluate(hal, oracle, po, count, which, bitrev, seed):
    rng = np.random.default_rng(seed)
    coeffs = rand_fp(rng, count * po)
    xs = rand_fp(rng, 4 * which.size)
    want = np.zeros(4 * which.size, np.uint32)
    oracle.zko_batch_evaluate_any(coeffs, coeffs.size, count, which, xs, which.size, want)
    dev = coeffs.copy()
    if bitrev:
        oracle.zko_batch_bit_reverse(dev, dev.size, count)       # the layout batch_interpolate_ntt leaves behind
    out = hal.alloc_extelem("out", which.size)
    fn = hal.batch_evaluate_any_bitrev if bitrev else hal.batch_evaluate_any
    fn(hal.copy_from("c", dev), count, hal.copy_from("w", which), hal.copy_from("x", xs), out)
    got = out.to_vec()
    bad = np.flatnonzero((got.reshape(-1, 4) != want.reshape(-1, 4)).any(axis=1))
    if bad.size:
        off, length = run_offsets(which)
        k = int(bad[0])
        raise AssertionError(f"{bad.size} of {which.size} entries wrong; first: entry {k} (column {which[k]}), offset {off[k]} inside its run of "
                             f"{length[k]}; offsets of the wrong entries inside their runs: {sorted(set(off[bad].tolist()))[:12]} ...")


@pytest.mark.parametrize("long_run", ["first", "last"])
@pytest.mark.parametrize("po,bitrev", [(300, False), (EV_CH + 1, False), (1 << 14, True), (1 << 15, True)])
def test_evaluate_runs_around_the_leadership_limits(hal, oracle, po, bitrev, long_run):
    """Runs of 5 ... 600 entries on one column.  Every (entry, chunk) partial sum has to be written by some block: entries from
    offset 260 of a run on had no leader when the back-scan stopped after 256 entries (256 % 5 != 0).  Longest run first: the
    back-scan arrives at entry 0; longest run last: the run ends with the array."""
    which = which_of_runs(RUNS[::-1] if long_run == "first" else RUNS)
    assert which[0] == 1 and which[-1] == 1 and which.size < 65536
    check_evaluate(hal, oracle, po, 3, which, bitrev, seed=po + (long_run == "first"))


@pytest.mark.parametrize("po,bitrev", [(300, False), (1 << 14, True)])
def test_evaluate_one_run_of_4000(hal, oracle, po, bitrev):
    check_evaluate(hal, oracle, po, 3, np.full(4000, 2, dtype=np.uint32), bitrev, seed=4000 + po)


# ---------------------------------------------------------------------------------------------------------------------
# B. evaluation points with structure
# ---------------------------------------------------------------------------------------------------------------------
def horner(col_words, x_words):
    """The polynomial with Montgomery coefficient words col_words at the Fp4 point x_words, in Python integers."""
    x, tot = tuple(hop.dec(w) for w in x_words), (0, 0, 0, 0)
    for w in col_words[::-1]:
        tot = hop.e_add(hop.e_mul(tot, x), (hop.dec(w), 0, 0, 0))
    return hop.e_words(tot)


@pytest.mark.parametrize("po,bitrev", [(300, False), (EV_CH + 1, False), (1 << 14, True), (1 << 15, True)])
def test_evaluate_at_zero_one_and_minus_one(hal, oracle, po, bitrev):
    """x = 0 gives coefficient 0 (position 0 in both layouts), x = 1 the sum of the coefficients; columns: random, every word P-1,
    zero.  Each column is evaluated at the four points as one run, and once more point by point with the columns interleaved."""
    rng = np.random.default_rng(po)
    coeffs = np.concatenate([rand_fp(rng, po), np.full(po, P - 1, np.uint32), np.zeros(po, np.uint32)])
    points = [[0, 0, 0, 0], [ONE, 0, 0, 0], [P - 1] * 4, list(rand_fp(rng, 4))]
    which = np.array([c for c in range(3) for _ in points] + [c for _ in points for c in range(3)], dtype=np.uint32)
    xs = np.array([points[p] for _ in range(3) for p in range(4)] + [points[p] for p in range(4) for _ in range(3)], dtype=np.uint32).reshape(-1)
    want = np.zeros(4 * which.size, np.uint32)
    oracle.zko_batch_evaluate_any(coeffs, coeffs.size, 3, which, xs, which.size, want)
    for k in range(which.size):                                                   # x = 0: the constant coefficient itself
        if not xs[4 * k: 4 * k + 4].any():
            assert list(want[4 * k: 4 * k + 4]) == [coeffs[which[k] * po], 0, 0, 0]
    if po <= 300:
        pure = np.array([horner(coeffs[c * po: (c + 1) * po], xs[4 * k: 4 * k + 4]) for k, c in enumerate(which)], dtype=np.uint32).reshape(-1)
        eq(want, pure)                                                            # the oracle agrees with plain integer arithmetic
    dev = coeffs.copy()
    if bitrev:
        oracle.zko_batch_bit_reverse(dev, dev.size, 3)
    out = hal.alloc_extelem("out", which.size)
    fn = hal.batch_evaluate_any_bitrev if bitrev else hal.batch_evaluate_any
    fn(hal.copy_from("c", dev), 3, hal.copy_from("w", which), hal.copy_from("x", xs), out)
    eq(out.to_vec(), want)


# ---------------------------------------------------------------------------------------------------------------------
# C. scan geometry
# ---------------------------------------------------------------------------------------------------------------------
SCAN_N = [2047, 2048, 2049, 4097, BL1 - 1, BL1, BL1 + 1, BL1 + 2049, (1 << 20) + 1]


def ext_ones(n):
    x = np.zeros(4 * n, np.uint32)
    x[0::4] = ONE
    return x


def check_prefix_products(hal, oracle, x):
    want = x.copy()
    oracle.zko_prefix_products(want, x.size // 4)
    buf = hal.copy_from("io", x)
    hal.prefix_products(buf)
    got = buf.to_vec()
    eq(got, want)
    return got


@pytest.mark.parametrize("fill", ["random", "all_p_minus_1", "ones_but_one"])
@pytest.mark.parametrize("n", SCAN_N)
def test_prefix_products_at_the_scan_block_edges(hal, oracle, n, fill):
    rng = np.random.default_rng(n)
    if fill == "random":
        x = rand_fp(rng, 4 * n)
    elif fill == "all_p_minus_1":
        x = np.full(4 * n, P - 1, np.uint32)
    else:                                                       # the one factor that is not 1 has to reach every later position unchanged
        x = ext_ones(n)
        at = n // 3
        x[4 * at: 4 * at + 4] = rand_fp(rng, 4)
    got = check_prefix_products(hal, oracle, x)
    if fill == "ones_but_one":
        eq(got[:4 * at], x[:4 * at])
        eq(got[4 * at:].reshape(-1, 4), np.broadcast_to(x[4 * at: 4 * at + 4], (n - at, 4)))


@pytest.mark.parametrize("n", SCAN_N)
def test_prefix_products_with_a_zero_inside(hal, oracle, n):
    """A zero ExtElem at the first position, at the first element of the second level-0 block (where n reaches it) and at the last
    position: everything from the zero on is zero, everything before it is the running product of the undisturbed input."""
    rng = np.random.default_rng(n + 1)
    x = rand_fp(rng, 4 * n)
    clean = x.copy()
    oracle.zko_prefix_products(clean, n)
    for pos in sorted({0, BL0, n - 1}):
        if pos >= n:
            continue
        z = x.copy()
        z[4 * pos: 4 * pos + 4] = 0
        got = check_prefix_products(hal, oracle, z)
        assert not got[4 * pos:].any(), f"zero at {pos}: non-zero products behind it"
        eq(got[:4 * pos], clean[:4 * pos])


def check_divide_by_two_points(hal, oracle, poly, pts):
    """One polynomial, in the middle of a three-combo buffer, divided by two points in turn: quotient, both remainders, neighbours."""
    cycles = poly.size // 4
    rng = np.random.default_rng(cycles)
    combos = np.concatenate([rand_fp(rng, 4 * cycles), poly, rand_fp(rng, 4 * cycles)])
    want, rems = combos.copy(), []
    q = poly.copy()
    for k in range(2):
        rem = np.zeros(4, np.uint32)
        oracle.zko_poly_divide(q, cycles, pts[4 * k: 4 * k + 4].copy(), rem)
        rems.append(rem)
    want[4 * cycles: 8 * cycles] = q
    buf = hal.copy_from("c", combos)
    rem_out = hal.alloc_extelem("r", 2)
    hal.combos_divide(buf, 1, cycles, pts, rem_out)
    eq(buf.to_vec(), want)
    eq(rem_out.to_vec(), np.concatenate(rems))


@pytest.mark.parametrize("fill", ["random", "all_p_minus_1"])
@pytest.mark.parametrize("n", SCAN_N)
def test_combos_divide_at_the_scan_block_edges(hal, oracle, n, fill):
    rng = np.random.default_rng(3 * n)
    poly = rand_fp(rng, 4 * n) if fill == "random" else np.full(4 * n, P - 1, np.uint32)
    check_divide_by_two_points(hal, oracle, poly, rand_fp(rng, 8))


@pytest.mark.parametrize("n", [BL0 + 1, BL1 + 2049])
def test_combos_divide_by_zero_and_one(hal, oracle, n):
    """z = 0: every scan weight is zero, the quotient is the polynomial shifted down and the remainder its constant term; z = 1:
    every weight is one, the quotient holds the suffix sums."""
    rng = np.random.default_rng(5 * n)
    poly = rand_fp(rng, 4 * n)
    check_divide_by_two_points(hal, oracle, poly, np.array([0, 0, 0, 0, ONE, 0, 0, 0], dtype=np.uint32))
    check_divide_by_two_points(hal, oracle, poly, np.array([ONE, 0, 0, 0, 0, 0, 0, 0], dtype=np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# D. combos_divide_all, every branch
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL = 0xDEADBEEF
DIVIDE_ALL_CYCLES = [64, 2049, 1 << 13]


def check_divide_all(hal, oracle, cycles, point_lists, seed):
    """combos_divide_all over len(point_lists) combos (one more polynomial lies behind them in the buffer) against dividing each
    polynomial by its points one after the other; combos without points, the polynomial behind and the remainder slot behind the
    last remainder have to come back bit-identical."""
    rng = np.random.default_rng(seed)
    n_combos, counts = len(point_lists), [len(p) for p in point_lists]
    combos = rand_fp(rng, 4 * cycles * (n_combos + 1))
    begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    n_pairs = int(begin[-1])
    pts = np.array([w for pl in point_lists for pt in pl for w in pt], dtype=np.uint32)
    if not n_pairs:
        pts = np.zeros(4, np.uint32)                              # never read: a host array of one unused point
    want, want_rem = combos.copy(), np.full(4 * (n_pairs + 1), SENTINEL, np.uint32)
    for i in range(n_combos):
        poly = want[4 * cycles * i: 4 * cycles * (i + 1)]
        for k in range(counts[i]):
            j = int(begin[i]) + k
            rem = np.zeros(4, np.uint32)
            oracle.zko_poly_divide(poly, cycles, pts[4 * j: 4 * j + 4].copy(), rem)
            want_rem[4 * j: 4 * j + 4] = rem
    dev = hal.copy_from("combos", combos)
    rem_out = hal.copy_from("rem", np.full(4 * (n_pairs + 1), SENTINEL, np.uint32))
    hal.combos_divide_all(dev, cycles, pts, begin, rem_out)
    hal.sync()
    got = dev.to_vec()
    for i in list(np.flatnonzero(np.array(counts) == 0)) + [n_combos]:
        sl = slice(4 * cycles * i, 4 * cycles * (i + 1))
        assert np.array_equal(got[sl], combos[sl]), f"polynomial {i} has no division points and was changed"
    for i in range(n_combos):
        sl = slice(4 * cycles * i, 4 * cycles * (i + 1))
        assert np.array_equal(got[sl], want[sl]), f"combo {i} ({counts[i]} points): wrong quotient"
    eq(rem_out.to_vec(), want_rem)


def rand_points(rng, count):
    return [list(rand_fp(rng, 4)) for _ in range(count)]


def points_along(rng, base, comp, count):
    """`count` distinct points that differ from `base` (the first of them) in component `comp` only."""
    deltas = [0] + [int(d) for d in rng.choice(np.arange(1, 1 << 20), size=count - 1, replace=False)]
    out = []
    for d in deltas:
        pt = [int(w) for w in base]
        pt[comp] = (pt[comp] + d * 1999) % P
        out.append(pt)
    return out


@pytest.mark.parametrize("cycles", DIVIDE_ALL_CYCLES)
def test_divide_all_fast_path_random_points(hal, oracle, cycles):
    """0 ... 8 points per combo: 8 is the capacity of the divided-difference table, 0 leaves the polynomial alone."""
    rng = np.random.default_rng(cycles)
    check_divide_all(hal, oracle, cycles, [rand_points(rng, c) for c in [1, 8, 7, 0, 2, 8, 0, 1]], seed=cycles + 1)


@pytest.mark.parametrize("cycles", DIVIDE_ALL_CYCLES)
def test_divide_all_fast_path_structured_points(hal, oracle, cycles):
    """The same counts with points whose differences are a base-field element or a pure x, x^2, x^3 term (one combo each: the
    inverse's norm tower then sees b2 = 0 or b0 = 0), a combo that starts with the point 0 and two that hold the point 1."""
    rng = np.random.default_rng(cycles + 7)
    zero, one = [0, 0, 0, 0], [ONE, 0, 0, 0]
    lists = [[zero],
             points_along(rng, rand_fp(rng, 4), 0, 8),
             points_along(rng, rand_fp(rng, 4), 1, 7),
             [],
             points_along(rng, zero, 2, 2),
             points_along(rng, one, 3, 8),
             [],
             [one]]
    assert [len(p) for p in lists] == [1, 8, 7, 0, 2, 8, 0, 1]
    check_divide_all(hal, oracle, cycles, lists, seed=cycles + 2)


@pytest.mark.parametrize("cycles", DIVIDE_ALL_CYCLES)
def test_divide_all_fast_path_no_points_first_and_last(hal, oracle, cycles):
    rng = np.random.default_rng(cycles + 11)
    check_divide_all(hal, oracle, cycles, [rand_points(rng, c) for c in [0, 3, 1, 5, 2, 4, 1, 0]], seed=cycles + 3)


@pytest.mark.parametrize("cycles", DIVIDE_ALL_CYCLES)
def test_divide_all_without_any_point_is_a_no_op(hal, oracle, cycles):
    check_divide_all(hal, oracle, cycles, [[] for _ in range(8)], seed=cycles + 4)


@pytest.mark.parametrize("case", ["nine_points", "repeated_point", "both"])
@pytest.mark.parametrize("cycles", DIVIDE_ALL_CYCLES)
def test_divide_all_fallback_rounds(hal, oracle, cycles, case):
    """More than 8 points in a combo, or a point twice in one combo (dividing twice by the same z is well defined one division
    after the other, the partial fractions are not), send the call to one set of launches per division step."""
    rng = np.random.default_rng(cycles + 13)
    lists = [rand_points(rng, c) for c in [2, 0, 5, 1, 3, 0, 8, 1, 2]]
    nine = rand_points(rng, 9)
    twice = rand_points(rng, 3)
    twice = [twice[0], twice[1], twice[0], twice[2]]
    if case == "nine_points":
        lists[3] = nine
    elif case == "repeated_point":
        lists[3] = twice
    else:
        lists[0], lists[3], lists[8] = twice, nine + [nine[4]], twice[:3]
    check_divide_all(hal, oracle, cycles, lists, seed=cycles + 5)
