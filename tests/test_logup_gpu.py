"""The built-in accumulate for arguments described as data (zkh_accumulate, csrc/accumulate.hip) on the GPU: bit for bit against the host
reference over a grid of argument shapes, SYN-LOOKUP's accum at po2 20 against the oracle's constraint check, seals through
prove_begin -> zkh_accumulate -> prove_finish accepted by both verifiers, the generated eval_check against the interpreter, the session
dispatch, and the refusals of a bad witness."""
import ctypes as C

import numpy as np
import pytest

from args_gpu import seal_host as _seal_host
import zko
from conftest import rand_fp
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.circuits.desc import GROUP_ACCUM, GROUP_CODE, GROUP_DATA
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu
P = 2013265921
NOISE = 0x10C0


def _noise_fn(seed):
    key = zhal.noise_key(seed)
    kp = key.ctypes.data_as(C.POINTER(C.c_uint32))
    lib = zhal.load_library()
    f = lib.zkh_noise_cell_host
    f.restype, f.argtypes = C.c_uint32, [C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32]

    def noise(po2, zk):
        n = 1 << po2
        return lambda col: np.array([f(kp, GROUP_ACCUM, col, r) for r in range(n - zk, n)], dtype=np.uint32)
    return noise


def _random_arguments(seed, k, wc=6, wd=10):
    """k accum columns of 1..3 terms (tuple widths 1..4, signs, selectors, code / data / constant multiplicities, tags) whose bus
    balances by construction: every term has a mirror of opposite sign in another column"""
    rng = np.random.default_rng(seed)
    sizes = [int(x) for x in rng.integers(1, 4, size=k)]
    while sum(sizes) % 2:
        sizes[int(rng.integers(0, k))] = 2
    slots = [c for c, s in enumerate(sizes) for _ in range(s)]
    rng.shuffle(slots)
    b = logup.LogupBuilder((4 * k, wc, wd), (4, 12), alpha=int(rng.integers(0, 9)), beta=int(rng.integers(0, 9)))
    for i in range(0, len(slots), 2):
        w = int(rng.integers(1, 5))
        tup = [(GROUP_CODE, int(rng.integers(0, wc))) if rng.random() < 0.3 else (GROUP_DATA, int(rng.integers(0, wd))) for _ in range(w)]
        sel = int(rng.integers(0, wc)) if rng.random() < 0.5 else None
        r = rng.random()
        mult = (GROUP_DATA, int(rng.integers(0, wd))) if r < 0.4 else (GROUP_CODE, int(rng.integers(0, wc))) if r < 0.6 else None
        tag = int(rng.integers(0, 4))
        sign = 1 if rng.random() < 0.5 else -1
        b.term(slots[i], tup, sign=sign, sel=sel, mult=mult, tag=tag)
        b.term(slots[i + 1], tup, sign=-sign, sel=sel, mult=mult, tag=tag)
    chain = b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 1), b.get(GROUP_CODE, 2))
    return b.finish_all(chain)


def _traces(rng, wc, wd, n):
    code, data = rand_fp(rng, wc * n), rand_fp(rng, wd * n)
    for a in (code, data):                       # the extreme operands
        a[::97] = 0
        a[5::89] = P - 1
    return code, data


GRID = [(8, 37, 3), (9, 100, 5), (10, 11, 2), (11, 1994 - 1024, 7), (12, 1994, 4), (13, 1994, 9), (14, 1994, 12), (14, 3, 6)]


@pytest.mark.parametrize("po2,zk,k", GRID)
def test_accumulate_bit_exact_vs_reference(hal, po2, zk, k):
    desc, blob = _random_arguments(po2 * 100 + k, k)
    c = hal.load_circuit(desc, jit=False)
    c.set_arguments(blob)
    assert c.has_arguments()
    args = logup.Arguments.parse(blob)
    n = 1 << po2
    rng = np.random.default_rng(po2 + 17 * k)
    code, data = _traces(rng, 6, 10, n)
    mix = rand_fp(rng, 12)
    want, total = logup.reference_accumulate(args, po2, zk, code, data, mix, noise=_noise_fn(NOISE)(po2, zk))
    assert total == [0, 0, 0, 0]
    dcode, ddata = hal.alloc_elem("code", code.size), hal.alloc_elem("data", data.size)
    dcode.write(code)
    ddata.write(data)
    acc = hal.alloc_elem("accum", 4 * k * n)
    hal.accumulate(c, po2, zk, NOISE, dcode, ddata, mix, acc)
    got = acc.to_vec()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} words differ, first at column {bad[0] // n}, row {bad[0] % n} (A = {n - zk})"


def test_set_arguments_validates_against_the_circuit(hal):
    desc, blob = syn_lookup.syn_lookup_tiny()
    c = hal.load_circuit(desc, jit=False)
    assert not c.has_arguments()
    for word, value, msg in [(2, 3, "accum group"), (3, 6, "mix words"), (8, 9, "accum column"), (8 + 6, 5, "tuple width"),
                             (8 + 9, 99, "tuple column"), (8 + 2, 50, "selector")]:
        bad = blob.copy()
        bad[word] = value
        with pytest.raises(HalError, match=msg):
            c.set_arguments(bad)
    assert not c.has_arguments()
    with pytest.raises(HalError, match="ZKA1"):
        c.set_arguments(blob[:5])
    c.set_arguments(blob)
    assert c.has_arguments()
    c.set_arguments(None)
    assert not c.has_arguments()


def test_refusals_of_a_bad_witness(hal):
    po2, zk = 10, 200
    desc, blob = syn_lookup.syn_lookup_tiny()
    c = hal.load_circuit(desc, jit=False)
    c.set_arguments(blob)
    code, data, out = syn_lookup.witness(syn_lookup.TINY, po2, zk, seed=7)
    dcode = hal.alloc_elem("code", code.size)
    dcode.write(code)
    ddata = hal.alloc_elem("data", data.size)
    acc = hal.alloc_elem("accum", 16 << po2)
    rng = np.random.default_rng(3)
    mix = rand_fp(rng, 8)
    bad = syn_lookup.corrupt_limb(syn_lookup.TINY, data, po2, row=123, word=1)
    ddata.write(bad)
    _, total = logup.reference_accumulate(logup.Arguments.parse(blob), po2, zk, code, bad, mix, check_balance=False)
    with pytest.raises(HalError, match=r"does not balance: total \(%d, %d, %d, %d\)" % tuple(total)):
        hal.accumulate(c, po2, zk, NOISE, dcode, ddata, mix, acc)
    assert not acc.to_vec().any()                                            # no accum is left behind
    ddata.write(data)
    hal.accumulate(c, po2, zk, NOISE, dcode, ddata, mix, acc)                # the honest witness is accepted
    mix[4:8] = [(1 << 32) % P, 0, 0, 0]                                      # beta = 1, alpha = limb 0 of word 0 on row 0
    mix[0:4] = [data.reshape(-1, 1 << po2)[2, 0], 0, 0, 0]
    with pytest.raises(HalError, match="denominator vanishes at row 0, accum column 0"):
        hal.accumulate(c, po2, zk, NOISE, dcode, ddata, mix, acc)


def test_unbalanced_witness_is_not_sealed(hal):
    po2 = 12
    desc, blob = syn_lookup.syn_lookup_tiny()
    prover = SegmentProver(hal, desc, arguments=blob)
    seg = Segment(index=0, po2=po2, noise_seed=NOISE)
    code, data, out = syn_lookup.witness(syn_lookup.TINY, po2, seg.zk_cycles, seed=1)
    bad = syn_lookup.corrupt_limb(syn_lookup.TINY, data, po2, row=5)
    with pytest.raises(HalError, match=r"does not balance: total \("):
        _seal_host(hal, prover, seg, code, bad, out)


@pytest.mark.parametrize("shape,po2", [(syn_lookup.TINY, 12), (syn_lookup.FULL, 20)])
def test_seal_through_accumulate_is_accepted_by_both_verifiers(hal, oracle, shape, po2):
    desc, blob = syn_lookup.build_syn_lookup(shape)
    prover = SegmentProver(hal, desc, arguments=blob)
    seg = Segment(index=0, po2=po2, noise_seed=NOISE)
    code, data, out = syn_lookup.witness(shape, po2, seg.zk_cycles, seed=po2)
    receipt = _seal_host(hal, prover, seg, code, data, out)
    dcode = hal.alloc_elem("code", code.size)
    dcode.write(code)
    root = prover.code_root(dcode, po2)
    oc = zko.OracleCircuit(oracle, desc)
    assert np.array_equal(root, oc.root_of_code(po2, code))
    receipt.verify(desc, root)                                               # zkh_verify_segment
    assert oc.verify(receipt.seal, root) is None                             # the oracle's verifier
    other = root.copy()
    other[0] ^= 1
    assert oc.verify(receipt.seal, other) is not None                        # ... under its own control root only


def test_syn_lookup_accum_at_po2_20_satisfies_the_oracle(hal, oracle):
    po2, zk = 20, zhal.ZK_CYCLES
    desc, blob = syn_lookup.syn_lookup()
    c = hal.load_circuit(desc, jit=False)
    c.set_arguments(blob)
    code, data, out = syn_lookup.witness(syn_lookup.FULL, po2, zk, seed=20)
    dcode, ddata = hal.alloc_elem("code", code.size), hal.alloc_elem("data", data.size)
    dcode.write(code)
    ddata.write(data)
    mix = rand_fp(np.random.default_rng(20), 8)
    acc = hal.alloc_elem("accum", int(desc[3]) << po2)
    hal.accumulate(c, po2, zk, NOISE, dcode, ddata, mix, acc)               # succeeds only with a zero bus total
    accum = acc.to_vec()
    A = (1 << po2) - zk
    tot = accum.reshape(-1, 1 << po2)[:, A - 1].reshape(-1, 4).astype(np.uint64).sum(axis=0) % P
    assert not tot.any()
    assert zko.OracleCircuit(oracle, desc).check_rows(po2, accum, code, data, out, mix) == -1


def test_generated_eval_check_equals_interpreter_on_syn_lookup(hal):
    po2 = 10
    n4 = 4 << po2
    desc, _ = syn_lookup.syn_lookup_tiny()
    jit = hal.load_circuit(desc, jit=True)
    assert jit.kernel_kind() == "attached"
    interp = hal.load_circuit(desc, jit=False)
    rng = np.random.default_rng(10)
    groups = []
    for w in (int(desc[3]), int(desc[4]), int(desc[5])):
        b = hal.alloc_elem("g", w * n4)
        b.write(rand_fp(rng, w * n4))
        groups.append(b)
    out, mix = hal.alloc_elem("out", 4), hal.alloc_elem("mix", 8)
    out.write(rand_fp(rng, 4))
    mix.write(rand_fp(rng, 8))
    pm = rand_fp(rng, 4)
    checks = []
    for c, use_interp in ((jit, False), (interp, True)):
        chk = hal.alloc_elem("check", 4 * n4)
        c.eval_check(chk, groups, [out, mix], pm, po2, use_interpreter=use_interp)
        checks.append(chk.to_vec())
    assert np.array_equal(checks[0], checks[1])


def test_session_with_caller_traces_uses_accumulate_or_the_callback(hal, oracle):
    from zeth_amd.host import Session
    po2 = 12
    desc, blob = syn_lookup.syn_lookup_tiny()
    args = logup.Arguments.parse(blob)
    segs = [Segment(index=i, po2=po2, noise_seed=NOISE + i) for i in range(2)]
    traces = [syn_lookup.witness(syn_lookup.TINY, po2, s.zk_cycles, seed=30 + i) for i, s in enumerate(segs)]
    oc = zko.OracleCircuit(oracle, desc)
    sess = Session(desc, lanes_per_device=1)
    with pytest.raises(HalError, match="no arguments and no accumulate callback"):
        sess.prove(segs[:1], host_traces=traces[:1])
    sess.set_arguments(blob)
    comp, _, _ = sess.prove(segs, host_traces=traces, verify=True)
    prover = SegmentProver(hal, desc, arguments=blob)
    for seg, (code, data, out), r in zip(segs, traces, comp.segments):
        root = oc.root_of_code(po2, code)
        assert oc.verify(r.seal, root) is None
        assert np.array_equal(r.seal, _seal_host(hal, prover, seg, code, data, out).seal)      # same traces, same noise: same seal
    # a callback still wins over the arguments
    calls = []
    lib = zhal.load_library()
    by_data = {}
    FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p)

    def cb(user, ctx, cir, p2, data_buf, mix_p, accum_buf):
        n = 1 << p2
        host = np.empty(int(desc[5]) * n, np.uint32)
        lib.zkh_read(ctx, data_buf, host.ctypes.data_as(C.POINTER(C.c_uint32)), 0, host.size)
        code = by_data[host.tobytes()]
        mix = np.ctypeslib.as_array(mix_p, shape=(8,)).copy()
        acc, _ = logup.reference_accumulate(args, p2, zhal.ZK_CYCLES, code, host, mix)
        calls.append(p2)
        lib.zkh_write(ctx, accum_buf, acc.ctypes.data_as(C.POINTER(C.c_uint32)), 0, acc.size)
        return None
    for code, data, _ in traces:
        by_data[np.ascontiguousarray(data, dtype=np.uint32).tobytes()] = code
    fn = FN(cb)
    lib.zkh_session_set_accumulate(sess.h, C.cast(fn, C.c_void_p), None)
    comp2, _, _ = sess.prove(segs, host_traces=traces, verify=True)
    assert calls == [po2, po2]
    for (code, _, _), r in zip(traces, comp2.segments):
        assert oc.verify(r.seal, oc.root_of_code(po2, code)) is None
    lib.zkh_session_set_accumulate(sess.h, None, None)
    sess.close()
