"""The claim rules of the session executor (zeth_amd/csrc/claims.h) as a unit: plain C++, driven without a GPU by
tests/cpp/claims_test.cpp.  Part A (structure, a toy hash) is checked inside the program: the fold shape against scheduler.h's
plan, the union order, parent's refusal, the P2-JOIN pair fold, membership paths, the layout of every node witness.  Part B
(values, the real hash_pair): the program prints the claims of fixed inputs and they are compared HERE, word for word, with the
independent twin zeth_amd/recursion.py — the expected values come from the Python side only."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2013265921


def stream(seed):
    """the input words both sides generate (claims_test.cpp Stream)"""
    x = seed
    while True:
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        yield x % P


def take(gen, k):
    return np.array([next(gen) for _ in range(k)], dtype=np.uint32)


def leaves_of(n):
    st = stream(100 + n)
    out, state = [], int(next(st))
    for _ in range(n):
        core = take(st, 8)
        pre, state = state, int(next(st))
        out.append((core, pre, state))
    return out


def assumed_of(m):
    st = stream(200 + m)
    return [take(st, 8) for _ in range(m)]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = tmp_path_factory.mktemp("claims") / "claims_test"
    # as tests/test_session_scheduler.py compiles its program; poseidon2.h carries hipcc's `#pragma unroll`
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "zeth_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "claims_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "claims ok" in r.stdout, r.stdout[-2000:] + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        if " = " in line:
            key, words = line.split(" = ")
            out[key] = np.array(words.split(), dtype=np.uint64).astype(np.uint32)
    return out


def test_structure_with_a_toy_hash(printed):
    """Part A ran inside the program (it exits non-zero at the first rule that does not hold)"""
    assert printed


def test_root_claims_equal_the_python_twin(printed):
    from zeth_amd import recursion as rec
    seen = 0
    for n in (1, 2, 3, 5, 7, 10):
        leaves = leaves_of(n)
        for ranks in ((1, 2) if n == 10 else (1,)):
            folded = rec.fold_leaf_claims(leaves, ranks)
            for m in (0, 1, 2, 3, 5):
                want = folded if m == 0 else rec.resolved_claim(folded, leaves[0][1], leaves[-1][2], rec.union_claims(assumed_of(m)))
                assert np.array_equal(printed[f"root n={n} ranks={ranks} m={m}"], want), (n, ranks, m)
                seen += 1
        core, pre, post = leaves[0]
        want = rec.resolved_claim(rec.wrap_claim(core, pre, post), pre, post, assumed_of(1)[0])
        assert np.array_equal(printed[f"resolved n={n}"], want), n
    assert seen == 35


def test_union_claims_equal_the_python_twin(printed):
    from zeth_amd import recursion as rec
    for m in (1, 2, 3, 5):
        want = rec.union_claims(assumed_of(m))
        assert np.array_equal(printed[f"union m={m}"], want), m
        assert np.array_equal(printed[f"root n=0 ranks=1 m={m}"], want), m          # no leaves: the union root alone


def test_allowed_tree_and_paths_equal_the_python_twin(printed):
    from zeth_amd import recursion as rec
    for k in (1, 7, 16):
        st = stream(300 + k)
        levels = rec.allowed_tree([take(st, 8) for _ in range(k)])
        assert len(levels) == 5
        for l, level in enumerate(levels):
            assert np.array_equal(printed[f"allowed k={k} level={l}"], np.concatenate(level)), (k, l)
        for index in range(16):
            assert np.array_equal(printed[f"path k={k} index={index}"], rec.membership_words(levels, index)), (k, index)
