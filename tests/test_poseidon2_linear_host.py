"""The partial rounds as one affine map through int8 digit products (zeth_amd/csrc/poseidon2_linear.h, the header the kernels
compile) on the host: tests/cpp/poseidon2_linear.cpp, once plain and once under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags,cases", [(["-O2"], "2000"), (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "200")],
                         ids=["plain", "asan-ubsan"])
def test_linear_partial_rounds_model_equals_literal_rounds(tmp_path, flags, cases):
    """The host model (the table's own digits, the XORed bytes, the recombination and the chain the device runs; the tile products
    as int32 loops) equals the literal 21 partial rounds on random words, every cell at +-(P-1) and +-(P-1)/2, and words whose
    bytes are all 0x00, 0x7f, 0x80 or 0xff; the whole permutation through it equals poseidon2_mix, the literal 29 rounds and the
    published known-answer vector; the largest digit sum, recombined word, reduced sum and output stay within the builder's exact
    bounds; a table with one digit altered is refused or caught.  Shipped tables."""
    exe = tmp_path / "poseidon2_linear"
    subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "zeth_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "poseidon2_linear.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), cases], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stderr + r.stdout
