"""The forms of the Poseidon2 permutation the Merkle kernels call (zeth_amd/csrc/poseidon2.h, the header the kernels compile)
on the host: tests/cpp/poseidon2_callers.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_poseidon2_caller_forms_equal_literal_permutation_and_sponge(tmp_path):
    """Kept-cell ranges (0..7, 16..23, all 24, and the sponge's selectable one) and the zero-capacity entry, each followed by
    p2_finish, equal the literal 29-round permutation on the kept cells; a three-block sponge with a signed capacity equals
    the literal sponge; the last partial group's update sum stays below P 2^31 at all-extreme operands; the table's forward
    scale chain ends at R.  Edge-valued constant fills, random mixtures and the shipped tables."""
    exe = tmp_path / "poseidon2_callers"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "zeth_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "poseidon2_callers.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "20000"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stderr + r.stdout
