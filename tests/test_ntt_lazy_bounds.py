"""The paired lazy NTT butterflies (zeth_amd/csrc/ntt_lazy.h, the header the kernels compile) on the host, at the edges of
their representation bounds: tests/cpp/ntt_lazy_bounds.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lazy_ntt_pairs_equal_radix2_layers_within_bounds(tmp_path):
    """Edge-valued and random blocks, and whole columns through every lazy round of k_ntt_low12 / k_ntt_high<10 | 8> with the
    library's centred table: every output congruent to the radix-2 layers, inside (-P, P), every reduced sum below P 2^31."""
    exe = tmp_path / "ntt_lazy_bounds"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "zeth_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "ntt_lazy_bounds.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "400000"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stderr + r.stdout
