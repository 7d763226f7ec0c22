"""Which kernels every transform of zeth_amd/csrc/ntt.hip runs (zeth_amd/csrc/ntt_plan.h, the header run_transform consumes), on the host:
tests/cpp/ntt_plan_test.cpp walks all 432 cases and asserts each kernel's preconditions; its lines are compared with the recorded plan
tests/golden/ntt_plan.json (kernel, L, R, log_t, first_layer, grid x, block, dynamic LDS bytes per pass, and lazy)."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ntt_plan.json")


def load_golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def kernels_of(entry):
    """['low12', 'high8', ...] of a fixture entry, in execution order"""
    return [p.split()[0] for p in entry.split(" | ")[0].split("; ")]


def test_plan_of_every_transform_matches_the_recorded_one(tmp_path):
    exe = tmp_path / "ntt_plan_test"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "zeth_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "ntt_plan_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    got = dict(ln.split("\t") for ln in r.stdout.splitlines())
    want = load_golden()
    assert len(want) == 432 and sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} plans differ from the recorded ones, e.g. " + "; ".join(
        f"{k}: {g!r} instead of {w!r}" for k, (g, w) in list(wrong.items())[:3])
    # the fixture itself: every kernel sequence the sizes are known to take is there (shape counts of the recorded plan)
    shapes = {}
    for k, v in want.items():
        key = (k.split()[0], "+".join(kernels_of(v)))
        shapes[key] = shapes.get(key, 0) + 1
    assert shapes == {("fwd", "pass"): 86, ("fwd", "pass+pass"): 74, ("fwd", "pass+high8"): 51, ("fwd", "pass+high8+top"): 56,
                      ("fwd", "pass+high10"): 18, ("fwd", "pass+high10+top"): 43, ("fwd", "low12"): 5, ("fwd", "low12+pass"): 10,
                      ("fwd", "low12+high8"): 5, ("fwd", "low12+high10"): 5, ("fwd", "low12+high8+top"): 15, ("fwd", "low12+high10+top"): 10,
                      ("inv", "pass"): 24, ("inv", "low12"): 2, ("inv", "pass+pass"): 6, ("inv", "high8+pass"): 4, ("inv", "pass+low12"): 4,
                      ("inv", "high8+low12"): 2, ("inv", "high10+low12"): 2, ("inv", "top+high8+low12"): 6, ("inv", "top+high10+low12"): 4}
