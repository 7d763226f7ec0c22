"""What the compiler makes of the table loads of k_hash_rows<true> and k_hash_fold<true>, read from a fresh `hipcc -S` of hash.hip
by tools/isa_histogram.py (no GPU).  hash.hip is built without the machine scheduler, so where the source requests a table word
is where the load issues; this holds the source to it:
  - no flat loads (a laundered pointer once turned every uniform table word into a per-lane flat load);
  - no scratch, four waves per SIMD;
  - no table load whose wait is the next instruction: none with zero VALU + MFMA instructions between the request and the
    s_waitcnt that covers it, which is the stronger reading (scalar loads return out of order, so one wait covers a group);
  - requesting ahead is not paid for in instructions: VALU per wave-permutation at most 1 % above what the kernels had before
    the loads moved (5 023 and 4 973)."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALU_BEFORE = {"rows": 5023, "fold": 4973}


def _tool():
    spec = importlib.util.spec_from_file_location("isa_histogram", os.path.join(ROOT, "tools", "isa_histogram.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def reports():
    tool = _tool()
    from zeth_amd import build as B
    if not (os.path.exists(B.HIPCC) or shutil.which(B.HIPCC)):
        pytest.skip("no hipcc")
    lines = tool.compile_asm()
    return tool, {k: tool.analyze(lines, k) for k in ("rows", "fold")}


@pytest.mark.parametrize("kernel", ("rows", "fold"))
def test_table_loads(reports, kernel):
    tool, rep = reports
    d = rep[kernel]
    tool.print_loads(d)
    kinds, _ = tool.loads_summary(d)
    res = d["resources"]
    n = {k: sum(1 for x in d["loads"] if x[1] == k) for k in kinds}
    assert "ILb1E" in d["name"], d["name"]
    assert n["flat"] == 0 and not any(l.strip().startswith("flat_") for l in d["body"]), "flat loads"
    assert n["scalar"] >= 20 and n["global"] + n["LDS"] >= 27, n        # the beta and constant rows; the 27 A fragments
    assert res["ScratchSize"] == 0 and not any(l.strip().startswith("scratch_") for l in d["body"]), res
    assert res["Occupancy"] >= 4 and res["NumVgprs"] + res.get("NumAgprs", 0) <= 128, res
    zero = [(i, k, d["body"][i].strip()) for i, k, dist in d["loads"] if dist == 0]
    assert not zero, zero
    assert sum(d["mfma"].values()) == 54, d["mfma"]
    assert d["total"] <= 1.01 * VALU_BEFORE[kernel], (d["total"], VALU_BEFORE[kernel])
