"""CHECK BUS on the host (zeth_amd/circuits/logup.py: reference_bus, describe_bus, bus_slots), the definition's twin of zkh_check_bus:
tied to the test the verifier enforces — reference_bus reports an unbalanced key exactly when reference_accumulate's total is not zero
under the suites' fixed mix, on every honest and forged witness the logup suites build — then against numbers stated by hand, and
the mirrors of the call (the exported symbol, the generated Rust block, the ctypes structs against sizeof over zkhal.h)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import check_bus_cases as cases
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.circuits.desc import GROUP_DATA, P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = syn_lookup.TINY


def _total(case):
    desc, blob, po2, zk, code, data = case[:6]
    _accum, total = logup.reference_accumulate(logup.Arguments.parse(blob), po2, zk, code, data, cases.MIX, check_balance=False)
    return total


# ---- agreement with the accumulate's test ----
@pytest.mark.parametrize("variant", sorted(cases.VARIANTS))
@pytest.mark.parametrize("po2,zk", cases.SIZES)
def test_an_honest_witness_has_no_unbalanced_key_and_the_accumulate_agrees(variant, po2, zk):
    case = cases.honest(variant, po2, zk)
    bus = cases.reference(case)
    assert (bus["term"], bus["row"], bus["unbalanced_keys"], bus["net"]) == (-1, -1, 0, 0) and bus["distinct_keys"] > 0
    assert not bus["per_term"][:, 0].any() and (bus["per_term"][:, 1:3] == -1).all()
    assert _total(case) == [0, 0, 0, 0]
    assert logup.describe_bus(bus, logup.Arguments.parse(case[1])) is None


@pytest.mark.parametrize("kind", cases.FORGERIES)
def test_a_forged_witness_has_an_unbalanced_key_exactly_when_the_accumulate_total_is_not_zero(kind):
    case = cases.forgery(kind)
    bus = cases.reference(case)
    assert (bus["unbalanced_keys"] > 0) == any(_total(case)) == (kind not in cases.BALANCED)
    assert (bus["row"] >= 0) == (bus["unbalanced_keys"] > 0)


@pytest.mark.parametrize("variant", ["derived", "ordered", "linked", "reads"])
def test_a_witness_before_its_derives_is_unbalanced_and_the_accumulate_agrees(variant):
    desc, blob, po2, zk, code, _data, uploaded = cases.honest(variant, 10, 300)
    case = (desc, blob, po2, zk, code, uploaded)
    assert cases.reference(case)["unbalanced_keys"] > 0 and any(_total(case))


# ---- expectations stated by hand ----
def test_a_limb_moved_out_of_the_table():
    po2, zk = 10, 300
    n = 1 << po2
    desc, blob = syn_lookup.syn_lookup_tiny()
    args = logup.Arguments.parse(blob)
    code, data, _out = syn_lookup.witness(TINY, po2, zk, seed=3)
    limb_col = syn_lookup.layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[1][0][0]           # limb 0 of word 0: blob term 0
    assert args.terms[0].tuple_cols == ((GROUP_DATA, limb_col),)
    limb = int(logup._dec(data.reshape(-1, n)[limb_col, 0]))
    bad = syn_lookup.corrupt_limb(TINY, data, po2, row=0, word=0)                          # row 0 of term 0: the lowest entry there is
    bus = logup.reference_bus(args, po2, zk, code, bad)
    # the forged value 16 + limb is in no table row: one entry, weight 1, nothing against it; the value it left is one lookup short
    assert (bus["term"], bus["row"], bus["tag"], bus["key"], bus["net"], bus["unbalanced_keys"]) == (0, 0, 0, (16 + limb, 0, 0, 0), 1, 2)
    assert bus["per_term"][0].tolist() == [1, 0, 0, 1] and not bus["per_term"][1:, 0].any()
    line = logup.describe_bus(bus, args)
    assert line.startswith(f"bus: key (tag 0; {16 + limb}, 0, 0, 0) does not balance, net 1: term 0 (+) has 1 entry, rows 0..0, weight 1; "
                           f"term 8 (−, sel code[5], m data[10]) has none; term 1 (+) has none; ")
    assert line.endswith(f"; … and 1 more; 2 of {bus['distinct_keys']} keys do not balance")
    assert line.count("term ") == 8


def test_a_table_multiplicity_raised_by_one():
    po2, zk = 10, 300
    n = 1 << po2
    desc, blob = syn_lookup.syn_lookup_tiny()
    args = logup.Arguments.parse(blob)
    code, data, _out = syn_lookup.witness(TINY, po2, zk, seed=3)
    d = data.reshape(-1, n).copy()
    d[10, 11] = (int(d[10, 11]) + cases.ONE) % P                                           # m of the table row of value 11
    limbs = logup._dec(d[2:10, :n - zk])                                                   # the eight limb columns, terms 0..7 in this order
    term, row = next((t, int(np.argmax(limbs[t] == 11))) for t in range(8) if (limbs[t] == 11).any())
    bus = logup.reference_bus(args, po2, zk, code, d.reshape(-1))
    assert (bus["term"], bus["row"], bus["tag"], bus["key"], bus["net"], bus["unbalanced_keys"]) == (term, row, 0, (11, 0, 0, 0), P - 1, 1)
    lookups = int((limbs == 11).sum())
    assert bus["per_term"][8].tolist() == [1, 11, 11, lookups + 1] and int(bus["per_term"][:8, 3].sum()) == lookups
    assert logup.describe_bus(bus, args).startswith(f"bus: key (tag 0; 11, 0, 0, 0) does not balance, net {P - 1}: term 8 (−, sel code[5], m data[10]) "
                                                    f"has 1 entry, rows 11..11, weight {lookups + 1}; term ")


def test_a_wrong_pval_leaves_two_keys_and_the_lower_representative_is_reported():
    desc, blob, po2, zk, code, wrong = cases.forgery("wrong_pval")
    n, A = 1 << po2, (1 << po2) - zk
    args = logup.Arguments.parse(blob)
    c_addr, c_val, c_time, c_linked, c_last, c_pval, c_ptime, *_ = syn_lookup.link_layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[0]
    w = wrong.reshape(-1, n)
    r2 = next(r for r in range(A // 3, A) if w[c_linked, r] == cases.ONE)                  # the forged row, as the forgery picks it
    addr, pval, ptime = (int(logup._dec(w[c, r2])) for c in (c_addr, c_pval, c_ptime))
    plus = next(i for i, t in enumerate(args.terms) if t.tag == 1 and t.sign == 1)
    minus = next(i for i, t in enumerate(args.terms) if t.tag == 1 and t.mult == (GROUP_DATA, c_linked))
    bus = logup.reference_bus(args, po2, zk, code, wrong)
    # (addr, pval - 1, ptime) is what row ptime stored and nothing removes: + term, row ptime (times are row numbers), net 1;
    # (addr, pval, ptime) is removed on row r2 and was never stored: - term, net P - 1.  The + term has the lower index.
    assert plus < minus and bus["unbalanced_keys"] == 2
    assert (bus["term"], bus["row"], bus["tag"], bus["key"], bus["net"]) == (plus, ptime, 1, (addr, pval - 1, ptime, 0), 1)
    assert bus["per_term"][plus].tolist() == [1, ptime, ptime, 1] and bus["per_term"][minus, 0] == 0
    assert f"term {minus} (−, m data[{c_linked}]) has none" in logup.describe_bus(bus, args)


@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_hand_built_pairs(name):
    case = cases.hand(name)
    bus = cases.reference(case)
    term, row, key, net, unbalanced, distinct = cases.HAND[name]
    assert (bus["term"], bus["row"], bus["key"], bus["net"], bus["unbalanced_keys"], bus["distinct_keys"]) == (term, row, key, net, unbalanced, distinct)
    assert bus["tag"] == (cases.PAIR_TAG if row >= 0 else 0) and bus["slots"] == 1024
    assert any(_total(case)) == (unbalanced > 0)


def test_the_culprit_is_in_the_per_term_table_when_it_is_not_the_representative():
    case = cases.hand("representative")
    bus = cases.reference(case)
    assert bus["per_term"].tolist() == [[2, 5, 300, 2], [2, 5, 300, 4]]
    assert logup.describe_bus(bus, logup.Arguments.parse(case[1])) == (
        f"bus: key (tag 5; 1005, 0, 0, 0) does not balance, net {P - 2}: term 0 (+, sel code[0], m data[2]) has 2 entries, rows 5..300, weight 2; "
        "term 1 (−, m data[3]) has 2 entries, rows 5..300, weight 4; 1 of 411 keys do not balance")


def test_the_table_size_rule_and_the_two_growth_shapes():
    assert [logup.bus_slots(A, 0) for A in (1, 32, 33, 724, 1024, 1025)] == [64, 64, 128, 2048, 2048, 4096]
    assert logup.bus_slots(724, 1024) == 2048 and logup.bus_slots(724, 1025) == 4096 and logup.bus_slots(724, 2188) == 8192
    tiny, multi = cases.reference(cases.honest("plain", 10, 300)), cases.reference(cases.honest("multi_sorted", 10, 300))
    start = logup.bus_slots(724, 0)
    assert tiny["distinct_keys"] <= start // 2 < multi["distinct_keys"]                    # on either side of half the starting table
    assert tiny["slots"] == start and multi["slots"] > start


# ---- the mirrors of the call ----
def test_the_symbol_is_exported_and_bound():
    from zeth_amd import hal
    lib = hal.load_library()
    assert "zkh_check_bus" in hal.ABI and lib.zkh_check_bus is not None


def test_the_generated_rust_block_matches_the_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rs = open(os.path.join(ROOT, "rust", "risc0-sys-hip", "src", "lib.rs")).read()
    assert re.search(r"pub fn zkh_check_bus\(a0: \*mut ZkhCtx, a1: \*const ZkhCircuit, po2: usize, zk_cycles: usize, code: \*const ZkhBuf, "
                     r"data: \*const ZkhBuf, per_term: \*mut ZkhBusTerm, n_terms: usize, result: \*mut ZkhCheckBusResult\) -> \*const c_char;", rs)
    body = re.search(r"pub struct ZkhCheckBusResult \{(.*?)\}", rs, re.S).group(1)
    assert re.findall(r"pub (\w+): ([^,]+),", body) == [("row", "i64"), ("term", "i32"), ("tag", "u32"), ("key", "[u32; 4]"), ("net", "u32"),
                                                         ("unbalanced_keys", "u32"), ("distinct_keys", "u32"), ("slots", "u32")]
    body = re.search(r"pub struct ZkhBusTerm \{(.*?)\}", rs, re.S).group(1)
    assert re.findall(r"pub (\w+): ([^,]+),", body) == [("count", "u32"), ("first_row", "u32"), ("last_row", "u32"), ("weight", "u32")]
    shim = open(os.path.join(ROOT, "rust", "hal_hip.rs")).read()
    assert "sys::zkh_check_bus(" in shim and "pub fn check_bus(" in shim


def test_the_ctypes_structs_have_the_header_s_sizes_and_offsets(tmp_path):
    import ctypes as C
    from zeth_amd import hal
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "zkhal.h"\nint main() {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(zkh_check_bus_result), offsetof(zkh_check_bus_result, row), '
                   'offsetof(zkh_check_bus_result, term), offsetof(zkh_check_bus_result, tag), offsetof(zkh_check_bus_result, key), '
                   'offsetof(zkh_check_bus_result, net), offsetof(zkh_check_bus_result, unbalanced_keys), offsetof(zkh_check_bus_result, distinct_keys), '
                   'offsetof(zkh_check_bus_result, slots));\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(zkh_bus_term), offsetof(zkh_bus_term, count), offsetof(zkh_bus_term, first_row), '
                   'offsetof(zkh_bus_term, last_row), offsetof(zkh_bus_term, weight));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    R, T = hal.CheckBusResult, hal.BusTerm
    assert [int(x) for x in lines[0].split()] == [C.sizeof(R)] + [getattr(R, f).offset for f in ("row", "term", "tag", "key", "net", "unbalanced_keys",
                                                                                              "distinct_keys", "slots")]
    assert [int(x) for x in lines[1].split()] == [C.sizeof(T)] + [getattr(T, f).offset for f in ("count", "first_row", "last_row", "weight")]
