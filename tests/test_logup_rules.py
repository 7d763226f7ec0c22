"""The rules of "arguments as data" against a recorded corpus (tests/golden/arguments_rules.json, tests/golden/make_golden_arguments.py):
8222 edits of one version-5 blob, each with the first message of the Python parser, of the Python rules with the circuit's widths and
of zkh_circuit_set_arguments on a GPU-less circuit, and the derived data columns of an accepted blob.  The corpus was recorded before
the checkers of the two record kinds were put behind one ownership view: the same first message, byte for byte, for every blob.  No GPU."""
import importlib.util
import json
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_arguments", os.path.join(HERE, "golden", "make_golden_arguments.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

MAX_GOLDEN_BYTES = 30349                                                     # the largest golden file before this one

# every message check_columns, check_links and the late-record rule can return, digits as N
RULE_MESSAGES = [
    "record N: kind N (N = LIMBS, N = ORDER)",
    "record N: N limbs of N bits (N..N limbs of N..N bits, at most N bits in all)",
    "record N: N sources (LIMBS: N; ORDER: N or N)",
    "record N: an ORDER record with two keys has at most N limbs (its flag column is the first destination)",
    "record N: a reserved word is not N (the unused source pair and the unused destination words)",
    "record N: a LINK of N carried columns and N limbs of N bits (N..N carried columns, N..N limbs of N..N bits, at most N bits in all)",
    "record N: a reserved word of a LINK is not N (words N, N, N, the unused carried pairs and the unused destination words)",
    "record N: selector N is not a code column",
    "record N: source (N, N) is not a code or data column",
    "record N: destination N is not a data column",
    "record N: its destination (data N) appears twice",
    "record N: its source (data N) is written by the sorted copy term N (a LINK reads what no derive writes)",
    "record N: its source (data N) is a destination of record N (records never chain)",
    "record N: its source (data N) is the derived multiplicity of term N",
    "record N: its destination (data N) is also written by record N",
    "record N: its destination (data N) is written by the sorted copy term N",
    "record N: its destination (data N) is the derived multiplicity of term N",
    "record N: its destination (data N) is read by record N (the links run after the columns, and never chain)",
    "record N: its destination (data N) is read by term N, the source of a sorted copy (the sort runs first)",
    "record N: its destination (data N) is the multiplicity of term N",
    "record N: its destination (data N) is the multiplicity of term N (of a LINK's destinations only linked and last may be)",
    "record N: a LIMBS / ORDER record after the LINK record N (LINK records come last)",
]
# what only a validator that knows the circuit says: the shape checks of set_arguments, which come before every rule, and the clauses
# of the records' rule (b) that need the groups' widths
KNOWS_THE_CIRCUIT = re.compile(r"accum Fp4 columns|alpha / beta|accum column|sign word|tuple width|is not a code column|"
                               r"is not a code or data column|is not a data column|not a ZKA1")


@pytest.fixture(scope="module")
def replay():
    return gen.record()


@pytest.fixture(scope="module")
def recorded():
    assert os.path.getsize(gen.PATH) <= MAX_GOLDEN_BYTES
    with open(gen.PATH) as fh:
        return json.load(fh)


def _show(cases):
    for edit, (parsed, sized, c_msg, cols) in cases:
        print(f"  words {[w for w, _ in edit]} = {[v for _, v in edit]}: python {gen.python_message(parsed, sized)!r}, C {c_msg!r}, derives {cols}")


def test_every_outcome_is_the_recorded_one(replay, recorded):
    corpus, single, double, extra = replay
    assert corpus["base"] == recorded["base"] and corpus["cases"] == recorded["cases"] == 8222
    bad = []
    for w, got, want in zip(gen.SINGLE_WORDS, corpus["single"], recorded["single"]):
        if got != want:
            bad.append(f"word {w}")
            print(f"word {w}: digest {got}, recorded {want}")
            _show(single[w])
    for i, (got, want) in enumerate(zip(corpus["double"], recorded["double"])):
        if got != want:
            bad.append(f"double edits {gen.DOUBLE_BATCH * i}..{gen.DOUBLE_BATCH * (i + 1) - 1}")
            print(f"double edits from {gen.DOUBLE_BATCH * i}: digest {got}, recorded {want}")
            _show(double[gen.DOUBLE_BATCH * i: gen.DOUBLE_BATCH * (i + 1)])
    for case, got, want in zip(extra, corpus["extra"], recorded["extra"]):
        if got != want:
            bad.append(f"extra edit {case[0]}")
            _show([case])
    assert not bad, bad
    assert corpus["templates"] == recorded["templates"] and corpus["accepted"] == recorded["accepted"]
    assert corpus == recorded


def test_the_c_message_is_the_python_message(replay):
    """Per case, whatever the file says.  The Python message is the parser's or, where the parser accepts, that of the rules with the
    circuit's widths.  Two kinds of case are left to the corpus alone: the parser's own refusals of a term's words (it meets them
    before any rule, the C validator inside check_sorted), and a C message that needs the circuit where the Python side had no widths
    (the parser refused) or where it comes from the shape checks that only set_arguments makes."""
    _, single, double, extra = replay
    compared = 0
    for edit, (parsed, sized, c_msg, _) in [c for w in gen.SINGLE_WORDS for c in single[w]] + double + extra:
        if parsed is not None and not parsed.startswith("ZKA1: "):
            continue
        if c_msg is not None and KNOWS_THE_CIRCUIT.search(c_msg) and (parsed is not None or not c_msg.startswith("set_arguments: record")):
            continue
        py = gen.python_message(parsed, sized)
        want = None if py is None else "set_arguments: " + (py[6:] if parsed is not None else py)
        assert c_msg == want, (edit, py, c_msg)
        compared += 1
    assert compared == 5399                                                  # of 8222: a function of the outcomes, which are the recorded ones


def test_every_rule_message_is_reached(recorded):
    reached = {t[6:] if t.startswith("ZKA1: ") else t for t in recorded["templates"]}
    assert [m for m in RULE_MESSAGES if m not in reached] == []
    assert len(recorded["templates"]) == 47
