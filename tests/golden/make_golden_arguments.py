#!/usr/bin/env python3
"""Regenerate tests/golden/arguments_rules.json (run from the repo root: python tests/golden/make_golden_arguments.py).

The corpus pins what the rules of "arguments as data" answer (zeth_amd/circuits/logup.py and csrc/arguments.hip: which blob is
refused, with which first message, and which data columns an accepted blob derives) against drift: it was recorded on the commit
before the two rule checkers were put behind one ownership view, and tests/test_logup_rules.py replays it.  No GPU.

The base blob is the version-5 blob of tests/test_logup_links.py plus an ORDER record over the sorted columns: 184 words, 5 terms,
4 records (LIMBS, ORDER, LINK, LINK).  The cases are edits of its words:
  * every single-word edit of words 1..4 and 8..183 to each value of VALUES that differs from the word;
  * 3000 double edits over words 8..183, drawn with numpy.random.default_rng(5);
  * EXTRA, the edits that reach a message no case above reaches.
Header words 5 and 6 (n_terms, n_records) are left alone: tests/test_logup_links.py edits them.
The outcome of a case is four fields: the parser's message; if it accepts, that of the rules with the circuit's widths; the message of
zkh_circuit_set_arguments on a GPU-less circuit; if that accepts, the list of zkh_circuit_derived_data_columns.  The file holds one
digest of the outcomes per edited word and one per 100 double edits, and the table of message templates (digits as N) with their counts."""
import hashlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from zeth_amd import hal as zhal  # noqa: E402
from zeth_amd.circuits import logup  # noqa: E402
from zeth_amd.circuits.desc import GROUP_CODE, GROUP_DATA  # noqa: E402

PATH = os.path.join(HERE, "arguments_rules.json")
SIZES = (8, 6, 40)
VALUES = sorted(set(range(26)) | {29, 40, logup.NONE, 0x12, 0x10032})
SINGLE_WORDS = list(range(1, 5)) + list(range(8, 184))
N_DOUBLE, DOUBLE_BATCH = 3000, 100
ORDER_AT = logup.ARGS_HEADER + 16 * 5 + 16                                   # record 1
# "an ORDER record with two keys has at most 7 limbs": nl = 8, and L = 4 so that L nl <= 32
EXTRA = [[(ORDER_AT + 1, 4), (ORDER_AT + 2, 8)]]


def base():
    """-> (description, blob): the builder of tests/test_logup_links.py::_builder plus an ORDER record over the sorted columns 2, 3"""
    b = logup.LogupBuilder(SIZES, (4, 8))
    b.term(0, [(GROUP_DATA, 0), (GROUP_DATA, 1)], tag=1)
    b.term(0, [(GROUP_DATA, 2), (GROUP_DATA, 3)], sign=-1, tag=1, sorted_from=0, sort_keys=(0, 1))
    b.term(1, [(GROUP_CODE, 1)], sign=-1, mult=(GROUP_DATA, 4), tag=0, derive=True)
    b.derive_links(3, (GROUP_DATA, 8), [(GROUP_DATA, 9), (GROUP_DATA, 10)], [11, 12, 13, 14, 15, 16, 17], 8)
    b.derive_limbs((GROUP_CODE, 2), [5, 6, 7], 5)
    b.derive_links(None, (GROUP_CODE, 4), [(GROUP_DATA, 18)], [19, 20, 21], 4)
    b.term(1, [(GROUP_DATA, 8), (GROUP_DATA, 14), (GROUP_DATA, 13)], sign=-1, mult=(GROUP_DATA, 11), tag=2)
    b.term(1, [(GROUP_DATA, 15)], tag=0)
    b.derive_order([(GROUP_DATA, 2), (GROUP_DATA, 3)], [22, 23, 24, 25], 7)
    desc, blob = b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 0)))
    assert blob.size == 184 and blob[1] == 5 and blob[5] == 5 and blob[6] == 4
    return desc, blob


def single_edits(blob):
    """-> {word: [edit, ...]}, an edit a list of (word, value)"""
    return {w: [[(w, v)] for v in VALUES if v != int(blob[w])] for w in SINGLE_WORDS}


def double_edits():
    rng = np.random.default_rng(5)
    words, values = rng.integers(8, 184, size=(N_DOUBLE, 2)), rng.integers(0, len(VALUES), size=(N_DOUBLE, 2))
    return [[(int(w), VALUES[int(v)]) for w, v in zip(ws, vs)] for ws, vs in zip(words, values)]


def outcome(hc, blob, edit):
    """-> (the parser's message or None, the rules' message with the circuit's widths or None, the C message or None, the derived columns)"""
    bad = blob.copy()
    for w, v in edit:
        bad[w] = v
    parsed = sized = c_msg = None
    try:
        a = logup.Arguments.parse(bad)
        sized = logup.check_sorted(a.terms) or logup.check_derived(a.terms) or logup._check_records(a.terms, a.records, SIZES)
    except ValueError as e:
        parsed = str(e)
    cols = []
    try:
        zhal._check(zhal._lib.zkh_circuit_set_arguments(hc.h, zhal._ptr(bad), bad.size))
        out, n = np.zeros(64, dtype=np.uint32), zhal.C.c_size_t()
        zhal._check(zhal._lib.zkh_circuit_derived_data_columns(hc.h, zhal._ptr(out), out.size, zhal.C.byref(n)))
        cols = [int(x) for x in out[:n.value]]
    except zhal.HalError as e:
        c_msg = str(e)
    return parsed, sized, c_msg, cols


def digest(outcomes):
    return hashlib.sha256("\n".join(json.dumps(o) for o in outcomes).encode()).hexdigest()[:10]


def template(msg):
    return re.sub(r"(?<![A-Za-z])(0x[0-9a-f]+|\d+)", "N", msg)


def python_message(parsed, sized):
    """the one message of the Python side: the parser's, else that of the rules with the circuit's widths"""
    return parsed if parsed is not None else sized


def record():
    """-> the corpus as the file holds it, and every (edit, outcome) behind it"""
    desc, blob = base()
    hc = zhal.HostCircuit(desc)
    run = lambda edits: [(e, outcome(hc, blob, e)) for e in edits]
    single = {w: run(edits) for w, edits in single_edits(blob).items()}
    double = run(double_edits())
    extra = run(EXTRA)
    cases = [c for w in SINGLE_WORDS for c in single[w]] + double + extra
    templates = {}
    for _, (parsed, sized, _, _) in cases:
        msg = python_message(parsed, sized)
        if msg is not None:
            templates[template(msg)] = templates.get(template(msg), 0) + 1
    corpus = {"generator": "tests/golden/make_golden_arguments.py",
              "base": hashlib.sha256(blob.astype("<u4").tobytes()).hexdigest()[:16],
              "cases": len(cases), "accepted": sum(o[2] is None for _, o in cases),
              "single": [digest([o for _, o in single[w]]) for w in SINGLE_WORDS],
              "double": [digest([o for _, o in double[i:i + DOUBLE_BATCH]]) for i in range(0, N_DOUBLE, DOUBLE_BATCH)],
              "extra": [digest([o]) for _, o in extra],
              "templates": dict(sorted(templates.items()))}
    return corpus, single, double, extra


if __name__ == "__main__":
    corpus = record()[0]
    with open(PATH, "w") as fh:
        json.dump(corpus, fh, indent=0)
    print(f"wrote {PATH}: {corpus['cases']} cases, {corpus['accepted']} accepted, {len(corpus['templates'])} templates")
