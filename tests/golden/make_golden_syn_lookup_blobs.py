#!/usr/bin/env python3
"""Regenerate tests/golden/syn_lookup_blobs.json (run from the repo root: python tests/golden/make_golden_syn_lookup_blobs.py).

The file pins, per builder call of zeth_amd/circuits/syn_lookup.py, a digest of the description and of the ZKA1 blob it returns.  It was
recorded on the commit before LINK records learnt to join a memory (ZKA1 version 9): every blob the builders wrote then must come out byte
for byte afterwards, and tests/test_logup_ports.py replays the calls.  No GPU."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from zeth_amd.circuits import syn_lookup as sl  # noqa: E402

PATH = os.path.join(HERE, "syn_lookup_blobs.json")
LINKED = [dict(link=True), dict(link=True, reads=True), dict(link=True, derive=True, limbs=True), dict(link=True, reads=True, derive=True, limbs=True)]
PAGED = [dict(link=True, reads=True, pages=True), dict(link=True, reads=True, pages=True, tied=True), dict(link=True, reads=True, pages=True, derive=True, limbs=True),
         dict(link=True, reads=True, pages=True, tied=True, derive=True, limbs=True)]
PLAIN = [dict(), dict(derive=True), dict(sort=True), dict(derive=True, sort=True), dict(limbs=True), dict(order=True), dict(sort=True, order=True, limbs=True, derive=True),
         dict(sort=True, sort_keys=(0,))]
FOUR_LIMBS = [("TINY", dict(link=True, order_limbs=4)), ("MULTI", dict(link=True, reads=True, order_limbs=4)), ("TINY", dict(link=True, reads=True, pages=True, order_limbs=4))]
WIDE = [("WIDE", dict()), ("WIDE", dict(derive=True, sort=True, limbs=True))]     # 16-bit limbs: no three limbs of an order, a link or a page fit 29 bits
CALLS = [(shape, kw) for shape in ("TINY", "FULL", "MULTI") for kw in PLAIN + LINKED] + [(shape, kw) for shape in ("TINY", "FULL") for kw in PAGED] + FOUR_LIMBS + WIDE


def digest(words):
    return hashlib.sha256(words.astype("<u4").tobytes()).hexdigest()[:16]


def record():
    """-> [[shape, kwargs, digest of the description, digest of the blob, the blob's version]]"""
    out = []
    for shape, kw in CALLS:
        desc, blob = sl.build_syn_lookup(getattr(sl, shape), **kw)
        out.append([shape, {k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()}, digest(desc), digest(blob), int(blob[1])])
    return out


if __name__ == "__main__":
    rows = record()
    with open(PATH, "w") as fh:
        json.dump(rows, fh, indent=0)
    print(f"wrote {PATH}: {len(rows)} builder calls")
