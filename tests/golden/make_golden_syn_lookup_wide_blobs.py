#!/usr/bin/env python3
"""Regenerate tests/golden/syn_lookup_wide_blobs.json (run from the repo root: python tests/golden/make_golden_syn_lookup_wide_blobs.py).

The file pins, per WIDE builder call of zeth_amd/circuits/syn_lookup.py (`build_syn_lookup(..., pages=True, wide=True)`: a paged memory of two
value words per address, ZKA1 version 10), a digest of the description and of the blob it returns; tests/test_logup_wide.py replays the
calls.  The calls without `wide` are pinned by syn_lookup_blobs.json and its own maker.  No GPU."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from zeth_amd.circuits import syn_lookup as sl  # noqa: E402

PATH = os.path.join(HERE, "syn_lookup_wide_blobs.json")
PAGED = dict(link=True, reads=True, pages=True, wide=True)
CALLS = [("TINY", PAGED), ("FULL", PAGED), ("TINY", dict(PAGED, derive=True, limbs=True)), ("FULL", dict(PAGED, derive=True, limbs=True)),
         ("MULTI", dict(PAGED, ports=True)), ("MULTI", dict(PAGED, ports=True, derive=True, limbs=True)), ("TINY", dict(PAGED, order_limbs=4))]


def digest(words):
    return hashlib.sha256(words.astype("<u4").tobytes()).hexdigest()[:16]


def record():
    """-> [[shape, kwargs, digest of the description, digest of the blob, the blob's version, header word 7]]"""
    out = []
    for shape, kw in CALLS:
        desc, blob = sl.build_syn_lookup(getattr(sl, shape), **kw)
        out.append([shape, kw, digest(desc), digest(blob), int(blob[1]), int(blob[7])])
    return out


if __name__ == "__main__":
    rows = record()
    with open(PATH, "w") as fh:
        json.dump(rows, fh, indent=0)
    print(f"wrote {PATH}: {len(rows)} builder calls")
