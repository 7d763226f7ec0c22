"""A witness checked against a circuit's own constraints, row by row: the definition's host twin and the explainer.

`reference_check_rows` is the reference of the library's zkh_check_rows (csrc/check_rows.hip; DESIGN.md §2 CHECK ROWS).  For a ZKC1
description (desc.py), a trace of n = 2^po2 rows and the two global groups, every constraint is evaluated exactly on every row r of
the trace domain — no mix, no probability:

  * a tap (g, col, back) reads row (r - back) mod n; a cell or a global word is read as its residue (raw % P; the words are
    Montgomery forms, decoded here, which keeps zero at zero);
  * value steps compute in Fp, and in Fp4 = Fp[x] / (x^4 + 11) downstream of a ConstExt;
  * over the mix steps, F = the lowest failing and_eqz step (an index into the step list) or NONE:
        F(true) = NONE
        F(and_eqz(x, v)) = min(F(x), v != 0 ? this step : NONE)
        F(and_cond(x, cond, inner)) = min(F(x), cond != 0 ? F(inner) : NONE)      (an Fp4 is non-zero when any component is)

Row r fails when F(ret) != NONE.  Fp4 being a field, that is "the constraint polynomial is not identically zero in the mix": it
names a row wherever a check under one fixed mix does, and more.  Everything is vectorised over the rows in numpy integers.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

from .desc import (Circuit, GLOBAL_MIX, GLOBAL_OUT, OP_ADD, OP_AND_COND, OP_AND_EQZ, OP_CONST, OP_CONST_EXT, OP_GET, OP_GET_GLOBAL, OP_MUL,
                   OP_SUB, OP_TRUE, P)

NONE = 0xFFFFFFFF
GROUP_NAMES = ("accum", "code", "data")
GLOBAL_NAMES = ("out", "mix")
_RINV = pow(1 << 32, -1, P)
_NB = np.uint64(P - 11)           # x^4 = -11
_P = np.uint64(P)


def _decode(raw) -> np.ndarray:
    """raw Montgomery words -> canonical values below P (a raw word >= P is its residue)"""
    return (np.asarray(raw, dtype=np.uint64) % _P) * np.uint64(_RINV) % _P


def _ext(v) -> np.ndarray:
    """a base value (...,) as an Fp4 (4, ...)"""
    v = np.asarray(v, dtype=np.uint64)
    out = np.zeros((4,) + v.shape, dtype=np.uint64)
    out[0] = v
    return out


def _ext_mul(a, b) -> np.ndarray:
    m = lambda x, y: x * y % _P
    h0 = (m(a[1], b[3]) + m(a[2], b[2]) + m(a[3], b[1])) % _P
    h1 = (m(a[2], b[3]) + m(a[3], b[2])) % _P
    h2 = m(a[3], b[3])
    return np.stack([(m(a[0], b[0]) + h0 * _NB) % _P,
                     (m(a[0], b[1]) + m(a[1], b[0]) + h1 * _NB) % _P,
                     (m(a[0], b[2]) + m(a[1], b[1]) + m(a[2], b[0]) + h2 * _NB) % _P,
                     (m(a[0], b[3]) + m(a[1], b[2]) + m(a[2], b[1]) + m(a[3], b[0])) % _P])


def _parse(desc) -> Circuit:
    return desc if isinstance(desc, Circuit) else Circuit.parse(desc)


def _run(c: Circuit, po2: int, accum, code, data, out, mix, rows: np.ndarray, probe: Optional[int] = None):
    """F(ret) on `rows` (uint32) and, with probe = an and_eqz step, that step's operand on them as (4, rows) canonical words"""
    n = 1 << po2
    groups = []
    for g, a in enumerate((accum, code, data)):
        a = np.asarray(a, dtype=np.uint32).reshape(-1)
        assert a.size == c.group_sizes[g] * n, f"group {GROUP_NAMES[g]}: {a.size} words, expected {c.group_sizes[g]} x {n}"
        groups.append(a.reshape(c.group_sizes[g], n))
    globals_ = [_decode(np.asarray(out, dtype=np.uint32).reshape(-1)), _decode(np.asarray(mix, dtype=np.uint32).reshape(-1))]
    # last reader of every value, so that a long step list holds only its live values
    last_f: Dict[int, int] = {}
    nf = 0
    for i, (op, a, b, cc, d) in enumerate(c.steps):
        if op in (OP_ADD, OP_SUB, OP_MUL):
            last_f[a] = last_f[b] = i
        elif op in (OP_AND_EQZ, OP_AND_COND):
            last_f[b] = i
        nf += op < OP_TRUE
    release: Dict[int, List[int]] = {}
    for v, i in last_f.items():
        release.setdefault(i, []).append(v)
    fp: Dict[int, np.ndarray] = {}
    is_ext: List[bool] = []
    mixv: List[Optional[np.ndarray]] = []
    shape = rows.shape
    none = np.full(shape, NONE, dtype=np.uint32)
    probed = None

    def nonzero(v: int) -> np.ndarray:
        x = fp[v]
        return np.broadcast_to((x != 0).any(axis=0) if is_ext[v] else x != 0, shape)

    for i, (op, a, b, cc, d) in enumerate(c.steps):
        if op < OP_TRUE:
            k = len(is_ext)
            ext = False
            if k not in last_f:                            # nothing reads it
                val = None
                ext = op == OP_CONST_EXT or (op in (OP_ADD, OP_SUB, OP_MUL) and (is_ext[a] or is_ext[b]))
            elif op == OP_CONST:
                val = np.uint64(a % P)
            elif op == OP_CONST_EXT:
                val, ext = np.array([[a % P], [b % P], [cc % P], [d % P]], dtype=np.uint64), True
            elif op == OP_GET:
                g, off, back = c.taps[a]
                val = _decode(groups[g][off, (rows.astype(np.int64) - back) % n])
            elif op == OP_GET_GLOBAL:
                val = globals_[a][b]
            else:
                ext = is_ext[a] or is_ext[b]
                x, y = fp[a], fp[b]
                if ext:
                    x, y = x if is_ext[a] else _ext(x), y if is_ext[b] else _ext(y)
                    if x.ndim != y.ndim:                   # (4, 1) constants against (4, rows)
                        x, y = np.broadcast_arrays(x.reshape(4, -1), y.reshape(4, -1))
                if op == OP_ADD:
                    val = (x + y) % _P
                elif op == OP_SUB:
                    val = (x + _P - y) % _P
                else:
                    val = _ext_mul(x, y) if ext else x * y % _P
            is_ext.append(ext)
            if val is not None:
                fp[k] = val
        elif op == OP_TRUE:
            mixv.append(none)
        elif op == OP_AND_EQZ:
            if probe == i:
                x = fp[b] if is_ext[b] else _ext(fp[b])
                probed = np.broadcast_to(x.reshape(4, -1), (4,) + shape).copy()
            mixv.append(np.minimum(mixv[a], np.where(nonzero(b), np.uint32(i), np.uint32(NONE))))
        elif op == OP_AND_COND:
            mixv.append(np.minimum(mixv[a], np.where(nonzero(b), mixv[cc], np.uint32(NONE))))
        else:
            raise ValueError(f"step {i}: unknown op {op}")
        for v in release.get(i, ()):
            fp.pop(v, None)
    return mixv[c.ret].astype(np.uint32), probed


def reference_check_rows(desc, po2: int, accum, code, data, out, mix, row_lo: int = 0, row_hi: Optional[int] = None) -> np.ndarray:
    """-> 2^po2 words: F(ret) of every row of the window [row_lo, row_hi) (the lowest failing and_eqz step of the row, an index into
    the ZKC1 step list, or NONE = 0xffffffff), NONE outside the window.  accum / code / data: the raw traces (W x 2^po2 Montgomery
    words each); out / mix: the global words."""
    c = _parse(desc)
    n = 1 << po2
    row_hi = n if row_hi is None else row_hi
    assert 0 <= row_lo < row_hi <= n, f"window [{row_lo}, {row_hi}) is empty or outside [0, {n}]"
    f = np.full(n, NONE, dtype=np.uint32)
    f[row_lo:row_hi], _ = _run(c, po2, accum, code, data, out, mix, np.arange(row_lo, row_hi, dtype=np.int64))
    return f


def reference_value(desc, po2: int, accum, code, data, out, mix, row: int, step: int) -> Tuple[int, int, int, int]:
    """the value the and_eqz step `step` requires to be zero, on `row`: four canonical words (a base value has zero upper ones)"""
    c = _parse(desc)
    assert 0 <= step < len(c.steps) and c.steps[step][0] == OP_AND_EQZ, f"step {step} is no and_eqz"
    _, v = _run(c, po2, accum, code, data, out, mix, np.array([row], dtype=np.int64), probe=step)
    return tuple(int(x) for x in v[:, 0])


def first_failure(per_row: np.ndarray) -> Tuple[int, int, int]:
    """(lowest failing row or -1, its step or NONE, failing rows) of a per-row array"""
    bad = np.flatnonzero(np.asarray(per_row) != NONE)
    return (int(bad[0]), int(per_row[bad[0]]), int(bad.size)) if bad.size else (-1, NONE, 0)


def explain_step(desc, step: int) -> dict:
    """What the and_eqz step `step` of the description constrains: {"taps": the (group, column, back) its value reads, sorted,
    "globals": the (group, offset) global words it reads, "conds": the and_cond steps that enclose it, outermost first} (a step
    that no chain from ret reaches has no enclosing condition)."""
    c = _parse(desc)
    assert 0 <= step < len(c.steps) and c.steps[step][0] == OP_AND_EQZ, f"step {step} is no and_eqz"
    fp_step, mix_step = [], []
    for i, s in enumerate(c.steps):
        (mix_step if s[0] >= OP_TRUE else fp_step).append(i)
    taps, globals_, seen, stack = set(), set(), set(), [c.steps[step][2]]
    while stack:
        v = stack.pop()
        if v in seen:
            continue
        seen.add(v)
        op, a, b, _, _ = c.steps[fp_step[v]]
        if op == OP_GET:
            taps.add(tuple(c.taps[a]))
        elif op == OP_GET_GLOBAL:
            globals_.add((a, b))
        elif op in (OP_ADD, OP_SUB, OP_MUL):
            stack += [a, b]
    conds: Tuple[int, ...] = ()
    visited, walk = set(), [(c.ret, ())]
    while walk:
        m, enclosing = walk.pop()
        while (m, enclosing) not in visited:               # down the chain x <- x <- ... <- true
            visited.add((m, enclosing))
            i = mix_step[m]
            op, a, b, cc, _ = c.steps[i]
            if op == OP_TRUE:
                break
            if i == step:
                conds, walk = enclosing, []
                break
            if op == OP_AND_COND:
                walk.append((cc, enclosing + (i,)))
            m = a
    return {"taps": sorted(taps), "globals": sorted(globals_), "conds": list(conds)}


def describe_reads(desc, step: int) -> str:
    """`data[3]@0, code[2]@1, out[4]`: the reads of explain_step in a message"""
    e = explain_step(desc, step)
    return ", ".join([f"{GROUP_NAMES[g]}[{col}]@{back}" for g, col, back in e["taps"]] + [f"{GLOBAL_NAMES[g]}[{off}]" for g, off in e["globals"]])
