"""The numpy float64 restatement of the score-boosting stage (include/hx.h: hx_formula): the
postfix program over whole arrays of pool positions -- every numpy float64 operation is one IEEE operation, as the
kernel's are --, hx_exp, the fp32 value, the drops, the threshold and a full sort by (value descending, position
ascending).  Shared by tests/test_formula_host.py and tests/test_gpu_formula.py."""
from __future__ import annotations

import math
import struct

import numpy as np

(F_CONST, F_SCORE, F_VAR, F_COND, F_ADD, F_MUL, F_NEG, F_ABS, F_DIV, F_SQRT, F_EXP, F_LIN_DECAY, F_EXP_DECAY,
 F_GAUSS_DECAY) = range(14)
F64_MISSING, F64_NULL = 0x7FF80000FFFFFFFF, 0x7FF80000FFFFFFFE
NAN_BITS = 0x7FF8000000000000
_C = [1.0 / float(math.factorial(i)) for i in range(14)]


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def from_bits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", int(b) & 0xFFFFFFFFFFFFFFFF))[0]


def hx_exp(x) -> np.ndarray:
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        xs = np.where((x >= -708.0) & (x <= 709.0), x, 0.0)           # (the branches' inputs; NaN compares false)
        k = np.rint(xs * 1.4426950408889634)
        r = (xs - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10
        p = np.full_like(xs, _C[13])
        for i in range(12, -1, -1):
            p = p * r + _C[i]
        y = np.ldexp(p, k.astype(np.int64))
    y = np.where(x > 709.0, np.inf, y)
    y = np.where(x < -708.0, 0.0, y)
    return np.where(x != x, x, y)


def orderable(v: np.ndarray) -> np.ndarray:
    u = np.asarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def make_keys(values, ids) -> np.ndarray:
    return (orderable(values).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(ids, np.uint64))


def key_scores(keys) -> np.ndarray:
    u = (np.asarray(keys, np.uint64) >> np.uint64(32)).astype(np.uint32)
    u = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32)
    return u.view(np.float32)


def key_ids(keys) -> np.ndarray:
    return (np.uint64(0xFFFFFFFF) - (np.asarray(keys, np.uint64) & np.uint64(0xFFFFFFFF))).astype(np.int64)


def run_program(ops, scores, rows, columns, planes) -> np.ndarray:
    """The double every position's program ends with: scores float32 [m], rows int64 [m], columns {col: uint64 cells per
    row}, planes [bool per row]."""
    m = len(rows)
    st = []
    with np.errstate(all="ignore"):
        for op, arg, imm in ops:
            c = from_bits(imm)
            if op == F_CONST:
                st.append(np.full(m, c, np.float64))
            elif op == F_SCORE:
                st.append(np.asarray(scores, np.float32).astype(np.float64))
            elif op == F_VAR:
                cell = np.asarray(columns[arg], np.uint64)[rows]
                cell = np.where((cell == np.uint64(F64_MISSING)) | (cell == np.uint64(F64_NULL)), np.uint64(imm), cell)
                st.append(cell.astype(np.uint64).view(np.float64).copy())
            elif op == F_COND:
                st.append(np.where(np.asarray(planes[arg], bool)[rows], 1.0, 0.0))
            elif op in (F_ADD, F_MUL, F_DIV):
                b = st.pop()
                a = st.pop()
                if op == F_ADD:
                    st.append(a + b)
                elif op == F_MUL:
                    st.append(a * b)
                else:
                    st.append(np.where(b == 0.0, c, a / np.where(b == 0.0, 1.0, b)))
            else:
                a = st.pop()
                if op == F_NEG:
                    st.append(-a)
                elif op == F_ABS:
                    st.append(np.abs(a))
                elif op == F_SQRT:
                    st.append(np.sqrt(a))
                elif op == F_EXP:
                    st.append(hx_exp(a))
                elif op == F_LIN_DECAY:
                    t = 1.0 - c * np.abs(a)
                    st.append(np.where(t < 0.0, 0.0, t))
                elif op == F_EXP_DECAY:
                    st.append(hx_exp(c * np.abs(a)))
                elif op == F_GAUSS_DECAY:
                    st.append(hx_exp(c * (a * a)))
                else:
                    raise ValueError(f"unknown op {op}")
    assert len(st) == 1
    return st[0]


def values_f32(x) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.asarray(x, np.float64).astype(np.float32) + np.float32(0.0)


def formula_stage(ops, planes, keys, counts, eligible, threshold, limit, columns, n_rows, id_base=0):
    """hx_formula: keys uint64 [B, stride] (ids = id_base + row), counts int [B] or None, eligible bool [n_rows] or None,
    threshold a float or None -> (out_keys uint64 [B, limit], out_pos int32 [B, limit], counts int32 [B], dropped
    int32 [B])."""
    keys = np.asarray(keys).view(np.uint64) if np.asarray(keys).dtype == np.int64 else np.asarray(keys, np.uint64)
    B, stride = keys.shape
    ok = np.zeros((B, limit), np.uint64)
    op_ = np.full((B, limit), -1, np.int32)
    oc = np.zeros(B, np.int32)
    od = np.zeros(B, np.int32)
    for b in range(B):
        n = stride if counts is None else max(0, min(int(counts[b]), stride))
        k = keys[b, :n]
        ids = key_ids(k)
        rows = ids - id_base
        on = (k != 0) & (rows >= 0) & (rows < n_rows)
        if eligible is not None:
            on &= np.asarray(eligible, bool)[np.where(on, rows, 0)]
        pos = np.nonzero(on)[0]
        if len(pos) == 0:
            continue
        v = values_f32(run_program(ops, key_scores(k[pos]), rows[pos], columns, planes))
        fin = np.isfinite(v)
        od[b] = int((~fin).sum())
        live = fin if threshold is None or threshold != threshold else fin & ~(v < np.float32(threshold))
        pos, v = pos[live], v[live]
        order = sorted(range(len(pos)), key=lambda i: (-float(v[i]), int(pos[i])))[:limit]
        m = len(order)
        oc[b] = m
        ok[b, :m] = make_keys(v[order], ids[pos[order]])
        op_[b, :m] = pos[order]
    return ok, op_, oc, od
