"""Host side of the late-interaction rerank (include/hx.h): the quantiser of token embeddings,
the packing of ragged token lists as the engine takes them, and `maxsim_scores`, the host statement of the score the
kernel computes (bit for bit: every product and sum below is one float32 operation, in the order hx.h fixes)."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

MAX_QTOKENS = 64                      # HX_MAXSIM_MAX_QTOKENS
MAX_DIM = 1024                        # HX_TOKENS_MAX_DIM
MISSING, NULL = 0xFFFFFFFF, 0xFFFFFFFE   # HX_PAY_U32_MISSING / _NULL: the heads of rows without tokens


def check_dim(dim: int) -> int:
    if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)) or not 64 <= dim <= MAX_DIM or dim % 64:
        raise ValueError(f"a token width must be a multiple of 64 in [64, {MAX_DIM}], got {dim!r}")
    return int(dim)


def quantize_tokens(arr) -> Tuple[np.ndarray, np.ndarray]:
    """[T, dim] floats -> ([T, dim] int8, [T] float32 scales), prep.hip's rule in float32: amax = max|x|, scale =
    amax / 127, x8 = clip(rint(x * (127 / amax)), -127, 127); an all-zero token gives x8 = 0 and scale 0.  Non-finite
    input raises ValueError."""
    x = np.asarray(arr, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("token embeddings: a [T, dim] array")
    if not np.isfinite(x).all():
        raise ValueError("token embeddings: non-finite value")
    amax = np.abs(x).max(axis=1) if x.shape[1] else np.zeros(x.shape[0], np.float32)
    amax = amax.astype(np.float32)
    scale = (amax / np.float32(127.0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        mul = np.where(amax > 0, np.float32(127.0) / amax, np.float32(0.0)).astype(np.float32)
    q = np.rint((x * mul[:, None]).astype(np.float32))
    x8 = np.clip(q, -127, 127).astype(np.int8)
    return x8, scale


def pad_dim(arr, dim: int) -> np.ndarray:
    """[T, d] -> [T, dim] float32, zero-padded on the right (no dot product changes); d > dim raises ValueError."""
    x = np.asarray(arr, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("token embeddings: a [T, dim] array")
    if x.shape[1] > dim:
        raise ValueError(f"token embeddings of {x.shape[1]} values for a token width of {dim}")
    if x.shape[1] == dim:
        return x
    out = np.zeros((x.shape[0], dim), np.float32)
    out[:, :x.shape[1]] = x
    return out


def pack_tokens(cells: Sequence[Optional[Tuple[np.ndarray, np.ndarray]]], dim: int, absent: int = MISSING):
    """Ragged quantised token lists as the engine takes them: cells[i] = None (a row without the vector: head `absent`)
    or (x8 [T, dim] int8, scales [T] float32), T >= 0.  Returns (heads [n] uint32, x8 [sum T, dim] int8, scales
    [sum T] float32, indptr [n + 1] int64 -- the first token of every cell)."""
    heads = np.empty(len(cells), np.uint32)
    xs: List[np.ndarray] = []
    ss: List[np.ndarray] = []
    indptr = np.zeros(len(cells) + 1, np.int64)
    for i, c in enumerate(cells):
        if c is None:
            heads[i] = absent
            indptr[i + 1] = indptr[i]
            continue
        x8, sc = np.asarray(c[0]), np.asarray(c[1])
        if x8.dtype != np.int8 or x8.ndim != 2 or x8.shape[1] != dim or sc.dtype != np.float32 or sc.shape != (x8.shape[0],):
            raise ValueError(f"cell {i}: want ([T, {dim}] int8, [T] float32)")
        heads[i] = x8.shape[0]
        indptr[i + 1] = indptr[i] + x8.shape[0]
        xs.append(x8)
        ss.append(sc)
    x8 = np.concatenate(xs, axis=0) if xs else np.zeros((0, dim), np.int8)
    sc = np.concatenate(ss) if ss else np.zeros((0,), np.float32)
    return heads, np.ascontiguousarray(x8), np.ascontiguousarray(sc), indptr


def pack_queries(queries, dim: int):
    """The query tokens of a batch: queries[b] = a [Tq, d <= dim] float array, 1 <= Tq <= 64.  Each is zero-padded to
    `dim` and quantised as stored tokens are.  Returns (x8 [sum Tq, dim] int8, scales float32, indptr [B + 1] int64)."""
    cells = []
    for b, q in enumerate(queries):
        x = pad_dim(q, dim)
        if not 1 <= x.shape[0] <= MAX_QTOKENS:
            raise ValueError(f"query {b}: a query holds 1 to {MAX_QTOKENS} tokens, got {x.shape[0]}")
        cells.append(quantize_tokens(x))
    _, x8, sc, indptr = pack_tokens(cells, dim)
    return x8, sc, indptr


def maxsim_scores(q8: np.ndarray, qscale: np.ndarray, rows) -> np.ndarray:
    """The MaxSim of one query (q8 [Tq, dim] int8, qscale [Tq] float32) against each of `rows` = (d8 [Td, dim] int8,
    dscale [Td] float32), Td >= 1, as include/hx.h states it: float32 [len(rows)]."""
    q8 = np.asarray(q8, np.int8)
    qscale = np.asarray(qscale, np.float32)
    tq = q8.shape[0]
    if not 1 <= tq <= MAX_QTOKENS:
        raise ValueError(f"a query holds 1 to {MAX_QTOKENS} tokens")
    out = np.empty(len(rows), np.float32)
    qi = q8.astype(np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        for n, (d8, dscale) in enumerate(rows):
            d8 = np.asarray(d8, np.int8)
            if d8.shape[0] < 1:
                raise ValueError("a row without tokens has no score")
            dots = (qi @ d8.astype(np.int32).T).astype(np.float32)          # exact: |I| < 2^24
            m = (dots * np.asarray(dscale, np.float32)[None, :]).max(axis=1)
            a = np.zeros(MAX_QTOKENS, np.float32)
            a[:tq] = m * qscale
            while a.shape[0] > 1:
                a = a[0::2] + a[1::2]
            out[n] = a[0] + np.float32(0.0)
    return out
