"""Host model of the recommend search (include/hx.h "recommend search"), in numpy float32.

sim(x, e) = spec_dot(x, e): zero-pad to a multiple of 64, lane l of 64 accumulates x[64 j + l] * e[64 j + l] for ascending
j from +0 (fp32 multiply, fp32 add, nothing fused), the lanes fold by off = 32 .. 1, + 0.0f -- the reshape of DESIGN.md
section 2.  The three strategies, the example-order sums and the key order (score descending, id ascending) are restated
here; the device is held to this model bit for bit."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

F32 = np.float32
AVERAGE, BEST_SCORE, SUM_SCORES = 0, 1, 2
NEG_INF = F32(-np.inf)


def pad64(a):
    a = np.ascontiguousarray(a, dtype=F32)
    d = a.shape[-1]
    dp = (d + 63) // 64 * 64
    if dp == d:
        return a
    out = np.zeros(a.shape[:-1] + (dp,), F32)
    out[..., :d] = a
    return out


def spec_dot(X, e):
    """X [n, D], e [D] -> [n] float32"""
    X, e = pad64(X), pad64(e)
    n, dp = X.shape
    Xr, er = X.reshape(n, dp // 64, 64), e.reshape(dp // 64, 64)
    p = np.zeros((n, 64), F32)
    for j in range(dp // 64):
        p = p + Xr[:, j, :] * er[j][None, :]
    for off in (32, 16, 8, 4, 2, 1):
        p = p[:, :off] + p[:, off:2 * off]
    return (p[:, 0] + F32(0.0)).astype(F32)


def example_mean(E):
    """(((e_0 + e_1) + ...) + e_{k-1}) / f32(k), element by element"""
    m = E[0].astype(F32).copy()
    for e in E[1:]:
        m = (m + e).astype(F32)
    return (m / F32(len(E))).astype(F32)


def average_query(examples, signs):
    """the raw dense query of the average strategy: p + (p - n), or p without a negative"""
    signs = np.asarray(signs)
    P, N = examples[signs == 1], examples[signs == -1]
    assert len(P) >= 1, "the average strategy needs a positive"
    pm = example_mean(P)
    if len(N) == 0:
        return pm
    nm = example_mean(N)
    return (pm + (pm - nm).astype(F32)).astype(F32)


def scores(rows, examples, signs, strategy):
    """the score of every row: rows [n, D] normalised, examples [E, D] normalised, signs [E] of +1 | -1"""
    rows = np.ascontiguousarray(rows, F32)
    examples = np.ascontiguousarray(examples, F32).reshape(len(signs), -1)
    signs = np.asarray(signs)
    n = rows.shape[0]
    if n == 0:
        return np.zeros(0, F32)
    if strategy == AVERAGE:
        q = average_query(examples, signs)
        assert np.isfinite(q).all()
        return spec_dot(rows, O.cosine_preprocess(q))
    pos = [spec_dot(rows, e) for e in examples[signs == 1]]
    neg = [spec_dot(rows, e) for e in examples[signs == -1]]
    if strategy == BEST_SCORE:
        sp = np.full(n, NEG_INF, F32)
        sm = np.full(n, NEG_INF, F32)
        for s in pos:
            sp = np.maximum(sp, s)
        for s in neg:
            sm = np.maximum(sm, s)
        with np.errstate(invalid="ignore", over="ignore"):
            out = np.where(sp > sm, sp, -(sm * sm).astype(F32)).astype(F32)
        return (out + F32(0.0)).astype(F32)
    assert strategy == SUM_SCORES
    acc = np.zeros(n, F32)
    for s in pos:
        acc = (acc + s).astype(F32)
    for s in neg:
        acc = (acc - s).astype(F32)
    return (acc + F32(0.0)).astype(F32)


def recommend(rows, examples, signs, strategy, limit, excluded, ids=None):
    """(scores [k], ids [k]) of the best k = min(limit, rows not excluded) rows: score descending, id ascending.
    excluded: bool [n]; ids: the rows' global ids (None: the row numbers)."""
    n = len(rows)
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    keep = ~np.asarray(excluded, bool)
    if n == 0 or not keep.any():
        return np.zeros(0, F32), np.zeros(0, np.int64)
    s = scores(rows, examples, signs, strategy)
    return O.topk(s[keep], ids[keep], limit)


def make_keys(sc, ids):
    """the engine's keys (hx.h): orderable(score) << 32 | (0xFFFFFFFF - id)"""
    u = np.asarray(sc, F32).view(np.uint32).astype(np.uint64)
    o = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return (o << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(ids, np.uint64))


def request_model(Xn, request, strategy, limit, keep=None, ids=None):
    """One request as HxIndex.recommend takes it -- [(local row | vector, sign)] -- over the normalised stored rows Xn:
    (keys [limit] uint64 with zeros past the count, count).  A stored row's vector is Xn[row], a raw vector goes through
    the query rule (cosine_preprocess); the stored examples and the rows keep drops are excluded."""
    n = len(Xn)
    excluded = np.zeros(n, bool) if keep is None else ~np.asarray(keep, bool)
    ex, signs = [], []
    for e, sign in request:
        if isinstance(e, (int, np.integer)):
            excluded[int(e)] = True
            ex.append(Xn[int(e)])
        else:
            ex.append(O.cosine_preprocess(np.asarray(e, F32)))
        signs.append(sign)
    sc, got = recommend(Xn, np.stack(ex), signs, strategy, limit, excluded, ids)
    keys = np.zeros(limit, np.uint64)
    keys[:len(got)] = make_keys(sc, got)
    return keys, len(got)
