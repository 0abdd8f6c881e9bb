"""Shared by the binary-quantization tests: the host model of the 1-bit copy and of the Hamming
scan stage in numpy, the comparison of a device list with it, and the oracle's stage set extended by `bin`.  A plain
helper module: nothing here is collected as a test.

The model: row bits = oracle.cosine_preprocess(X) > 0 (the STORED normalised value), query bits = the raw query > 0,
score = dim - 2 popcount(xor) as fp32, the best `limit` by oracle.topk -- score descending, id ascending; a mask restricts
the rows."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from tests.query_tree_filter_helpers import FilteredOracleStages, FilterRecorder


def row_bits(X) -> np.ndarray:
    """bool [n, dim]: the sign bits of the stored rows"""
    X = np.ascontiguousarray(X, dtype=np.float32)
    return O.cosine_preprocess(X) > 0 if len(X) else np.zeros(X.shape, bool)


def query_bits(Q) -> np.ndarray:
    return np.ascontiguousarray(Q, dtype=np.float32) > 0


def words(bits) -> np.ndarray:
    """bool [n, dim] -> uint32 [n, dim_pad / 32] (dim_pad = dim rounded up to 64): bit j & 31 of word j >> 5"""
    bits = np.atleast_2d(np.asarray(bits, dtype=bool))
    n, dim = bits.shape
    pad = np.zeros((n, (dim + 63) // 64 * 64), dtype=bool)
    pad[:, :dim] = bits
    return np.packbits(pad.reshape(n, -1, 32), axis=-1, bitorder="little").view(np.uint32).reshape(n, -1)


def scores(xbits, qbits) -> np.ndarray:
    """fp32 [B, n]: dim - 2 * (differing bits), exact integers"""
    xb, qb = np.asarray(xbits, dtype=bool), np.atleast_2d(np.asarray(qbits, dtype=bool))
    dim = xb.shape[1]
    # differing bits = |x| + |q| - 2 x.q; the product of 0 / 1 values in fp32 is exact (sums below 2^24)
    both = (qb.astype(np.float32) @ xb.astype(np.float32).T).astype(np.int32)
    diff = xb.sum(axis=1, dtype=np.int32)[None, :] + qb.sum(axis=1, dtype=np.int32)[:, None] - 2 * both
    return (dim - 2 * diff).astype(np.float32)


def search(xbits, Q, limit, mask=None, id_base=0, ids=None):
    """The stage: (keys uint64 [B, limit], counts int32 [B]).  mask: a bool array over the rows, or None; ids: the
    rows' global ids (default id_base + row)."""
    xb = np.asarray(xbits, dtype=bool)
    Q = np.atleast_2d(np.ascontiguousarray(Q, dtype=np.float32))
    rows = np.arange(xb.shape[0]) if mask is None else np.flatnonzero(np.asarray(mask, dtype=bool))
    gid = (id_base + rows if ids is None else np.asarray(ids, dtype=np.int64)[rows]).astype(np.int64)
    keys = np.zeros((Q.shape[0], limit), dtype=np.uint64)
    cnt = np.zeros(Q.shape[0], dtype=np.int32)
    if len(rows):
        S = scores(xb[rows], query_bits(Q))
        for b in range(Q.shape[0]):
            sc, ids_b = O.topk(S[b], gid, limit)
            keys[b, :len(ids_b)] = O.order_key(sc, ids_b)
            cnt[b] = len(ids_b)
    return keys, cnt


def cut(lists, B, limit):
    """The lists of the first B queries at a shorter or longer limit: a ranked list's prefix is the shorter list, and a
    limit above the list's length pads with empty slots (lists = search(...) at a limit of at least min(limit, rows))."""
    keys, cnt = lists
    out = np.zeros((B, limit), dtype=np.uint64)
    w = min(limit, keys.shape[1])
    out[:, :w] = keys[:B, :w]
    return out, np.minimum(cnt[:B], limit).astype(np.int32)


def assert_same_lists(got, want, what=""):
    """A device list against the model, key for key: ids and fp32 score bits of the first `count` slots, the counts, and
    zero slots behind the count."""
    gk, gc = (np.asarray(a) for a in got)
    wk, wc = want
    gk = gk.view(np.uint64)
    assert gk.shape == wk.shape, f"{what}: shape {gk.shape}, want {wk.shape}"
    assert gc.tolist() == wc.tolist(), f"{what}: counts {gc.tolist()}, want {wc.tolist()}"
    if not np.array_equal(gk, wk):
        b, s = (int(x[0]) for x in np.nonzero(gk != wk))
        raise AssertionError(f"{what}: query {b} slot {s} of count {int(wc[b])}: key {int(gk[b, s]):#018x}, want "
                             f"{int(wk[b, s]):#018x} ({int((gk != wk).sum())} slots differ)")
    for b in range(wk.shape[0]):
        assert not gk[b, int(wc[b]):].any(), f"{what}: query {b}: a slot behind the count is not zero"


class BinaryOracleStages(FilteredOracleStages):
    """The oracle's stages (masks and keep included) with `bin` = the model above over the same rows."""

    def __init__(self, rows, dim, msizes, masks=None, fuse=None, ix=None):
        super().__init__(rows, dim, msizes, masks or {}, fuse=fuse, ix=ix)
        self.xbits = row_bits(rows[0])

    def bin(self, Q, limit, mask=None):
        self.calls.append(("bin", Q.shape[0], limit) + (() if mask is None else (mask,)))
        return search(self.xbits, Q, limit, None if mask is None else self.masks[mask])


class BinaryRecorder(FilterRecorder):
    def bin(self, Q, limit, **kw):
        return self._keep("bin", dict(limit=limit, **kw), self.stages.bin(Q, limit, **kw))
