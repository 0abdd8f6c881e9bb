"""Shared by the tests of the asymmetric binary stage: the numpy model of the query codes, of their
bit planes and of the stage, and the oracle's stage set extended by `bin_asym`.  A plain helper module: nothing here is
collected as a test.

The model: per query, m = max |q|, code = rint(fp32(fp32(q / m) * QMAX)) with QMAX = 2^(bits-1) - 1 (np.rint rounds half
to even; m == 0 gives zeros); row bits = tests/binary_helpers.row_bits; score = sum_j code_j * (bit_j ? +1 : -1) as fp32
-- an fp32 matrix product of integers whose every partial sum is below 2^24, so it is exact -- and the best `limit` by
oracle.topk: score descending, id ascending; a mask restricts the rows."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from tests import binary_helpers as BH

QMAX = {4: 7, 8: 127}


def codes(Q, qmax) -> np.ndarray:
    """int32 [B, dim]: one fp32 division, one fp32 multiplication, round half to even"""
    Q = np.atleast_2d(np.ascontiguousarray(Q, dtype=np.float32))
    m = np.abs(Q).max(axis=1, keepdims=True) if Q.shape[1] else np.zeros((Q.shape[0], 1), np.float32)
    safe = np.where(m > 0, m, np.float32(1)).astype(np.float32)
    d = (Q / safe).astype(np.float32)
    t = (d * np.float32(qmax)).astype(np.float32)
    return np.where(m > 0, np.rint(t), 0).astype(np.int32)


def planes(c, P) -> np.ndarray:
    """int32 codes [B, dim] -> uint32 [B, P, dim_pad / 32]: bit j & 31 of word j >> 5 of plane k = bit k of the two's
    complement of code j"""
    c = np.atleast_2d(np.asarray(c, dtype=np.int32))
    return np.stack([np.stack([BH.words(((c[b] >> k) & 1).astype(bool)[None, :])[0] for k in range(P)])
                     for b in range(c.shape[0])])


def unplanes(pl, dim) -> np.ndarray:
    """the codes the planes hold: the top plane weighs -2^(P-1)"""
    pl = np.asarray(pl, dtype=np.uint32)
    B, P, W = pl.shape
    bits = np.unpackbits(pl.view(np.uint8).reshape(B, P, W * 4), axis=-1, bitorder="little")[:, :, :dim].astype(np.int32)
    w = np.array([1 << k for k in range(P - 1)] + [-(1 << (P - 1))], dtype=np.int32)
    return (bits * w[None, :, None]).sum(axis=1, dtype=np.int32)


def scores(xbits, c) -> np.ndarray:
    """fp32 [B, n]: codes @ (+-1 rows), exact; + 0 because an integer sum has no negative zero (0 * -1 is -0.0 in fp32)"""
    pm = (2 * np.asarray(xbits, dtype=bool).astype(np.int32) - 1).astype(np.float32)
    return np.atleast_2d(c).astype(np.float32) @ pm.T + np.float32(0)


def search(xbits, Q, limit, query_bits, mask=None, id_base=0, ids=None):
    """The stage: (keys uint64 [B, limit], counts int32 [B]), as binary_helpers.search returns them."""
    xb = np.asarray(xbits, dtype=bool)
    Q = np.atleast_2d(np.ascontiguousarray(Q, dtype=np.float32))
    rows = np.arange(xb.shape[0]) if mask is None else np.flatnonzero(np.asarray(mask, dtype=bool))
    gid = (id_base + rows if ids is None else np.asarray(ids, dtype=np.int64)[rows]).astype(np.int64)
    keys = np.zeros((Q.shape[0], limit), dtype=np.uint64)
    cnt = np.zeros(Q.shape[0], dtype=np.int32)
    if len(rows):
        S = scores(xb[rows], codes(Q, QMAX[query_bits]))
        for b in range(Q.shape[0]):
            sc, ids_b = O.topk(S[b], gid, limit)
            keys[b, :len(ids_b)] = O.order_key(sc, ids_b)
            cnt[b] = len(ids_b)
    return keys, cnt


class AsymOracleStages(BH.BinaryOracleStages):
    """BinaryOracleStages with `bin_asym` = the model above over the same rows."""

    def bin_asym(self, Q, limit, query_bits, mask=None):
        self.calls.append(("bin_asym", Q.shape[0], limit, query_bits) + (() if mask is None else (mask,)))
        return search(self.xbits, Q, limit, query_bits, None if mask is None else self.masks[mask])
