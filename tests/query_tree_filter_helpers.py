"""Shared by the node-filter tests of the query trees: the oracle's stage interface extended by
masks and the list-filtering stage, the scalar model of hx_list_keep, a recorder that also keeps the new nodes, and the
CSR of a subset of rows.  A plain helper module: nothing here is collected as a test."""
from __future__ import annotations

import struct

import numpy as np

from oracle import oracle as O
from tests.query_tree_helpers import OracleStages, Recorder, key_ids


def key_scores(keys) -> np.ndarray:
    """the fp32 scores the keys carry (hx_common.hpp: orderable_f32 of the high word)"""
    u = (np.asarray(keys, dtype=np.uint64) >> np.uint64(32)).astype(np.uint32)
    bits = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u)
    return bits.astype(np.uint32).view(np.float32)


def csr_rows(ip, si, sv, rows):
    """the CSR of the listed rows, in their order"""
    lens = (ip[1:] - ip[:-1])[rows]
    nip = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=nip[1:])
    take = np.concatenate([np.arange(ip[r], ip[r + 1]) for r in rows]) if len(rows) else np.zeros(0, np.int64)
    return nip, si[take].astype(np.int64), sv[take].astype(np.float32)


def sub_oracle(rows, dim, msizes, kept):
    """The contract of DESIGN.md section 13: an OracleIndex holding only the kept rows, added in their order."""
    X, ip, si, sv = rows
    ora = O.OracleIndex(dim, msizes)
    ora.add(X[kept], *csr_rows(ip, si, sv, kept))
    ora.finalize()
    return ora


def _score(k: int) -> float:
    u = k >> 32
    bits = (u & 0x7FFFFFFF) if u & 0x80000000 else (~u & 0xFFFFFFFF)
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def list_keep_model(keys, counts, limit, keep_row=None, thresholds=None, id_of=None):
    """hx_list_keep, one slot at a time, in Python integers.  keys uint64 [B, stride]; counts [B] or None; keep_row: a
    bool array over this index's rows, or None; id_of(global id) -> this index's row or -1 (None: ids are rows);
    thresholds float32 [B] or None (two fp32 values compare as doubles exactly as they compare in fp32).  Returns (out
    uint64 [B, limit], counts int32 [B])."""
    keys = np.asarray(keys, dtype=np.uint64)
    B, stride = keys.shape
    out = np.zeros((B, limit), dtype=np.uint64)
    cnt = np.zeros(B, dtype=np.int32)
    kept_rows = None if keep_row is None else np.asarray(keep_row, dtype=bool).tolist()
    for b in range(B):
        n = stride if counts is None else min(max(int(counts[b]), 0), stride)
        thr = None if thresholds is None else float(np.float32(thresholds[b]))
        w = 0
        for k in keys[b, :n].tolist():
            if w == limit:
                break
            if k == 0:
                continue
            if kept_rows is not None:
                gid = 0xFFFFFFFF - (k & 0xFFFFFFFF)
                row = gid if id_of is None else id_of(gid)
                if not 0 <= row < len(kept_rows) or not kept_rows[row]:
                    continue
            if thr is not None and _score(k) < thr:
                continue
            out[b, w] = k
            w += 1
        cnt[b] = w
    return out, cnt


class FilteredOracleStages(OracleStages):
    """OracleStages with masks: per mask an OracleIndex of the kept rows, ids mapped back through the ascending list of
    kept rows; keep() is list_keep_model.  rows = (X, indptr, idx, val); masks = {filter key: bool array over the rows}."""

    def __init__(self, rows, dim, msizes, masks, fuse=None, ix=None):
        from tests.query_tree_helpers import oracle_index
        super().__init__(oracle_index(rows, dim, msizes) if ix is None else ix, fuse)
        self.masks = {k: np.asarray(m, dtype=bool) for k, m in masks.items()}
        self.kept = {k: np.flatnonzero(m) for k, m in self.masks.items()}
        self.sub = {k: sub_oracle(rows, dim, msizes, kept) if len(kept) else None for k, kept in self.kept.items()}

    def _masked(self, mask, limit, per_query):
        kept, sub = self.kept[mask], self.sub[mask]
        if sub is None:
            return self._pack([(np.zeros(0, np.float32), np.zeros(0, np.int64))] * per_query[0], limit)
        return self._pack([(sc, kept[np.asarray(ids, dtype=np.int64)]) for sc, ids in per_query[1](sub)], limit)

    def dense(self, Q, limit, prefix, mask=None):
        if mask is None:
            return super().dense(Q, limit, prefix)
        self.calls.append(("dense", Q.shape[0], limit, prefix, mask))
        return self._masked(mask, limit, (len(Q), lambda ix: [ix.search_dense(q, limit, prefix) for q in Q]))

    def i8(self, Q, limit, mask=None):
        if mask is None:
            return super().i8(Q, limit)
        self.calls.append(("i8", Q.shape[0], limit, mask))
        return self._masked(mask, limit, (len(Q), lambda ix: [ix.search_i8(q, limit) for q in Q]))

    def sparse(self, pairs, limit, mask=None):
        if mask is None:
            return super().sparse(pairs, limit)
        self.calls.append(("sparse", len(pairs), limit, mask))
        return self._masked(mask, limit, (len(pairs), lambda ix: [ix.search_sparse(i, v, limit) for i, v in pairs]))

    def keep(self, lists, mask, thresholds, limit):
        if isinstance(lists, tuple):
            keys, counts = lists
        else:                                                # side by side: a stage's slots past its count are 0
            keys, counts = np.concatenate([k for k, _ in lists], axis=1), None
        self.calls.append(("keep", keys.shape[0], limit, mask, thresholds is not None))
        return list_keep_model(keys, counts, limit, None if mask is None else self.masks[mask], thresholds)


class FilterRecorder(Recorder):
    """Recorder that also keeps the masked leaves and the keep nodes."""

    def dense(self, Q, limit, prefix, **kw):
        return self._keep("dense", dict(limit=limit, prefix=prefix, **kw), self.stages.dense(Q, limit, prefix, **kw))

    def i8(self, Q, limit, **kw):
        return self._keep("i8", dict(limit=limit, **kw), self.stages.i8(Q, limit, **kw))

    def sparse(self, pairs, limit, **kw):
        return self._keep("sparse", dict(limit=limit, terms=[len(i) for i, _ in pairs], **kw),
                          self.stages.sparse(pairs, limit, **kw))

    def keep(self, lists, mask, thresholds, limit):
        one = isinstance(lists, tuple)
        asked = dict(limit=limit, mask=mask, thresholds=None if thresholds is None else np.asarray(thresholds).tolist(),
                     strides=[int(lists[0].shape[1])] if one else [int(k.shape[1]) for k, _ in lists])
        return self._keep("keep", asked, self.stages.keep(lists, mask, thresholds, limit))

    def begin_run(self):
        begin = getattr(self.stages, "begin_run", None)
        if begin is not None:
            begin()
