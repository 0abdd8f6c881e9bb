"""Host model of the discovery and context search (include/hx.h "discovery and context search"),
in numpy float32, on top of tests/reco_helpers.py: sim(x, e) = spec_dot(x, e), raw vectors through O.cosine_preprocess,
the key order of O.topk (score descending, id ascending).  Every operation is one fp32 operation; the device is held to
this model bit for bit."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from tests.reco_helpers import make_keys, spec_dot  # noqa: F401  (make_keys: re-exported for the tests)

F32 = np.float32
EPS = F32(2.0 ** -23)


def fast_sigmoid(v):
    """v / (1 + |v|): one fp32 add, one correctly rounded fp32 division"""
    v = np.asarray(v, F32)
    return (v / (F32(1.0) + np.abs(v)).astype(F32)).astype(F32)


def scores(rows, target, pairs):
    """the score of every row: rows [n, D] normalised; target a normalised vector [D] or None; pairs a sequence of
    (pos [D], neg [D]) normalised vectors"""
    rows = np.ascontiguousarray(rows, F32)
    n = rows.shape[0]
    if n == 0:
        return np.zeros(0, F32)
    acc = np.zeros(n, F32)
    if target is not None:                                  # discovery: every pair votes, the target breaks the rank's ties
        for pos, neg in pairs:
            sp, sn = spec_dot(rows, pos), spec_dot(rows, neg)
            c = np.where(sp > sn, F32(1.0), np.where(sp < sn, F32(-1.0), F32(0.0))).astype(F32)
            acc = (acc + c).astype(F32)
        t = (fast_sigmoid(spec_dot(rows, target)) + F32(1.0)).astype(F32)
        acc = (acc + (F32(0.5) * t).astype(F32)).astype(F32)
    else:                                                   # context: what a row lacks to each pair's positive side
        assert len(pairs) >= 1, "a context search needs a pair"
        for pos, neg in pairs:
            d = ((spec_dot(rows, pos) - spec_dot(rows, neg)).astype(F32) - EPS).astype(F32)
            acc = (acc + fast_sigmoid(np.where(d < 0, d, F32(0.0)).astype(F32))).astype(F32)
    return (acc + F32(0.0)).astype(F32)


def discover(rows, target, pairs, limit, excluded, ids=None):
    """(scores [k], ids [k]) of the best k = min(limit, rows not excluded) rows: score descending, id ascending"""
    n = len(rows)
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    keep = ~np.asarray(excluded, bool)
    if n == 0 or not keep.any():
        return np.zeros(0, F32), np.zeros(0, np.int64)
    s = scores(rows, target, pairs)
    return O.topk(s[keep], ids[keep], limit)


def request_model(Xn, request, limit, keep=None, ids=None):
    """One request as HxIndex.discover takes it -- (target | None, [(pos, neg), ...]), an example a local row or a raw
    vector -- over the normalised stored rows Xn: (keys [limit] uint64 with zeros past the count, count).  A stored row's
    vector is Xn[row], a raw vector goes through the query rule; the stored examples and the rows keep drops are excluded."""
    n = len(Xn)
    excluded = np.zeros(n, bool) if keep is None else ~np.asarray(keep, bool)

    def vec(e):
        if isinstance(e, (int, np.integer)):
            excluded[int(e)] = True
            return Xn[int(e)]
        return O.cosine_preprocess(np.asarray(e, F32))
    target, pairs = request
    t = None if target is None else vec(target)
    pv = [(vec(p), vec(q)) for p, q in pairs]
    sc, got = discover(Xn, t, pv, limit, excluded, ids)
    keys = np.zeros(limit, np.uint64)
    keys[:len(got)] = make_keys(sc, got)
    return keys, len(got)
