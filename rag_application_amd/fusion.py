"""The host model of hx_fuse (include/hx.h states the arithmetic): N ranked lists -> one, by
weighted reciprocal-rank fusion or by distribution-based score fusion, in numpy, bit for bit what the kernel computes.
It validates what the product hands the engine (the refusals are the entry's) and is the model its tests compare
against.  Lists travel as the engine's 64-bit keys (score in the high word, 0xFFFFFFFF - id in the low one)."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

F32, F64 = np.float32, np.float64
RRF, DBSF = 0, 1
METHODS = {"rrf": RRF, "dbsf": DBSF}
MAX_LISTS = 8
MAX_SLOTS = 4096
MAX_STRIDE = 2048
MAX_LIMIT = 2048
RRF_K = 2.0
RRF_RANK_BASE = 0
RRF_RANK_BASE_MAX = 1 << 30


# -- keys -------------------------------------------------------------------------------------------------------------
def make_keys(scores, ids) -> np.ndarray:
    """uint64 keys whose descending order is (score descending, id ascending)."""
    u = np.ascontiguousarray(scores, dtype=F32).view(np.uint32).astype(np.uint64)
    u = np.where(u & np.uint64(0x80000000), (~u) & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    return (u << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(ids).astype(np.uint64))


def key_scores(keys) -> np.ndarray:
    u = (np.asarray(keys).astype(np.uint64) >> np.uint64(32)).astype(np.uint32)
    u = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u)
    return np.ascontiguousarray(u, dtype=np.uint32).view(F32)


def key_ids(keys) -> np.ndarray:
    return (np.uint64(0xFFFFFFFF) - (np.asarray(keys).astype(np.uint64) & np.uint64(0xFFFFFFFF))).astype(np.int64)


# -- refusals ---------------------------------------------------------------------------------------------------------
def check_rrf(rrf_k, rank_base) -> None:
    k = F32(rrf_k)
    with np.errstate(all="ignore"):
        ok = bool(np.isfinite(k)) and k > 0 and bool(np.isfinite(F32(2.0 / float(k))))
    if not ok:
        raise ValueError("rrf_k must be finite and positive, with 2 / rrf_k finite")
    if isinstance(rank_base, bool) or int(rank_base) != rank_base or not 0 <= int(rank_base) <= RRF_RANK_BASE_MAX:
        raise ValueError("rrf_rank_base must be in [0, 2^30]")


def check(method, strides: Sequence[int], weights, limit, rrf_k=RRF_K, rank_base=RRF_RANK_BASE) -> Tuple[int, np.ndarray]:
    """What hx_fuse refuses, as ValueError.  Returns (method code, the float32 weights)."""
    if isinstance(method, str):
        if method not in METHODS:
            raise ValueError(f"fusion must be one of {tuple(METHODS)}, got {method!r}")
        method = METHODS[method]
    if method not in (RRF, DBSF):
        raise ValueError(f"unknown fusion method {method!r}")
    n = len(strides)
    if not 1 <= n <= MAX_LISTS:
        raise ValueError(f"a fusion takes 1 to {MAX_LISTS} lists, got {n}")
    for s in strides:
        if not 1 <= int(s) <= MAX_STRIDE:
            raise ValueError(f"a fused list holds 1 to {MAX_STRIDE} entries, got {s}")
    if sum(int(s) for s in strides) > MAX_SLOTS:
        raise ValueError(f"the fused lists hold more than {MAX_SLOTS} entries together")
    if isinstance(limit, bool) or int(limit) != limit or not 1 <= int(limit) <= MAX_LIMIT:
        raise ValueError(f"limit must be an integer in [1, {MAX_LIMIT}], got {limit!r}")
    if weights is None:
        w = np.ones(n, dtype=F32)
    else:
        try:
            with np.errstate(all="ignore"):
                w = np.asarray(list(weights), dtype=F64).astype(F32)
        except (TypeError, ValueError):
            raise ValueError("weights must be numbers") from None
        if w.ndim != 1 or w.shape[0] != n:
            raise ValueError(f"{n} lists need {n} weights, got {w.shape}")
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError("a weight must be finite and not negative")
    if method == RRF:
        check_rrf(rrf_k, rank_base)
    return method, w


# -- arithmetic -------------------------------------------------------------------------------------------------------
def tree_sum(v) -> np.float64:
    """T(v): v padded with +0.0 to the next power of two, then halves folded onto each other, fp64."""
    v = np.asarray(v, dtype=F64)
    p = 1
    while p < v.shape[0]:
        p <<= 1
    t = np.zeros(p, dtype=F64)
    t[:v.shape[0]] = v
    h = p >> 1
    while h >= 1:
        t[:h] = t[:h] + t[h:2 * h]
        h >>= 1
    return t[0]


def rrf_contrib(n: int, rrf_k=RRF_K, rank_base=RRF_RANK_BASE) -> np.ndarray:
    """1 / (f32(r + rank_base) + k) for r < n: the reciprocal through fp64, as the engine forms it."""
    x = ((np.arange(n, dtype=np.int64) + int(rank_base)).astype(F32) + F32(rrf_k)).astype(F32)
    with np.errstate(all="ignore"):
        return (F64(1.0) / x.astype(F64)).astype(F32)


def dbsf_norm(scores) -> np.ndarray:
    """The normalised scores of one list: (s - (mean - 3 sd)) / (6 sd) in fp64, rounded once to fp32; 0.5 for a list of
    one entry or without a positive standard deviation."""
    s = np.ascontiguousarray(scores, dtype=F32).astype(F64)
    n = s.shape[0]
    flat = np.full(n, 0.5, dtype=F32)
    if n <= 1:
        return flat
    with np.errstate(all="ignore"):
        mean = tree_sum(s) / F64(n)
        d = s - mean
        sd = np.sqrt(tree_sum(d * d) / F64(n - 1))
        if not sd > 0:
            return flat
        lo = mean - F64(3.0) * sd
        return ((s - lo) / (F64(6.0) * sd)).astype(F32)


def fuse_lists(lists, method=RRF, weights=None, limit: int = 10, rrf_k=RRF_K, rank_base=RRF_RANK_BASE):
    """One query.  lists: [(ids, scores)], best first (scores may be None for RRF).  Returns (scores, ids) of the fused
    list, at most `limit`.  No refusals here: see check()."""
    w = np.ones(len(lists), dtype=F32) if weights is None else np.asarray(weights, dtype=F32)
    ids_l, con_l = [], []
    for l, (ids, scores) in enumerate(lists):
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        n = ids.shape[0]
        c = rrf_contrib(n, rrf_k, rank_base) if method == RRF else dbsf_norm(np.asarray(scores, dtype=F32).reshape(-1)[:n])
        with np.errstate(all="ignore"):
            c = (w[l] * c).astype(F32)
        _, first = np.unique(ids, return_index=True)           # a list's first entry of an id counts
        first.sort()
        ids_l.append(ids[first])
        con_l.append(c[first])
    allids = np.unique(np.concatenate(ids_l)) if ids_l else np.zeros(0, np.int64)
    fused = np.zeros(allids.shape[0], dtype=F32)
    for ids, c in zip(ids_l, con_l):                           # ascending list order, one fp32 addition per list
        at = np.searchsorted(allids, ids)
        with np.errstate(all="ignore"):
            fused[at] = (fused[at] + c).astype(F32)
    keys = np.sort(make_keys(fused, allids))[::-1][:int(limit)]
    return key_scores(keys), key_ids(keys)


def fuse_keys(keys: Sequence[np.ndarray], counts: Sequence[np.ndarray], method=RRF, weights=None, limit: int = 10,
              rrf_k=RRF_K, rank_base=RRF_RANK_BASE):
    """hx_fuse on the host: keys[l] [B, stride_l] uint64 (or int64 holding the same bits), counts[l] [B].  Returns
    (keys [B, limit] uint64, 0-padded, counts [B] int32).  Raises ValueError for what hx_fuse refuses."""
    keys = [np.ascontiguousarray(k).view(np.uint64) if np.asarray(k).dtype == np.int64 else np.asarray(k, dtype=np.uint64)
            for k in keys]
    if len(keys) != len(counts):
        raise ValueError("one count array per list")
    method, w = check(method, [k.shape[1] for k in keys] if keys else [], weights, limit, rrf_k, rank_base)
    B = keys[0].shape[0]
    out = np.zeros((B, int(limit)), dtype=np.uint64)
    cnt = np.zeros(B, dtype=np.int32)
    for b in range(B):
        lists = []
        for k, c in zip(keys, counts):
            n = min(max(int(np.asarray(c)[b]), 0), k.shape[1])
            lists.append((key_ids(k[b, :n]), key_scores(k[b, :n])))
        sc, ids = fuse_lists(lists, method, w, limit, rrf_k, rank_base)
        out[b, :ids.shape[0]] = make_keys(sc, ids)
        cnt[b] = ids.shape[0]
    return out, cnt
