"""An independent restatement of hx_fuse's arithmetic contract (include/hx.h), written from the header: plain loops over
Python lists with np.float32 / np.float64 scalars, one IEEE operation per statement.  The oracle of
tests/test_fusion_host.py (against rag_application_amd/fusion.py) and of the GPU tests; nothing the product imports."""
from __future__ import annotations

import struct

import numpy as np

F32, F64 = np.float32, np.float64
RRF, DBSF = 0, 1


def make_key(score, pid: int) -> int:
    (u,) = struct.unpack("<I", struct.pack("<f", float(F32(score))))
    u = (~u) & 0xFFFFFFFF if u & 0x80000000 else u | 0x80000000
    return (u << 32) | (0xFFFFFFFF - int(pid))


def key_score(key: int) -> np.float32:
    u = (int(key) >> 32) & 0xFFFFFFFF
    u = u & 0x7FFFFFFF if u & 0x80000000 else (~u) & 0xFFFFFFFF
    return F32(struct.unpack("<f", struct.pack("<I", u))[0])


def key_id(key: int) -> int:
    return 0xFFFFFFFF - (int(key) & 0xFFFFFFFF)


def tree(values) -> np.float64:
    p = 1
    while p < len(values):
        p *= 2
    v = [F64(x) for x in values] + [F64(0.0)] * (p - len(values))
    h = p // 2
    while h >= 1:
        for i in range(h):
            v[i] = F64(v[i] + v[i + h])
        h //= 2
    return v[0]


def rrf_contributions(n, w, k, rank_base):
    out = []
    for r in range(n):
        x = F32(F32(r + rank_base) + F32(k))
        rcp = F32(F64(1.0) / F64(x))
        out.append(F32(F32(w) * rcp))
    return out


def dbsf_contributions(scores, w):
    n = len(scores)
    s = [F64(F32(x)) for x in scores]
    norm = [F32(0.5)] * n
    if n > 1:
        with np.errstate(all="ignore"):
            mean = F64(tree(s) / F64(n))
            sq = []
            for x in s:
                d = F64(x - mean)
                sq.append(F64(d * d))
            var = F64(tree(sq) / F64(n - 1))
            sd = F64(np.sqrt(var))
            if sd > 0:
                lo = F64(mean - F64(F64(3.0) * sd))
                den = F64(F64(6.0) * sd)
                norm = [F32(F64(F64(x - lo) / den)) for x in s]
    return [F32(F32(w) * x) for x in norm]


def fuse_query(lists, method, weights=None, limit=10, k=2.0, rank_base=0):
    """lists: [[key, ...]] of one query, best first (Python ints).  Returns the fused keys, best first, at most limit."""
    fused, order = {}, []
    for l, keys in enumerate(lists):
        w = F32(1.0) if weights is None else F32(weights[l])
        if method == RRF:
            c = rrf_contributions(len(keys), w, k, rank_base)
        else:
            c = dbsf_contributions([key_score(x) for x in keys], w)
        seen = set()
        for r, key in enumerate(keys):
            pid = key_id(key)
            if pid in seen:
                continue
            seen.add(pid)
            if pid not in fused:
                fused[pid] = F32(0.0)
                order.append(pid)
            fused[pid] = F32(fused[pid] + c[r])
    out = sorted((make_key(fused[pid], pid) for pid in order), reverse=True)
    return out[:limit]


def fuse_batch(keys, counts, method, weights=None, limit=10, k=2.0, rank_base=0):
    """keys[l] [B, stride_l] uint64, counts[l] [B] -> (keys [B, limit] uint64 0-padded, counts [B] int32)."""
    B = keys[0].shape[0]
    out = np.zeros((B, limit), dtype=np.uint64)
    cnt = np.zeros(B, dtype=np.int32)
    for b in range(B):
        lists = []
        for kk, cc in zip(keys, counts):
            n = min(max(int(cc[b]), 0), kk.shape[1])
            lists.append([int(x) for x in kk[b, :n]])
        f = fuse_query(lists, method, weights, limit, k, rank_base)
        for i, x in enumerate(f):
            out[b, i] = np.uint64(x)
        cnt[b] = len(f)
    return out, cnt


def random_lists(rng, B, strides, id_range, counts="mixed", ties="some", negative=True, replace=False):
    """Test data: per list [B, stride] uint64 keys sorted best first and [B] int32 counts.  ids drawn from [0, id_range)
    (replace: an id may repeat inside a list); scores from a coarse grid so that exact ties occur.  Slots past a count
    hold keys that must not be read."""
    keys, cnts = [], []
    for s in strides:
        k = np.zeros((B, s), dtype=np.uint64)
        c = np.zeros(B, dtype=np.int32)
        for b in range(B):
            if counts == "mixed":
                n = int(rng.choice([0, 1, 2, max(s - 1, 0), s, s, s]))
            else:
                n = s
            n = min(n, s) if replace else min(n, s, id_range)
            ids = rng.choice(id_range, size=n, replace=replace)
            if ties == "all":
                sc = np.full(n, 0.25, dtype=F32)
            else:
                sc = (rng.integers(-40 if negative else 0, 41, size=n).astype(F32) / F32(16.0)).astype(F32)
                if ties == "none":
                    sc = (sc + rng.random(n).astype(F32) * F32(0.01)).astype(F32)
            lst = sorted((make_key(x, i) for x, i in zip(sc, ids)), reverse=True)
            for j, x in enumerate(lst):
                k[b, j] = np.uint64(x)
            for j in range(n, s):                                # past the count: a top score, never to be read
                k[b, j] = np.uint64(make_key(1000.0, id_range + j))
            c[b] = n
        keys.append(k)
        cnts.append(c)
    return keys, cnts
