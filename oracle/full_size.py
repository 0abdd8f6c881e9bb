"""Chunked host reference over a corpus that is never resident at once.  TEST INFRASTRUCTURE ONLY.

Only ``tests/`` may import this module; the product and ``bench.py`` never do.

The synthetic corpus can be regenerated at any row (``CO.synth_dense`` / ``CO.synth_sparse_docs``), so the lists of every
stage of the reference query over 10M rows need no resident copy: ONE pass over the rows, chunk by chunk, gives each
query of a fixed sample its merged top-``Lmax`` list of every whole-collection stage --

    "dense"           full-vector dense cosine            (OracleIndex.search_dense, prefix 0)
    "m64" / "m128" /  prefix-d dense cosine               (OracleIndex.search_dense, prefix d)
    "i8"              the int8 ``quantized`` vector       (OracleIndex.search_i8)
    "sparse"          the sparse vector                   (OracleIndex.search_sparse)

-- every chunk's list computed by the C restatement with ``id_base`` = the chunk's first row and merged under the total
order (score desc, id asc).  A top-L list is then the first L entries of the top-``Lmax`` one.  The composed queries
(``tree``: O.hybrid_tree step for step; ``h1``: O.hybrid_h1) regenerate only the candidate rows they re-score, by id.

On any corpus that fits in memory the lists are the bits of O.OracleIndex / O.hybrid_tree / O.hybrid_h1
(tests/test_full_size_reference.py checks that, chunk boundaries cutting through tie runs and top lists)."""
from __future__ import annotations

import os
import time

import numpy as np

from . import c_oracle as CO
from . import oracle as O

F32 = np.float32


class SynthSource:
    """The synthetic corpus of SURVEY.md §8(d): rows [0, n), regenerated wherever they are asked for."""

    def __init__(self, n, dim, tables, seed_dense=O.SEED_CORPUS, seed_sparse=O.SEED_SPDOC):
        self.n, self.dim, self.tables = int(n), int(dim), tables
        self.seed_dense, self.seed_sparse = seed_dense, seed_sparse

    def dense(self, r0, n):
        return CO.synth_dense(self.seed_dense, r0, n, self.dim)

    def sparse(self, r0, n):
        return CO.synth_sparse_docs(self.seed_sparse, r0, n, self.tables)

    def rows(self, ids):
        out = np.empty((len(ids), self.dim), F32)
        for k, r in enumerate(np.asarray(ids, np.int64).tolist()):
            out[k] = CO.synth_dense(self.seed_dense, r, 1, self.dim)[0]
        return out


class ArraySource:
    """Rows held in host memory (raw dense [n, dim], doc-major sparse CSR): the same interface as SynthSource."""

    def __init__(self, X, ip, si, sv):
        self.X, self.ip = np.ascontiguousarray(X, F32), np.asarray(ip, np.int64)
        self.si, self.sv = np.asarray(si), np.asarray(sv, F32)
        self.n, self.dim = self.X.shape

    def dense(self, r0, n):
        return self.X[r0:r0 + n]

    def sparse(self, r0, n):
        a, b = self.ip[r0], self.ip[r0 + n]
        return self.ip[r0:r0 + n + 1] - a, self.si[a:b], self.sv[a:b]

    def rows(self, ids):
        return self.X[np.asarray(ids, np.int64)]


def _merge(best, s, i, c, L):
    """Per query: top L of (the kept list) u (this chunk's list) under (score desc, id asc); ids never repeat."""
    out = []
    for b, (bs, bi) in enumerate(best):
        out.append(O.topk(np.concatenate([bs, s[b, :c[b]]]), np.concatenate([bi, i[b, :c[b]]]), L))
    return out


class FullSizeReference:
    """One pass over `source` for the queries `Q` (raw dense [nq, dim]) and `sparse_q` (CSR, ascending term ids per
    query): top-`limits[stage]` lists of every stage named in `limits` ("dense", "m<d>", "i8", "sparse").
    `drop_chunk`: skip that chunk of the pass (a reference that MUST disagree: the tests' proof that they can fail)."""

    def __init__(self, source, Q, sparse_q, limits, chunk_rows=1_000_000, threads=None, drop_chunk=None):
        self.src = source
        self.dim = source.dim
        self.Q = np.ascontiguousarray(Q, F32)
        self.nq = self.Q.shape[0]
        self.qip, self.qix, self.qv = (np.asarray(sparse_q[0], np.int64), np.asarray(sparse_q[1], np.int32),
                                       np.asarray(sparse_q[2], F32))
        self.limits = dict(limits)
        self.msizes = sorted(int(k[1:]) for k in self.limits if k.startswith("m"))
        self.chunk_rows = int(chunk_rows)
        CO.set_num_threads(threads or min(16, os.cpu_count() or 1))
        # the query side, once: normalised full vector and prefixes, int8 copy
        self.qn = {0: CO.cosine_preprocess(self.Q)}
        for d in self.msizes:
            self.qn[d] = CO.cosine_preprocess(self.Q, d)
        self.q8, self.q8_rinv = CO.quantize_i8(self.Q)
        self._rows = {}
        self.chunks = 0
        t0 = time.perf_counter()
        self._pass(drop_chunk)
        self.seconds = time.perf_counter() - t0

    # ---- the pass ------------------------------------------------------------------------------------------------------
    def _pass(self, drop_chunk):
        empty = (np.zeros(0, F32), np.zeros(0, np.int64))
        best = {k: [empty] * self.nq for k in self.limits}
        n = self.src.n
        for k, r0 in enumerate(range(0, n, self.chunk_rows)):
            self.chunks += 1
            if k == drop_chunk:
                continue
            m = min(self.chunk_rows, n - r0)
            raw = self.src.dense(r0, m)
            if "dense" in self.limits:
                L = self.limits["dense"]
                best["dense"] = _merge(best["dense"], *CO.search_dense(CO.cosine_preprocess(raw), self.qn[0], L, r0), L)
            for d in self.msizes:
                L = self.limits[f"m{d}"]
                best[f"m{d}"] = _merge(best[f"m{d}"], *CO.search_dense(CO.cosine_preprocess(raw, d), self.qn[d], L, r0), L)
            if "i8" in self.limits:
                L = self.limits["i8"]
                x8, rx = CO.quantize_i8(raw)
                best["i8"] = _merge(best["i8"], *CO.search_i8(x8, rx, self.q8, self.q8_rinv, L, r0), L)
            del raw
            if "sparse" in self.limits:
                L = self.limits["sparse"]
                ip, si, sv = self.src.sparse(r0, m)
                best["sparse"] = _merge(best["sparse"],
                                        *CO.sparse_brute(ip, si, sv, self.qip, self.qix, self.qv, L, r0), L)
        self.lists = best

    # ---- whole-collection stages ---------------------------------------------------------------------------------------
    def stage(self, name, b, L):
        """(scores, ids) of query b's top-L list of stage `name`: a prefix of the pass's top-Lmax list."""
        assert L <= self.limits[name], f"{name}: limit {L} above the pass's {self.limits[name]}"
        s, i = self.lists[name][b]
        return s[:L], i[:L]

    def dense(self, b, L, prefix=0):
        return self.stage(f"m{prefix}" if prefix else "dense", b, L)

    def i8(self, b, L):
        return self.stage("i8", b, L)

    def sparse(self, b, L):
        return self.stage("sparse", b, L)

    # ---- candidate re-scoring: only the candidate rows, regenerated by id ---------------------------------------------
    def _raw_rows(self, ids):
        miss = [r for r in ids.tolist() if r not in self._rows]
        if miss:
            for r, x in zip(miss, self.src.rows(np.asarray(miss, np.int64))):
                self._rows[r] = x
        return np.stack([self._rows[r] for r in ids.tolist()]) if len(ids) else np.zeros((0, self.dim), F32)

    def rescore(self, b, cand, L, prefix=0):
        """OracleIndex.rescore: the distinct candidates re-scored with one named vector, top L."""
        u = np.unique(np.asarray(cand, np.int64))
        if len(u) == 0:
            return np.zeros(0, F32), np.zeros(0, np.int64)
        Xn = CO.cosine_preprocess(self._raw_rows(u), prefix or self.dim)
        # positions stand in for the ids: u ascends, so (score desc, position asc) is (score desc, id asc)
        s, pos = CO.rescore(Xn, self.qn[prefix][b], np.arange(len(u), dtype=np.int64), L)
        return s, u[pos]

    # ---- composed queries ----------------------------------------------------------------------------------------------
    def tree(self, b, params):
        """O.hybrid_tree step for step."""
        m = self.msizes
        limits = [params[f"matryoshka_{d}_limit"] for d in m]
        _, c = self.dense(b, limits[0], prefix=m[0])
        for d, lim in zip(m[1:], limits[1:]):
            _, c = self.rescore(b, c, lim, prefix=d)
        _, cand_a = self.rescore(b, c, params["dense_limit"])
        _, cq = self.i8(b, params["quantized_limit"])
        _, cand_q = self.rescore(b, cq, params["dense_limit"])
        _, cand_s = self.sparse(b, params["sparse_limit"])
        _, cand_r = CO.rrf(cand_q, cand_s, O.RRF_K, O.RRF_RANK_BASE, O.PREFETCH_DEFAULT_LIMIT)
        return self.rescore(b, np.concatenate([cand_a, cand_r]), params["final_limit"])

    def h1(self, b, dense_limit=100, sparse_limit=100, limit=10):
        """O.hybrid_h1: dense top-L (+) sparse top-L -> RRF -> top `limit` (RRF scores)."""
        _, cd = self.dense(b, dense_limit)
        _, cs = self.sparse(b, sparse_limit)
        return CO.rrf(cd, cs, O.RRF_K, O.RRF_RANK_BASE, limit)
