"""Thin Python face of libhx: one `HxIndex` = one user collection on one GPU.

torch is plumbing only (device buffers, the current stream); every computation is a
HIP kernel behind the C ABI of include/hx.h.  Ranked lists travel between stages as
int64 tensors holding the engine's 64-bit keys (see hx.h)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import HX_MODE_H1, HX_MODE_TREE, HxError, HxParams, HxProf, HxStats, check
from .filters import pack_rows

# payload index (hx.h): the column kinds; the cell codes and the ops of a program are in payload_index.py
PAY_U32, PAY_F64, PAY_LIST_U32, PAY_LIST_F64, PAY_TEXT = 1, 2, 3, 4, 5
PAY_TOKENS = 6                        # made by payload_create_tokens (hx.h: late-interaction rerank)
MAXSIM_MAX_QTOKENS = 64

SEARCH_PARAM_KEYS = ("matryoshka_64_limit", "matryoshka_128_limit", "matryoshka_256_limit",
                     "dense_limit", "quantized_limit", "sparse_limit", "final_limit", "hnsw_ef")


def make_params(search_params: dict, mode: int = HX_MODE_TREE, rrf_k: float = 2.0,
                rrf_rank_base: int = 0, rrf_limit: int = 10) -> HxParams:
    """search_params dict (hybrid_search_workflow.py:8-19) -> hx_params.  Indexes the
    dict unconditionally like the reference (qdrant_handler.py:314-369): a missing
    key raises KeyError, None raises TypeError."""
    p = HxParams()
    for k in SEARCH_PARAM_KEYS:
        setattr(p, k, int(search_params[k]))
    p.rrf_k = float(rrf_k)
    p.rrf_rank_base = int(rrf_rank_base)
    p.rrf_limit = int(rrf_limit)
    p.mode = int(mode)
    return p


def _ptr(t) -> int:
    if t is None:
        return 0
    if isinstance(t, torch.Tensor):
        return t.data_ptr()
    return t.ctypes.data


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need_cuda(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype):
        raise HxError(f"{name} must be a cuda tensor of dtype {dtype}")
    return t.contiguous()


class HxIndex:
    def __init__(self, dim: int = 768, matryoshka_sizes: Sequence[int] = (64, 128, 256),
                 device: int = 0, id_base: int = 0):
        self._h = C.c_void_p()
        self.dim = int(dim)
        self.msizes = tuple(int(m) for m in matryoshka_sizes)
        self.device = int(device)
        self.id_base = int(id_base)
        ms = (C.c_int32 * max(len(self.msizes), 1))(*self.msizes)
        check(_lib.lib().hx_create(self.dim, ms, len(self.msizes), self.device, self.id_base,
                                   C.byref(self._h)))
        self._tdev = torch.device("cuda", self.device)

    # -- persistence (hx.h: hx_save / hx_load) -----------------------------------------
    def save(self, path: str) -> None:
        check(_lib.lib().hx_save(self._h, str(path).encode()))

    @classmethod
    def load(cls, path: str, device: int = 0) -> "HxIndex":
        """A new index from a file written by save(): same rows, same search results bit for bit."""
        import struct
        with open(path, "rb") as f:
            head = f.read(8 + 6 * 4 + 4 * 8)
        magic, dim, n_pre, p0, p1, p2, _r, id_base, _n, _sr, _nnz = struct.unpack("<8s6i4q", head)
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        check(_lib.lib().hx_load(str(path).encode(), int(device), C.byref(self._h)))
        self.dim = int(dim)
        self.msizes = tuple(int(m) for m in (p0, p1, p2)[:n_pre])
        self.device = int(device)
        self.id_base = int(id_base)
        self._tdev = torch.device("cuda", self.device)
        return self

    # -- lifecycle -------------------------------------------------------------------
    def close(self):
        if self._h:
            check(_lib.lib().hx_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- ingest ----------------------------------------------------------------------
    def reserve(self, n_rows: int, nnz: int = 0):
        check(_lib.lib().hx_reserve(self._h, n_rows, nnz))

    def add(self, dense: np.ndarray, sp_indptr=None, sp_idx=None, sp_val=None):
        dense = np.ascontiguousarray(dense, dtype=np.float32)
        if dense.ndim != 2 or dense.shape[1] != self.dim:
            raise ValueError(f"Dense vector dimension mismatch. Expected {self.dim}, got {dense.shape[-1]}")
        n = dense.shape[0]
        if sp_indptr is None:
            sp_indptr = np.zeros(n + 1, dtype=np.int64)
            sp_idx = np.zeros(0, dtype=np.int32)
            sp_val = np.zeros(0, dtype=np.float32)
        sp_indptr = np.ascontiguousarray(sp_indptr, dtype=np.int64)
        sp_idx = np.ascontiguousarray(sp_idx, dtype=np.int32)
        sp_val = np.ascontiguousarray(sp_val, dtype=np.float32)
        if sp_indptr.shape[0] != n + 1:
            raise ValueError("sparse indptr must have n+1 entries")
        # dense and sparse vectors of a batch are committed together or not at all (hx_add_rows)
        check(_lib.lib().hx_add_rows(self._h, _ptr(dense), _ptr(sp_indptr), _ptr(sp_idx), _ptr(sp_val), n))

    def add_device(self, dense: torch.Tensor, sp_indptr=None, sp_idx=None, sp_val=None):
        """`add` for dense rows that already live on the GPU (an encoder's output): hx_add_dense_dev."""
        dense = _need_cuda(dense, torch.float32, "dense")
        if dense.ndim != 2 or dense.shape[1] != self.dim:
            raise ValueError(f"Dense vector dimension mismatch. Expected {self.dim}, got {dense.shape[-1]}")
        n = dense.shape[0]
        if sp_indptr is None:
            sp_indptr = np.zeros(n + 1, dtype=np.int64)
            sp_idx = np.zeros(0, dtype=np.int32)
            sp_val = np.zeros(0, dtype=np.float32)
        sp_indptr = np.ascontiguousarray(sp_indptr, dtype=np.int64)
        sp_idx = np.ascontiguousarray(sp_idx, dtype=np.int32)
        sp_val = np.ascontiguousarray(sp_val, dtype=np.float32)
        if sp_indptr.shape[0] != n + 1:
            raise ValueError("sparse indptr must have n+1 entries")
        # committed together or not at all, like `add` (hx_add_rows_dev)
        check(_lib.lib().hx_add_rows_dev(self._h, _ptr(dense), _ptr(sp_indptr), _ptr(sp_idx), _ptr(sp_val), n, _stream()))

    def set_next_id(self, first_id: int):
        """Row sharding: the next add's rows get the global ids first_id, first_id + 1, ... (hx_set_next_id)."""
        check(_lib.lib().hx_set_next_id(self._h, int(first_id)))

    def truncate(self, n_rows: int):
        """Roll back to the first n_rows rows (hx_truncate)."""
        check(_lib.lib().hx_truncate(self._h, int(n_rows)))

    def retain(self, keep) -> int:
        """Per-point delete (hx_retain_rows): keep only the rows of `keep` -- a bool array of length count() or packed
        uint32 words, as `_mask` takes them -- and compact the index on the device.  Returns the rows removed."""
        words, rows = self._mask(keep)
        removed = C.c_int64()
        check(_lib.lib().hx_retain_rows(self._h, _ptr(words), rows, C.byref(removed)))
        return removed.value

    @staticmethod
    def _rows(rows) -> np.ndarray:
        """the row list of a replace call: 1-d integers, unique (the engine checks the range)"""
        r = np.asarray(rows)
        if r.ndim != 1 or r.dtype.kind not in "iu":
            raise TypeError("rows: a 1-d integer array")
        r = np.ascontiguousarray(r, dtype=np.int64)
        if np.unique(r).shape[0] != r.shape[0]:
            raise ValueError("rows must be unique")
        return r

    def replace(self, rows, dense: np.ndarray, sp_indptr=None, sp_idx=None, sp_val=None):
        """Upsert by an existing id (hx_replace_rows): the stored rows `rows` (any order, unique) take the raw vectors
        `dense` [len(rows), dim] and the sparse vectors of the CSR, in that order, and stay where they are.
        sp_indptr None = their sparse vectors stay as they are.  All or nothing."""
        rows = self._rows(rows)
        dense = np.ascontiguousarray(dense, dtype=np.float32)
        if dense.ndim != 2 or dense.shape[1] != self.dim:
            raise ValueError(f"Dense vector dimension mismatch. Expected {self.dim}, got {dense.shape[-1]}")
        m = rows.shape[0]
        if dense.shape[0] != m:
            raise ValueError(f"{m} rows but {dense.shape[0]} dense vectors")
        if sp_indptr is None:
            if sp_idx is not None or sp_val is not None:
                raise ValueError("sparse indices / values without indptr")
            check(_lib.lib().hx_replace_rows(self._h, _ptr(rows), m, _ptr(dense), 0, 0, 0))
            return
        sp_indptr = np.ascontiguousarray(sp_indptr, dtype=np.int64)
        sp_idx = np.ascontiguousarray(sp_idx if sp_idx is not None else [], dtype=np.int32)
        sp_val = np.ascontiguousarray(sp_val if sp_val is not None else [], dtype=np.float32)
        if sp_indptr.shape[0] != m + 1:
            raise ValueError("sparse indptr must have n+1 entries")
        if m and (sp_idx.shape[0] < sp_indptr[-1] or sp_val.shape[0] < sp_indptr[-1]):
            raise ValueError("sparse indices / values are shorter than indptr says")
        check(_lib.lib().hx_replace_rows(self._h, _ptr(rows), m, _ptr(dense), _ptr(sp_indptr), _ptr(sp_idx), _ptr(sp_val)))

    def synth_fill(self, n: int, seed_dense: int, seed_sparse: int = 0, tables=None):
        if tables is not None:
            cdf = np.ascontiguousarray(tables[0], dtype=np.uint32)
            lens = np.ascontiguousarray(tables[1], dtype=np.uint16)
            check(_lib.lib().hx_synth_fill(self._h, n, seed_dense, seed_sparse, _ptr(cdf), cdf.shape[0],
                                           _ptr(lens), 1))
        else:
            check(_lib.lib().hx_synth_fill(self._h, n, seed_dense, 0, 0, 0, 0, 0))

    def finalize(self):
        check(_lib.lib().hx_finalize(self._h))

    def rebuild_sparse(self):
        """Build the inverted index again (hx_rebuild_sparse): a measurement aid."""
        check(_lib.lib().hx_rebuild_sparse(self._h))

    def count(self) -> int:
        n = C.c_int64()
        check(_lib.lib().hx_count(self._h, C.byref(n)))
        return n.value

    def stats(self) -> dict:
        s = HxStats()
        check(_lib.lib().hx_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in HxStats._fields_}

    def set_dense_candidates(self, kind: str):
        """'i8' (default) or 'f16': which copy nominates the dense stage's candidates (hx_set_dense_candidates)."""
        check(_lib.lib().hx_set_dense_candidates(self._h, {"f16": 0, "i8": 1}[kind]))

    def dense_candidates(self) -> str:
        """'i8' when the int8 copy nominates the dense candidates now, else 'f16' (hx_dense_candidates)."""
        k = C.c_int32()
        check(_lib.lib().hx_dense_candidates(self._h, C.byref(k)))
        return "i8" if k.value else "f16"

    def set_stream_overlap(self, on: bool):
        """False: every stage of a hybrid call on the caller's stream (a kernel's profiled duration is then its own)."""
        check(_lib.lib().hx_set_stream_overlap(self._h, 1 if on else 0))

    def profile(self, enable: bool):
        check(_lib.lib().hx_profile(self._h, 1 if enable else 0))

    def profile_read(self) -> dict:
        p = HxProf()
        check(_lib.lib().hx_profile_read(self._h, C.byref(p)))
        names = ("scan_f16", "scan_i8", "sparse", "scan_cand8", "prep_rows")
        return {n: dict(launches=p.launches[i], ms=p.ms[i], flops=p.flops[i], bytes=p.bytes[i])
                for i, n in enumerate(names)}

    def debug_row(self, which: int, row: int) -> np.ndarray:
        if which in (4, 5):
            out = np.zeros(self.dim, dtype=np.int8)
        elif which == 6:
            out = np.zeros(1, dtype=np.float32)
        elif which == 0:
            out = np.zeros(self.dim, dtype=np.float32)
        else:
            out = np.zeros(self.msizes[which - 1], dtype=np.float32)
        check(_lib.lib().hx_debug_row(self._h, which, row, _ptr(out)))
        return out

    # -- stages (device tensors) -----------------------------------------------------
    def _out(self, B: int, L: int):
        return (torch.empty((B, L), dtype=torch.int64, device=self._tdev),
                torch.empty((B,), dtype=torch.int32, device=self._tdev))

    # `flag` (a zeroed int32 device tensor of one element): the stage is only ENQUEUED -- no host round trip -- and
    # adds to flag[0] the number of queries whose lists are not final (hx_*_async); the caller reads the word once
    # behind all the stages of its query and redoes the batch without `flag` when it is not zero.
    deferred_stages = True

    # `mask` (None = every row; else as `_dev_mask` takes it): the stage over the rows the mask keeps (hx_search_*_masked) --
    # the list of an index holding only those rows, ids mapped back.  The deferred forms have no masked twin.
    @staticmethod
    def _no_masked_flag(mask, flag):
        if mask is not None and flag is not None:
            raise ValueError("mask and flag together: the deferred (flag=) stage forms have no masked twin")

    def search_dense(self, q: torch.Tensor, limit: int, prefix: int = 0, flag: Optional[torch.Tensor] = None, mask=None):
        HxIndex._no_masked_flag(mask, flag)
        q = _need_cuda(q, torch.float32, "q")
        keys, cnt = self._out(q.shape[0], limit)
        if mask is not None:
            words, rows = self._dev_mask(mask)
            check(_lib.lib().hx_search_dense_masked(self._h, _ptr(q), q.shape[0], prefix, limit, _ptr(words), rows,
                                                    _ptr(keys), _ptr(cnt), _stream()))
        elif flag is not None:
            check(_lib.lib().hx_search_dense_async(self._h, _ptr(q), q.shape[0], prefix, limit, _ptr(keys), _ptr(cnt),
                                                   _ptr(_need_cuda(flag, torch.int32, "flag")), _stream()))
        else:
            check(_lib.lib().hx_search_dense(self._h, _ptr(q), q.shape[0], prefix, limit, _ptr(keys), _ptr(cnt),
                                             _stream()))
        return keys, cnt

    def search_i8(self, q: torch.Tensor, limit: int, flag: Optional[torch.Tensor] = None, mask=None):
        HxIndex._no_masked_flag(mask, flag)
        q = _need_cuda(q, torch.float32, "q")
        keys, cnt = self._out(q.shape[0], limit)
        if mask is not None:
            words, rows = self._dev_mask(mask)
            check(_lib.lib().hx_search_i8_masked(self._h, _ptr(q), q.shape[0], limit, _ptr(words), rows, _ptr(keys),
                                                 _ptr(cnt), _stream()))
        elif flag is not None:
            check(_lib.lib().hx_search_i8_async(self._h, _ptr(q), q.shape[0], limit, _ptr(keys), _ptr(cnt),
                                                _ptr(_need_cuda(flag, torch.int32, "flag")), _stream()))
        else:
            check(_lib.lib().hx_search_i8(self._h, _ptr(q), q.shape[0], limit, _ptr(keys), _ptr(cnt), _stream()))
        return keys, cnt

    # -- binary quantization (hx.h: hx_binary_*, hx_search_bin) -----------------
    def binary_enable(self):
        """Keep a 1-bit copy of the rows from now on (hx_binary_enable; idempotent): search_bin needs it."""
        check(_lib.lib().hx_binary_enable(self._h))

    def binary_enabled(self) -> bool:
        on = C.c_int32()
        check(_lib.lib().hx_binary_enabled(self._h, C.byref(on)))
        return bool(on.value)

    def binary_row(self, row: int) -> np.ndarray:
        """The stored sign bits of one row (hx_binary_debug_row): dim rounded up to 64, / 32, uint32 words."""
        out = np.zeros((self.dim + 63) // 64 * 2, dtype=np.uint32)
        check(_lib.lib().hx_binary_debug_row(self._h, int(row), _ptr(out), out.shape[0]))
        return out

    def search_bin(self, q: torch.Tensor, limit: int, mask=None):
        """The Hamming scan stage (hx_search_bin): keys [B, limit] with the integer scores dim - 2 popcount(xor), counts."""
        q = _need_cuda(q, torch.float32, "q")
        keys, cnt = self._out(q.shape[0], limit)
        if mask is not None:
            words, rows = self._dev_mask(mask)
            check(_lib.lib().hx_search_bin_masked(self._h, _ptr(q), q.shape[0], limit, _ptr(words), rows, _ptr(keys),
                                                  _ptr(cnt), _stream()))
        else:
            check(_lib.lib().hx_search_bin(self._h, _ptr(q), q.shape[0], limit, _ptr(keys), _ptr(cnt), _stream()))
        return keys, cnt

    def search_bin_asym(self, q: torch.Tensor, limit: int, query_bits: int, mask=None):
        """The asymmetric stage over the 1-bit copy (hx_search_bin_asym): the query keeps query_bits
        = 4 or 8 bits per dimension; keys [B, limit] with the integer scores sum_j code_j * (+-1 of the row), counts."""
        q = _need_cuda(q, torch.float32, "q")
        keys, cnt = self._out(q.shape[0], limit)
        if mask is not None:
            words, rows = self._dev_mask(mask)
            check(_lib.lib().hx_search_bin_asym_masked(self._h, _ptr(q), q.shape[0], limit, int(query_bits), _ptr(words),
                                                       rows, _ptr(keys), _ptr(cnt), _stream()))
        else:
            check(_lib.lib().hx_search_bin_asym(self._h, _ptr(q), q.shape[0], limit, int(query_bits), _ptr(keys),
                                                _ptr(cnt), _stream()))
        return keys, cnt

    def binary_query_planes(self, q: torch.Tensor, query_bits: int):
        """What the asymmetric stage makes of a batch of queries (hx_bin_asym_debug_query): (planes uint32 [B, query_bits,
        dim rounded up to 64, / 32], totals int32 [B]) on the host -- bit j & 31 of word j >> 5 of plane k is bit k of
        the two's complement of column j's code."""
        q = _need_cuda(q, torch.float32, "q")
        B, P = q.shape[0], int(query_bits)
        planes = np.zeros((B, max(P, 0), (self.dim + 63) // 64 * 2), dtype=np.uint32)
        totals = np.zeros(B, dtype=np.int32)
        check(_lib.lib().hx_bin_asym_debug_query(self._h, _ptr(q), B, P, _ptr(planes), _ptr(totals), planes.size))
        return planes, totals

    def search_sparse(self, q_indptr: torch.Tensor, q_idx: torch.Tensor, q_val: torch.Tensor, limit: int,
                      flag: Optional[torch.Tensor] = None, mask=None):
        HxIndex._no_masked_flag(mask, flag)
        q_indptr = _need_cuda(q_indptr, torch.int64, "q_indptr")
        q_idx = _need_cuda(q_idx, torch.int32, "q_idx")
        q_val = _need_cuda(q_val, torch.float32, "q_val")
        B = q_indptr.shape[0] - 1
        keys, cnt = self._out(B, limit)
        if mask is not None:
            words, rows = self._dev_mask(mask)
            check(_lib.lib().hx_search_sparse_masked(self._h, _ptr(q_indptr), _ptr(q_idx), _ptr(q_val), B, limit,
                                                     _ptr(words), rows, _ptr(keys), _ptr(cnt), _stream()))
        elif flag is not None:
            check(_lib.lib().hx_search_sparse_async(self._h, _ptr(q_indptr), _ptr(q_idx), _ptr(q_val), B, limit,
                                                    _ptr(keys), _ptr(cnt), _ptr(_need_cuda(flag, torch.int32, "flag")),
                                                    _stream()))
        else:
            check(_lib.lib().hx_search_sparse(self._h, _ptr(q_indptr), _ptr(q_idx), _ptr(q_val), B, limit,
                                              _ptr(keys), _ptr(cnt), _stream()))
        return keys, cnt

    def list_keep(self, keys: torch.Tensor, counts: Optional[torch.Tensor], limit: int, mask=None, thresholds=None):
        """The ranked lists keys [B, stride] (+ counts [B], None = every slot) filtered in rank order (hx_list_keep): a
        slot stays when its key is not 0, (mask: a row mask as `_dev_mask` takes it) its id is a row of this index whose
        bit is set and (thresholds: B float32 values, a tensor or anything numpy reads) its score is not below its
        query's threshold.  Returns (out_keys [B, limit] int64 -- the first `limit` kept keys unchanged, 0 after them --,
        counts [B] int32).  Only enqueues work."""
        keys, counts, B, stride = self._pool_args(keys, counts)
        L = int(limit)
        words, rows = self._dev_mask(mask)
        thr = None
        if thresholds is not None:
            if not isinstance(thresholds, torch.Tensor):
                thresholds = torch.from_numpy(np.ascontiguousarray(thresholds, dtype=np.float32).reshape(-1))
            thr = _need_cuda(thresholds.to(keys.device), torch.float32, "thresholds")
            if thr.dim() != 1 or thr.shape[0] != B:
                raise HxError(f"thresholds: want {B} values, one per query")
        out = torch.empty((B, L if 1 <= L <= 8192 else 1), dtype=torch.int64, device=keys.device)   # (the engine refuses)
        cnt = torch.empty((B,), dtype=torch.int32, device=keys.device)
        check(_lib.lib().hx_list_keep(self._h, _ptr(keys), stride, _ptr(counts), B, _ptr(words), rows, _ptr(thr), L,
                                      _ptr(out), _ptr(cnt), _stream()))
        return out, cnt

    # -- collection term statistics and the IDF modifier (hx.h: hx_sparse_df / hx_sparse_idf_*) ----
    def sparse_df(self, q_idx: torch.Tensor):
        """(df [nnz] int64, n_docs [1] int64) on the device for a flat tensor of term ids; nothing is read back."""
        q_idx = _need_cuda(q_idx, torch.int32, "q_idx").reshape(-1)
        nnz = q_idx.shape[0]
        df = torch.empty((nnz,), dtype=torch.int64, device=self._tdev)
        n_docs = torch.empty((1,), dtype=torch.int64, device=self._tdev)
        check(_lib.lib().hx_sparse_df(self._h, _ptr(q_idx), nnz, _ptr(df), _ptr(n_docs), _stream()))
        return df, n_docs

    def sparse_idf(self, q_idx: torch.Tensor, q_val: torch.Tensor) -> torch.Tensor:
        """q_val scaled by the collection's IDF of its term, on the device (a new tensor)."""
        df, n_docs = self.sparse_df(q_idx)
        return sparse_idf_apply(q_val, df, n_docs)

    def sparse_idf_host(self, idx: np.ndarray, val: np.ndarray, want_stats: bool = False):
        """numpy in, numpy out (hx_sparse_idf_host): the scaled float32 weights; with want_stats also df [nnz] int64
        and N."""
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        val = np.ascontiguousarray(val, dtype=np.float32).reshape(-1)
        if idx.shape != val.shape:
            raise HxError("sparse_idf_host: as many values as indices")
        out = np.empty(idx.shape[0], np.float32)
        df = np.empty(idx.shape[0], np.int64) if want_stats else None
        n_docs = C.c_int64(0)
        check(_lib.lib().hx_sparse_idf_host(self._h, _ptr(idx), _ptr(val), idx.shape[0], _ptr(out), _ptr(df),
                                            C.byref(n_docs) if want_stats else None))
        return (out, df, int(n_docs.value)) if want_stats else out

    def h1_local(self, q: torch.Tensor, q_indptr: torch.Tensor, q_idx: torch.Tensor, q_val: torch.Tensor,
                 dense_limit: int, sparse_limit: int) -> torch.Tensor:
        """This shard's dense and sparse lists side by side, [B, dense_limit + sparse_limit] (hx_h1_local)."""
        q = _need_cuda(q, torch.float32, "q")
        q_indptr = _need_cuda(q_indptr, torch.int64, "q_indptr")
        q_idx = _need_cuda(q_idx, torch.int32, "q_idx")
        q_val = _need_cuda(q_val, torch.float32, "q_val")
        B = q.shape[0]
        keys = torch.empty((B, dense_limit + sparse_limit), dtype=torch.int64, device=q.device)
        check(_lib.lib().hx_h1_local(self._h, _ptr(q), _ptr(q_indptr), _ptr(q_idx), _ptr(q_val), B, dense_limit,
                                     sparse_limit, _ptr(keys), _stream()))
        return keys

    def h1_local_async(self, q: torch.Tensor, q_indptr: torch.Tensor, q_idx: torch.Tensor, q_val: torch.Tensor,
                       dense_limit: int, sparse_limit: int) -> torch.Tensor:
        """h1_local without the host round trip (hx_h1_local_async): [B + 1, dense_limit + sparse_limit]; row B,
        element 0 = queries whose lists are not final (then the batch must be redone through h1_local)."""
        q = _need_cuda(q, torch.float32, "q")
        q_indptr = _need_cuda(q_indptr, torch.int64, "q_indptr")
        q_idx = _need_cuda(q_idx, torch.int32, "q_idx")
        q_val = _need_cuda(q_val, torch.float32, "q_val")
        B = q.shape[0]
        keys = torch.empty((B + 1, dense_limit + sparse_limit), dtype=torch.int64, device=q.device)
        check(_lib.lib().hx_h1_local_async(self._h, _ptr(q), _ptr(q_indptr), _ptr(q_idx), _ptr(q_val), B, dense_limit,
                                           sparse_limit, _ptr(keys), _stream()))
        return keys

    # -- candidates-first sharded H1 (hx.h: hx_h1_nominate_async / hx_h1_rescore_async; distributed.H1Pipeline) ----------
    def sparse_wmax(self):
        """(largest document weight of this shard, whether it holds a non-positive weight)"""
        w, npos = C.c_float(), C.c_int32()
        check(_lib.lib().hx_sparse_wmax(self._h, C.byref(w), C.byref(npos)))
        return float(w.value), bool(npos.value)

    def set_sparse_wmax(self, wmax: float):
        """The largest document weight of ANY shard: one scale for the integer BM25 scores of all shards."""
        check(_lib.lib().hx_set_sparse_wmax(self._h, float(wmax)))

    def h1_nominate_async(self, q, q_indptr, q_idx, q_val, dense_limit: int, sparse_limit: int, k1: int, k2: int,
                          lout: Optional[int] = None):
        """This shard's nominations (hx_h1_nominate_async): flat int64, the first B * (k1 + k2 + 2) words are what the
        shards exchange, the B * (lout + 1) words behind them stay with the batch on this rank (h1_rescore_async)."""
        q = _need_cuda(q, torch.float32, "q")
        q_indptr = _need_cuda(q_indptr, torch.int64, "q_indptr")
        q_idx = _need_cuda(q_idx, torch.int32, "q_idx")
        q_val = _need_cuda(q_val, torch.float32, "q_val")
        B = q.shape[0]
        if lout is None:
            lout = h1_plan(dense_limit, sparse_limit, 1)[4]
        nom = torch.empty((B * (k1 + k2 + 2) + B * (lout + 1),), dtype=torch.int64, device=q.device)
        check(_lib.lib().hx_h1_nominate_async(self._h, _ptr(q), _ptr(q_indptr), _ptr(q_idx), _ptr(q_val), B, dense_limit,
                                              sparse_limit, k1, k2, _ptr(nom), _stream()))
        return nom

    def h1_rescore_async(self, q, q_indptr, q_idx, q_val, nom: torch.Tensor, gathered: torch.Tensor, world: int, rank: int,
                         dense_limit: int, sparse_limit: int, k1: int, k2: int, lp: int, k3: int):
        """Exact scores of this shard's rows among the global candidates, flat [B * (lp + world * k3 + world + 4)]
        (hx_h1_rescore_async).  `nom`: this rank's own h1_nominate_async result; `gathered`: every rank's public part."""
        q = _need_cuda(q, torch.float32, "q")
        q_indptr = _need_cuda(q_indptr, torch.int64, "q_indptr")
        q_idx = _need_cuda(q_idx, torch.int32, "q_idx")
        q_val = _need_cuda(q_val, torch.float32, "q_val")
        gathered = _need_cuda(gathered, torch.int64, "gathered")
        nom = _need_cuda(nom, torch.int64, "nom")
        B = q.shape[0]
        if gathered.numel() != world * B * (k1 + k2 + 2):
            raise HxError("gathered nominations have the wrong size")
        res = torch.empty((B * (lp + world * k3 + world + 4),), dtype=torch.int64, device=q.device)
        check(_lib.lib().hx_h1_rescore_async(self._h, _ptr(q), _ptr(q_indptr), _ptr(q_idx), _ptr(q_val), B, _ptr(nom),
                                             _ptr(gathered), world, rank, dense_limit, sparse_limit, k1, k2, lp, k3,
                                             _ptr(res), _stream()))
        return res

    def rescore(self, q: torch.Tensor, cand_keys: torch.Tensor, cand_counts: Optional[torch.Tensor],
                limit: int, prefix: int = 0):
        q = _need_cuda(q, torch.float32, "q")
        cand_keys = _need_cuda(cand_keys, torch.int64, "cand_keys")
        if cand_counts is not None:
            cand_counts = _need_cuda(cand_counts, torch.int32, "cand_counts")
        B = q.shape[0]
        keys, cnt = self._out(B, limit)
        check(_lib.lib().hx_rescore(self._h, _ptr(q), B, prefix, _ptr(cand_keys), cand_keys.shape[1],
                                    _ptr(cand_counts), limit, _ptr(keys), _ptr(cnt), _stream()))
        return keys, cnt

    def _mask(self, mask):
        """(packed uint32 words, mask_rows) of a row mask: a bool array of one entry per row, or the packed words
        themselves (ceil(count / 32) of them, bit r & 31 of word r >> 5 = row r)."""
        m = np.asarray(mask)
        if m.dtype == np.bool_:
            return pack_rows(m), int(m.shape[0])
        if m.dtype != np.uint32:
            raise TypeError("mask: a bool array (one entry per row) or packed np.uint32 words")
        n = self.count()
        if m.shape[0] != (n + 31) // 32:
            raise ValueError(f"mask: {m.shape[0]} words for {n} rows (want {(n + 31) // 32})")
        return np.ascontiguousarray(m), n

    # -- what every entry does with its queries, its masks, its pools and its outputs ---------------------------------
    def _host_mask(self, mask):
        """(words, mask_rows) of a *_host call: None = every row, else as `_mask` takes it"""
        return (None, 0) if mask is None else self._mask(mask)

    def _dev_mask(self, mask):
        """(words, mask_rows) of a device call: None = every row; the packed words on the device (an int32 / uint32
        tensor, as payload_mask returns them) go as they are, ceil(count / 32) of them; a bool mask (host or device) or
        host words are packed on the host (`_mask`) and uploaded."""
        if mask is None:
            return None, 0
        if isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dtype != torch.bool:
            if mask.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not mask.is_contiguous():
                raise TypeError("device mask: a contiguous int32 / uint32 tensor holding the packed words, or a bool tensor")
            rows = self.count()
            if mask.shape[0] != (rows + 31) // 32:
                raise ValueError(f"mask: {mask.shape[0]} words for {rows} rows")
            return mask, rows
        packed, rows = self._mask(mask.cpu().numpy() if isinstance(mask, torch.Tensor) else mask)
        return torch.from_numpy(packed.view(np.int32)).to(self._tdev), rows

    def _host_queries(self, q, q_indptr, q_idx, q_val):
        """the batch of a *_host call as the engine reads it: (q [B, dim] float32, the sparse CSR int64 / int32 /
        float32, B)"""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, self.dim)
        return (q, np.ascontiguousarray(q_indptr, dtype=np.int64), np.ascontiguousarray(q_idx, dtype=np.int32),
                np.ascontiguousarray(q_val, dtype=np.float32), q.shape[0])

    @staticmethod
    def _pool_args(keys, counts):
        """the ranked pools of a stage: (keys [B, stride] int64, counts [B] int32 or None, B, stride)"""
        keys = _need_cuda(keys, torch.int64, "keys")
        if keys.dim() != 2:
            raise HxError("keys must be a [B, stride] tensor")
        if counts is not None:
            counts = _need_cuda(counts, torch.int32, "counts")
        return keys, counts, int(keys.shape[0]), int(keys.shape[1])

    @staticmethod
    def _host_out(B: int, L: int, bound: Optional[int] = None, extra: int = 0):
        """(scores [B, L] float32, ids [B, L] int64, counts [B] int32, then `extra` more float32 planes [B, L]) for a
        *_host entry to fill.  bound: an L outside [1, bound] gets one slot (the engine refuses; nothing huge is
        allocated)."""
        if bound is not None and not 1 <= L <= bound:
            L = 1
        return (np.empty((B, L), dtype=np.float32), np.empty((B, L), dtype=np.int64), np.empty((B,), dtype=np.int32),
                *(np.empty((B, L), dtype=np.float32) for _ in range(extra)))

    def hybrid_query(self, q: torch.Tensor, q_indptr: torch.Tensor, q_idx: torch.Tensor,
                     q_val: torch.Tensor, params: HxParams, mask=None):
        """mask: None = every row; else a packed uint32 tensor / array or a bool array (hx_hybrid_query_dev_masked)."""
        q = _need_cuda(q, torch.float32, "q")
        q_indptr = _need_cuda(q_indptr, torch.int64, "q_indptr")
        q_idx = _need_cuda(q_idx, torch.int32, "q_idx")
        q_val = _need_cuda(q_val, torch.float32, "q_val")
        B = q.shape[0]
        keys, cnt = self._out(B, params.final_limit)
        if mask is None:
            check(_lib.lib().hx_hybrid_query_dev(self._h, _ptr(q), _ptr(q_indptr), _ptr(q_idx), _ptr(q_val), B,
                                                 C.byref(params), _ptr(keys), _ptr(cnt), _stream()))
            return keys, cnt
        words, rows = self._dev_mask(mask)
        check(_lib.lib().hx_hybrid_query_dev_masked(self._h, _ptr(q), _ptr(q_indptr), _ptr(q_idx), _ptr(q_val), B,
                                                    C.byref(params), _ptr(words), rows, _ptr(keys), _ptr(cnt),
                                                    _stream()))
        return keys, cnt

    def release_mask_view(self):
        """Free the gathered copies pre-filtered queries keep between calls (hx_release_mask_view)."""
        check(_lib.lib().hx_release_mask_view(self._h))

    # -- payload index (hx.h: hx_payload_*; payload_index.py compiles filters to the programs) ----------------------
    def payload_create(self, kind: int) -> int:
        """A new empty column of `kind` (PAY_U32 / PAY_F64 / PAY_LIST_U32 / PAY_LIST_F64 / PAY_TEXT); returns its id
        (hx_payload_create)."""
        col = C.c_int32()
        check(_lib.lib().hx_payload_create(self._h, int(kind), C.byref(col)))
        return col.value

    def payload_drop(self, col: int) -> None:
        check(_lib.lib().hx_payload_drop(self._h, int(col)))

    def payload_append(self, col: int, cells: np.ndarray) -> None:
        """The cells of the next len(cells) rows of the column: np.uint32 codes (a U32 column) or np.uint64 bit patterns
        of doubles (an F64 column; np.float64 is taken as it is).  Refused past count() (hx_payload_append)."""
        cells = np.ascontiguousarray(cells)
        if cells.dtype not in (np.uint32, np.uint64, np.float64) or cells.ndim != 1:
            raise TypeError("payload cells: a 1-d np.uint32 (U32 column) or np.uint64 / np.float64 (F64 column) array")
        check(_lib.lib().hx_payload_append(self._h, int(col), _ptr(cells), cells.shape[0]))

    def payload_append_lists(self, col: int, heads: np.ndarray, values: np.ndarray) -> None:
        """The cells of the next len(heads) rows of a list column (hx_payload_append_lists): heads np.uint32 -- MISSING,
        NULL or the row's element count --, values the rows' elements one after another, np.uint32 codes (PAY_LIST_U32)
        or np.float64 (PAY_LIST_F64)."""
        heads, values = np.ascontiguousarray(heads), np.ascontiguousarray(values)
        if heads.dtype != np.uint32 or heads.ndim != 1 or values.dtype not in (np.uint32, np.float64) or values.ndim != 1:
            raise TypeError("payload lists: 1-d np.uint32 heads and 1-d np.uint32 / np.float64 values")
        check(_lib.lib().hx_payload_append_lists(self._h, int(col), _ptr(heads), heads.shape[0], _ptr(values),
                                                 values.shape[0]))

    def payload_replace(self, col: int, rows, cells: np.ndarray) -> None:
        """New cells for the stored rows `rows` of a scalar column (hx_payload_replace): `cells` as payload_append takes
        them, one per row, in the order of `rows`."""
        rows = self._rows(rows)
        cells = np.ascontiguousarray(cells)
        if cells.dtype not in (np.uint32, np.uint64, np.float64) or cells.ndim != 1:
            raise TypeError("payload cells: a 1-d np.uint32 (U32 column) or np.uint64 / np.float64 (F64 column) array")
        if cells.shape[0] != rows.shape[0]:
            raise ValueError(f"{rows.shape[0]} rows but {cells.shape[0]} cells")
        check(_lib.lib().hx_payload_replace(self._h, int(col), _ptr(rows), rows.shape[0], _ptr(cells)))

    def payload_replace_lists(self, col: int, rows, heads: np.ndarray, values: np.ndarray) -> None:
        """New cells for the stored rows `rows` of a list column (hx_payload_replace_lists): heads / values as
        payload_append_lists takes them, in the order of `rows`."""
        rows = self._rows(rows)
        heads, values = np.ascontiguousarray(heads), np.ascontiguousarray(values)
        if heads.dtype != np.uint32 or heads.ndim != 1 or values.dtype not in (np.uint32, np.float64) or values.ndim != 1:
            raise TypeError("payload lists: 1-d np.uint32 heads and 1-d np.uint32 / np.float64 values")
        if heads.shape[0] != rows.shape[0]:
            raise ValueError(f"{rows.shape[0]} rows but {heads.shape[0]} heads")
        check(_lib.lib().hx_payload_replace_lists(self._h, int(col), _ptr(rows), rows.shape[0], _ptr(heads), _ptr(values),
                                                  values.shape[0]))

    def payload_list(self, col: int, row: int, kind: int):
        """One row of a list column (hx_payload_debug_list): (head, elements) -- head = MISSING, NULL or the element
        count; elements np.uint32 codes or np.float64."""
        head, count = C.c_uint32(), C.c_int64()
        check(_lib.lib().hx_payload_debug_list(self._h, int(col), int(row), C.byref(head), None, 0, C.byref(count)))
        out = np.zeros(max(count.value, 1), dtype=np.uint32 if kind == PAY_LIST_U32 else np.float64)
        check(_lib.lib().hx_payload_debug_list(self._h, int(col), int(row), C.byref(head), _ptr(out), count.value,
                                               C.byref(count)))
        return head.value, out[:count.value]

    @staticmethod
    def _text_cells(heads, data):
        heads = np.ascontiguousarray(heads)
        if isinstance(data, (bytes, bytearray, memoryview)):
            data = np.frombuffer(bytes(data), np.uint8)
        data = np.ascontiguousarray(data)
        if heads.dtype != np.uint32 or heads.ndim != 1 or data.dtype != np.uint8 or data.ndim != 1:
            raise TypeError("payload text: 1-d np.uint32 heads and the rows' bytes (bytes or a 1-d np.uint8 array)")
        return heads, data

    def payload_append_text(self, col: int, heads: np.ndarray, data) -> None:
        """The cells of the next len(heads) rows of a text column (hx_payload_append_text): heads np.uint32 -- MISSING,
        NULL or the row's byte length --, data the rows' bytes one after another (bytes or np.uint8)."""
        heads, data = self._text_cells(heads, data)
        check(_lib.lib().hx_payload_append_text(self._h, int(col), _ptr(heads), heads.shape[0], _ptr(data), data.shape[0]))

    def payload_replace_text(self, col: int, rows, heads: np.ndarray, data) -> None:
        """New cells for the stored rows `rows` of a text column (hx_payload_replace_text): heads / data as
        payload_append_text takes them, in the order of `rows`."""
        rows = self._rows(rows)
        heads, data = self._text_cells(heads, data)
        if heads.shape[0] != rows.shape[0]:
            raise ValueError(f"{rows.shape[0]} rows but {heads.shape[0]} heads")
        check(_lib.lib().hx_payload_replace_text(self._h, int(col), _ptr(rows), rows.shape[0], _ptr(heads), _ptr(data),
                                                 data.shape[0]))

    def payload_debug_text(self, col: int, row: int):
        """One row of a text column (hx_payload_debug_text): (head, bytes) -- head = MISSING, NULL or the byte length."""
        head, count = C.c_uint32(), C.c_int64()
        check(_lib.lib().hx_payload_debug_text(self._h, int(col), int(row), C.byref(head), None, 0, C.byref(count)))
        out = np.zeros(max(count.value, 1), dtype=np.uint8)
        check(_lib.lib().hx_payload_debug_text(self._h, int(col), int(row), C.byref(head), _ptr(out), count.value,
                                               C.byref(count)))
        return head.value, out[:count.value].tobytes()

    def payload_rows(self, col: int) -> int:
        n = C.c_int64()
        check(_lib.lib().hx_payload_rows(self._h, int(col), C.byref(n)))
        return n.value

    def payload_cell(self, col: int, row: int, kind: int) -> int:
        """The stored bits of one cell (hx_payload_debug_cell): a code, or the bit pattern of a double."""
        out = np.zeros(1, dtype=np.uint64)
        check(_lib.lib().hx_payload_debug_cell(self._h, int(col), int(row), _ptr(out)))
        return int(out[0]) & (0xFFFFFFFF if kind == PAY_U32 else 0xFFFFFFFFFFFFFFFF)

    def payload_mask(self, ops, sets=(), want_count: bool = True):
        """Evaluate a program (hx_payload_mask).  ops: (op, col, imm) triples, imm an int (a code, the bits of a double, a
        set index); sets: sorted 1-d arrays, np.uint32 or np.float64, or -- the pattern blob of TEXT_ALL -- bytes.  Returns (mask, n_kept): the packed words as an int32
        device tensor of ceil(count() / 32) entries -- what hybrid_query takes as `mask` -- and the number of set bits
        (None when want_count is False: the call then only enqueues work).  mask_host(mask) gives the numpy form."""
        arr = (_lib.HxPayOp * max(len(ops), 1))()
        for k, (op, col, imm) in enumerate(ops):
            arr[k].op, arr[k].col, arr[k].imm = int(op), int(col), int(imm) & 0xFFFFFFFFFFFFFFFF
        keep = []
        sarr = (_lib.HxPaySet * max(len(sets), 1))()
        for k, s in enumerate(sets):
            if isinstance(s, (bytes, bytearray)):         # a pattern blob: n = its bytes
                s = np.frombuffer(bytes(s), np.uint8)
            s = np.ascontiguousarray(s)
            if s.dtype not in (np.uint32, np.float64, np.uint8) or s.ndim != 1:
                raise TypeError("payload set: a 1-d np.uint32 or np.float64 array, or the bytes of a pattern blob")
            keep.append(s)
            sarr[k].vals, sarr[k].n = s.ctypes.data, s.shape[0]
        nw = (self.count() + 31) // 32
        mask = torch.empty((max(nw, 1),), dtype=torch.int32, device=self._tdev)   # (an empty index: still a valid pointer)
        kept = C.c_int64()
        check(_lib.lib().hx_payload_mask(self._h, arr, len(ops), sarr, len(sets), _ptr(mask),
                                         C.byref(kept) if want_count else None, _stream()))
        return mask[:nw], (kept.value if want_count else None)

    def payload_same_offsets(self, col_a: int, col_b: int) -> bool:
        """Whether two list columns are element-aligned (hx_payload_same_offsets): filled alike, with equal heads and
        equal offsets for every row -- what the columns of one nested block must be.  Synchronises."""
        same = C.c_int32()
        check(_lib.lib().hx_payload_same_offsets(self._h, int(col_a), int(col_b), C.byref(same)))
        return bool(same.value)

    @staticmethod
    def mask_host(mask: torch.Tensor) -> np.ndarray:
        """A device mask of payload_mask as packed np.uint32 words (what filters.row_mask returns)."""
        return mask.cpu().numpy().view(np.uint32).copy()

    def hybrid_query_host(self, q: np.ndarray, q_indptr: np.ndarray, q_idx: np.ndarray, q_val: np.ndarray,
                          params: HxParams, mask=None):
        """mask: None = every row; else a bool array (one entry per row) or packed np.uint32 words
        (hx_hybrid_query_host_masked: the lists of the same query on an index of the kept rows only)."""
        q, q_indptr, q_idx, q_val, B = self._host_queries(q, q_indptr, q_idx, q_val)
        scores, ids, counts = self._host_out(B, params.final_limit)
        if mask is None:
            check(_lib.lib().hx_hybrid_query_host(self._h, _ptr(q), _ptr(q_indptr), _ptr(q_idx), _ptr(q_val), B,
                                                  C.byref(params), _ptr(scores), _ptr(ids), _ptr(counts)))
            return scores, ids, counts
        words, rows = self._mask(mask)
        check(_lib.lib().hx_hybrid_query_host_masked(self._h, _ptr(q), _ptr(q_indptr), _ptr(q_idx), _ptr(q_val), B,
                                                     C.byref(params), _ptr(words), rows, _ptr(scores), _ptr(ids),
                                                     _ptr(counts)))
        return scores, ids, counts

    # -- payload facets (hx.h: hx_payload_facet / hx_facet_top / hx_payload_facet_host) --------
    def payload_facet(self, col: int, n_codes: int, mask: Optional[torch.Tensor] = None, counts=None, stray=None):
        """How many kept rows hold each code below n_codes of the U32 or LIST_U32 column `col` (hx_payload_facet).  mask:
        None = every row, or a row mask as hybrid_query takes it (payload_mask's device words go as they are).  Returns (counts
        [n_codes] int32 holding the uint32 counts, stray [1] int64: the kept cells / elements with a code at or above
        n_codes).  counts / stray: the tensors to write (tests hand in sentinels).  Only enqueues work."""
        n_codes = int(n_codes)
        if not 0 <= n_codes <= 0xFFFFFFFF:
            raise HxError("facet: n_codes out of range [1, 0xFFFFFFFE]")
        mask, rows = self._dev_mask(mask)
        if counts is None:
            counts = torch.empty((n_codes if 1 <= n_codes <= 0xFFFFFFFE else 1,), dtype=torch.int32, device=self._tdev)
        if stray is None:
            stray = torch.empty((1,), dtype=torch.int64, device=self._tdev)
        check(_lib.lib().hx_payload_facet(self._h, int(col), _ptr(mask), rows, n_codes, _ptr(counts),
                                          _ptr(stray), _stream()))
        return counts, stray

    def facet_top(self, counts: torch.Tensor, limit: int, rank: Optional[torch.Tensor] = None, out=None, out_count=None):
        """The at most `limit` codes of counts [n_codes] with a non-zero count (hx_facet_top): keys [limit] int64, each
        count << 32 | (0xFFFFFFFF - rank), sorted descending, 0 past the hits, and the number of hits [1] int32.  rank:
        None (a code ranks as itself) or the int32 device tensor [n_codes] holding the uint32 position of each code's
        value in sorted order.  out / out_count: the tensors to write.  Only enqueues work."""
        counts = _need_cuda(counts, torch.int32, "counts")
        if rank is not None:
            rank = _need_cuda(rank, torch.int32, "rank")
            if rank.shape[0] != counts.shape[0]:
                raise ValueError(f"rank: {rank.shape[0]} entries for {counts.shape[0]} codes")
        L = int(limit)
        if out is None:
            out = torch.empty((L if 1 <= L <= 2048 else 1,), dtype=torch.int64, device=counts.device)
        if out_count is None:
            out_count = torch.empty((1,), dtype=torch.int32, device=counts.device)
        check(_lib.lib().hx_facet_top(self._h, _ptr(counts), int(counts.shape[0]), _ptr(rank), L, _ptr(out),
                                      _ptr(out_count), _stream()))
        return out, out_count

    def payload_facet_host(self, col: int, n_codes: int, limit: int, rank: Optional[np.ndarray] = None, mask=None):
        """The whole facet, host in, host out (hx_payload_facet_host): the `limit` codes of the column with the largest
        counts among the rows of `mask` (None, a bool array or packed np.uint32 words, as hybrid_query_host takes it).
        rank: None, or np.uint32 [n_codes], the position of each code's value in sorted order.  Returns (ranks_or_codes
        np.uint32 [hits] -- ranks when `rank` is given, codes otherwise --, counts np.uint32 [hits], stray: int)."""
        n_codes, L = int(n_codes), int(limit)
        if not 1 <= L <= 2048:
            raise HxError("facet: limit out of range [1, 2048]")
        if not 0 <= n_codes <= 0xFFFFFFFF:
            raise HxError("facet: n_codes out of range [1, 0xFFFFFFFE]")
        if rank is not None:
            rank = np.ascontiguousarray(rank, dtype=np.uint32)
            if rank.shape[0] != n_codes:
                raise ValueError(f"rank: {rank.shape[0]} entries for {n_codes} codes")
        words, rows = self._host_mask(mask)
        first = np.empty((L,), dtype=np.uint32)
        counts = np.empty((L,), dtype=np.uint32)
        n_out, stray = C.c_int32(), C.c_uint64()
        check(_lib.lib().hx_payload_facet_host(self._h, int(col), _ptr(words), rows, n_codes, _ptr(rank), L,
                                               _ptr(first), _ptr(counts), C.byref(n_out), C.byref(stray)))
        return first[:n_out.value], counts[:n_out.value], int(stray.value)

    # -- scroll (hx.h: hx_scroll_rows / hx_payload_order and their _host forms) ----------------
    def scroll_rows(self, limit: int, start_row: int = 0, mask: Optional[torch.Tensor] = None, out=None, out_count=None):
        """The first `limit` rows r >= start_row whose mask bit is set, ascending (hx_scroll_rows).  Returns (rows [limit]
        int32 holding the uint32 rows, 0 past the hits; count [1] int32).  out / out_count: the tensors to write (tests
        hand in sentinels).  Only enqueues work."""
        L = int(limit)
        mask, rows = self._dev_mask(mask)
        if out is None:
            out = torch.empty((L if 1 <= L <= 2048 else 1,), dtype=torch.int32, device=self._tdev)
        if out_count is None:
            out_count = torch.empty((1,), dtype=torch.int32, device=self._tdev)
        check(_lib.lib().hx_scroll_rows(self._h, _ptr(mask), rows, int(start_row), L, _ptr(out), _ptr(out_count),
                                        _stream()))
        return out, out_count

    @staticmethod
    def _order_bounds(start_from, after):
        flags = (1 if start_from is not None else 0) | (2 if after is not None else 0)
        av, ar = after if after is not None else (0.0, 0)
        return flags, float(start_from if start_from is not None else 0.0), float(av), int(ar)

    def payload_order(self, col: int, limit: int, desc: bool = False, start_from: Optional[float] = None,
                      after=None, mask: Optional[torch.Tensor] = None, out=None, out_bits=None, out_count=None,
                      direction: Optional[int] = None, flags: Optional[int] = None):
        """The best `limit` eligible rows of the F64 column `col` in the order (value in the direction, row ascending)
        (hx_payload_order; hx.h states eligibility): start_from = an inclusive bound, after = (value, row), the cursor
        the page lies strictly after.  Returns (rows [limit] int32 holding the uint32 rows, bits [limit] int64 holding
        the stored cells, count [1] int32), zeros past the hits.  direction / flags: raw values instead of the ones
        derived (tests).  Only enqueues work."""
        L = int(limit)
        mask, rows = self._dev_mask(mask)
        fl, sf, av, ar = self._order_bounds(start_from, after)
        n = L if 1 <= L <= 2048 else 1
        if out is None:
            out = torch.empty((n,), dtype=torch.int32, device=self._tdev)
        if out_bits is None:
            out_bits = torch.empty((n,), dtype=torch.int64, device=self._tdev)
        if out_count is None:
            out_count = torch.empty((1,), dtype=torch.int32, device=self._tdev)
        check(_lib.lib().hx_payload_order(self._h, int(col), _ptr(mask), rows,
                                          int(desc) if direction is None else int(direction),
                                          fl if flags is None else int(flags), sf, av, ar, L, _ptr(out), _ptr(out_bits),
                                          _ptr(out_count), _stream()))
        return out, out_bits, out_count

    def scroll_rows_host(self, limit: int, start_row: int = 0, mask=None) -> np.ndarray:
        """hx_scroll_rows, host in, host out: mask None, a bool array or packed np.uint32 words (as hybrid_query_host
        takes it).  Returns the rows, np.uint32 [hits]."""
        L = int(limit)
        if not 1 <= L <= 2048:
            raise HxError("scroll: limit out of range [1, 2048]")
        words, rows = self._host_mask(mask)
        out = np.empty((L,), dtype=np.uint32)
        n_out = C.c_int32()
        check(_lib.lib().hx_scroll_rows_host(self._h, _ptr(words), rows, int(start_row), L, _ptr(out), C.byref(n_out)))
        return out[:n_out.value]

    def payload_order_host(self, col: int, limit: int, desc: bool = False, start_from: Optional[float] = None,
                           after=None, mask=None):
        """hx_payload_order, host in, host out.  Returns (rows np.uint32 [hits], bits np.uint64 [hits]: the stored
        cells)."""
        L = int(limit)
        if not 1 <= L <= 2048:
            raise HxError("scroll: limit out of range [1, 2048]")
        words, rows = self._host_mask(mask)
        fl, sf, av, ar = self._order_bounds(start_from, after)
        out = np.empty((L,), dtype=np.uint32)
        bits = np.empty((L,), dtype=np.uint64)
        n_out = C.c_int32()
        check(_lib.lib().hx_payload_order_host(self._h, int(col), _ptr(words), rows, int(desc), fl, sf, av, ar, L,
                                               _ptr(out), _ptr(bits), C.byref(n_out)))
        return out[:n_out.value], bits[:n_out.value]

    # -- grouped search (hx.h: hx_group / hx_hybrid_query_groups_host) -------------------------
    def group(self, col: int, keys: torch.Tensor, counts: Optional[torch.Tensor], n_groups: int, group_size: int):
        """The best n_groups groups of the ranked lists keys [B, stride] (+ counts [B], None = every slot), at most
        group_size hits each, grouped by the cells of the U32 column `col` (hx_group).  Returns (out_keys
        [B, n_groups, group_size] int64, 0 = an empty slot; group_codes [B, n_groups] int32 holding the uint32 codes,
        -1 = HX_PAY_U32_MISSING = no such group; group_counts [B] int32).  Only enqueues work."""
        keys, counts, B, stride = self._pool_args(keys, counts)
        G, S = int(n_groups), int(group_size)
        slots = G * S if 1 <= G <= 2048 and 1 <= S <= 2048 else 0      # (the engine refuses; nothing huge is allocated)
        out = torch.empty((B, max(slots, 1)), dtype=torch.int64, device=keys.device)
        codes = torch.empty((B, G if slots else 1), dtype=torch.int32, device=keys.device)
        cnt = torch.empty((B,), dtype=torch.int32, device=keys.device)
        check(_lib.lib().hx_group(self._h, int(col), _ptr(keys), stride, _ptr(counts), B, G, S, _ptr(out), _ptr(codes),
                                  _ptr(cnt), _stream()))
        return out.view(B, G, S), codes, cnt

    def hybrid_query_groups_host(self, q: np.ndarray, q_indptr: np.ndarray, q_idx: np.ndarray, q_val: np.ndarray,
                                 params: HxParams, col: int, n_groups: int, group_size: int, group_pool: int = 0,
                                 mask=None):
        """hybrid_query_host grouped by the U32 column `col` (hx_hybrid_query_groups_host): the query runs with
        final_limit = the pool (group_pool = 0: the mode's whole pool; params.final_limit is not used), the pool is
        grouped on the device.  Returns (scores [B, n_groups, group_size] float32, ids [B, n_groups, group_size] int64 --
        empty slots (-inf, -1) --, group_codes [B, n_groups] uint32, group_counts [B] int32).  mask as hybrid_query_host."""
        q, q_indptr, q_idx, q_val, B = self._host_queries(q, q_indptr, q_idx, q_val)
        G, S = int(n_groups), int(group_size)
        if not (1 <= G <= 2048 and 1 <= S <= 2048 and G * S <= 2048):
            raise HxError("group: n_groups and group_size must be at least 1 and n_groups * group_size at most 2048")
        scores, ids, counts = self._host_out(B, G * S)
        scores, ids = scores.reshape(B, G, S), ids.reshape(B, G, S)
        codes = np.empty((B, G), dtype=np.uint32)
        words, rows = self._host_mask(mask)
        check(_lib.lib().hx_hybrid_query_groups_host(self._h, _ptr(q), _ptr(q_indptr), _ptr(q_idx), _ptr(q_val), B,
                                                     C.byref(params), _ptr(words), rows, int(col), int(group_pool), G, S,
                                                     _ptr(scores), _ptr(ids), _ptr(codes), _ptr(counts)))
        return scores, ids, codes, counts

    # -- MMR search (hx.h: hx_mmr / hx_hybrid_query_mmr_host) ----------------------------------
    def mmr(self, keys: torch.Tensor, counts: Optional[torch.Tensor], limit: int, diversity: float, eligible=None):
        """Maximal marginal relevance over the ranked pools keys [B, stride] (+ counts [B], None = every slot): `limit`
        picks per query (hx_mmr).  eligible: None, or a row mask as hybrid_query takes it (a bool array of one entry
        per row, or packed uint32 words); rows whose bit is clear are never picked.  Returns (out_keys [B, limit] int64, 0
        past the picks; values [B, limit] float32, the picks' MMR values; counts [B] int32).  Only enqueues work."""
        keys, counts, B, stride = self._pool_args(keys, counts)
        L = int(limit)
        slots = L if 1 <= L <= 256 else 1                   # (the engine refuses; nothing huge is allocated)
        words, rows = self._dev_mask(eligible)
        out = torch.empty((B, slots), dtype=torch.int64, device=keys.device)
        val = torch.empty((B, slots), dtype=torch.float32, device=keys.device)
        cnt = torch.empty((B,), dtype=torch.int32, device=keys.device)
        check(_lib.lib().hx_mmr(self._h, _ptr(keys), stride, _ptr(counts), B, L, float(diversity), _ptr(words), rows,
                                _ptr(out), _ptr(val), _ptr(cnt), _stream()))
        return out, val, cnt

    def hybrid_query_mmr_host(self, q: np.ndarray, q_indptr: np.ndarray, q_idx: np.ndarray, q_val: np.ndarray,
                              params: HxParams, limit: int, diversity: float, candidates_limit: int = 0, mask=None,
                              mask_root_only: bool = False):
        """hybrid_query_host followed by MMR over its pool (hx_hybrid_query_mmr_host): the query runs with final_limit =
        the pool (candidates_limit = 0: the mode's whole pool; params.final_limit is not used), `limit` hits are picked on
        the device.  mask as hybrid_query_host; mask_root_only: the query runs unmasked and only the picks honour the mask
        (tree mode).  Returns (scores [B, limit] float32 -- the dense cosines, in both modes --, ids [B, limit] int64,
        values [B, limit] float32, counts [B] int32) in pick order, the slots past the picks (-inf, -1, 0)."""
        q, q_indptr, q_idx, q_val, B = self._host_queries(q, q_indptr, q_idx, q_val)
        L = int(limit)
        if not 1 <= L <= 256:
            raise HxError("mmr: limit out of range [1, 256]")
        scores, ids, counts, values = self._host_out(B, L, extra=1)
        words, rows = self._host_mask(mask)
        check(_lib.lib().hx_hybrid_query_mmr_host(self._h, _ptr(q), _ptr(q_indptr), _ptr(q_idx), _ptr(q_val), B,
                                                  C.byref(params), _ptr(words), rows, int(bool(mask_root_only)),
                                                  int(candidates_limit), L, float(diversity), _ptr(scores), _ptr(ids),
                                                  _ptr(values), _ptr(counts)))
        return scores, ids, values, counts

    # -- score-boosting search (hx.h: hx_formula / hx_hybrid_query_formula_host) -----------------
    @staticmethod
    def _formula_ops(ops):
        arr = (_lib.HxFormulaOp * max(len(ops), 1))()
        for k, (op, arg, imm) in enumerate(ops):
            arr[k].op, arr[k].arg, arr[k].imm = int(op), int(arg), int(imm) & 0xFFFFFFFFFFFFFFFF
        return arr

    def formula(self, ops, keys: torch.Tensor, counts: Optional[torch.Tensor], limit: int, planes=(),
                score_threshold: Optional[float] = None, eligible=None, out=None):
        """The pools keys [B, stride] (+ counts [B], None = every slot) ranked again by the value the postfix program
        `ops` -- (op, arg, imm) triples, imm an int holding the bits of a double -- gives every position (hx_formula).
        planes: the condition planes, row masks as hybrid_query takes them; eligible: None or one more such mask;
        score_threshold None = no cut.  out: None, or the four output tensors to write into.  Returns (out_keys [B, limit]
        int64, 0 past the hits; positions [B, limit] int32, -1 past them; counts [B] int32; dropped [B] int32).  Only
        enqueues work."""
        keys, counts, B, stride = self._pool_args(keys, counts)
        L = int(limit)
        slots = L if 1 <= L <= 2048 else 1                  # (the engine refuses; nothing huge is allocated)
        dev_planes, rows = [], 0
        for m in planes:
            w, rows = self._dev_mask(m)
            dev_planes.append(w)
        parr = (C.c_void_p * max(len(dev_planes), 1))(*[t.data_ptr() for t in dev_planes])
        words, erows = self._dev_mask(eligible)
        if out is None:
            out = (torch.empty((B, slots), dtype=torch.int64, device=keys.device),
                   torch.empty((B, slots), dtype=torch.int32, device=keys.device),
                   torch.empty((B,), dtype=torch.int32, device=keys.device),
                   torch.empty((B,), dtype=torch.int32, device=keys.device))
        okeys, opos, ocnt, odrop = out
        thr = float("nan") if score_threshold is None else float(score_threshold)
        check(_lib.lib().hx_formula(self._h, self._formula_ops(ops), len(ops), parr if dev_planes else None,
                                    len(dev_planes), rows, _ptr(keys), stride, _ptr(counts), B, L, thr, _ptr(words), erows,
                                    _ptr(okeys), _ptr(opos), _ptr(ocnt), _ptr(odrop), _stream()))
        return okeys, opos, ocnt, odrop

    def hybrid_query_formula_host(self, q: np.ndarray, q_indptr: np.ndarray, q_idx: np.ndarray, q_val: np.ndarray,
                                  params: HxParams, ops, limit: int, planes=(), score_threshold: Optional[float] = None,
                                  candidates_limit: int = 0, mask=None, mask_root_only: bool = False):
        """hybrid_query_host followed by the formula stage over its pool (hx_hybrid_query_formula_host): the query runs
        with final_limit = the pool (candidates_limit = 0: the mode's whole pool; params.final_limit is not used) and keeps
        the scores its mode hands out; the best `limit` positions by the program's value come back.  ops / planes /
        score_threshold as `formula` takes them, mask / mask_root_only as hybrid_query_mmr_host.  Returns (scores
        [B, limit] float32 -- the values --, ids [B, limit] int64, base_scores [B, limit] float32 -- the scores the pool
        carried --, counts [B] int32, dropped [B] int32); the slots past the hits (-inf, -1, -inf)."""
        q, q_indptr, q_idx, q_val, B = self._host_queries(q, q_indptr, q_idx, q_val)
        L = int(limit)
        if not 1 <= L <= 2048:
            raise HxError("formula: limit out of range [1, 2048]")
        host_planes = []
        for m in planes:
            w, rows = self._mask(m)
            if rows != self.count():
                raise HxError("formula: a condition plane must hold one bit per row of the index (hx_count)")
            host_planes.append(w)
        parr = (C.c_void_p * max(len(host_planes), 1))(*[w.ctypes.data for w in host_planes])
        scores, ids, counts, base = self._host_out(B, L, extra=1)
        dropped = np.empty((B,), dtype=np.int32)
        words, rows = self._host_mask(mask)
        thr = float("nan") if score_threshold is None else float(score_threshold)
        check(_lib.lib().hx_hybrid_query_formula_host(
            self._h, _ptr(q), _ptr(q_indptr), _ptr(q_idx), _ptr(q_val), B, C.byref(params), _ptr(words), rows,
            int(bool(mask_root_only)), int(candidates_limit), self._formula_ops(ops), len(ops),
            parr if host_planes else None, len(host_planes), L, thr, _ptr(scores), _ptr(ids), _ptr(base), _ptr(counts),
            _ptr(dropped)))
        return scores, ids, base, counts, dropped

    # -- recommend search (hx.h: hx_recommend / hx_recommend_host) --------------------------------
    def _example(self, ex, rows: list, vecs: list, what: str) -> None:
        """one example onto the flat lists: a local row (an int) -> that row; anything else -> a vector of `dim`
        float32 numbers and the row -1.  what: "recommend" | "discover", for the refusal."""
        if isinstance(ex, (int, np.integer)) and not isinstance(ex, bool):
            rows.append(int(ex))
        else:
            v = np.asarray(ex, dtype=np.float32).reshape(-1)
            if v.shape[0] != self.dim:
                raise HxError(f"{what}: an example vector of {v.shape[0]} values, the index holds {self.dim}")
            rows.append(-1)
            vecs.append(v)

    @staticmethod
    def _examples_csr(indptr, rows, vecs):
        """(indptr int64 [R + 1], rows int64 [E], vecs float32 [n_raw, dim] or None) of the flat lists"""
        return (np.asarray(indptr, np.int64), np.asarray(rows, np.int64).reshape(-1),
                np.ascontiguousarray(np.stack(vecs)) if vecs else None)

    def _reco_examples(self, requests):
        """requests: per request a sequence of (example, sign) -- example = a local row (an int) or a vector of `dim`
        numbers, sign = +1 | -1 -> (indptr int64 [R + 1], rows int64 [E] with -1 for a raw vector, signs int8 [E], vecs
        float32 [n_raw, dim] or None), as hx_recommend takes them."""
        indptr, rows, signs, vecs = [0], [], [], []
        for req in requests:
            for ex, sign in req:
                self._example(ex, rows, vecs, "recommend")
                signs.append(int(sign))
            indptr.append(len(rows))
        indptr, rows, vecs = self._examples_csr(indptr, rows, vecs)
        return indptr, rows, np.asarray(signs, np.int64).clip(-128, 127).astype(np.int8).reshape(-1), vecs

    def recommend(self, requests, strategy: int, limit: int, mask=None, keys=None, counts=None):
        """Points like given examples (hx_recommend): requests as _reco_examples takes them, strategy = RECO_AVERAGE |
        RECO_BEST_SCORE | RECO_SUM_SCORES, mask = None or a row mask as hybrid_query takes it.  Returns (keys [R, limit]
        int64, counts [R] int32) on the device (keys / counts: tensors to write into); the call synchronises."""
        indptr, rows, signs, vecs = self._reco_examples(requests)
        R, L = len(indptr) - 1, int(limit)
        if keys is None or counts is None:
            keys, counts = self._out(max(R, 1), L if 1 <= L <= 1024 else 1)   # (the engine refuses; nothing huge is allocated)
        words, mrows = self._dev_mask(mask)
        check(_lib.lib().hx_recommend(self._h, int(strategy), R, _ptr(indptr), _ptr(rows), _ptr(signs), _ptr(vecs),
                                      _ptr(words), mrows, L, _ptr(keys), _ptr(counts), _stream()))
        return keys, counts

    def recommend_host(self, requests, strategy: int, limit: int, mask=None):
        """recommend, host in, host out (hx_recommend_host): (scores [R, limit] float32, ids [R, limit] int64, counts [R]
        int32), the slots past a request's count (-inf, -1)."""
        indptr, rows, signs, vecs = self._reco_examples(requests)
        R, L = len(indptr) - 1, int(limit)
        scores, ids, counts = self._host_out(max(R, 1), L, 1024)
        words, mrows = self._host_mask(mask)
        check(_lib.lib().hx_recommend_host(self._h, int(strategy), R, _ptr(indptr), _ptr(rows), _ptr(signs), _ptr(vecs),
                                           _ptr(words), mrows, L, _ptr(scores), _ptr(ids), _ptr(counts)))
        return scores[:R], ids[:R], counts[:R]

    # -- discovery and context search (hx.h: hx_discover / hx_discover_host) --------------------------
    def _discover_examples(self, requests):
        """requests: per request (target | None, [(pos, neg), ...]) -- an example = a local row (an int) or a vector of
        `dim` numbers -> (indptr int64 [R + 1], rows int64 [E] with -1 for a raw vector, vecs float32 [n_raw, dim] or
        None, has_target int32 [R]), as hx_discover takes them: the target first, then pos_0, neg_0, pos_1, ..."""
        indptr, rows, vecs, has_target = [0], [], [], []
        for target, pairs in requests:
            flat = [] if target is None else [target]
            for pair in pairs:
                pos, neg = pair
                flat += [pos, neg]
            for ex in flat:
                self._example(ex, rows, vecs, "discover")
            has_target.append(0 if target is None else 1)
            indptr.append(len(rows))
        return (*self._examples_csr(indptr, rows, vecs), np.asarray(has_target, np.int32).reshape(-1))

    def discover(self, requests, limit: int, mask=None, keys=None, counts=None):
        """Discovery (a target and context pairs) and context search (pairs only) in one exact scan (hx_discover):
        requests as _discover_examples takes them, mask = None or a row mask as hybrid_query takes it.  Returns (keys
        [R, limit] int64, counts [R] int32) on the device (keys / counts: tensors to write into); the call synchronises."""
        indptr, rows, vecs, has_target = self._discover_examples(requests)
        R, L = len(indptr) - 1, int(limit)
        if keys is None or counts is None:
            keys, counts = self._out(max(R, 1), L if 1 <= L <= 1024 else 1)   # (the engine refuses; nothing huge is allocated)
        words, mrows = self._dev_mask(mask)
        check(_lib.lib().hx_discover(self._h, R, _ptr(indptr), _ptr(rows), _ptr(vecs), _ptr(has_target), _ptr(words), mrows,
                                     L, _ptr(keys), _ptr(counts), _stream()))
        return keys, counts

    def discover_host(self, requests, limit: int, mask=None):
        """discover, host in, host out (hx_discover_host): (scores [R, limit] float32, ids [R, limit] int64, counts [R]
        int32), the slots past a request's count (-inf, -1)."""
        indptr, rows, vecs, has_target = self._discover_examples(requests)
        R, L = len(indptr) - 1, int(limit)
        scores, ids, counts = self._host_out(max(R, 1), L, 1024)
        words, mrows = self._host_mask(mask)
        check(_lib.lib().hx_discover_host(self._h, R, _ptr(indptr), _ptr(rows), _ptr(vecs), _ptr(has_target), _ptr(words),
                                          mrows, L, _ptr(scores), _ptr(ids), _ptr(counts)))
        return scores[:R], ids[:R], counts[:R]

    def discover_redone(self) -> int:
        """requests of this index that overflowed their candidate buffer and were redone in fixed chunks, so far"""
        n = C.c_int64(0)
        check(_lib.lib().hx_discover_redone(self._h, C.byref(n)))
        return int(n.value)

    # -- distance matrix search (hx.h: hx_search_matrix / hx_search_matrix_host) ----------------------
    @staticmethod
    def _matrix_args(rows, limit, score_threshold):
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        S, L = int(rows.shape[0]), int(limit)
        thr = float("-inf") if score_threshold is None else float(score_threshold)
        # (the engine refuses a bad S or limit; nothing huge is allocated for the outputs of a refused call)
        return rows, S, L, thr, (max(S, 1) if S <= 4096 else 1), (L if 1 <= L <= 1024 else 1)

    def search_matrix(self, rows, limit: int, score_threshold=None, keys=None, counts=None):
        """For every local row of the sample `rows` (distinct, any order) its nearest neighbours among the other rows of
        the sample (hx_search_matrix): score_threshold = None or the smallest sim a neighbour may have.  Returns (keys
        [S, limit] int64, counts [S] int32) on the device (keys / counts: tensors to write into); the call synchronises."""
        rows, S, L, thr, out_rows, out_cols = self._matrix_args(rows, limit, score_threshold)
        if keys is None or counts is None:
            keys, counts = self._out(out_rows, out_cols)
        check(_lib.lib().hx_search_matrix(self._h, _ptr(rows), S, L, thr, _ptr(keys), _ptr(counts), _stream()))
        return keys, counts

    def search_matrix_host(self, rows, limit: int, score_threshold=None):
        """search_matrix, host out (hx_search_matrix_host): (scores [S, limit] float32, ids [S, limit] int64, counts [S]
        int32), the slots past a row's count (-inf, -1)."""
        rows, S, L, thr, out_rows, out_cols = self._matrix_args(rows, limit, score_threshold)
        scores, ids, counts = self._host_out(out_rows, out_cols)
        check(_lib.lib().hx_search_matrix_host(self._h, _ptr(rows), S, L, thr, _ptr(scores), _ptr(ids), _ptr(counts)))
        return scores[:S], ids[:S], counts[:S]

    # -- late-interaction rerank (hx.h: HX_PAY_TOKENS / hx_maxsim / hx_hybrid_query_rerank_host) --
    def payload_create_tokens(self, dim_t: int) -> int:
        """A new empty token column of `dim_t` int8 values per token (hx_payload_create_tokens); returns its id."""
        col = C.c_int32()
        check(_lib.lib().hx_payload_create_tokens(self._h, int(dim_t), C.byref(col)))
        return col.value

    @staticmethod
    def _token_cells(heads, x8, scales):
        heads, x8, scales = np.ascontiguousarray(heads), np.ascontiguousarray(x8), np.ascontiguousarray(scales)
        if (heads.dtype != np.uint32 or heads.ndim != 1 or x8.dtype != np.int8 or x8.ndim != 2
                or scales.dtype != np.float32 or scales.ndim != 1):
            raise TypeError("payload tokens: 1-d np.uint32 heads, [n_tokens, dim_t] np.int8 tokens, 1-d np.float32 scales")
        if x8.shape[0] != scales.shape[0]:
            raise ValueError(f"{x8.shape[0]} tokens but {scales.shape[0]} scales")
        return heads, x8, scales

    def _token_dim(self, col: int) -> int:
        head, count, dim_t = C.c_uint32(), C.c_int64(), C.c_int32()
        if self.payload_rows(col) == 0:
            return 0                                          # (nothing stored: the engine checks the bytes it is given)
        check(_lib.lib().hx_payload_debug_tokens(self._h, int(col), 0, C.byref(head), None, None, 0, C.byref(count),
                                                 C.byref(dim_t)))
        return dim_t.value

    def payload_append_tokens(self, col: int, heads: np.ndarray, x8: np.ndarray, scales: np.ndarray) -> None:
        """The cells of the next len(heads) rows of a token column (hx_payload_append_tokens): heads np.uint32 -- MISSING,
        NULL or the row's token count --, x8 [n_tokens, dim_t] np.int8 the rows' tokens one after another, scales
        [n_tokens] np.float32 (late_interaction.quantize_tokens makes both)."""
        heads, x8, scales = self._token_cells(heads, x8, scales)
        check(_lib.lib().hx_payload_append_tokens(self._h, int(col), _ptr(heads), heads.shape[0], _ptr(x8), _ptr(scales),
                                                  x8.shape[0]))

    def payload_replace_tokens(self, col: int, rows, heads: np.ndarray, x8: np.ndarray, scales: np.ndarray) -> None:
        """New cells for the stored rows `rows` of a token column (hx_payload_replace_tokens), in the order of `rows`."""
        rows = self._rows(rows)
        heads, x8, scales = self._token_cells(heads, x8, scales)
        if heads.shape[0] != rows.shape[0]:
            raise ValueError(f"{rows.shape[0]} rows but {heads.shape[0]} heads")
        check(_lib.lib().hx_payload_replace_tokens(self._h, int(col), _ptr(rows), rows.shape[0], _ptr(heads), _ptr(x8),
                                                   _ptr(scales), x8.shape[0]))

    def payload_debug_tokens(self, col: int, row: int):
        """One row of a token column (hx_payload_debug_tokens): (head, x8 [Td, dim_t] np.int8, scales [Td] np.float32) --
        head = MISSING, NULL or the token count."""
        head, count, dim_t = C.c_uint32(), C.c_int64(), C.c_int32()
        check(_lib.lib().hx_payload_debug_tokens(self._h, int(col), int(row), C.byref(head), None, None, 0, C.byref(count),
                                                 C.byref(dim_t)))
        x8 = np.zeros((max(count.value, 1), dim_t.value), dtype=np.int8)
        sc = np.zeros(max(count.value, 1), dtype=np.float32)
        check(_lib.lib().hx_payload_debug_tokens(self._h, int(col), int(row), C.byref(head), _ptr(x8), _ptr(sc), count.value,
                                                 C.byref(count), C.byref(dim_t)))
        return head.value, x8[:count.value], sc[:count.value]

    @staticmethod
    def _query_tokens(q8, qscale, q_indptr):
        q8, qscale = np.ascontiguousarray(q8), np.ascontiguousarray(qscale)
        q_indptr = np.ascontiguousarray(q_indptr, dtype=np.int64)
        if q8.dtype != np.int8 or q8.ndim != 2 or qscale.dtype != np.float32 or qscale.ndim != 1 or q_indptr.ndim != 1:
            raise TypeError("query tokens: [n_tokens, dim_t] np.int8, [n_tokens] np.float32 scales, [B + 1] offsets")
        if q8.shape[0] != qscale.shape[0] or q_indptr.shape[0] < 2 or q_indptr[-1] != q8.shape[0]:
            raise ValueError("query tokens: the offsets, the tokens and the scales disagree")
        return q8, qscale, q_indptr

    def maxsim(self, col: int, keys: torch.Tensor, counts: Optional[torch.Tensor], q8: np.ndarray, qscale: np.ndarray,
               q_indptr: np.ndarray, limit: int, eligible=None, out=None, out_counts=None):
        """The pools keys [B, stride] (+ counts [B], None = every slot) ordered by the MaxSim of the queries' tokens
        against the rows' tokens in the token column `col` (hx_maxsim).  q8 [n_tokens, dim_t] np.int8 / qscale [n_tokens]
        np.float32: the queries' tokens one after another, q_indptr [B + 1] the first token of every query.  eligible as
        mmr takes it.  Returns (out_keys [B, limit] int64 carrying the MaxSim scores, 0 past the eligible positions;
        counts [B] int32).  out / out_counts: the tensors to write (tests hand in sentinels).  Only enqueues work."""
        keys, counts, B, stride = self._pool_args(keys, counts)
        q8, qscale, q_indptr = self._query_tokens(q8, qscale, q_indptr)
        L = int(limit)
        if q_indptr.shape[0] != B + 1:
            raise ValueError(f"{q_indptr.shape[0] - 1} queries' tokens for {B} pools")
        dim_t = self._token_dim(col)
        if dim_t and q8.shape[1] != dim_t:
            raise ValueError(f"query tokens of {q8.shape[1]} values for a column of {dim_t}")
        slots = L if 1 <= L <= 2048 else 1                  # (the engine refuses; nothing huge is allocated)
        words, rows = self._dev_mask(eligible)
        dq8 =torch.from_numpy(q8.reshape(-1) if q8.size else np.zeros(16, np.int8)).to(keys.device)
        dqs = torch.from_numpy(qscale if qscale.size else np.zeros(1, np.float32)).to(keys.device)
        dip = torch.from_numpy(q_indptr).to(keys.device)
        if out is None:
            out = torch.empty((B, slots), dtype=torch.int64, device=keys.device)
        if out_counts is None:
            out_counts = torch.empty((B,), dtype=torch.int32, device=keys.device)
        check(_lib.lib().hx_maxsim(self._h, int(col), _ptr(keys), stride, _ptr(counts), B, _ptr(dq8), _ptr(dqs), _ptr(dip),
                                   _ptr(q_indptr), _ptr(words), rows, L, _ptr(out), _ptr(out_counts), _stream()))
        return out, out_counts

    def hybrid_query_rerank_host(self, q: np.ndarray, q_indptr: np.ndarray, q_idx: np.ndarray, q_val: np.ndarray,
                                 params: HxParams, col: int, q8: np.ndarray, qscale: np.ndarray, qtok_indptr: np.ndarray,
                                 limit: int, candidates_limit: int = 0, mask=None, mask_root_only: bool = False):
        """hybrid_query_host followed by the MaxSim rerank of its pool (hx_hybrid_query_rerank_host): the query runs with
        final_limit = the pool (candidates_limit = 0: the mode's whole pool; params.final_limit is not used), the pool's
        rows that hold tokens come back ordered by MaxSim.  q8 / qscale / qtok_indptr as maxsim takes them; mask /
        mask_root_only as hybrid_query_mmr_host.  Returns (scores [B, limit] float32 -- MaxSim --, ids [B, limit] int64,
        first_scores [B, limit] float32 -- what the pool carried --, counts [B] int32), the slots past the counts
        (-inf, -1, -inf)."""
        q, q_indptr, q_idx, q_val, B = self._host_queries(q, q_indptr, q_idx, q_val)
        q8, qscale, qtok_indptr = self._query_tokens(q8, qscale, qtok_indptr)
        L = int(limit)
        if qtok_indptr.shape[0] != B + 1:
            raise ValueError(f"{qtok_indptr.shape[0] - 1} queries' tokens for {B} queries")
        if not 1 <= L <= 2048:
            raise HxError("maxsim: limit out of range [1, 2048]")
        dim_t = self._token_dim(col)
        if dim_t and q8.shape[1] != dim_t:
            raise ValueError(f"query tokens of {q8.shape[1]} values for a column of {dim_t}")
        scores, ids, counts, first = self._host_out(B, L, extra=1)
        words, rows = self._host_mask(mask)
        check(_lib.lib().hx_hybrid_query_rerank_host(self._h, _ptr(q), _ptr(q_indptr), _ptr(q_idx), _ptr(q_val), B,
                                                     C.byref(params), _ptr(words), rows, int(bool(mask_root_only)),
                                                     int(candidates_limit), int(col), _ptr(q8), _ptr(qscale),
                                                     _ptr(qtok_indptr), L, _ptr(scores), _ptr(ids), _ptr(first),
                                                     _ptr(counts)))
        return scores, ids, first, counts


# -- index-free stages -------------------------------------------------------------------
def rrf(a_keys: torch.Tensor, a_cnt: torch.Tensor, b_keys: torch.Tensor, b_cnt: torch.Tensor,
        limit: int = 10, k: float = 2.0, rank_base: int = 0):
    dev = a_keys.device
    B = a_keys.shape[0]
    keys = torch.empty((B, limit), dtype=torch.int64, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    check(_lib.lib().hx_rrf(dev.index or 0, _ptr(a_keys.contiguous()), a_keys.shape[1], _ptr(a_cnt),
                            _ptr(b_keys.contiguous()), b_keys.shape[1], _ptr(b_cnt), B, k, rank_base, limit,
                            _ptr(keys), _ptr(cnt), _stream()))
    return keys, cnt


def sparse_idf_apply(q_val: torch.Tensor, df: torch.Tensor, n_docs: torch.Tensor, out: Optional[torch.Tensor] = None):
    """q_val * idf(n_docs, df) per position (hx_sparse_idf_apply; include/hx.h states the arithmetic): q_val float32
    [nnz], df int64 [nnz], n_docs int64 [1], all on one device.  `out` may be q_val; a new tensor when None."""
    q_val = _need_cuda(q_val, torch.float32, "q_val").reshape(-1)
    df = _need_cuda(df, torch.int64, "df").reshape(-1)
    n_docs = _need_cuda(n_docs, torch.int64, "n_docs").reshape(-1)
    if df.shape != q_val.shape or n_docs.shape[0] != 1:
        raise HxError("sparse_idf_apply: one df per value and one n_docs")
    if out is None:
        out = torch.empty_like(q_val)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
              and out.numel() == q_val.numel()):
        raise HxError("sparse_idf_apply: out must be a contiguous cuda float32 tensor of q_val's size")
    check(_lib.lib().hx_sparse_idf_apply(q_val.device.index or 0, _ptr(q_val), _ptr(df), _ptr(n_docs), q_val.shape[0],
                                         _ptr(out), _stream()))
    return out


FUSE_RRF, FUSE_DBSF = 0, 1
FUSE_METHODS = {"rrf": FUSE_RRF, "dbsf": FUSE_DBSF}


def fuse(lists: Sequence[torch.Tensor], counts: Sequence[torch.Tensor], method="rrf", weights=None, limit: int = 10,
         k: float = 2.0, rank_base: int = 0):
    """N ranked lists -> one (hx_fuse; include/hx.h states the arithmetic): lists[l] [B, stride_l] int64 keys, counts[l]
    [B] int32, method "rrf" | "dbsf" (or the HX_FUSE_* code), weights = one number per list or None (all 1).  Returns
    (keys [B, limit], counts [B]).  What the entry refuses raises HxError."""
    if len(lists) == 0 or len(lists) != len(counts):
        raise HxError("fuse: one count tensor per list, at least one list")
    lists = [_need_cuda(t, torch.int64, "lists") for t in lists]
    counts = [_need_cuda(c, torch.int32, "counts") for c in counts]
    dev = lists[0].device
    B = lists[0].shape[0]
    if any(t.dim() != 2 or t.shape[0] != B or t.device != dev for t in lists) or \
            any(c.numel() != B or c.device != dev for c in counts):
        raise HxError("fuse: every list is [B, stride] and every count [B], on one device")
    n = len(lists)
    code = FUSE_METHODS.get(method, method) if isinstance(method, str) else method
    if isinstance(code, str):
        raise HxError(f"fuse: unknown method {method!r}")
    kp = (C.c_void_p * n)(*[t.data_ptr() for t in lists])
    cp = (C.c_void_p * n)(*[c.data_ptr() for c in counts])
    st = (C.c_int32 * n)(*[t.shape[1] for t in lists])
    wp = None
    if weights is not None:
        weights = [float(w) for w in weights]
        if len(weights) != n:
            raise HxError(f"fuse: {n} lists need {n} weights")
        wp = (C.c_float * n)(*weights)
    keys = torch.empty((B, limit), dtype=torch.int64, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    check(_lib.lib().hx_fuse(dev.index or 0, int(code), n, kp, st, cp, wp, B, float(k), int(rank_base), int(limit),
                             _ptr(keys), _ptr(cnt), _stream()))
    return keys, cnt


def h1_fuse(gathered: torch.Tensor, world: int, dense_limit: int, sparse_limit: int, limit: int = 10,
            k: float = 2.0, rank_base: int = 0):
    """gathered: [world * B, dense_limit + sparse_limit], rank-major (all_gather_into_tensor of h1_local):
    global dense and sparse lists, then RRF (hx_h1_fuse)."""
    dev = gathered.device
    gathered = gathered.contiguous()
    B = gathered.shape[0] // world
    keys = torch.empty((B, limit), dtype=torch.int64, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    check(_lib.lib().hx_h1_fuse(dev.index or 0, _ptr(gathered), world, B, dense_limit, sparse_limit, limit, k,
                                rank_base, _ptr(keys), _ptr(cnt), _stream()))
    return keys, cnt


def h1_plan(dense_limit: int, sparse_limit: int, world: int):
    """(k1, k2, lp, k3, lout) of the candidates-first exchange for `world` shards (hx_h1_plan)."""
    v = [C.c_int32() for _ in range(5)]
    check(_lib.lib().hx_h1_plan(dense_limit, sparse_limit, world, *[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def dense_route(B: int, L: int, cand: str = "i8", retry_level: int = 0):
    """(lp, cap, finish_e, compact_nw, compact_e) of search_dense's full-vector stage for B queries and limit L
    (hx_dense_route; cand "i8" | "f16"): finish_e 0 = three launches, else k_dense_finish's keys per lane; compact
    (0, 0) = the LDS sort.  No index and no device are involved."""
    if cand not in ("i8", "f16"):
        raise ValueError("cand must be 'i8' or 'f16'")
    v = [C.c_int32() for _ in range(5)]
    check(_lib.lib().hx_dense_route(B, L, 1 if cand == "i8" else 0, retry_level, *[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def scan8_form(B: int, row_bytes: int, kind: str = "i8") -> int:
    """Kernel of the whole-collection candidate scan for B queries over rows of row_bytes bytes (hx_scan8_form): 0 = k_scan,
    1 = k_scan8 (256 x 256 tile), 2 = its 256 x 128 form, 3 = k_scan8q, the query-stationary form.  No index, no device."""
    if kind not in ("i8", "f16"):
        raise ValueError("kind must be 'i8' or 'f16'")
    v = C.c_int32()
    check(_lib.lib().hx_scan8_form(B, row_bytes, 1 if kind == "i8" else 0, C.byref(v)))
    return int(v.value)


def scan8_log_waves(tiles: int, nq_tiles: int, qs: bool) -> float:
    """Waves that share the log appends of a scan launch over `tiles` 256-row tiles (hx_scan8_log_waves)."""
    v = C.c_double()
    check(_lib.lib().hx_scan8_log_waves(tiles, nq_tiles, 1 if qs else 0, C.byref(v)))
    return float(v.value)


def scan8q_items(row_begin: int, row_end: int, nq_tiles: int, perm_mul: int, perm_n: int, block: int):
    """The walk of workgroup `block` of a k_scan8q launch (hx_scan8q_items: the kernel's cursor on the host): (tiles,
    rows), the physical 256-row tile and the first physical row of every 64-row item, in order.  No index, no device."""
    n = C.c_int32()
    check(_lib.lib().hx_scan8q_items(row_begin, row_end, nq_tiles, perm_mul, perm_n, block, 0, None, None, C.byref(n)))
    tiles = (C.c_uint32 * max(n.value, 1))()
    rows = (C.c_int64 * max(n.value, 1))()
    check(_lib.lib().hx_scan8q_items(row_begin, row_end, nq_tiles, perm_mul, perm_n, block, n.value, tiles, rows, C.byref(n)))
    return list(tiles[:n.value]), list(rows[:n.value])


def h1_finish(reduced: torch.Tensor, world: int, B: int, lp: int, k3: int, dense_limit: int, sparse_limit: int,
              limit: int = 10, k: float = 2.0, rank_base: int = 0, nfail: Optional[torch.Tensor] = None):
    """reduced: the all-reduced (integer sum over the `world` ranks) result of h1_rescore_async.  Returns (keys [B, limit],
    counts [B], nfail [1]): nfail = queries whose lists are not final (hx_h1_finish adds to it)."""
    dev = reduced.device
    reduced = reduced.contiguous()
    keys = torch.empty((B, limit), dtype=torch.int64, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    if nfail is None:
        nfail = torch.zeros((1,), dtype=torch.int32, device=dev)
    check(_lib.lib().hx_h1_finish(dev.index or 0, _ptr(reduced), world, B, lp, k3, dense_limit, sparse_limit, limit, k,
                                  rank_base, _ptr(keys), _ptr(cnt), _ptr(nfail), _stream()))
    return keys, cnt, nfail


def merge(keys_in: torch.Tensor, counts_in: Optional[torch.Tensor], limit: int, dedupe: bool = False):
    dev = keys_in.device
    keys_in = keys_in.contiguous()
    B = keys_in.shape[0]
    keys = torch.empty((B, limit), dtype=torch.int64, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    check(_lib.lib().hx_merge(dev.index or 0, _ptr(keys_in), keys_in.shape[1], _ptr(counts_in), B, limit,
                              1 if dedupe else 0, _ptr(keys), _ptr(cnt), _stream()))
    return keys, cnt


def unpack(keys: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    keys = keys.contiguous()
    scores = torch.empty(keys.shape, dtype=torch.float32, device=keys.device)
    ids = torch.empty(keys.shape, dtype=torch.int64, device=keys.device)
    check(_lib.lib().hx_unpack(keys.device.index or 0, _ptr(keys), keys.numel(), _ptr(scores), _ptr(ids),
                               _stream()))
    return scores, ids


def synth_queries_dense(dim: int, q0: int, B: int, seed: int, device: int = 0) -> torch.Tensor:
    q = torch.empty((B, dim), dtype=torch.float32, device=torch.device("cuda", device))
    check(_lib.lib().hx_synth_queries_dense(dim, q0, B, seed, _ptr(q), _stream()))
    return q
