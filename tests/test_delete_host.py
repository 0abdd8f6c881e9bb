"""CPU: the host side of per-point deletes -- hx_retain_rows' argument checks (nothing touches a device), the handler's
delete_points over a stub index that records the keep mask it is given, the mask cache after a delete, and the
refusals.  No GPU needed."""
from __future__ import annotations

import asyncio
import ctypes as C

import numpy as np
import pytest

from rag_application_amd import filters as F


def unpack(words, n):
    return np.unpackbits(np.asarray(words, np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)


# ---- the C entry -----------------------------------------------------------------------------------------------------
def test_retain_rows_argument_errors_need_no_device():
    from rag_application_amd import _lib, build
    build.build()
    lib = _lib.lib()
    removed = C.c_int64(-7)
    words = (C.c_uint32 * 4)(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert lib.hx_retain_rows(None, C.addressof(words), 100, C.byref(removed)) != 0
    assert b"NULL" in lib.hx_last_error()
    assert lib.hx_retain_rows(None, None, 100, C.byref(removed)) != 0
    assert lib.hx_last_error()
    # a NULL mask with mask_rows > 0 is refused before the index is looked at: `fake` is never read
    fake = (C.c_uint8 * 65536)()
    assert lib.hx_retain_rows(C.addressof(fake), None, 100, C.byref(removed)) != 0
    assert b"mask is NULL" in lib.hx_last_error()
    assert lib.hx_retain_rows(C.addressof(fake), None, -1, C.byref(removed)) != 0
    assert removed.value == -7                              # a refused call reports nothing


def test_binding_and_index_method_exist():
    from rag_application_amd import _lib, engine
    assert "hx_retain_rows" in _lib.EXPORTS
    assert callable(engine.HxIndex.retain)


# ---- the handler -----------------------------------------------------------------------------------------------------
class _StubIndex:
    """stands in for the engine index: records every keep mask, counts rows the way the engine would"""

    def __init__(self, n):
        self.n = n
        self.retained = []

    def retain(self, keep):
        words = np.asarray(keep)
        assert words.dtype == np.uint32 and words.shape == ((self.n + 31) // 32,)
        self.retained.append(words.copy())
        kept = int(unpack(words, self.n).sum())
        removed, self.n = self.n - kept, kept
        return removed

    def add(self, dense, *a):
        self.n += len(dense)

    def count(self):
        return self.n

    def hybrid_query_host(self, *a, **k):
        raise AssertionError("the engine was searched")

    def close(self):
        pass


def _handler(n, seed=0):
    from rag_application_amd.handler import QdrantHandler, _Collection
    rng = np.random.default_rng(seed)
    h = QdrantHandler()
    col = _Collection.__new__(_Collection)
    col.dim, col.msizes, col.index, col.sparse_enabled = 4, (), _StubIndex(n), True
    col.ids = [f"id{r}" for r in range(n)]
    col.payloads = [{"document_id": f"doc{int(rng.integers(0, 9))}", "chunk_number": r} for r in range(n)]
    col._masks = {}
    h._collections["u"] = col
    return h, col


def _doc(k):
    return {"must": [{"key": "document_id", "match": {"value": f"doc{k}"}}]}


@pytest.mark.parametrize("n", [1, 31, 32, 33, 100, 1000])
def test_delete_by_filter(n):
    h, col = _handler(n, seed=n)
    ids0, pay0 = list(col.ids), list(col.payloads)
    flt = _doc(3)
    hit = np.array([p["document_id"] == "doc3" for p in pay0], bool)
    want_mask = ~F.row_mask(ids0, pay0, flt)
    if n % 32:
        want_mask[-1] &= np.uint32((1 << (n % 32)) - 1)
    got = asyncio.run(h.delete_points("u", filters=flt))
    assert got == int(hit.sum())
    if got:
        assert len(col.index.retained) == 1
        np.testing.assert_array_equal(col.index.retained[0], want_mask)      # bit for bit ~row_mask, bits past n clear
    else:
        assert col.index.retained == []
    assert col.ids == [i for i, d in zip(ids0, hit) if not d]
    assert col.payloads == [p for p, d in zip(pay0, hit) if not d]
    assert asyncio.run(h.get_collection_chunk_count("u")) == n - got
    assert asyncio.run(h.get_collection_chunk_count("u", filters=flt)) == 0
    other = int(sum(p["document_id"] == "doc4" for p in pay0))
    assert asyncio.run(h.get_collection_chunk_count("u", filters=_doc(4))) == other


def test_delete_by_ids_and_by_both():
    n = 500
    h, col = _handler(n, seed=5)
    ids0, pay0 = list(col.ids), list(col.payloads)
    listed = ["id0", "id7", "id31", "id32", "id499", "no-such-id"]
    assert asyncio.run(h.delete_points("u", point_ids=listed)) == 5
    gone = np.isin(np.arange(n), [0, 7, 31, 32, 499])
    np.testing.assert_array_equal(unpack(col.index.retained[-1], n), ~gone)
    assert col.ids == [i for i, d in zip(ids0, gone) if not d]
    # the same ids again: nothing left to delete, the engine is not called
    assert asyncio.run(h.delete_points("u", point_ids=listed)) == 0
    assert len(col.index.retained) == 1
    # a filter and ids together: the union
    ids1, pay1 = list(col.ids), list(col.payloads)
    by_flt = np.array([p["document_id"] == "doc2" for p in pay1], bool)
    by_id = np.array([i in ("id100", "id101") for i in ids1], bool)
    both = by_flt | by_id
    assert asyncio.run(h.delete_points("u", filters=_doc(2), point_ids=["id100", "id101"])) == int(both.sum())
    np.testing.assert_array_equal(unpack(col.index.retained[-1], len(ids1)), ~both)
    assert col.ids == [i for i, d in zip(ids1, both) if not d]
    assert col.payloads == [p for p, d in zip(pay1, both) if not d]
    assert col.index.count() == len(col.ids) == n - 5 - int(both.sum())


def test_a_delete_followed_by_as_many_adds_does_not_serve_a_stale_mask():
    """the cache decides staleness by the row count: k rows deleted, k rows added -- the count is the old one, the rows
    are not"""
    n = 300
    h, col = _handler(n, seed=9)
    flt = _doc(1)
    before = asyncio.run(h.get_collection_chunk_count("u", filters=flt))          # caches the filter's mask
    assert F.filter_key(flt) in col._masks and before > 0
    k = asyncio.run(h.delete_points("u", point_ids=[f"id{r}" for r in range(0, 40, 2)]))
    assert k == 20 and col._masks == {}
    col.ids.extend(f"new{r}" for r in range(k))                                     # k rows arrive, every one matches
    col.payloads.extend({"document_id": "doc1", "chunk_number": 1000 + r} for r in range(k))
    col.index.add(np.zeros((k, 4), np.float32))
    assert len(col.ids) == n
    fresh = F.row_mask(col.ids, col.payloads, flt)
    np.testing.assert_array_equal(col.row_mask(flt), fresh)
    assert asyncio.run(h.get_collection_chunk_count("u", filters=flt)) == int(unpack(fresh, n).sum())


def test_refusals():
    h, col = _handler(50)
    for kw in ({}, {"filters": None, "point_ids": None}, {"filters": {}, "point_ids": []}):
        with pytest.raises(ValueError, match="filter or point ids"):
            asyncio.run(h.delete_points("u", **kw))
    with pytest.raises(KeyError):
        asyncio.run(h.delete_points("nobody", point_ids=["id1"]))
    with pytest.raises(ValueError, match="unsupported filter clause"):
        asyncio.run(h.delete_points("u", filters={"musst": []}))
    assert col.index.retained == [] and len(col.ids) == 50


def test_an_engine_refusal_leaves_ids_and_payloads_alone():
    h, col = _handler(50)

    def refuse(keep):
        raise RuntimeError("refused")
    col.index.retain = refuse
    with pytest.raises(RuntimeError):
        asyncio.run(h.delete_points("u", point_ids=["id3"]))
    assert len(col.ids) == 50 and len(col.payloads) == 50


def test_sharded_handler_refuses_without_touching_its_ranks():
    from rag_application_amd.handler import QdrantHandler
    from rag_application_amd.sharded import ShardedHandler
    assert QdrantHandler._point_deletes and not ShardedHandler._point_deletes
    h = ShardedHandler.__new__(ShardedHandler)              # no process group: any command to a rank would fail loudly

    def no_command(*a, **k):
        raise AssertionError("a command was sent to the ranks")
    h._command = no_command
    _, col = _handler(10)
    h._collections = {"u": col}
    with pytest.raises(ValueError, match="sharded collection"):
        asyncio.run(h.delete_points("u", point_ids=["id1"]))
    assert col.index.retained == [] and len(col.ids) == 10
