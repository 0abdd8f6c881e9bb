"""Drop-in for the reference's `QdrantHandler`
(app/core/vector_store/qdrant/qdrant_handler.py:14-481): same class name, same async
methods, same argument meaning and the same error conventions -- search and count
never raise (they return [] / 0, :384-386, :479-481), mutations re-raise (:196-198,
:265-267, :437-439), `create_collection` raises ValueError on an empty user id
(:39-40).  Where the reference ships a Prefetch tree to a Qdrant server over HTTP
(:363-372), this class calls the HIP engine through the C ABI (include/hx.h).

Additive: `hybrid_search_batch` (the reference is strictly one query per call) and a
configurable dense size (the reference hard-codes 768, :138-139; that stays the
default)."""
from __future__ import annotations

import asyncio
import itertools
import json
import logging
import os
import threading
import uuid
from dataclasses import asdict, dataclass, field
from typing import Any, Dict, List, Optional

import numpy as np

from . import boosting as _boosting
from . import engine as _engine
from . import faceting as _faceting
from . import filters as _filters
from . import fusion as _fusion
from . import grouping as _grouping
from . import late_interaction as _late
from . import matrix as _matrix
from . import payload_index as _pindex
from . import query_tree as _query_tree
from . import scrolling as _scrolling
from .matrix import MatrixOffsets, MatrixPair
from ._lib import HX_MODE_H1, HX_MODE_TREE


@dataclass
class ScoredPoint:
    """What callers duck-type on (qdrant_handler.py:377;
    app/services/agents/search_orchestration_workflow.py:70-73, 168-175)."""
    id: str
    version: int
    score: float
    payload: Optional[Dict[str, Any]] = None
    vector: Optional[Any] = None
    shard_key: Optional[Any] = None
    order_value: Optional[Any] = None

    def dict(self):
        return asdict(self)

    model_dump = dict


@dataclass
class PointGroup:
    """One group of hybrid_search_groups (shape-compatible with qdrant_client.http.models.PointGroup): `id` = the value
    of the group_by field its hits share (a str, a bool or an int), `hits` = its ScoredPoints, best first."""
    id: Any
    hits: List[ScoredPoint] = field(default_factory=list)


@dataclass
class FacetHit:
    """One value of a facet (shape-compatible with qdrant_client.http.models.FacetValueHit): `value` = a value of the
    faceted field (a str, a bool or an int), `count` = the points holding it."""
    value: Any
    count: int


@dataclass
class Record:
    """One point of scroll / retrieve (shape-compatible with qdrant_client.http.models.Record): `order_value` = the
    value an ordered scroll placed the point by (a number; a datetime's integer microseconds since the epoch), None
    otherwise."""
    id: str
    payload: Optional[Dict[str, Any]] = None
    vector: Optional[Any] = None
    shard_key: Optional[Any] = None
    order_value: Optional[Any] = None

    def dict(self):
        return asdict(self)

    model_dump = dict


@dataclass
class MmrPoint(ScoredPoint):
    """One hit of hybrid_search_mmr: a ScoredPoint whose `score` is its relevance (the dense cosine to the query) and
    whose `mmr_score` is the value it was picked at, (1 - diversity) * score - diversity * (its largest similarity to
    the hits picked before it)."""
    mmr_score: float = 0.0


@dataclass
class RerankedPoint(ScoredPoint):
    """One hit of hybrid_search_rerank: a ScoredPoint whose `score` is the MaxSim of the query's tokens against the
    point's tokens and whose `first_score` is the score the point carried in the hybrid pool."""
    first_score: float = 0.0


@dataclass
class BoostedPoint(ScoredPoint):
    """One hit of hybrid_search_boost: a ScoredPoint whose `score` is the value the formula gave the point and whose
    `base_score` is the score the point carried in the hybrid pool (the formula's "$score")."""
    base_score: float = 0.0


@dataclass
class SparseVector:
    """Shape-compatible with qdrant_client.http.models.SparseVector."""
    indices: List[int] = field(default_factory=list)
    values: List[float] = field(default_factory=list)


def _sparse_parts(sv):
    """Accept {"indices": [...], "values": [...]} or an object with .indices/.values
    (qdrant_handler.py:348-351)."""
    if isinstance(sv, dict):
        return sv["indices"], sv["values"]
    return sv.indices, sv.values


def _check_modifier(m):
    """the sparse modifier of a collection: None, or "idf" (Qdrant's Modifier.IDF)"""
    m = getattr(m, "value", m)
    if m is not None and not (isinstance(m, str) and m.lower() == "idf"):
        raise ValueError(f"sparse_modifier must be None or 'idf', got {m!r}")
    return None if m is None else "idf"


class _Collection:
    """One user collection: the engine index (anything with HxIndex's add / hybrid_query_host / count / save /
    close: sharded.ShardedHandler plugs in a row-sharded one) plus the point ids and payloads, which never cross
    the C ABI and are indexed by the engine's row id = insertion order."""

    def __init__(self, dim, msizes, device, index=None):
        self.dim = dim
        self.msizes = tuple(msizes)
        self.index = index if index is not None else _engine.HxIndex(dim, self.msizes, device=device)
        self.ids: List[str] = []
        self.payloads: List[Dict[str, Any]] = []
        self.sparse_enabled = True
        self.sparse_modifier: Optional[str] = None     # None | "idf" 
        self.binary_quantization = False               # the index keeps a 1-bit copy of the rows
        self._masks: Dict[str, Any] = {}
        self.pindex: Optional[_pindex.PayloadIndex] = None
        self.tokens: Optional[Dict[str, Any]] = None

    MASK_CACHE = 64   # filters whose row masks a collection keeps (least recently used first out): n / 8 bytes each

    def row_mask(self, flt) -> np.ndarray:
        """The packed row mask of `flt` (filters.row_mask), cached by the filter's canonical JSON: rows appended since
        the last evaluation are the only rows evaluated again.  The cache holds the MASK_CACHE most recent filters."""
        key = _filters.filter_key(flt)
        n = len(self.ids)
        done, prev = self._masks.pop(key, (0, None))
        if done != n:
            dev = self._device_mask(flt, n)               # a payload index and a filter that compiles: one kernel
            prev = dev if dev is not None else _filters.row_mask(self.ids, self.payloads, flt, start=done, prev=prev)
        self._masks[key] = (n, prev)                      # (dicts keep insertion order: the last used is last)
        while len(self._masks) > self.MASK_CACHE:
            del self._masks[next(iter(self._masks))]
        return prev

    # -- payload index (payload_index.py) ---------------------------------------------------------
    def _id_rows(self) -> Optional[Dict[str, int]]:
        """id -> row, built lazily, extended by the rows appended since, discarded by a delete; None when two rows
        share an id (has_id then goes the Python way)."""
        m = getattr(self, "_idrows", None)
        if m is None:
            m = self._idrows = {}
            self._idrows_n = 0
        for r in range(self._idrows_n, len(self.ids)):
            m[self.ids[r]] = r
        self._idrows_n = len(self.ids)
        return m if len(m) == len(self.ids) else None

    def first_rows(self) -> Dict[str, int]:
        """id -> row for the searches that take point ids; an id held twice: the first row that holds it"""
        rows = self._id_rows()
        if rows is None:
            rows = {}
            for r, pid in enumerate(self.ids):
                rows.setdefault(pid, r)
        return rows

    def _device_mask(self, flt, n: int) -> Optional[np.ndarray]:
        """The packed row mask of `flt` from hx_payload_mask, or None: no payload index, or the filter is declined."""
        pi = getattr(self, "pindex", None)
        if pi is None:
            return None
        prog = pi.compile(flt, self._id_rows)
        if prog is not None:
            try:
                if self.index.count() != n:
                    raise RuntimeError("the engine's row count differs from the payloads'")
                mask, _ = self.index.payload_mask(prog[0], prog[1], want_count=False)
                words = self.index.mask_host(mask)
                pi.device_evals += 1
                return words
            except Exception as e:                        # never a wrong mask: the Python loop is always right
                logging.warning("payload index: device evaluation failed, Python path taken: %s", e)
                pi.declined["engine refused"] = pi.declined.get("engine refused", 0) + 1
        pi.python_evals += 1
        return None

    FACET_SCHEMAS = ("keyword", "bool", "keyword_list", "bool_list")

    def facet(self, key: str, flt, limit: int):
        """[(value, count)] of the field `key` over the rows `flt` keeps: at most `limit` values, count descending, then
        value ascending (faceting.py states the rules).  A key with a live keyword / bool (or _list) column is counted
        and ranked on the device (hx_payload_facet_host) under the packed mask of `flt`; everything else -- an unindexed
        or poisoned key, another schema, a limit above 2048, an engine refusal, a stray code -- is counted by faceting.py
        over the payloads under the same mask."""
        _faceting.check_limit(limit)
        if not isinstance(key, str) or not key:
            raise ValueError("key must be a non-empty string (a payload key, dotted paths allowed)")
        mask = self.row_mask(flt) if flt else None
        pi = getattr(self, "pindex", None)
        k = pi.keys.get(key) if pi is not None else None
        if (k is not None and k.col is not None and k.schema in self.FACET_SCHEMAS and not k.array
                and limit <= _faceting.MAX_LIMIT
                and hasattr(self.index, "payload_facet_host")):
            n_codes = len(k.codes) if k.elem == "keyword" else 2
            try:
                if n_codes == 0:                          # a keyword column that never saw a keyword: nothing to count
                    pi.facet_device_calls += 1
                    return []
                if self.index.count() != len(self.ids):
                    raise RuntimeError("the engine's row count differs from the payloads'")
                first, counts, stray = self.index.payload_facet_host(k.col, n_codes, limit, rank=k.ranks(), mask=mask)
                if stray == 0:
                    pi.facet_device_calls += 1
                    return [(k.value_at(r), c) for r, c in zip(first.tolist(), counts.tolist())]
                logging.warning("facet on %r: %d cells outside the dictionary, Python path taken", key, stray)
            except Exception as e:                        # never a wrong count: the walk over the payloads is always right
                logging.warning("facet on %r: the device path failed, Python path taken: %s", key, e)
        if pi is not None:
            pi.facet_python_calls += 1
        return _faceting.facet_top(_faceting.facet_counts(self.payloads, key, keep=mask), limit)

    SCROLL_SCHEMAS = ("number", "datetime")

    def _row_of(self, point_id) -> int:
        """The row of a point id (the first one, should two rows share it); ValueError for an id the collection does not
        hold."""
        rows = self._id_rows()
        try:
            r = rows.get(point_id) if rows is not None else self.ids.index(point_id)
        except (TypeError, ValueError):
            r = None
        if r is None:
            raise ValueError(f"offset: the collection holds no point with id {point_id!r}")
        return r

    def scroll(self, flt, limit: int, offset=None, order_by=None):
        """([(row, order value or None)], next_page_offset) of one page of `limit` points (scrolling.py states the
        rules).  No order_by: the kept rows from the row of the id `offset` on (hx_scroll_rows_host).  order_by on a key
        with a live "number" / "datetime" column: the ordered page under the packed mask of `flt` (hx_payload_order_host),
        continued after the cursor offset = {"value": v, "id": point_id}.  Everything else -- an unindexed or poisoned
        key, another schema, a bound no double holds, an engine refusal -- is walked by scrolling.py over the payloads
        under the same mask.  One more point than the page is asked for: it says whether anything follows."""
        _scrolling.check_limit(limit, _scrolling.MAX_LIMIT - 1)
        n = len(self.ids)
        pi = getattr(self, "pindex", None)
        device = hasattr(self.index, "scroll_rows_host")
        if order_by is None:
            start = 0 if offset is None else self._row_of(offset)
            mask = self.row_mask(flt) if flt else None
            rows = None
            if device:
                try:
                    if self.index.count() != n:
                        raise RuntimeError("the engine's row count differs from the payloads'")
                    rows = self.index.scroll_rows_host(limit + 1, start, mask=mask).tolist()
                    if pi is not None:
                        pi.scroll_device_calls += 1
                except Exception as e:                    # never a wrong page: the walk over the mask is always right
                    logging.warning("scroll: the device path failed, Python path taken: %s", e)
            if rows is None:
                if pi is not None:
                    pi.scroll_python_calls += 1
                rows = _scrolling.scroll_rows(n, mask, start, limit + 1)
            nxt = self.ids[rows[limit]] if len(rows) > limit else None
            return [(r, None) for r in rows[:limit]], nxt
        key, desc, start_from = _scrolling.check_order_by(order_by)
        after = None
        if offset is not None:
            if not isinstance(offset, dict) or set(offset) != {"value", "id"}:
                raise ValueError('offset of an ordered scroll must be {"value": ..., "id": ...} (a next_page_offset)')
            av = _scrolling.order_value(offset["value"])
            if av is None:
                raise ValueError("offset: value must be a number that is not a NaN, a datetime or an RFC 3339 string")
            after = (av, self._row_of(offset["id"]))
        mask = self.row_mask(flt) if flt else None
        k = pi.keys.get(key) if pi is not None else None
        hits = None
        if device and k is not None and k.col is not None and k.schema in self.SCROLL_SCHEMAS and not k.array:
            sf = None if start_from is None else _pindex.exact_double(start_from)
            af = None if after is None else _pindex.exact_double(after[0])
            if (start_from is None or sf is not None) and (after is None or af is not None):
                try:
                    if self.index.count() != n:
                        raise RuntimeError("the engine's row count differs from the payloads'")
                    rows, _ = self.index.payload_order_host(k.col, limit + 1, desc=desc, start_from=sf,
                                                            after=None if after is None else (af, after[1]), mask=mask)
                    # the order value as the payload holds it (an int stays an int): what the Python path returns
                    hits = [(r, _scrolling.order_value(_filters._get(self.payloads[r], key))) for r in rows.tolist()]
                    pi.scroll_device_calls += 1
                except Exception as e:
                    logging.warning("scroll by %r: the device path failed, Python path taken: %s", key, e)
                    hits = None
        if hits is None:
            if pi is not None:
                pi.scroll_python_calls += 1
            hits = _scrolling.ordered_rows(self.payloads, key, desc, keep=mask, start_from=start_from, after=after,
                                           limit=limit + 1)
        page = hits[:limit]
        nxt = {"value": page[-1][1], "id": self.ids[page[-1][0]]} if len(hits) > limit else None
        return page, nxt

    def _poison(self, key: str) -> None:
        k = self.pindex.keys[key]
        if k.col is not None:
            try:
                self.index.payload_drop(k.col)
            except Exception as e:
                logging.warning("payload index: dropping the column of %r failed: %s", key, e)
        k.col = None

    def create_payload_index(self, key: str, schema: str) -> bool:
        """Index `key` (again): encode every stored row in one pass and append the cells to a new column.  True when
        the key is live, False when a stored value poisoned it."""
        if not hasattr(self.index, "payload_create"):
            raise ValueError("this collection's engine index has no payload columns")
        if getattr(self, "pindex", None) is None:
            self.pindex = _pindex.PayloadIndex()
        pi = self.pindex
        if key in pi.keys:
            self._poison(key)
        elif len(pi.keys) >= _pindex.MAX_COLUMNS:
            raise ValueError(f"a collection takes at most {_pindex.MAX_COLUMNS} payload indexes")
        k = _pindex._Key(schema, key)                     # (ValueError for a malformed array key "A[].f")
        if k.array and not hasattr(self.index, "payload_same_offsets"):
            raise ValueError("this collection's engine index has no nested blocks")
        if k.is_list and not hasattr(self.index, "payload_append_lists"):
            raise ValueError("this collection's engine index has no list columns")
        if k.is_text and not hasattr(self.index, "payload_append_text"):
            raise ValueError("this collection's engine index has no text columns")
        pi.keys[key] = k
        cells = pi.encode(key, self.payloads)
        if cells is None:
            return False
        col = self.index.payload_create(k.kind)
        try:
            self._append_cells(k, col, cells)
            if k.array and not self._aligned(key, col):
                logging.warning("payload index: %r is not aligned with its siblings, the key is dropped", key)
                self.index.payload_drop(col)
                return False
        except Exception:
            self.index.payload_drop(col)
            raise
        k.col = col
        return True

    def _aligned(self, key: str, col: int) -> bool:
        """Whether the new column of an array key has the heads and offsets of a live key of the same parent
        (hx_payload_same_offsets; one check when a second key of a parent goes live: a nested block needs it)."""
        parent = self.pindex.keys[key].array[0]
        for name, other in self.pindex.keys.items():
            if name != key and other.col is not None and other.array and other.array[0] == parent:
                return self.index.payload_same_offsets(other.col, col)
        return True

    def _append_cells(self, k, col: int, cells) -> None:
        if k.is_list:                                     # (heads, values): hx_payload_append_lists
            self.index.payload_append_lists(col, cells[0], cells[1])
        elif k.is_text:                                   # (heads, bytes): hx_payload_append_text
            self.index.payload_append_text(col, cells[0], cells[1])
        else:
            self.index.payload_append(col, cells)

    def delete_payload_index(self, key: str) -> bool:
        pi = getattr(self, "pindex", None)
        if pi is None or key not in pi.keys:
            return False
        self._poison(key)
        del pi.keys[key]
        return True

    def append_payload_cells(self, payloads) -> None:
        """The cells of rows just added, for every live key.  A value that poisons a key, or an engine failure, drops
        that key's column; the upsert stands."""
        pi = getattr(self, "pindex", None)
        if pi is None:
            return
        heads_of: Dict[str, np.ndarray] = {}              # one heads array per array parent and batch
        for key in pi.live_keys():
            try:
                cells = pi.encode(key, payloads, heads_of)
                if cells is not None:
                    self._append_cells(pi.keys[key], pi.keys[key].col, cells)
                    continue
            except Exception as e:
                logging.warning("payload index: appending to %r failed, the key is dropped: %s", key, e)
            self._poison(key)

    def replace_payload_cells(self, rows, payloads) -> None:
        """The cells of rows replaced in place, for every live key (hx_payload_replace / _replace_lists / _replace_text).  A value that
        poisons a key, or an engine failure, drops that key's column, as append_payload_cells does."""
        pi = getattr(self, "pindex", None)
        if pi is None:
            return
        rows = np.asarray(rows, np.int64)
        heads_of: Dict[str, np.ndarray] = {}
        for key in pi.live_keys():
            k = pi.keys[key]
            try:
                cells = pi.encode(key, payloads, heads_of)
                if cells is not None:
                    if k.is_list:
                        self.index.payload_replace_lists(k.col, rows, cells[0], cells[1])
                    elif k.is_text:
                        self.index.payload_replace_text(k.col, rows, cells[0], cells[1])
                    else:
                        self.index.payload_replace(k.col, rows, cells)
                    continue
            except Exception as e:
                logging.warning("payload index: replacing cells of %r failed, the key is dropped: %s", key, e)
            self._poison(key)

    # -- token multivectors (late_interaction.py) ---------------------------------------------------
    # self.tokens = None, or {"dim": the token width, "col": the engine column or None (dropped: rebuilt on next use),
    # "cells": one entry per row, None (no vector) or (x8 [T, dim] int8, scales [T] float32)}: the quantised tokens stay on
    # the host as the payloads do, the column is derived from them.
    def create_token_index(self, dim: int) -> None:
        if not hasattr(self.index, "payload_create_tokens"):
            raise ValueError("this collection's engine index has no token columns")
        dim = _late.check_dim(dim)
        tk = getattr(self, "tokens", None)
        if tk is not None:
            if tk["dim"] != dim:
                raise ValueError(f"the collection holds a token index of width {tk['dim']}")
            return
        self.tokens = {"dim": dim, "col": None, "cells": [None] * len(self.ids)}
        self._token_column()

    def token_cells_of(self, items) -> Optional[list]:
        """The quantised token cells of chunks (None for a chunk without "token_embeddings"); None when the collection
        has no token index and no chunk brings tokens.  Everything that can raise comes before the engine is touched."""
        tk = getattr(self, "tokens", None)
        have = [item.get("token_embeddings") is not None for item in items]
        if tk is None:
            if any(have):
                raise ValueError('"token_embeddings" needs a token index: call create_token_index first')
            return None
        return [_late.quantize_tokens(_late.pad_dim(item["token_embeddings"], tk["dim"])) if h else None
                for item, h in zip(items, have)]

    def _token_column(self) -> int:
        """The live token column, rebuilt from the host cells when there is none (never made, dropped by a delete it
        lagged, or lost to an engine failure)."""
        tk = self.tokens
        if tk["col"] is not None:
            try:
                if self.index.payload_rows(tk["col"]) == len(self.ids):
                    return tk["col"]
                self.index.payload_drop(tk["col"])
            except Exception:
                pass                                       # (the engine dropped it)
            tk["col"] = None
        col = self.index.payload_create_tokens(tk["dim"])
        try:
            if tk["cells"]:
                self.index.payload_append_tokens(col, *_late.pack_tokens(tk["cells"], tk["dim"])[:3])
        except Exception:
            self.index.payload_drop(col)
            raise
        tk["col"] = col
        return col

    def _token_fail(self, what: str, e: Exception) -> None:
        logging.warning("token index: %s failed, the column is dropped and rebuilt on next use: %s", what, e)
        tk = self.tokens
        if tk["col"] is not None:
            try:
                self.index.payload_drop(tk["col"])
            except Exception:
                pass
        tk["col"] = None

    def append_token_cells(self, cells) -> None:
        """The token cells of rows just added (`cells` from token_cells_of; None = no token index)."""
        tk = getattr(self, "tokens", None)
        if tk is None:
            return
        cells = cells if cells is not None else []
        n0 = len(tk["cells"])
        tk["cells"].extend(cells)
        if tk["col"] is None:
            return
        try:
            if self.index.payload_rows(tk["col"]) != n0:
                raise RuntimeError("the column's row count differs from the cells'")
            self.index.payload_append_tokens(tk["col"], *_late.pack_tokens(cells, tk["dim"])[:3])
        except Exception as e:
            self._token_fail("appending", e)

    def replace_token_cells(self, rows, cells) -> None:
        """The token cells of rows replaced in place (hx_payload_replace_tokens)."""
        tk = getattr(self, "tokens", None)
        if tk is None:
            return
        for r, c in zip(rows, cells):
            tk["cells"][r] = c
        if tk["col"] is None:
            return
        try:
            self.index.payload_replace_tokens(tk["col"], np.asarray(rows, np.int64), *_late.pack_tokens(cells, tk["dim"])[:3])
        except Exception as e:
            self._token_fail("replacing", e)

    def close(self):
        self.index.close()

    # on-disk form (the reference asks Qdrant for on_disk storage, qdrant_handler.py:47-55, 62):
    # <dir>/<user>.hx = the engine's file, <dir>/<user>.json = point ids + payloads, <dir>/<user>.tokens.npz = the
    # quantised tokens of a collection with a token index (the JSON names the index)
    def save(self, base: str):
        self.index.save(base + ".hx")
        tk = getattr(self, "tokens", None)
        if tk is not None:
            state = np.asarray([0 if c is None else 1 for c in tk["cells"]], np.uint8)
            _, x8, sc, indptr = _late.pack_tokens(tk["cells"], tk["dim"])
            with open(base + ".tokens.npz", "wb") as f:
                np.savez(f, state=state, x8=x8, scales=sc, indptr=indptr)
        elif os.path.exists(base + ".tokens.npz"):
            os.remove(base + ".tokens.npz")
        with open(base + ".json", "w") as f:
            json.dump({"dim": self.dim, "msizes": list(self.msizes), "sparse_enabled": self.sparse_enabled,
                       "sparse_modifier": getattr(self, "sparse_modifier", None),
                       "binary_quantization": bool(getattr(self, "binary_quantization", False)),
                       "ids": self.ids, "payloads": self.payloads,
                       "payload_indexes": self.pindex.definitions() if getattr(self, "pindex", None) else {},
                       "token_index": {"dim": tk["dim"]} if tk is not None else None}, f)

    @classmethod
    def load(cls, base: str, device: int, index_loader=None):
        with open(base + ".json") as f:
            meta = json.load(f)
        self = cls.__new__(cls)
        self.dim = int(meta["dim"])
        self.msizes = tuple(meta["msizes"])
        self.index = (index_loader(base + ".hx", meta) if index_loader is not None
                      else _engine.HxIndex.load(base + ".hx", device=device))
        self.ids = list(meta["ids"])
        self.payloads = list(meta["payloads"])
        self.sparse_enabled = bool(meta["sparse_enabled"])
        self.sparse_modifier = _check_modifier(meta.get("sparse_modifier"))   # (an old file has no such key)
        # the 1-bit copy is derived data (the engine's file does not hold it): made again here, before the first search
        self.binary_quantization = bool(meta.get("binary_quantization", False))
        if self.binary_quantization:
            self.index.binary_enable()
        self._masks = {}
        self.pindex = None
        # the payload indexes are derived data: the sidecar names them (old files have none), the payloads rebuild them
        if hasattr(self.index, "payload_create"):
            for key, schema in (meta.get("payload_indexes") or {}).items():
                self.create_payload_index(str(key), _pindex.schema_of(schema))
        self.tokens = None
        tdef = meta.get("token_index")
        if tdef and hasattr(self.index, "payload_create_tokens"):
            dim = _late.check_dim(int(tdef["dim"]))
            with np.load(base + ".tokens.npz") as z:
                state, x8, sc, indptr = z["state"], z["x8"], z["scales"], z["indptr"]
            if state.shape[0] != len(self.ids) or indptr.shape[0] != len(self.ids) + 1 or x8.shape[1:] != (dim,):
                raise ValueError("the token sidecar does not belong to this collection")
            cells = [(np.ascontiguousarray(x8[indptr[r]:indptr[r + 1]]), np.ascontiguousarray(sc[indptr[r]:indptr[r + 1]]))
                     if state[r] else None for r in range(len(self.ids))]
            self.tokens = {"dim": dim, "col": None, "cells": cells}
            self._token_column()
        return self


FILTER_STAGES = ("root", "all")
QUERY_FILTER_STAGES = ("root", "node", "all")   # of query_points: "node" = every node's own filter
RECO_MAX_LIMIT, RECO_MAX_REQUESTS, RECO_MAX_EXAMPLES = 1024, 16, 32   # HX_RECO_MAX_* of hx.h
RECO_STRATEGIES = {"average_vector": 0, "best_score": 1, "sum_scores": 2}   # HX_RECO_AVERAGE / _BEST_SCORE / _SUM_SCORES
MMR_MAX_LIMIT = 256                   # HX_MMR_MAX_LIMIT of hx.h: most hits hybrid_search_mmr picks per query
BOOST_MAX_LIMIT = _boosting.MAX_LIMIT  # most hits hybrid_search_boost returns per query (hx.h: hx_formula)


class QdrantHandler:
    """Handles vector operations for hybrid search with dense and sparse vectors."""

    # filter_stages="all" (the engine's pre-filtered query) needs one engine index per collection
    _masked_search = True
    # delete_points renumbers the rows of ONE engine index (hx_retain_rows)
    _point_deletes = True
    # upsert_points replaces rows of ONE engine index in place (hx_replace_rows)
    _point_upserts = True
    # payload columns live in ONE engine index, beside the rows whose payloads this process holds
    _payload_indexes = True
    # hybrid_search_groups groups the pool of ONE engine index, by a column of that index or by this process's payloads
    _grouped_search = True
    # hybrid_search_mmr picks from the pool of ONE engine index, by the rows of that index
    _mmr_search = True
    # facet counts the payload columns of ONE engine index, or this process's payloads
    _facets = True
    # token columns live in ONE engine index; hybrid_search_rerank reranks the pool of that index
    _late_rerank = True
    # hybrid_search_boost values the pool of ONE engine index by the payload columns of that index
    _boost_search = True
    # recommend scans the rows of ONE engine index and looks its examples up in this process's ids
    _recommend = True
    # discover scans the rows of ONE engine index and looks its examples up in this process's ids
    _discover = True
    # scroll pages the rows of ONE engine index and the ids and payloads this process holds
    _scroll = True
    # search_matrix_pairs / _offsets compare rows of ONE engine index with each other
    _matrix_search = True
    # query_points runs a caller's tree over the stage entries of ONE engine index
    _query_tree = True
    # sparse_modifier="idf" reads the term statistics of ONE engine index
    _sparse_modifiers = True
    # binary_quantization=True keeps a 1-bit copy of the rows of ONE engine index
    _binary_quantization = True

    def __init__(self, reranker=None, device: int = 0, persist_dir: Optional[str] = None):
        # The reference loads jinaai/jina-colbert-v2 here (:17-22) and falls back to the
        # un-reranked list whenever reranking raises (:410-412).  `reranker` is any object
        # with rerank_documents(query, documents, max_tokens) -> list of indices.
        self.reranker = reranker
        self.device = device
        # persist_dir (additive): collections found there are loaded on first use, `save_collection`
        # writes them back.  None = in-memory only.
        self.persist_dir = persist_dir
        self._collections: Dict[str, _Collection] = {}
        self._lock = threading.Lock()

    async def _run(self, fn, *a):
        loop = asyncio.get_running_loop()

        def locked():
            with self._lock:
                return fn(*a)
        return await loop.run_in_executor(None, locked)

    # ------------------------------------------------- what the search entries share
    async def _guarded(self, what, user_id, empty, fn, *a, failed=None):
        """The async face of a search entry: fn(*a) under the lock; a ValueError is logged and raised, any other failure
        is logged and answered with `empty`.  what / failed: how the two log lines name the call ("... for %s")."""
        try:
            return await self._run(fn, *a)
        except ValueError as ve:
            logging.error(what + " refused: %s", user_id, ve)
            raise
        except Exception as e:
            logging.error((failed or what) + " failed: %s", user_id, e)
            return empty

    @staticmethod
    def _check_int(name, v, lo, hi):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")

    @staticmethod
    def _check_candidates(candidates_limit):
        if candidates_limit is not None and (isinstance(candidates_limit, bool) or not isinstance(candidates_limit, int)
                                             or candidates_limit < 1):
            raise ValueError(f"candidates_limit must be a positive integer or None, got {candidates_limit!r}")

    @staticmethod
    def _is_number(v) -> bool:
        """an int or a float that is no bool and no NaN"""
        return not isinstance(v, bool) and isinstance(v, (int, float)) and v == v

    @staticmethod
    def _check_stages(filter_stages):
        if filter_stages not in FILTER_STAGES:
            raise ValueError(f"filter_stages must be one of {FILTER_STAGES}, got {filter_stages!r}")

    @staticmethod
    def _check_mode(mode):
        if mode not in ("tree", "h1"):
            raise ValueError("mode must be 'tree' (the reference query) or 'h1'")

    @staticmethod
    def _root_filter(filters, mode, filter_stages) -> bool:
        """whether `filters` is the root's filter (:297, :371), which only the reference query has"""
        root_filter = bool(filters) and filter_stages == "root"
        if root_filter and mode != "tree":
            raise ValueError("filters belong to the reference query's root (:297, :371): use mode='tree' "
                             "(or filter_stages='all')")
        return root_filter

    def _routing(self, filters, mode, filter_stages) -> bool:
        """The routing arguments of a pool entry, checked in this order: filter_stages, mode, a root filter outside the
        reference query.  Returns whether `filters` is a root filter.  (_search_sync runs the three checks between
        steps of its own, in the order it always had.)"""
        self._check_stages(filter_stages)
        self._check_mode(mode)
        return self._root_filter(filters, mode, filter_stages)

    @staticmethod
    def _pool_max(hp, mode) -> int:
        """the longest pool the mode hands out: tree = the root's re-scored union, h1 = the fused list"""
        return min(int(hp.dense_limit) + int(hp.rrf_limit if mode == "tree" else hp.sparse_limit), 2048)

    def _pool_size(self, hp, mode, want) -> int:
        """the pool of a pool entry: `want` (candidates_limit / group_pool) clipped to the mode's maximum, None = the
        maximum; an empty pool is refused"""
        pool_max = self._pool_max(hp, mode)
        if pool_max < 1:
            raise ValueError("the search_params leave an empty pool")
        return pool_max if want is None else min(want, pool_max)

    @staticmethod
    def _check_filter(filters) -> None:
        if filters:
            _filters.matches({}, filters)                  # validates the clause names before any GPU work

    def _filter_mask(self, col, filters):
        """the packed row mask of `filters` (None = no filter), its clause names validated first"""
        self._check_filter(filters)
        return col.row_mask(filters) if filters else None

    @staticmethod
    def _points(col, scores, rows, counts, cls=ScoredPoint, extra=None):
        """Per query the first counts[b] (score, row) pairs as points of `cls`.  extra: one more float column [B, L] for
        the one field a subclass adds behind ScoredPoint's seven (mmr_score / first_score / base_score)."""
        cids, cpay = col.ids, col.payloads
        if extra is None:                                  # (python floats / ints in one go)
            return [[cls(id=cids[r], version=0, score=s, payload=cpay[r]) for s, r in zip(sc[:n], rw[:n])]
                    for sc, rw, n in zip(scores.tolist(), rows.tolist(), counts.tolist())]
        return [[cls(cids[r], 0, s, cpay[r], None, None, None, x) for s, r, x in zip(sc[:n], rw[:n], ex[:n])]
                for sc, rw, ex, n in zip(scores.tolist(), rows.tolist(), extra.tolist(), counts.tolist())]

    @staticmethod
    def _example_resolver(col, what):
        """example -> its stored row (a point id: a str or an int) or a float32 vector of `dim` finite numbers (anything
        else); what: "recommend" | "discover", for the refusals"""
        id_rows = None

        def example(ex):
            nonlocal id_rows
            if isinstance(ex, (str, int)) and not isinstance(ex, bool):
                if id_rows is None:
                    id_rows = col.first_rows()
                if str(ex) not in id_rows:
                    raise ValueError(f"{what}: unknown point id {ex!r}")
                return id_rows[str(ex)]
            try:
                v = np.asarray(ex, dtype=np.float32).reshape(-1)
            except (TypeError, ValueError):
                raise ValueError(f"{what}: an example is a point id or a vector of numbers") from None
            if v.shape[0] != col.dim:
                raise ValueError(f"example dimension {v.shape[0]} != collection dimension {col.dim}")
            if not np.isfinite(v).all():
                raise ValueError(f"{what}: example vector values must be finite")
            return v
        return example

    # ---------------------------------------------------------------- create_collection
    async def create_collection(self, user_id: str, dense_vector_size: int = 768,
                                matryoshka_sizes: list = [64, 128, 256], quantized_size: int = 768,
                                sparse_enabled: bool = True, force_recreate: bool = False,
                                sparse_modifier: Optional[str] = None, binary_quantization: bool = False):
        """sparse_modifier (additive): None = the reference's collection (no IDF, :24-32), "idf" = Qdrant's
        SparseVectorParams(modifier=Modifier.IDF): every sparse query weight is multiplied by the collection's IDF of
        its term at query time.  It is fixed at creation.
        binary_quantization (additive): True = Qdrant's quantization_config=BinaryQuantization: the engine keeps one sign
        bit per dimension beside the rows, a using="binary" node of query_points and search_binary rank by it (DESIGN.md
        section 33).  It is fixed at creation and stored with the collection."""
        try:
            if not user_id:
                raise ValueError("user_id cannot be empty")
            user_id = str(user_id)
            sparse_modifier = _check_modifier(sparse_modifier)
            if not isinstance(binary_quantization, (bool, np.bool_)):
                raise ValueError(f"binary_quantization must be True or False, got {binary_quantization!r}")
            binary_quantization = bool(binary_quantization)
            if binary_quantization and not self._binary_quantization:
                raise ValueError("binary_quantization=True is not supported on a sharded collection: the shard command "
                                 "protocol has no binary stage")
            if sparse_modifier and not self._sparse_modifiers:
                raise ValueError("sparse_modifier='idf' is not supported on a sharded collection: the shard command "
                                 "protocol carries no collection statistics (sharded.ShardedCollection does)")
            if user_id in self._collections and not force_recreate:
                have = getattr(self._collections[user_id], "sparse_modifier", None)
                if have != sparse_modifier:
                    raise ValueError(f"collection {user_id} exists with sparse_modifier={have!r}: the modifier of a "
                                     "live collection cannot change (force_recreate=True makes a new one)")
                have = bool(getattr(self._collections[user_id], "binary_quantization", False))
                if have != binary_quantization:
                    raise ValueError(f"collection {user_id} exists with binary_quantization={have!r}: the quantization of "
                                     "a live collection cannot change (force_recreate=True makes a new one)")
                logging.info("create_collection: %s is already there", user_id)
                return
            if quantized_size != dense_vector_size:
                raise ValueError("quantized_size must equal dense_vector_size")

            def make():
                old = self._collections.pop(user_id, None)
                if old is not None:
                    self._drop(user_id, old)
                col = self._open_collection(
                    user_id, int(dense_vector_size), [int(m) for m in matryoshka_sizes], bool(sparse_enabled),
                    bool(force_recreate))
                have = getattr(col, "sparse_modifier", None)
                if have != sparse_modifier:
                    if have is not None or getattr(col, "ids", None):   # a stored collection keeps what it was created with
                        self._drop(user_id, col)
                        raise ValueError(f"stored collection has sparse_modifier={have!r}")
                    col.sparse_modifier = sparse_modifier
                have = bool(getattr(col, "binary_quantization", False))
                if have != binary_quantization:
                    if have or getattr(col, "ids", None):               # ... and so does its quantization
                        self._drop(user_id, col)
                        raise ValueError(f"stored collection has binary_quantization={have!r}")
                    col.index.binary_enable()
                    col.binary_quantization = True
                self._collections[user_id] = col
            await self._run(make)
            logging.info("create_collection: new collection for %s", user_id)
        except ValueError as ve:
            logging.error("create_collection(%s) refused: %s", user_id, ve)
            raise
        except Exception as e:
            logging.critical(f"Collection creation failed for user {user_id}: {str(e)}")
            raise

    # the two places a collection's engine index is made and dropped: sharded.ShardedHandler overrides them
    def _open_collection(self, user_id, dim, msizes, sparse_enabled, force_recreate) -> _Collection:
        base = self._base(user_id)
        if base and not force_recreate and os.path.exists(base + ".hx") and os.path.exists(base + ".json"):
            col = _Collection.load(base, self.device)
            if col.dim != dim:
                col.close()
                raise ValueError("stored collection has another vector size")
        else:
            col = _Collection(dim, msizes, self.device)
            col.sparse_enabled = sparse_enabled
        return col

    def _drop(self, user_id, col: _Collection) -> None:
        col.close()

    def _base(self, user_id: str) -> Optional[str]:
        if not self.persist_dir:
            return None
        safe = "".join(ch if ch.isalnum() or ch in "-_." else "_" for ch in str(user_id))
        return os.path.join(self.persist_dir, safe)

    async def save_collection(self, user_id: str) -> None:
        """Write the collection to persist_dir (additive; Qdrant persists on its own)."""
        if not self.persist_dir:
            raise ValueError("handler was created without persist_dir")
        col = self._collections[str(user_id)]
        os.makedirs(self.persist_dir, exist_ok=True)
        await self._run(col.save, self._base(user_id))

    # ------------------------------------------------------------------- payload indexes
    async def create_payload_index(self, user_id: str, field_name: str, field_schema: str = "keyword") -> bool:
        """Qdrant's create_payload_index (additive: the reference creates none): index the payload field `field_name` (a
        dotted path) as "keyword" | "number" ("integer" / "float" mean the same) | "bool".  Filters on indexed fields are
        then evaluated by one kernel over the collection's columns instead of a Python loop over its payloads
        (payload_index.py); the results are the same.  Returns True when the field is live, False when a stored value is
        not of the schema (a list, a dict, another type, NaN, an int beyond 2^53): such a field stays on the Python path.
        List-valued fields (the reference's `languages`; lists of scalars) take the opt-in schemas
        "keyword_list" | "number_list" ("integer_list" / "float_list") | "bool_list": a value is then None, a list of
        values of the element schema or one such value (the one-element list); a tuple, a nested list or dict, a None
        element or an element of another type makes the field stay on the Python path.
        Text fields (the reference's `content`, `file_description`, `document_summary`, `context`) take the opt-in schema
        "text": a value is then None or a `str`, and `match text` on the field is evaluated on the device (DESIGN.md
        section 19); any other value makes the field stay on the Python path.
        Datetime fields (the chat messages' `timestamp`) take the opt-in schema "datetime": a value is then None, a
        `datetime.datetime` or an RFC 3339 string, stored as its microseconds since the epoch; the field serves ordered
        scrolls, filters on it stay on the Python path.
        Arrays of objects (the reference's `entities` and `relationships`) take array keys: `field_name` = "A[].f" with
        exactly one "[]" and the schema "keyword" | "number" | "bool" indexes the field `f` of the objects of the array
        `A`; {"key": "A[].f", ...} (some object matches) and {"nested": {"key": "A", "filter": ...}} (ONE object meets the
        whole filter) are then evaluated on the device.  A value of another type, or -- under
        "number" -- an object without the field, makes the key stay on the Python path; the other keys of `A` go on.
        Raises ValueError for a bad schema, a malformed array key, a sharded collection, or an engine index without payload
        (list, text) columns; KeyError for an unknown collection."""
        try:
            if not self._payload_indexes:
                raise ValueError("create_payload_index is not supported on a sharded collection")
            schema = _pindex.schema_of(field_schema)
            if not isinstance(field_name, str) or not field_name:
                raise ValueError("field_name must be a non-empty string")
            col = self._collections[str(user_id)]          # KeyError if absent: re-raised
            return bool(await self._run(col.create_payload_index, field_name, schema))
        except Exception as e:
            logging.error("create_payload_index(%s, %s) failed: %s", user_id, field_name, e)
            raise

    async def delete_payload_index(self, user_id: str, field_name: str) -> bool:
        """Drop the index on `field_name`; True when there was one.  Filters on the field go the Python way again."""
        try:
            col = self._collections[str(user_id)]
            return bool(await self._run(col.delete_payload_index, field_name))
        except Exception as e:
            logging.error("delete_payload_index(%s, %s) failed: %s", user_id, field_name, e)
            raise

    # --------------------------------------------------------------------------- upserts
    async def _store(self, user_id, items, emb_key_payload):
        if str(user_id) not in self._collections:
            await self.create_collection(user_id=user_id)
        col = self._collections[str(user_id)]
        dense, indptr, idx, val, ids, payloads = [], [0], [], [], [], []
        for item in items:
            if len(item["dense_embedding"]) != col.dim:
                raise ValueError(
                    f"Dense vector dimension mismatch. Expected {col.dim}, got {len(item['dense_embedding'])}")
            dense.append(np.asarray(item["dense_embedding"], dtype=np.float32))
            si, sv = _sparse_parts(item["sparse_embedding"]) if col.sparse_enabled else ([], [])
            idx.extend(int(i) for i in si)
            val.extend(float(v) for v in sv)
            indptr.append(len(idx))
            ids.append(str(uuid.uuid4()))
            payloads.append(emb_key_payload(item))
        if not dense:
            return 0
        tcells = col.token_cells_of(items)                 # (quantised here: a refusal comes before the engine)

        def add():
            col.index.add(np.stack(dense), np.asarray(indptr, np.int64), np.asarray(idx, np.int32),
                          np.asarray(val, np.float32))
            col.ids.extend(ids)
            col.payloads.extend(payloads)
            col.append_payload_cells(payloads)
            col.append_token_cells(tcells)
        await self._run(add)
        return len(dense)

    @staticmethod
    def _document_payload(chunk):
        """the payload of one document chunk (qdrant_handler.py:165-185)"""
        metadata = chunk["chunk_metadata"]
        return {
            "document_id": metadata["document_id"],
            "user_id": metadata["user_id"],
            "file_name": metadata["file_name"],
            "mime_type": metadata["mime_type"],
            "file_size": metadata["file_size"],
            "file_description": metadata["description"],
            "file_path": metadata["file_path"],
            "context_version": metadata["context_version"],
            "chunk_number": metadata["chunk_number"],
            "entities": metadata.get("entities"),
            "relationships": metadata.get("relationships"),
            "context": metadata.get("context"),
            "document_summary": metadata["doc_summary"],
            "content": str(chunk["content"]),
            "page_number": metadata.get("page_number"),
            "languages": metadata.get("languages"),
            "element_id": metadata.get("element_id"),
            "is_continuation": metadata.get("is_continuation"),
            "category": metadata.get("category"),
        }

    async def store_document_vectors(self, embedded_chunks: List[Dict[str, Any]], user_id: str):
        """Stores document chunks with multi-stage embeddings (qdrant_handler.py:120-198)."""
        try:
            n = await self._store(user_id, embedded_chunks, self._document_payload)
            logging.info("store_document_vectors: %d chunks added for %s", n, user_id)
        except Exception as e:
            logging.error("store_document_vectors failed: %s", e)
            raise

    # --------------------------------------------------------------------- upsert by id
    def _upsert_sync(self, user_id, items, point_ids) -> int:
        col = self._collections[str(user_id)]
        if len(items) != len(point_ids):
            raise ValueError(f"{len(items)} chunks but {len(point_ids)} point ids")
        named = [str(p) for p in point_ids if p is not None]
        if len(set(named)) != len(named):
            raise ValueError("upsert_points: a point id is listed twice")
        for item in items:
            if len(item["dense_embedding"]) != col.dim:
                raise ValueError(
                    f"Dense vector dimension mismatch. Expected {col.dim}, got {len(item['dense_embedding'])}")
        id_rows = col._id_rows()
        if id_rows is None:
            raise ValueError("upsert_points: the collection holds one id twice")

        def pack(sel):
            dense, indptr, idx, val = [], [0], [], []
            for k in sel:
                item = items[k]
                dense.append(np.asarray(item["dense_embedding"], dtype=np.float32))
                si, sv = _sparse_parts(item["sparse_embedding"]) if col.sparse_enabled else ([], [])
                idx.extend(int(i) for i in si)
                val.extend(float(v) for v in sv)
                indptr.append(len(idx))
            return (np.stack(dense), np.asarray(indptr, np.int64), np.asarray(idx, np.int32), np.asarray(val, np.float32))
        old = [k for k, p in enumerate(point_ids) if p is not None and str(p) in id_rows]
        new = [k for k, p in enumerate(point_ids) if p is None or str(p) not in id_rows]
        rows = [id_rows[str(point_ids[k])] for k in old]
        payloads = [self._document_payload(item) for item in items]
        tcells = col.token_cells_of(items)
        packed_new = pack(new) if new else None             # (everything that can raise in Python comes before the engine)
        packed_old = pack(old) if old else None
        n0 = len(col.ids)
        # append first, then replace: a refused replace rolls the appended rows back, the call is all or nothing
        if new:
            col.index.add(*packed_new)
            col.ids.extend(str(point_ids[k]) if point_ids[k] is not None else str(uuid.uuid4()) for k in new)
            col.payloads.extend(payloads[k] for k in new)
            col.append_payload_cells([payloads[k] for k in new])
            col.append_token_cells([tcells[k] for k in new] if tcells is not None else None)
        if not old:
            return 0
        try:
            col.index.replace(np.asarray(rows, np.int64), *packed_old)
        except Exception:
            if new:
                col.index.truncate(n0)                      # (the payload columns are cut with the rows)
                del col.ids[n0:]
                del col.payloads[n0:]
                if getattr(col, "tokens", None) is not None:
                    del col.tokens["cells"][n0:]
                col._idrows = None
            raise
        for r, k in zip(rows, old):
            col.payloads[r] = payloads[k]
        col.replace_payload_cells(rows, [payloads[k] for k in old])
        if tcells is not None:
            col.replace_token_cells(rows, [tcells[k] for k in old])
        col._masks.clear()                                  # a cached mask may be wrong for a replaced row
        return len(old)

    async def upsert_points(self, user_id: str, embedded_chunks: List[Dict[str, Any]],
                            point_ids: List[Optional[str]]) -> int:
        """client.upsert with ids the caller names (qdrant_handler.py:190-193; additive: the reference always draws a
        fresh uuid4).  embedded_chunks as store_document_vectors takes them, point_ids one entry per chunk.  An id the
        collection holds: that point is replaced IN PLACE -- dense vector, sparse vector, payload -- and keeps its row,
        hence its rank among equal scores (hx_replace_rows).  An unknown id is appended under that id, None under a fresh
        uuid4.  Returns the number of points replaced.  A duplicate id within the call, a length or dimension mismatch
        or an empty user_id raises ValueError before anything changes; a batch the engine refuses leaves the collection
        as it was.  Nothing is saved: call save_collection."""
        try:
            if not user_id:
                raise ValueError("user_id cannot be empty")
            if not self._point_upserts:
                raise ValueError("upsert_points is not supported on a sharded collection")
            if len(embedded_chunks) != len(point_ids):
                raise ValueError(f"{len(embedded_chunks)} chunks but {len(point_ids)} point ids")
            if str(user_id) not in self._collections:
                await self.create_collection(user_id=user_id)
            n = await self._run(self._upsert_sync, user_id, list(embedded_chunks), list(point_ids))
            logging.info("upsert_points: %d points replaced for %s", n, user_id)
            return n
        except Exception as e:
            logging.error("upsert_points(%s) failed: %s", user_id, e)
            raise

    async def store_chat_vectors(self, embedded_payload: List[Dict[str, Any]], user_id: str):
        """Stores chat message vectors (qdrant_handler.py:200-267)."""
        try:
            def payload(chat):
                ts = chat["timestamp"]
                return {
                    "chat_id": chat["chat_id"],
                    "user_id": user_id,
                    "message_type": chat["message_type"],
                    "timestamp": ts.isoformat() if hasattr(ts, "isoformat") else ts,
                    "entities": chat["entities"],
                    "relationships": chat["relationships"],
                    "chat_summary": chat["chat_summary"],
                    "content": chat["message"],
                    "is_chat": True,
                }
            n = await self._store(user_id, embedded_payload, payload)
            logging.info("store_chat_vectors: %d messages added for %s", n, user_id)
        except Exception as e:
            logging.error("store_chat_vectors failed: %s", e)
            raise

    # ---------------------------------------------------------------------------- search
    @staticmethod
    def _pack_queries(col, dense_vectors, sparse_vectors):
        """the batch as the engine takes it: dense [B, dim] float32, the sparse queries as one CSR"""
        q = np.asarray(dense_vectors, dtype=np.float32).reshape(len(sparse_vectors), -1)
        if q.shape[1] != col.dim:
            raise ValueError(f"query dimension {q.shape[1]} != collection dimension {col.dim}")
        parts = [_sparse_parts(sv) for sv in sparse_vectors]
        indptr = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([len(si) for si, _ in parts], out=indptr[1:])
        nnz = int(indptr[-1])
        # (one pass over the batch's terms, no per-element int() / float() calls: the packing of a 1024-query batch is host
        # time the GPU waits for)
        idx = np.fromiter(itertools.chain.from_iterable(si for si, _ in parts), dtype=np.int64, count=nnz)
        val = np.fromiter(itertools.chain.from_iterable(vv for _, vv in parts), dtype=np.float64, count=nnz)
        if nnz and (idx.min() < -2 ** 31 or idx.max() >= 2 ** 31):
            raise ValueError("sparse index out of range")
        if getattr(col, "sparse_modifier", None) == "idf":
            # Modifier.IDF: the weights the engine sees are q_t * idf_t, made on the device from the collection's own
            # statistics.  This is the one place the hybrid_search* entries pack their queries.
            val = col.index.sparse_idf_host(idx, val)
        return q, indptr, idx, val

    def _search_sync(self, user_id, dense_vectors, sparse_vectors, search_params, filters, mode="tree",
                     filter_stages="root"):
        self._check_stages(filter_stages)
        if filter_stages == "all" and not self._masked_search:
            raise ValueError("filter_stages='all' is not supported on a sharded collection: use filter_stages='root'")
        col = self._collections[str(user_id)]
        q, indptr, idx, val = self._pack_queries(col, dense_vectors, sparse_vectors)
        self._check_mode(mode)
        # KeyError/TypeError like the reference when search_params lacks a key / is None
        hp = _engine.make_params(search_params, mode=HX_MODE_TREE if mode == "tree" else HX_MODE_H1)
        final_limit = int(hp.final_limit)
        if filters and filter_stages == "all":
            # the filter applies to every stage: the engine searches the kept rows only, the root included
            mask = self._filter_mask(col, filters)
            return self._points(col, *col.index.hybrid_query_host(q, indptr, idx.astype(np.int32),
                                                                  val.astype(np.float32), hp, mask=mask))
        if self._root_filter(filters, mode, filter_stages):
            # query_filter belongs to the ROOT query only (:297, :371): the union of the branches'
            # candidates (<= dense_limit + the fusion's 10) is re-scored, filtered, cut to final_limit.
            # So: ask the engine for the whole re-scored union and filter it here.
            self._check_filter(filters)
            hp.final_limit = self._pool_max(hp, mode)
        out = self._points(col, *col.index.hybrid_query_host(q, indptr, idx.astype(np.int32), val.astype(np.float32), hp))
        if filters:
            out = [[p for p in pts if _filters.matches(p.payload, filters, p.id)][:final_limit] for pts in out]
        return out

    async def hybrid_search(self, user_id: str, query_text: str, dense_vector: List[float],
                            sparse_vector: Dict[str, List[float]], image_embedding: Optional[List[float]] = None,
                            top_k: int = 10, search_params: Optional[Dict[str, Any]] = None,
                            filters: Optional[Dict] = None, filter_stages: str = "root") -> List[Dict]:
        """Matryoshka cascade, quantized + dense refinement, sparse, RRF, dense root
        re-score, reranking hook (qdrant_handler.py:269-386).  filter_stages (additive): "root" = the
        filter on the root query only, as the reference passes it (:297, :371); "all" = every stage
        searches only the rows the filter keeps (the engine's pre-filtered query)."""
        try:
            results = (await self._run(self._search_sync, user_id, [dense_vector], [sparse_vector],
                                       search_params, filters, "tree", filter_stages))[0]
            max_tokens_per_doc = 8000 // top_k
            documents = [res.payload["content"] for res in results
                         if hasattr(res, "payload") and res.payload and "content" in res.payload]
            reranked_results = await self.rerank_with_colbert(query_text, documents, results, max_tokens_per_doc)
            return reranked_results[:top_k]
        except Exception as e:
            logging.error("hybrid search for %s failed: %s", user_id, e)
            return []

    async def hybrid_search_batch(self, user_id: str, dense_vectors, sparse_vectors, top_k: int = 10,
                                  search_params: Optional[Dict[str, Any]] = None,
                                  filters: Optional[Dict] = None, mode: str = "tree",
                                  filter_stages: str = "root") -> List[List[ScoredPoint]]:
        """B queries in one engine call (additive; no reranking hook).  mode "tree" = the reference query
        (:305-372), "h1" = dense top-dense_limit (+) sparse top-sparse_limit -> RRF -> final_limit.
        filter_stages as in hybrid_search; mode "h1" takes filters with filter_stages="all" only."""
        try:
            res = await self._run(self._search_sync, user_id, dense_vectors, sparse_vectors, search_params, filters,
                                  mode, filter_stages)
            return [r[:top_k] for r in res]
        except Exception as e:
            logging.error("hybrid search for %s failed: %s", user_id, e)
            return []

    # -------------------------------------------------------------------- grouped search
    def _groups_sync(self, user_id, dense_vectors, sparse_vectors, group_by, limit, group_size, search_params, filters,
                     mode, filter_stages, group_pool):
        if not self._grouped_search:
            raise ValueError("hybrid_search_groups is not supported on a sharded collection")
        _grouping.check_sizes(limit, group_size)
        if not isinstance(group_by, str) or not group_by:
            raise ValueError("group_by must be a non-empty string (a payload key, dotted paths allowed)")
        root_filter = self._routing(filters, mode, filter_stages)
        hp = _engine.make_params(search_params, mode=HX_MODE_TREE if mode == "tree" else HX_MODE_H1)
        pool_max = self._pool_max(hp, mode)                 # (_grouping.MAX_SLOTS is the pools' 2048)
        if group_pool is not None and (isinstance(group_pool, bool) or not isinstance(group_pool, int)
                                       or not 1 <= group_pool <= pool_max):
            raise ValueError(f"group_pool must be an integer in [1, {pool_max}] (this mode's pool) or None, "
                             f"got {group_pool!r}")
        pool = self._pool_size(hp, mode, group_pool)
        col = self._collections[str(user_id)]
        q, indptr, idx, val = self._pack_queries(col, dense_vectors, sparse_vectors)
        idx, val = idx.astype(np.int32), val.astype(np.float32)
        self._check_filter(filters)
        cids, cpay = col.ids, col.payloads
        pi = getattr(col, "pindex", None)
        k = pi.keys.get(group_by) if pi is not None else None
        if k is None:
            reason = "group by an unindexed key"
        elif k.col is None:
            reason = "group by a poisoned key"
        elif k.schema not in ("keyword", "bool") or k.array:
            reason = "group by a key of another schema"
        elif root_filter:
            reason = "group with a root filter"
        elif not hasattr(col.index, "hybrid_query_groups_host"):
            reason = "group on an index without the grouped query"
        else:
            reason = None
        if reason is None:
            try:
                mask = col.row_mask(filters) if filters else None
                scores, rows, codes, counts = col.index.hybrid_query_groups_host(
                    q, indptr, idx, val, hp, k.col, limit, group_size, group_pool=pool, mask=mask)
                out = []
                for sc, rw, cd, n in zip(scores.tolist(), rows.tolist(), codes.tolist(), counts.tolist()):
                    out.append([PointGroup(id=k.value_of(cd[g]),
                                           hits=[ScoredPoint(id=cids[r], version=0, score=s, payload=cpay[r])
                                                 for s, r in zip(sc[g], rw[g]) if r >= 0])
                                for g in range(n)])
                pi.group_device_calls += 1
                return out
            except Exception as e:                          # never a wrong group: the walk over the payloads is always right
                logging.warning("grouped search: the device path failed, Python path taken: %s", e)
                reason = "engine refused"
        logging.warning("grouped search by %r takes the Python path: %s", group_by, reason)
        if pi is not None:
            pi.declined[reason] = pi.declined.get(reason, 0) + 1
        hp.final_limit = pool
        if filters and not root_filter:
            scores, rows, counts = col.index.hybrid_query_host(q, indptr, idx, val, hp, mask=col.row_mask(filters))
        else:
            scores, rows, counts = col.index.hybrid_query_host(q, indptr, idx, val, hp)
        out = []
        for pts in self._points(col, scores, rows, counts):
            if root_filter:                                 # the root's filter comes before the grouping, as in Qdrant
                pts = [p for p in pts if _filters.matches(p.payload, filters, p.id)]
            values = [_grouping.group_value(p.payload, group_by) for p in pts]
            out.append([PointGroup(id=values[g[0]][1], hits=[pts[r] for r in g])
                        for g in _grouping.group_ranked(values, limit, group_size)])
        return out

    async def hybrid_search_groups(self, user_id: str, dense_vectors, sparse_vectors, group_by: str, limit: int = 10,
                                   group_size: int = 3, search_params: Optional[Dict[str, Any]] = None,
                                   filters: Optional[Dict] = None, mode: str = "tree", filter_stages: str = "root",
                                   group_pool: Optional[int] = None) -> List[List[PointGroup]]:
        """Qdrant's query_points_groups for B queries in one engine call (additive; no reranking hook): per query the
        best `limit` groups of the payload field `group_by` (a dotted path), at most `group_size` hits each, groups
        ordered by their best hit, hits by rank (grouping.py states the walk).  What is grouped is the query's POOL: the
        ranked list the engine returns with final_limit = the pool size -- mode "tree" the root's re-scored union,
        min(dense_limit + 10, 2048) rows; mode "h1" the fused list, min(dense_limit + sparse_limit, 2048).  group_pool
        asks for a shorter pool (1 .. that maximum).  search_params["final_limit"] must be there, as in every search, and
        is NOT used: `limit` and `group_size` say how much comes back.  filters / filter_stages as in hybrid_search_batch:
        "all" = the pool of the pre-filtered query, "root" (tree only) = the filter applied to the pool before grouping.
        Points without the field, or with None there, are in no group; `str`, `bool` and `int` values form groups (1 and
        True are different groups); floats, lists and dicts are skipped.
        A field with a live "keyword" or "bool" payload index is grouped by one kernel over the pool on the device
        (hx_hybrid_query_groups_host), with no filter or filter_stages="all"; everything else -- another schema, an
        unindexed or poisoned key, a root filter, an engine refusal -- walks the pool's payloads in Python, logs a warning
        and counts itself in the payload index's `declined`.  Both ways give the same groups.
        Raises ValueError for arguments no search can serve (limit or group_size below 1, limit * group_size above 2048,
        a group_pool out of range, mode "h1" with a root filter, a sharded collection, an unknown mode, filter_stages
        or filter clause); any other failure is logged and gives [], as in every search."""
        return await self._guarded("grouped hybrid search for %s", user_id, [], self._groups_sync, user_id, dense_vectors,
                                   sparse_vectors, group_by, limit, group_size, search_params, filters, mode,
                                   filter_stages, group_pool)

    # ------------------------------------------------------------------------ MMR search
    def _mmr_sync(self, user_id, dense_vectors, sparse_vectors, limit, diversity, candidates_limit, search_params, filters,
                  mode, filter_stages):
        if not self._mmr_search:
            raise ValueError("hybrid_search_mmr is not supported on a sharded collection")
        self._check_int("limit", limit, 1, MMR_MAX_LIMIT)
        if not self._is_number(diversity) or not 0.0 <= diversity <= 1.0:
            raise ValueError(f"diversity must be a number in [0, 1], got {diversity!r}")
        self._check_candidates(candidates_limit)
        root_filter = self._routing(filters, mode, filter_stages)
        hp = _engine.make_params(search_params, mode=HX_MODE_TREE if mode == "tree" else HX_MODE_H1)
        pool = self._pool_size(hp, mode, candidates_limit)
        col = self._collections[str(user_id)]
        q, indptr, idx, val = self._pack_queries(col, dense_vectors, sparse_vectors)
        mask = self._filter_mask(col, filters)
        scores, rows, values, counts = col.index.hybrid_query_mmr_host(
            q, indptr, idx.astype(np.int32), val.astype(np.float32), hp, limit, float(diversity), candidates_limit=pool,
            mask=mask, mask_root_only=root_filter)
        return self._points(col, scores, rows, counts, MmrPoint, values)

    async def hybrid_search_mmr(self, user_id: str, dense_vectors, sparse_vectors, limit: int = 10, diversity: float = 0.5,
                                candidates_limit: Optional[int] = 100, search_params: Optional[Dict[str, Any]] = None,
                                filters: Optional[Dict] = None, mode: str = "tree",
                                filter_stages: str = "root") -> List[List[MmrPoint]]:
        """Qdrant's NearestQuery(mmr=Mmr(diversity, candidates_limit)) for B queries in one engine call (additive; no
        reranking hook): per query `limit` hits of the query's POOL, picked one by one by maximal marginal relevance --
        the next hit is the one with the largest (1 - diversity) * relevance - diversity * (largest similarity to the hits
        picked so far); include/hx.h states the arithmetic.  Relevance is the dense cosine to the query and similarity
        the dense cosine between two stored rows, in both modes.  The pool is the ranked list the engine returns with
        final_limit = the pool size -- mode "tree" the root's re-scored union, min(dense_limit + 10, 2048) rows; mode
        "h1" the fused list, min(dense_limit + sparse_limit, 2048), re-scored by the dense cosine (so `score` is that
        cosine, NOT the fused score hybrid_search_batch returns in this mode).  candidates_limit asks for a shorter pool;
        above the pool's maximum it is clipped to it, None = the maximum.  search_params["final_limit"] must be there, as
        in every search, and is NOT used.  filters / filter_stages as in hybrid_search_batch: "all" = the pool of the
        pre-filtered query, "root" (tree only) = the pool of the unfiltered query, of which only the points the filter
        keeps can be picked.  Returns per query the hits in pick order: `score` = the relevance, `mmr_score` = the value
        the hit was picked at.  All of it runs on the device (hx_hybrid_query_mmr_host); there is no Python path.
        Raises ValueError for arguments no search can serve (a limit outside [1, 256], a diversity outside [0, 1], a
        candidates_limit below 1, mode "h1" with a root filter, a sharded collection, an unknown mode, filter_stages or
        filter clause); any other failure is logged and gives [], as in every search."""
        return await self._guarded("MMR hybrid search for %s", user_id, [], self._mmr_sync, user_id, dense_vectors,
                                   sparse_vectors, limit, diversity, candidates_limit, search_params, filters, mode,
                                   filter_stages)

    # ------------------------------------------------------------- late-interaction rerank
    async def create_token_index(self, user_id: str, dim: int) -> None:
        """Qdrant's multivector with comparator=MAX_SIM (additive): give the collection ONE token
        column of `dim` values per token, a multiple of 64 in [64, 1024] (a model that emits fewer zero-pads; the handler
        pads for it).  Points stored so far hold no tokens; store_document_vectors / upsert_points then take an optional
        "token_embeddings" [T, d <= dim] per chunk, quantised on the host (late_interaction.quantize_tokens) and kept
        beside the payloads.  Calling it again with the same width does nothing.  Raises ValueError for a bad or another
        width, a sharded collection, or an engine index without token columns; KeyError for an unknown collection."""
        try:
            if not self._late_rerank:
                raise ValueError("create_token_index is not supported on a sharded collection")
            _late.check_dim(dim)
            col = self._collections[str(user_id)]          # KeyError if absent: re-raised
            await self._run(col.create_token_index, dim)
        except Exception as e:
            logging.error("create_token_index(%s, %r) failed: %s", user_id, dim, e)
            raise

    def _rerank_sync(self, user_id, dense_vectors, sparse_vectors, query_tokens, limit, candidates_limit, search_params,
                     filters, mode, filter_stages):
        if not self._late_rerank:
            raise ValueError("hybrid_search_rerank is not supported on a sharded collection")
        self._check_int("limit", limit, 1, 2048)
        self._check_candidates(candidates_limit)
        root_filter = self._routing(filters, mode, filter_stages)
        hp = _engine.make_params(search_params, mode=HX_MODE_TREE if mode == "tree" else HX_MODE_H1)
        pool = self._pool_size(hp, mode, candidates_limit)
        col = self._collections[str(user_id)]
        tk = getattr(col, "tokens", None)
        if tk is None:
            raise ValueError("hybrid_search_rerank needs a token index: call create_token_index first")
        if len(query_tokens) != len(sparse_vectors):
            raise ValueError(f"{len(sparse_vectors)} queries but {len(query_tokens)} token lists")
        q8, qs, qtip = _late.pack_queries(query_tokens, tk["dim"])      # ValueError: 0 or > 64 tokens, too wide, non-finite
        q, indptr, idx, val = self._pack_queries(col, dense_vectors, sparse_vectors)
        mask = self._filter_mask(col, filters)
        scores, rows, first, counts = col.index.hybrid_query_rerank_host(
            q, indptr, idx.astype(np.int32), val.astype(np.float32), hp, col._token_column(), q8, qs, qtip, limit,
            candidates_limit=pool, mask=mask, mask_root_only=root_filter)
        return self._points(col, scores, rows, counts, RerankedPoint, first)

    async def hybrid_search_rerank(self, user_id: str, dense_vectors, sparse_vectors, query_tokens, limit: int = 10,
                                   candidates_limit: Optional[int] = 100,
                                   search_params: Optional[Dict[str, Any]] = None, filters: Optional[Dict] = None,
                                   mode: str = "tree", filter_stages: str = "root") -> List[List[RerankedPoint]]:
        """Qdrant's hybrid + ColBERT recipe for B queries in one engine call (additive): the hybrid query is the prefetch,
        the points of its POOL that hold tokens are rescored by MaxSim against query_tokens[b] -- a [Tq, d <= dim] float
        array, 1 <= Tq <= 64, quantised as stored tokens are -- and the best `limit` come back, MaxSim descending, pool
        order on a tie; include/hx.h states the arithmetic.  The pool is the ranked list the engine returns with
        final_limit = the pool size, as hybrid_search_batch would (mode "tree": the root's re-scored union, min(dense_limit
        + 10, 2048) rows; mode "h1": the fused list, min(dense_limit + sparse_limit, 2048)); candidates_limit asks for a
        shorter pool, above the maximum it is clipped, None = the maximum.  search_params["final_limit"] must be there and
        is NOT used.  A point stored without "token_embeddings" is not scored and never comes back.  filters /
        filter_stages as in hybrid_search_mmr.  `score` = MaxSim, `first_score` = the score the pool carried.  All of it
        runs on the device (hx_hybrid_query_rerank_host); there is no Python path.
        Raises ValueError for arguments no search can serve (a limit outside [1, 2048], a candidates_limit below 1, a
        query with no or more than 64 tokens or tokens wider than the index, a collection without a token index, mode
        "h1" with a root filter, a sharded collection, an unknown mode, filter_stages or filter clause); any other
        failure is logged and gives [], as in every search."""
        return await self._guarded("rerank hybrid search for %s", user_id, [], self._rerank_sync, user_id, dense_vectors,
                                   sparse_vectors, query_tokens, limit, candidates_limit, search_params, filters, mode,
                                   filter_stages)

    # ---------------------------------------------------------------------- score boosting
    def _boost_sync(self, user_id, dense_vectors, sparse_vectors, formula, defaults, limit, candidates_limit,
                    score_threshold, search_params, filters, mode, filter_stages):
        if not self._boost_search:
            raise ValueError("hybrid_search_boost is not supported on a sharded collection")
        self._check_int("limit", limit, 1, BOOST_MAX_LIMIT)
        self._check_candidates(candidates_limit)
        if score_threshold is not None and not self._is_number(score_threshold):
            raise ValueError(f"score_threshold must be a number that is not a NaN or None, got {score_threshold!r}")
        if defaults is not None and not isinstance(defaults, dict):
            raise ValueError("defaults must be a dict (variable -> value) or None")
        root_filter = self._routing(filters, mode, filter_stages)
        defaults = defaults or {}
        _boosting.check(formula, defaults)                 # ValueError: a formula no evaluation can serve
        hp = _engine.make_params(search_params, mode=HX_MODE_TREE if mode == "tree" else HX_MODE_H1)
        pool = self._pool_size(hp, mode, candidates_limit)
        col = self._collections[str(user_id)]
        q, indptr, idx, val = self._pack_queries(col, dense_vectors, sparse_vectors)
        idx, val = idx.astype(np.int32), val.astype(np.float32)
        self._check_filter(filters)
        cids, cpay = col.ids, col.payloads
        pi = getattr(col, "pindex", None)
        prog = _boosting.compile(formula, defaults, pi, col._id_rows)
        if prog is None:
            reason = "formula declined"
        elif not hasattr(col.index, "hybrid_query_formula_host"):
            reason = "boost on an index without the formula query"
        else:
            reason = None
        if reason is None:
            try:
                if prog[1] and col.index.count() != len(cids):
                    raise RuntimeError("the engine's row count differs from the payloads'")
                planes = [col.row_mask(f) for f in prog[1]]
                mask = col.row_mask(filters) if filters else None
                scores, rows, base, counts, dropped = col.index.hybrid_query_formula_host(
                    q, indptr, idx, val, hp, prog[0], limit, planes=planes, score_threshold=score_threshold,
                    candidates_limit=pool, mask=mask, mask_root_only=root_filter)
                for b, d in enumerate(dropped.tolist()):
                    if d:
                        logging.warning("boosted search: query %d dropped %d points whose value was not finite", b, d)
                if pi is not None:
                    pi.boost_device_calls += 1
                return self._points(col, scores, rows, counts, BoostedPoint, base)
            except Exception as e:                          # never a wrong rank: the walk over the payloads is always right
                logging.warning("boosted search: the device path failed, Python path taken: %s", e)
                reason = "engine refused"
        logging.warning("boosted search takes the Python path: %s", reason)
        if pi is not None and reason != "formula declined":  # (compile counted its own reason)
            pi.declined[reason] = pi.declined.get(reason, 0) + 1
        hp.final_limit = pool
        if filters and not root_filter:
            scores, rows, counts = col.index.hybrid_query_host(q, indptr, idx, val, hp, mask=col.row_mask(filters))
        else:
            scores, rows, counts = col.index.hybrid_query_host(q, indptr, idx, val, hp)
        out = []
        for b, (sc, rw, n) in enumerate(zip(scores.tolist(), rows.tolist(), counts.tolist())):
            values = []
            for s, r in zip(sc[:n], rw[:n]):
                if root_filter and not _filters.matches(cpay[r], filters, cids[r]):
                    values.append(None)                     # the root's filter: the point is not eligible
                else:
                    values.append(_boosting.value_f32(_boosting.evaluate(formula, defaults, s, cpay[r], cids[r])))
            hits, dropped = _boosting.rank(values, limit, score_threshold)
            if dropped:
                logging.warning("boosted search: query %d dropped %d points whose value was not finite", b, dropped)
            out.append([BoostedPoint(id=cids[rw[i]], version=0, score=float(values[i]), payload=cpay[rw[i]],
                                     base_score=sc[i]) for i in hits])
        return out

    async def hybrid_search_boost(self, user_id: str, dense_vectors, sparse_vectors, formula, defaults=None,
                                  limit: int = 10, candidates_limit: Optional[int] = 100,
                                  score_threshold: Optional[float] = None,
                                  search_params: Optional[Dict[str, Any]] = None, filters: Optional[Dict] = None,
                                  mode: str = "tree", filter_stages: str = "root") -> List[List[BoostedPoint]]:
        """Qdrant's FormulaQuery ("score boosting") for B queries in one engine call (additive): the hybrid query is the
        prefetch, every point of its POOL is valued by `formula` -- an expression over "$score" (the score the pool
        carried: mode "tree" the dense cosine, mode "h1" the fused RRF score), payload variables with `defaults`,
        conditions, sum / mult / neg / abs / div / sqrt / exp / pow / ln / log10, datetime / datetime_key and the three
        decays; boosting.py states the grammar and the arithmetic -- and the best `limit` come back, value descending, pool
        order on a tie.  A point whose value is not finite (a NaN, an infinity) is dropped, and the query logs a warning
        with the count; score_threshold cuts the points whose value lies under it.  The pool is the ranked list the
        engine returns with final_limit = the pool size, as in hybrid_search_mmr; candidates_limit asks for a shorter
        pool, above the maximum it is clipped, None = the maximum.  search_params["final_limit"] must be there and is
        NOT used.  filters / filter_stages as in hybrid_search_mmr.  `score` = the value, `base_score` = the pool's score.
        A formula that compiles (boosting.compile: its variables have live "number" / "datetime" payload indexes, its
        conditions compile, no pow / ln / log10) is valued and ranked by one kernel over the pool on the device
        (hx_hybrid_query_formula_host), each condition one row mask of the collection's mask cache; everything else walks
        the pool's payloads in Python (boosting.evaluate), logs a warning and counts itself in the payload index's
        `declined`.  Both ways give the same hits.
        Raises ValueError for arguments no search can serve (a limit outside [1, 2048], a candidates_limit below 1, a
        score_threshold that is no number, a malformed formula, a variable without a default, a scale <= 0, a midpoint
        outside (0, 1), mode "h1" with a root filter, a sharded collection, an unknown mode, filter_stages or filter
        clause); any other failure is logged and gives [], as in every search."""
        return await self._guarded("boosted hybrid search for %s", user_id, [], self._boost_sync, user_id, dense_vectors,
                                   sparse_vectors, formula, defaults, limit, candidates_limit, score_threshold,
                                   search_params, filters, mode, filter_stages)

    async def rerank_with_colbert(self, query: str, documents: List[str], results: List[Dict],
                                  max_tokens: int) -> List[Dict]:
        """qdrant_handler.py:388-412: reorder by reranker indices; any failure keeps the order."""
        try:
            client = getattr(self.reranker, "client", self.reranker)
            ranked_indices = client.rerank_documents(query, documents, max_tokens)
            if not ranked_indices:
                return results
            return [results[i] for i in ranked_indices]
        except Exception as e:
            logging.error("reranker raised, order kept: %s", e)
            return results

    # ------------------------------------------------------------------------ query trees
    def _query_points_sync(self, user_id, requests):
        if not self._query_tree:
            raise ValueError("query_points is not supported on a sharded collection")
        requests = list(requests)
        out: List[Optional[List[ScoredPoint]]] = [None] * len(requests)
        # every request's own "filter_stages": "root" (the default) takes the path it always took, untouched
        root, node = [], []
        for i, req in enumerate(requests):
            how = req.get("filter_stages") if isinstance(req, dict) else getattr(req, "filter_stages", None)
            how = "root" if how is None else how
            if how not in QUERY_FILTER_STAGES:
                raise ValueError(f"filter_stages must be one of {QUERY_FILTER_STAGES}, got {how!r}")
            if isinstance(req, dict) and "filter_stages" in req:
                req = {k: v for k, v in req.items() if k != "filter_stages"}
            (root if how == "root" else node).append((i, req, how))
        col = self._collections[str(user_id)]
        if root:
            for (i, _, _), res in zip(root, self._query_points_root(col, [r for _, r, _ in root])):
                out[i] = res
        if node:
            for (i, _, _), res in zip(node, self._query_points_nodes(col, [r for _, r, _ in node], [h for _, _, h in node])):
                out[i] = res
        return out

    def _query_points_nodes(self, col, requests, hows):
        """filter_stages "node" | "all" (DESIGN.md section 32): every node's own filter and score_threshold, served on the
        device by the masked stage entries and hx_list_keep; "all" pushes the root's filter into every leaf first."""
        parsed, roots = [], []
        filters: Dict[str, Any] = {}
        for req, how in zip(requests, hows):
            shape, vecs, thrs, flts = _query_tree.parse_nodes(req, col.dim, col.msizes, self._check_filter,
                                                              prefetch_filters=how == "node")
            self._check_binary(col, shape)
            if how == "all":
                shape = _query_tree.push_to_leaves(shape)
            filters.update(flts)
            get = req.get if isinstance(req, dict) else (lambda k, d=None, r=req: getattr(r, k, d))
            with_payload = get("with_payload", True)
            parsed.append(shape)
            roots.append((vecs, thrs, True if with_payload is None else bool(with_payload)))
        out: List[Optional[List[ScoredPoint]]] = [None] * len(requests)
        stages = _query_tree.DeviceStages(col.index, _engine, sparse_modifier=getattr(col, "sparse_modifier", None),
                                          masks=lambda key: col.row_mask(filters[key]))
        cids, cpay = col.ids, col.payloads
        for shape, members in _query_tree.group_by_shape(parsed).items():
            vectors = _query_tree.batch_vectors([roots[i][0] for i in members])
            thresholds = _query_tree.batch_thresholds([roots[i][1] for i in members])
            keys, counts = stages.to_host(*_query_tree.run(shape, vectors, stages, thresholds=thresholds))
            for b, i in enumerate(members):
                k = keys[b, :int(counts[b])]
                with_payload = roots[i][2]
                out[i] = [ScoredPoint(id=cids[r], version=0, score=s, payload=cpay[r] if with_payload else None)
                          for s, r in zip(_fusion.key_scores(k).tolist(), _fusion.key_ids(k).tolist())]
        return out

    def _query_points_root(self, col, requests):
        parsed, roots = [], []
        for req in requests:
            shape, vecs = _query_tree.parse(req, col.dim, col.msizes)
            self._check_binary(col, shape)
            get = req.get if isinstance(req, dict) else (lambda k, d=None, r=req: getattr(r, k, d))
            flt = get("filters") if get("filters") is not None else get("filter")
            thr = get("score_threshold")
            if thr is not None and not self._is_number(thr):
                raise ValueError(f"score_threshold must be a number, got {thr!r}")
            if flt:
                if not shape[-1]:
                    raise ValueError("filters on a root without prefetch are not supported: the stage entries take no row "
                                     "mask (filter the root of a tree with prefetches, or use hybrid_search_batch with "
                                     "filter_stages='all')")
                self._check_filter(flt)
            with_payload = get("with_payload", True)
            parsed.append((shape, bool(flt)))
            roots.append((vecs, flt or None, thr, True if with_payload is None else bool(with_payload)))
        out: List[Optional[List[ScoredPoint]]] = [None] * len(requests)
        stages = _query_tree.DeviceStages(col.index, _engine, sparse_modifier=getattr(col, "sparse_modifier", None))
        cids, cpay = col.ids, col.payloads
        for (shape, filtered), members in _query_tree.group_by_shape(parsed).items():
            limit = _query_tree.shape_limit(shape)
            # a filter is the ROOT's (:297, :371): its candidates are filtered before its cut, so the root stage runs at
            # the width of its input and the rows are tested against the packed row mask here
            width = min(_query_tree.input_width(shape), 2048) if filtered else None
            vectors = _query_tree.batch_vectors([roots[i][0] for i in members])
            keys, counts = stages.to_host(*_query_tree.run(shape, vectors, stages, root_limit=width))
            for b, i in enumerate(members):
                _, flt, thr, with_payload = roots[i]
                k = keys[b, :int(counts[b])]
                rows, scores = _fusion.key_ids(k), _fusion.key_scores(k)
                if flt:
                    words = col.row_mask(flt)
                    keep = (words[rows >> 5] >> (rows & 31).astype(words.dtype)) & 1 != 0
                    rows, scores = rows[keep], scores[keep]
                if thr is not None:
                    keep = ~(scores < np.float32(thr))
                    rows, scores = rows[keep], scores[keep]
                out[i] = [ScoredPoint(id=cids[r], version=0, score=s, payload=cpay[r] if with_payload else None)
                          for s, r in zip(scores[:limit].tolist(), rows[:limit].tolist())]
        return out

    @staticmethod
    def _check_binary(col, shape):
        if _query_tree.uses_binary(shape) and not getattr(col, "binary_quantization", False):
            raise ValueError("using='binary' needs a collection created with binary_quantization=True")

    async def query_points_batch(self, user_id: str, requests) -> List[List[ScoredPoint]]:
        """The reference's general call, client.query_points(prefetch=[...], query=..., using=..., limit=...), for many
        requests at once (additive).  A request is a dict (or an object with the same attributes):
        "prefetch", "query", "using", "limit" as query_tree.py states them, and for the root "filters" (or "filter"),
        "score_threshold", "with_payload", "filter_stages" (query_points states it; "root" when absent: a batch may mix
        them).  The requests are grouped by shape -- the tree without its vectors -- and every
        group runs as one batch over the engine's stage entries, fusion nodes through hx_fuse; results come back in
        request order.  Raises ValueError for a tree no stage can serve (query_tree.parse names the reason) and on a
        sharded collection; any other failure is logged and gives [], as in every search."""
        return await self._guarded("query_points for %s", user_id, [], self._query_points_sync, user_id, requests)

    async def query_points(self, user_id: str, prefetch=None, query=None, using: str = "dense", limit: int = 10,
                           filters: Optional[Dict] = None, score_threshold: Optional[float] = None,
                           with_payload: bool = True, filter_stages: str = "root") -> List[ScoredPoint]:
        """One request of query_points_batch.  `filters` is the root's filter, as in the reference (:297, :371): the
        root's candidates are filtered before its cut; a root without prefetch takes none.  `score_threshold` drops
        root hits that score below it.  filter_stages, as hybrid_search's: "root" = the above;
        "node" = every node of the tree may carry its own "filter" and "score_threshold" (Qdrant's Prefetch(filter=...)),
        the root's being `filters` / `score_threshold`, each served on the device -- a root without prefetch and with
        `filters` is a filtered nearest-neighbour search; "all" = `filters` pushed into every leaf (a filter inside a
        prefetch is refused)."""
        if filter_stages not in QUERY_FILTER_STAGES:
            raise ValueError(f"filter_stages must be one of {QUERY_FILTER_STAGES}, got {filter_stages!r}")
        res = await self.query_points_batch(user_id, [{"prefetch": prefetch, "query": query, "using": using,
                                                       "limit": limit, "filters": filters,
                                                       "score_threshold": score_threshold,
                                                       "with_payload": with_payload,
                                                       **({} if filter_stages == "root" else
                                                          {"filter_stages": filter_stages})}])
        return res[0] if res else []

    # ------------------------------------------------------------------------ binary quantization
    async def search_binary_batch(self, user_id: str, dense_vectors, limit: int = 10, oversampling: float = 4.0,
                                  rescore: bool = True, filters: Optional[Dict] = None,
                                  filter_stages: str = "root", query_encoding: str = "binary") -> List[List[ScoredPoint]]:
        """Qdrant's search under quantization_config=BinaryQuantization with QuantizationSearchParams(oversampling,
        rescore), for B query vectors (additive): the sign bits nominate min(ceil(limit *
        oversampling), 2048) candidates per query with XOR and popcount, the exact vectors re-score them and the best
        `limit` come back -- the tree query_tree.binary_request builds, run by query_points_batch.  rescore=False returns
        the binary stage's own list at `limit`.  ScoredPoint.score is the cosine after a re-score and the integer score
        dim - 2 * (differing sign bits) without one.  filters / filter_stages as query_points takes them ("root": the
        re-scoring root's candidates are filtered before its cut, so rescore=False takes no filter there; "node" / "all":
        on the device).  query_encoding (additive) is Qdrant's BinaryQuantization.query_encoding:
        "binary" = the above; "scalar4bits" / "scalar8bits" = the rows stay at one bit and the query keeps 4 or 8 bits per
        dimension, which nominates far better candidates at the same oversampling (the score without a re-score is then
        the integer sum of the query's codes signed by the row's bits).  Raises ValueError for a collection created
        without binary_quantization, a limit outside [1, 2048], an oversampling that is no finite number >= 1, an
        unknown query_encoding, and on a sharded collection; any other failure is logged and gives [], as in every
        search."""
        if filter_stages not in QUERY_FILTER_STAGES:
            raise ValueError(f"filter_stages must be one of {QUERY_FILTER_STAGES}, got {filter_stages!r}")
        if not isinstance(query_encoding, str) or query_encoding not in _query_tree.QUERY_ENCODINGS:
            raise ValueError(f"query_encoding must be one of {tuple(_query_tree.QUERY_ENCODINGS)}, got {query_encoding!r}")
        try:
            vectors = [v for v in dense_vectors]
        except TypeError:
            raise ValueError("dense_vectors: a list of query vectors") from None
        reqs = [dict(_query_tree.binary_request(v, limit, oversampling, rescore, filters, query_encoding),
                     **({} if filter_stages == "root" else {"filter_stages": filter_stages})) for v in vectors]
        return await self.query_points_batch(user_id, reqs)

    async def search_binary(self, user_id: str, dense_vector, limit: int = 10, oversampling: float = 4.0,
                            rescore: bool = True, filters: Optional[Dict] = None,
                            filter_stages: str = "root", query_encoding: str = "binary") -> List[ScoredPoint]:
        """One query of search_binary_batch."""
        res = await self.search_binary_batch(user_id, [dense_vector], limit, oversampling, rescore, filters, filter_stages,
                                             query_encoding)
        return res[0] if res else []

    # ------------------------------------------------------------------------ term statistics
    def _term_stats_sync(self, user_id, indices):
        if not self._sparse_modifiers:
            raise ValueError("term_stats is not supported on a sharded collection")
        col = self._collections[str(user_id)]
        try:
            idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError("term_stats: indices must be integers") from None
        if idx.size and (idx.min() < -2 ** 31 or idx.max() >= 2 ** 31):
            raise ValueError("sparse index out of range")
        _, df, n_docs = col.index.sparse_idf_host(idx.astype(np.int32), np.ones(idx.shape[0], np.float32),
                                                  want_stats=True)
        return {"n_docs": int(n_docs), "df": [int(d) for d in df]}

    async def term_stats(self, user_id: str, indices) -> Dict[str, Any]:
        """The collection's sparse statistics (additive): {"n_docs": points that hold a sparse
        vector, "df": per given term id the points whose sparse vector holds it}.  These are what sparse_modifier="idf"
        weighs queries with; they are there whatever the collection's modifier.  Raises ValueError for indices that
        are no int32 and on a sharded collection; KeyError for an unknown collection."""
        return await self._run(self._term_stats_sync, user_id, indices)

    # ------------------------------------------------------------------------ recommend
    def _recommend_sync(self, user_id, requests, limit, filters):
        if not self._recommend:
            raise ValueError("recommend is not supported on a sharded collection")
        self._check_int("limit", limit, 1, RECO_MAX_LIMIT)
        requests = list(requests)
        if not 1 <= len(requests) <= RECO_MAX_REQUESTS:
            raise ValueError(f"a recommend batch takes 1 to {RECO_MAX_REQUESTS} requests, got {len(requests)}")
        col = self._collections[str(user_id)]
        dim_pad = (col.dim + 63) // 64 * 64
        example = self._example_resolver(col, "recommend")
        strategies, packed = set(), []
        for req in requests:
            positive, negative, strategy = req.get("positive"), req.get("negative"), req.get("strategy", "average_vector")
            positive = [] if positive is None else list(positive)
            negative = [] if negative is None else list(negative)
            if strategy not in RECO_STRATEGIES:
                raise ValueError(f"strategy must be one of {tuple(RECO_STRATEGIES)}, got {strategy!r}")
            strategies.add(strategy)
            examples = []
            for group, sign in ((positive, 1), (negative, -1)):
                examples.extend((example(ex), sign) for ex in group)
            if not examples:
                raise ValueError("recommend: a request needs at least one example")
            if len(examples) > RECO_MAX_EXAMPLES or len(examples) * dim_pad > 32768:
                raise ValueError(f"recommend: too many examples ({len(examples)}): at most {RECO_MAX_EXAMPLES}, and "
                                 f"examples x padded width at most 32768 (width {dim_pad})")
            if strategy == "average_vector" and not positive:
                raise ValueError("recommend: the average_vector strategy needs a positive example")
            packed.append(examples)
        if len(strategies) != 1:
            raise ValueError("recommend_batch: one strategy per batch")
        mask = self._filter_mask(col, filters)
        return self._points(col, *col.index.recommend_host(packed, RECO_STRATEGIES[strategies.pop()], limit, mask=mask))

    async def recommend_batch(self, user_id: str, requests, limit: int = 10,
                              filters: Optional[Dict] = None) -> List[List[ScoredPoint]]:
        """Qdrant's RecommendQuery for up to 16 requests in one engine call (additive).  A request
        is a dict {"positive": [...], "negative": [...], "strategy": "average_vector" | "best_score" | "sum_scores"}; an
        example is a point id (looked up in the collection, it becomes a stored row) or a vector of `dim` numbers.  All
        requests of a batch share one strategy.  The examples given as point ids are never returned; `filters` keeps
        only the rows the filter keeps (through the payload index where there is one) -- an example need not pass it.
        `score` is the strategy's score (include/hx.h states the arithmetic).  All of it runs on the device
        (hx_recommend_host); there is no Python path.  Raises ValueError for arguments no search can serve (an unknown
        point id or strategy, no example, average_vector without a positive, too many examples, a limit outside [1,
        1024], a vector of the wrong length or with a non-finite element, a sharded collection); any other failure is
        logged and gives [], as in every search."""
        return await self._guarded("recommend for %s", user_id, [], self._recommend_sync, user_id, requests, limit,
                                   filters)

    async def recommend(self, user_id: str, positive, negative=None, strategy: str = "average_vector", limit: int = 10,
                        filters: Optional[Dict] = None) -> List[ScoredPoint]:
        """One request of recommend_batch: the `limit` points most like the positive examples and least like the
        negative ones, the examples themselves left out."""
        res = await self.recommend_batch(user_id, [{"positive": positive, "negative": negative, "strategy": strategy}],
                                         limit=limit, filters=filters)
        return res[0] if res else []

    # ------------------------------------------------------------------------ discovery / context
    def _discover_sync(self, user_id, requests, limit, filters):
        if not self._discover:
            raise ValueError("discover is not supported on a sharded collection")
        self._check_int("limit", limit, 1, RECO_MAX_LIMIT)
        requests = list(requests)
        if not 1 <= len(requests) <= RECO_MAX_REQUESTS:
            raise ValueError(f"a discover batch takes 1 to {RECO_MAX_REQUESTS} requests, got {len(requests)}")
        col = self._collections[str(user_id)]
        dim_pad = (col.dim + 63) // 64 * 64
        example = self._example_resolver(col, "discover")
        packed = []
        for req in requests:
            target, context = req.get("target"), req.get("context")
            if context is not None and not isinstance(context, (list, tuple)):
                raise ValueError('discover: context is a list of pairs {"positive": x, "negative": y}')
            context = [] if context is None else list(context)
            pairs = []
            for pair in context:
                if not isinstance(pair, dict) or set(pair) != {"positive", "negative"} \
                        or pair["positive"] is None or pair["negative"] is None:
                    raise ValueError('discover: a context pair is {"positive": x, "negative": y}')
                pairs.append((example(pair["positive"]), example(pair["negative"])))
            if target is None and not pairs:
                raise ValueError("discover: a request needs a target or a context pair")
            n_ex = (target is not None) + 2 * len(pairs)
            if n_ex > RECO_MAX_EXAMPLES or n_ex * dim_pad > 32768:
                raise ValueError(f"discover: too many examples ({n_ex}, the target and two per pair): at most "
                                 f"{RECO_MAX_EXAMPLES}, and examples x padded width at most 32768 (width {dim_pad})")
            packed.append((None if target is None else example(target), pairs))
        mask = self._filter_mask(col, filters)
        return self._points(col, *col.index.discover_host(packed, limit, mask=mask))

    async def discover_batch(self, user_id: str, requests, limit: int = 10,
                             filters: Optional[Dict] = None) -> List[List[ScoredPoint]]:
        """Qdrant's DiscoverQuery / ContextQuery for up to 16 requests in one engine call (additive; DESIGN.md section
        29).  A request is a dict {"target": x | None, "context": [{"positive": x, "negative": y}, ...]}; x and y are each
        a point id (looked up in the collection, it becomes a stored row) or a vector of `dim` numbers.  With a target
        (discovery) the hits come from the cell that agrees with the most pairs, nearest the target first; without one
        (context search) `score` is 0 for every point on the positive side of every pair and negative elsewhere, equal
        scores in the order the points were stored.  Examples given as point ids are never returned; `filters` keeps only
        the rows the filter keeps -- an example need not pass it.  include/hx.h states the arithmetic.  All of it runs on
        the device (hx_discover_host); there is no Python path.  Raises ValueError for arguments no search can serve (an
        unknown point id, neither target nor pair, a malformed pair, too many examples, a limit outside [1, 1024], a
        vector of the wrong length or with a non-finite element, a sharded collection); any other failure is logged and
        gives [], as in every search."""
        return await self._guarded("discover for %s", user_id, [], self._discover_sync, user_id, requests, limit, filters)

    async def discover(self, user_id: str, target=None, context=(), limit: int = 10,
                       filters: Optional[Dict] = None) -> List[ScoredPoint]:
        """One request of discover_batch; target=None is context search."""
        res = await self.discover_batch(user_id, [{"target": target, "context": context}], limit=limit, filters=filters)
        return res[0] if res else []

    # ------------------------------------------------------------------------ distance matrix
    def _search_matrix_sync(self, user_id, sample, limit, filters, point_ids, seed, score_threshold):
        """(the sample's point ids, scores [S, limit], neighbours as sample positions [S, limit], counts [S]) of one
        engine call, or None when fewer than two points are sampled"""
        if not self._matrix_search:
            raise ValueError("search_matrix is not supported on a sharded collection")
        self._check_int("sample", sample, 1, _matrix.MAX_SAMPLE)
        self._check_int("limit", limit, 1, _matrix.MAX_LIMIT)
        if score_threshold is not None:                    # (anything float() takes, unlike the boost and tree entries)
            try:
                score_threshold = float(score_threshold)
            except (TypeError, ValueError):
                raise ValueError(f"score_threshold must be a number, got {score_threshold!r}") from None
            if score_threshold != score_threshold:
                raise ValueError("score_threshold must not be NaN")
        col = self._collections[str(user_id)]
        n = len(col.ids)
        mask = self._filter_mask(col, filters)
        if point_ids is not None:                          # exactly these points, in the order given
            point_ids = list(point_ids)
            if len(point_ids) > _matrix.MAX_SAMPLE:
                raise ValueError(f"search_matrix: at most {_matrix.MAX_SAMPLE} point ids, got {len(point_ids)}")
            id_rows = col.first_rows()
            rows, seen = [], set()
            for pid in point_ids:
                if isinstance(pid, bool) or not isinstance(pid, (str, int)) or str(pid) not in id_rows:
                    raise ValueError(f"search_matrix: unknown point id {pid!r}")
                r = id_rows[str(pid)]
                if r in seen:
                    raise ValueError(f"search_matrix: point id {pid!r} is listed twice")
                seen.add(r)
                if mask is None or (int(mask[r >> 5]) >> (r & 31)) & 1:
                    rows.append(r)
            rows = np.asarray(rows, dtype=np.int64)
        else:
            rows = _matrix.choose_rows(mask, n, sample, seed)
        if len(rows) < 2:
            return None
        scores, nbr_rows, counts = col.index.search_matrix_host(rows, limit, score_threshold)
        ids = [col.ids[r] for r in rows.tolist()]
        return ids, scores, _matrix.neighbour_positions(rows.tolist(), nbr_rows, counts), counts

    async def _search_matrix(self, user_id, sample, limit, filters, point_ids, seed, score_threshold):
        return await self._guarded("search_matrix for %s", user_id, None, self._search_matrix_sync, user_id, sample,
                                   limit, filters, point_ids, seed, score_threshold)

    async def search_matrix_pairs(self, user_id: str, sample: int = 10, limit: int = 3, filters: Optional[Dict] = None,
                                  point_ids=None, seed=None, score_threshold=None) -> List[MatrixPair]:
        """Qdrant's search_matrix_pairs (additive): a sample of at most `sample` of the points
        `filters` keeps (matrix.choose_rows: `seed` makes it repeatable) -- or exactly the points `point_ids` names, in
        that order, less those the filter drops -- and for each sample point, in sample order, its `limit` nearest
        neighbours among the other sample points, best first, as MatrixPair(a, b, score); `score_threshold` keeps only
        neighbours that score at least that.  Symmetric pairs are not merged.  One engine call on the device
        (hx_search_matrix_host) that reads the sample's rows only; there is no Python path.  Fewer than two sample points
        give [].  Raises ValueError for arguments no search can serve (sample outside [1, 4096], limit outside [1, 1024],
        a NaN threshold, an unknown or repeated point id, more than 4096 point ids, a sharded collection); any other
        failure is logged and gives [], as in every search."""
        res = await self._search_matrix(user_id, sample, limit, filters, point_ids, seed, score_threshold)
        return [] if res is None else _matrix.pairs(*res)

    async def search_matrix_offsets(self, user_id: str, sample: int = 10, limit: int = 3, filters: Optional[Dict] = None,
                                    point_ids=None, seed=None, score_threshold=None) -> MatrixOffsets:
        """search_matrix_pairs in Qdrant's offsets form: MatrixOffsets(offsets_row, offsets_col, scores, ids), entry k
        saying that ids[offsets_col[k]] is a neighbour of ids[offsets_row[k]]; `ids` = the sample in sample order.  Fewer
        than two sample points give an empty response."""
        res = await self._search_matrix(user_id, sample, limit, filters, point_ids, seed, score_threshold)
        return MatrixOffsets([], [], [], []) if res is None else _matrix.offsets(*res)

    # ------------------------------------------------------------------------ collections
    async def get_all_containers(self) -> List[str]:
        try:
            return list(self._collections.keys())
        except Exception as e:
            logging.error("get_all_containers failed: %s", e)
            return []

    async def delete_collection(self, user_id: str):
        try:
            def drop():
                col = self._collections.pop(str(user_id))   # KeyError if absent: re-raised
                self._drop(str(user_id), col)
            await self._run(drop)
            logging.info("delete_collection: %s dropped", user_id)
        except Exception as e:
            logging.error("delete_collection(%s) failed: %s", user_id, e)
            raise

    def _delete_sync(self, user_id, filters, point_ids) -> int:
        col = self._collections[str(user_id)]              # KeyError if absent: re-raised
        n = len(col.ids)
        gone = np.zeros(n, dtype=bool)
        if filters:                                        # (the clause names are validated before anything moves)
            gone |= np.unpackbits(self._filter_mask(col, filters).view(np.uint8), bitorder="little")[:n].astype(bool)
        if point_ids:
            listed = {str(p) for p in point_ids}
            gone |= np.fromiter((i in listed for i in col.ids), dtype=bool, count=n)
        keep = ~gone
        removed = int(gone.sum())
        if removed == 0:
            return 0
        # the engine first (it refuses before it moves anything), then the ids and payloads the same way
        col.index.retain(_filters.pack_rows(keep))
        col.ids = [i for i, k in zip(col.ids, keep) if k]
        col.payloads = [p for p, k in zip(col.payloads, keep) if k]
        if getattr(col, "tokens", None) is not None:       # (the column was compacted with the rows, or dropped if it lagged)
            col.tokens["cells"] = [c for c, k in zip(col.tokens["cells"], keep) if k]
        # the cached row masks speak of the old rows: dropped, not patched (a delete of k rows followed by an add of k
        # rows would pass the cache's `done != n` test with a stale mask)
        col._masks.clear()
        col._idrows = None                                 # (the payload columns were compacted with the rows: the keys stay live)
        return removed

    async def delete_points(self, user_id: str, filters: Optional[Dict] = None,
                            point_ids: Optional[List[str]] = None) -> int:
        """Delete the points the payload filter matches and / or the points with the listed ids (additive: the
        reference's handler has no delete, the application around it deletes a file's chunks when the file is deleted
        or uploaded again).  Returns the number of points deleted.  The engine index is compacted on the GPU
        (hx_retain_rows): later searches run the ordinary path on an index that holds only the survivors.  Both
        selectors None or empty raises ValueError (dropping everything is delete_collection's job); an unknown
        collection raises KeyError.  Nothing is saved: call save_collection."""
        try:
            if not self._point_deletes:
                raise ValueError("delete_points is not supported on a sharded collection")
            if not filters and not point_ids:
                raise ValueError("delete_points needs a filter or point ids (delete_collection drops a whole collection)")
            if str(user_id) not in self._collections:
                raise KeyError(str(user_id))
            n = await self._run(self._delete_sync, user_id, filters, point_ids)
            logging.info("delete_points: %d points deleted for %s", n, user_id)
            return n
        except Exception as e:
            logging.error("delete_points(%s) failed: %s", user_id, e)
            raise

    def _facet_sync(self, user_id, key, filters, limit):
        self._check_filter(filters)
        return [FacetHit(value=v, count=c) for v, c in self._collections[str(user_id)].facet(key, filters, limit)]

    async def facet(self, user_id: str, key: str, filters: Optional[Dict] = None, limit: int = 10,
                    exact: bool = True) -> List[FacetHit]:
        """Qdrant's facet(collection, key, facet_filter, limit, exact) (additive; parity unpinned): for every value of the
        payload field `key` (a dotted path) the number of points `filters` keeps that hold it, and of those the `limit`
        values with the largest counts -- count descending, then value ascending (bool < int < str between types).  A
        list-valued field holds each of its elements, a point counts once per value; points without the field, with
        None or [] there count nowhere; `str`, `bool` and `int` values are counted, everything else is ignored
        (faceting.py states the rules).  `exact` is accepted and ignored: every count is exact.
        A field with a live "keyword", "bool", "keyword_list" or "bool_list" payload index is counted and ranked by
        kernels over the whole column (hx_payload_facet_host); a "number" key, an unindexed or
        poisoned key, a limit above 2048 or an engine refusal is counted over the payloads in Python.  Both ways give
        the same hits; `PayloadIndex.facet_device_calls` / `facet_python_calls` say which one ran.
        A read call: it never raises -- an unknown collection or any error is logged and gives [] -- except on a
        sharded collection, which refuses it with a ValueError as it refuses the other payload-column features."""
        if not self._facets:
            raise ValueError("facet is not supported on a sharded collection")
        try:
            if str(user_id) not in self._collections:
                logging.warning("facet: no collection for %s", user_id)
                return []
            return await self._run(self._facet_sync, user_id, key, filters, limit)
        except Exception as e:
            logging.error("facet(%s, %r) failed: %s", user_id, key, e)
            return []

    def _scroll_sync(self, user_id, filters, limit, offset, order_by, with_payload):
        self._check_filter(filters)
        col = self._collections[str(user_id)]
        page, nxt = col.scroll(filters, limit, offset, order_by)
        return [Record(id=col.ids[r], payload=col.payloads[r] if with_payload else None, order_value=v)
                for r, v in page], nxt

    async def scroll(self, user_id: str, filters: Optional[Dict] = None, limit: int = 10, offset=None, order_by=None,
                     with_payload: bool = True):
        """Qdrant's scroll(collection, scroll_filter, limit, offset, order_by) (additive; parity unpinned): one page of
        at most `limit` points `filters` keeps, as (records, next_page_offset); next_page_offset is None when nothing
        follows, otherwise what the next call takes as `offset`.
        Without order_by the points come in insertion order, `offset` is a point id (the page starts there, inclusive)
        and next_page_offset is the id of the first point after the page.
        order_by = {"key": K, "direction": "asc" | "desc", "start_from": v} (or the bare key) orders by the number or
        datetime field K -- an int or float that is no bool and no NaN, a datetime, or an RFC 3339 string; every other
        point is left out -- then by insertion order in BOTH directions; start_from is inclusive.  Qdrant has no cursor
        here; this project's is next_page_offset = {"value": the last record's order_value, "id": its id}: the next page
        continues strictly after that pair, so chained pages neither repeat nor lose a point however many share a value.
        Each record's `order_value` is the number it was placed by (a datetime's microseconds since the epoch).
        A key with a live "number" or "datetime" payload index is selected by kernels over the whole column
        (hx_payload_order_host), a plain scroll by hx_scroll_rows_host; an unindexed or poisoned
        key or an engine refusal is walked over the payloads in Python.  Both ways give the same pages;
        `PayloadIndex.scroll_device_calls` / `scroll_python_calls` say which one ran.
        Raises ValueError for arguments no scroll can serve (a limit outside [1, 2047], a malformed order_by or offset,
        an offset id the collection does not hold, a sharded collection); an unknown collection gives ([], None), any
        other failure is logged and gives ([], None), as in every read call."""
        if not self._scroll:
            raise ValueError("scroll is not supported on a sharded collection")
        _scrolling.check_limit(limit, _scrolling.MAX_LIMIT - 1)
        if order_by is not None:
            _scrolling.check_order_by(order_by)
        if str(user_id) not in self._collections:
            logging.warning("scroll: no collection for %s", user_id)
            return [], None
        return await self._guarded("scroll for %s", user_id, ([], None), self._scroll_sync, user_id, filters, limit,
                                   offset, order_by, with_payload, failed="scroll(%s)")

    async def retrieve(self, user_id: str, point_ids, with_payload: bool = True) -> List[Record]:
        """Qdrant's retrieve(collection, ids) (additive): the points with the given ids, in the order asked, unknown ids
        skipped -- what a caller does next with a page's ids.  Host only: ids and payloads never cross the C ABI.  An
        unknown collection gives []; a sharded collection refuses with a ValueError."""
        if not self._scroll:
            raise ValueError("retrieve is not supported on a sharded collection")
        if isinstance(point_ids, (str, bytes)) or not hasattr(point_ids, "__iter__"):
            raise ValueError("point_ids must be a list of point ids")
        col = self._collections.get(str(user_id))
        if col is None:
            logging.warning("retrieve: no collection for %s", user_id)
            return []

        def fetch():
            out = []
            for p in point_ids:
                try:
                    r = col._row_of(p)
                except ValueError:
                    continue
                out.append(Record(id=col.ids[r], payload=col.payloads[r] if with_payload else None))
            return out
        return await self._run(fetch)

    async def get_collection_chunk_count(self, user_id: str, filters: Optional[Dict] = None) -> int:
        try:
            if str(user_id) not in self._collections:
                logging.warning("get_collection_chunk_count: no collection for %s", user_id)
                return 0
            col = self._collections[str(user_id)]
            if filters:   # :464-470: count the points the filter keeps (the popcount of its cached row mask)
                return await self._run(lambda: int(np.unpackbits(col.row_mask(filters).view(np.uint8)).sum()))
            return await self._run(col.index.count)
        except Exception as e:
            logging.error("get_collection_chunk_count(%s) failed: %s", user_id, e)
            return 0
