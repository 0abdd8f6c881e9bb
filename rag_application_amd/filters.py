"""Payload filters of the reference's search path.

`hybrid_search(..., filters=...)` turns the dict into `qdrant_client.models.Filter(**filters)` and
passes it as `query_filter` of the ROOT query only (app/core/vector_store/qdrant/qdrant_handler.py:297,
371; the prefetches carry no filter), i.e. the union of the two branches' candidates is re-scored by
the dense vector, filtered, and cut to `final_limit`.  `get_collection_chunk_count(filters=...)`
counts the points the filter keeps (:464-470).  No call site of the reference passes filters today.

Qdrant is absent from the image, so the condition semantics are restated from its documented model
(PARITY UNPINNED): a Filter has `must` (all hold), `should` (at least one holds, when any is listed;
`min_should` is not supported), `must_not` (none holds); a condition is a nested Filter or one of
  {"key": k, "match": {"value": v}}      payload[k] == v, or v in payload[k] when that is a list
  {"key": k, "match": {"any": [...]}}    payload[k] (or one of its elements) is in the list
  {"key": k, "match": {"except": [...]}} payload[k] exists and is not in the list
  {"key": k, "match": {"text": s}}       every whitespace-separated word of s occurs in str(payload[k])
  {"key": k, "range": {"gt"|"gte"|"lt"|"lte": x}}   numeric comparison
  {"is_empty": {"key": k}}               k missing, None or []
  {"is_null": {"key": k}}                k present with value None
  {"has_id": [ids]}                      the point id is listed
  {"nested": {"key": a, "filter": f}}    payload[a] is a list and ONE of its elements that is a dict passes the Filter
                                         f, whose keys are relative to that element
Keys may be dotted paths ("chunk_metadata.page").

Arrays of objects (the reference stores `entities` and `relationships` so: entity_relation_extractor.py:235-301).  A
path step `name[]` projects over the list at `name`: when the dict holds the literal key "name[]" that key is read, as
ever (the literal wins); otherwise, when `name` holds a `list`, the rest of the path is read from every element that is
a dict and the values found are collected, in element order, into a new list -- elements that are not dicts or lack the
path contribute nothing, so the result may be [] -- and when `name` is missing, None or not a list the key is missing.
A final `name[]` with no step behind it is the list itself.  match / range / is_empty / is_null then see that list as
they see a stored list: {"key": "entities[].entity_type", "match": {"value": "PERSON"}} = some entity is a PERSON.
Conditions on two projections may be met by DIFFERENT elements; `nested` asks ONE element to meet its whole filter.  Its
key is a dotted path (a trailing "[]" is accepted and ignored); it is false when the value is missing, None, not a
list, empty or holds no dict.  A `nested` inside its filter is `matches` recursing on the element; a `has_id` anywhere
inside it raises ValueError (an element has no id).

`row_mask` evaluates a filter over every stored row at once, as the packed row mask of the engine's
pre-filtered query (include/hx.h: hx_hybrid_query_*_masked): the filter then applies to every stage,
not to the root alone (QdrantHandler.hybrid_search(..., filter_stages="all"))."""
from __future__ import annotations

import json
from typing import Any, Dict, Iterable, Optional, Sequence

import numpy as np

_MISSING = object()


def _get(payload: Dict[str, Any], key: str):
    cur: Any = payload
    parts = str(key).split(".")
    for i, part in enumerate(parts):
        if isinstance(cur, dict) and part in cur:
            cur = cur[part]
        elif isinstance(cur, dict) and part.endswith("[]") and type(cur.get(part[:-2], _MISSING)) is list:
            arr = cur[part[:-2]]
            if i + 1 == len(parts):
                return arr
            rest = ".".join(parts[i + 1:])
            found = (_get(el, rest) for el in arr if isinstance(el, dict))
            return [v for v in found if v is not _MISSING]
        else:
            return _MISSING
    return cur


def _values(v) -> Iterable[Any]:
    return v if isinstance(v, (list, tuple)) else (v,)


def _match(value, m: Dict[str, Any]) -> bool:
    if value is _MISSING or value is None:
        return False
    if "value" in m:
        return any(x == m["value"] and type(x) is type(m["value"]) or (x == m["value"] and not isinstance(x, bool)
                   and not isinstance(m["value"], bool)) for x in _values(value))
    if "any" in m:
        return any(x in m["any"] for x in _values(value))
    if "except" in m:
        return all(x not in m["except"] for x in _values(value))
    if "text" in m:
        hay = str(value).lower()
        return all(w in hay for w in str(m["text"]).lower().split())
    raise ValueError(f"unsupported match condition: {m}")


def _range(value, r: Dict[str, Any]) -> bool:
    def ok(x):
        if isinstance(x, bool) or not isinstance(x, (int, float)):
            return False
        return ((("gt" not in r) or r["gt"] is None or x > r["gt"]) and (("gte" not in r) or r["gte"] is None or x >= r["gte"])
                and (("lt" not in r) or r["lt"] is None or x < r["lt"]) and (("lte" not in r) or r["lte"] is None or x <= r["lte"]))
    return value is not _MISSING and any(ok(x) for x in _values(value))


def _refuse_has_id(flt) -> None:
    """ValueError when a has_id condition occurs anywhere inside the filter of a `nested` condition."""
    if not isinstance(flt, dict):
        return
    for clause in ("must", "should", "must_not"):
        for c in _as_list(flt.get(clause)):
            if not isinstance(c, dict):
                continue
            if "has_id" in c:
                raise ValueError("has_id inside a nested filter: an element has no id")
            _refuse_has_id(c)                             # (a sub-filter)
            if isinstance(c.get("nested"), dict):
                _refuse_has_id(c["nested"].get("filter"))


def _nested(c: Dict[str, Any], payload: Dict[str, Any]) -> bool:
    nd = c["nested"]
    if not isinstance(nd, dict) or "key" not in nd:
        raise ValueError(f"unsupported filter condition: {c}")
    flt = nd.get("filter")
    _refuse_has_id(flt)
    key = str(nd["key"])
    v = _get(payload, key[:-2] if key.endswith("[]") else key)
    if type(v) is not list:
        return False
    return any(matches(el, flt) for el in v if isinstance(el, dict))


def _condition(c: Dict[str, Any], payload: Dict[str, Any], point_id) -> bool:
    if any(k in c for k in ("must", "should", "must_not")):
        return matches(payload, c, point_id)
    if "nested" in c:
        return _nested(c, payload)
    if "has_id" in c:
        return point_id in c["has_id"]
    if "is_empty" in c:
        v = _get(payload, c["is_empty"]["key"])
        return v is _MISSING or v is None or v == []
    if "is_null" in c:
        return _get(payload, c["is_null"]["key"]) is None
    if "key" in c:
        v = _get(payload, c["key"])
        if "match" in c:
            return _match(v, c["match"])
        if "range" in c:
            return _range(v, c["range"])
    raise ValueError(f"unsupported filter condition: {c}")


def _as_list(x):
    if x is None:
        return []
    return list(x) if isinstance(x, (list, tuple)) else [x]


def matches(payload: Dict[str, Any], flt: Optional[Dict[str, Any]], point_id=None) -> bool:
    """True when the point (payload, id) passes the filter; an empty / None filter passes all."""
    if not flt:
        return True
    unknown = set(flt) - {"must", "should", "must_not"}
    if unknown:
        raise ValueError(f"unsupported filter clause(s): {sorted(unknown)}")
    must, should, must_not = _as_list(flt.get("must")), _as_list(flt.get("should")), _as_list(flt.get("must_not"))
    if not all(_condition(c, payload, point_id) for c in must):
        return False
    if any(_condition(c, payload, point_id) for c in must_not):
        return False
    if should and not any(_condition(c, payload, point_id) for c in should):
        return False
    return True


def pack_rows(keep) -> np.ndarray:
    """bool per row -> the engine's row mask: ceil(n / 32) uint32 words, bit r & 31 of word r >> 5 (LSB first) = row r."""
    keep = np.asarray(keep, dtype=bool).ravel()
    nw = (keep.shape[0] + 31) // 32
    b = np.packbits(keep, bitorder="little")
    b = np.concatenate([b, np.zeros(nw * 4 - b.shape[0], np.uint8)])
    return b.view("<u4").astype(np.uint32)


def row_mask(ids: Sequence[Any], payloads: Sequence[Dict[str, Any]], flt: Optional[Dict[str, Any]],
             start: int = 0, prev: Optional[np.ndarray] = None) -> np.ndarray:
    """The packed row mask of `flt` over the rows (ids[r], payloads[r]): bit r set when `matches` holds for row r.
    start / prev: the rows before `start` are already evaluated in the packed mask `prev` (rows appended since),
    only rows [start, n) are evaluated."""
    n = len(ids)
    keep = np.zeros(n, dtype=bool)
    if prev is not None and start > 0:
        keep[:start] = np.unpackbits(np.asarray(prev, np.uint32).view(np.uint8), bitorder="little")[:start].astype(bool)
    for r in range(start, n):
        keep[r] = matches(payloads[r], flt, ids[r])
    return pack_rows(keep)


def filter_key(flt: Optional[Dict[str, Any]]) -> str:
    """Canonical JSON of a filter: the key of a collection's mask cache."""
    return json.dumps(flt, sort_keys=True, separators=(",", ":"), default=str)
