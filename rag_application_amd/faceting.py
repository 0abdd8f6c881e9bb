"""Payload facets on the host: the model of hx_payload_facet / hx_facet_top and the path a facet
takes when its key has no live `keyword` / `bool` (or `_list`) column.

Qdrant's `facet(collection, key, facet_filter, limit, exact)`, as this project states it (parity unpinned): for every
value v of the payload field `key`, count(v) = the number of points the filter keeps whose field holds v.

  the field's values are read as `filters.matches` reads them (`filters._get` / `_values`: a scalar is its own
  one-element list, a dotted path walks nested dicts);
  a list-valued field holds v when some element equals v: a point counts ONCE per value however often the value repeats;
  missing, None and [] contribute nothing;
  values of type `str`, `bool` and `int` (not bool) are counted, every other value (a float, a dict, a nested list, None
  inside a list) is ignored.

The result is at most `limit` pairs (value, count) with count > 0, ordered by count descending, then value ascending
(Python's order on `str` and on `int`; False < True); between types bool < int < str.

True == 1 and hash(True) == hash(1) in Python, so a dict keyed by the values themselves would merge the two.  The counts
are therefore keyed as `grouping.group_value` keys a group: (tag, value) with tag "bool" | "int" | "str".  `facet_top`
returns the plain values.

The counts are integers, so the kernels (facet.hip) are tested against `facet_counts` / `facet_top` for exact equality,
as `filters.matches` is both the oracle and the fallback of the payload index's masks."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import filters as _filters

MAX_LIMIT = 2048      # the most hits the device path ranks (hx.h: hx_facet_top); the host path takes any limit >= 1
_ORDER = {"bool": 0, "int": 1, "str": 2}

FacetKey = Tuple[str, Any]


def facet_key(v) -> Optional[FacetKey]:
    """(tag, v) for a value a facet counts, None for one it ignores."""
    if type(v) is bool:
        return ("bool", v)
    if type(v) is int:
        return ("int", v)
    if type(v) is str:
        return ("str", v)
    return None


def keep_rows(keep, n: int) -> Optional[np.ndarray]:
    """A row selection as one bool per row: None (every row), a bool sequence of n entries, or the packed np.uint32 words
    of a row mask (bit r & 31 of word r >> 5 = row r, what filters.row_mask and hx_payload_mask give)."""
    if keep is None:
        return None
    k = np.asarray(keep)
    if k.dtype == np.uint32:
        if k.shape[0] != (n + 31) // 32:
            raise ValueError(f"keep: {k.shape[0]} words for {n} rows (want {(n + 31) // 32})")
        return np.unpackbits(np.ascontiguousarray(k).view(np.uint8), bitorder="little")[:n].astype(bool)
    k = k.astype(bool)
    if k.shape[0] != n:
        raise ValueError(f"keep: {k.shape[0]} entries for {n} rows")
    return k


def facet_counts(payloads: Sequence[Any], key: str, keep=None) -> Dict[FacetKey, int]:
    """{(tag, value): count} over the rows of `payloads` that `keep` keeps (see keep_rows)."""
    rows = keep_rows(keep, len(payloads))
    counts: Dict[FacetKey, int] = {}
    for r, p in enumerate(payloads):
        if rows is not None and not rows[r]:
            continue
        v = _filters._get(p, key)
        if v is _filters._MISSING or v is None:
            continue
        seen = set()
        for x in _filters._values(v):
            k = facet_key(x)
            if k is not None and k not in seen:
                seen.add(k)
                counts[k] = counts.get(k, 0) + 1
    return counts


def check_limit(limit) -> None:
    if isinstance(limit, bool) or not isinstance(limit, int) or limit < 1:
        raise ValueError(f"limit must be a positive integer, got {limit!r}")


def facet_top(counts: Dict[FacetKey, int], limit: int) -> List[Tuple[Any, int]]:
    """The at most `limit` (value, count) pairs with count > 0: count descending, then bool < int < str, then value
    ascending."""
    check_limit(limit)
    hits = [(k, c) for k, c in counts.items() if c > 0]
    hits.sort(key=lambda kc: (-kc[1], _ORDER[kc[0][0]], kc[0][1]))
    return [(k[1], c) for k, c in hits[:limit]]
