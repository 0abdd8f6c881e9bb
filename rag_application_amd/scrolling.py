"""Scroll on the host: the model of hx_scroll_rows / hx_payload_order and the path a scroll takes
when its order key has no live `number` / `datetime` column.

Qdrant's `scroll(collection, scroll_filter, limit, offset, order_by)`, as this project states it (parity unpinned).

Plain scroll: the points the filter keeps, in ROW order (the engine's insertion order, which every tie of this project
uses).  A page starts at the row of the point whose id is `offset` (inclusive) and holds at most `limit` points;
`next_page_offset` is the id of the first kept point after the page, or None.

Ordered scroll, order_by = {"key": K, "direction": "asc" | "desc", "start_from": v}: a point is ORDERABLE when
`filters._get(payload, K)` is

  an `int` or `float` that is neither a `bool` nor a NaN -- its order value is itself;
  a `datetime.datetime` -- its order value is its integer microseconds since the epoch (a naive one is read as UTC);
  a `str` that parses as RFC 3339 (`Z` accepted, a time without an offset read as UTC) -- the same microseconds.

A missing or None value, a list, or anything else leaves the point out (Qdrant's once-per-list-element rule is out of
scope).  The order is the order value in the given direction, then the row ASCENDING -- for both directions; -0.0 equals
0.0 (Python's comparison).  `start_from` is inclusive: >= for asc, <= for desc.  Qdrant offers no cursor with order_by;
this project's is the pair (order value, row): a page continues STRICTLY after the pair of the previous page's last
point, so the pages of one scan partition the ordered list however many points share a value.

Every comparison here is Python's exact int / float comparison, so the kernels (scroll.hip), which compare the bits of
exact doubles, are tested against this module for exact equality."""
from __future__ import annotations

import datetime as _dt
import re
from typing import Any, List, Optional, Sequence, Tuple

from . import faceting as _faceting
from . import filters as _filters

MAX_LIMIT = 2048      # the most rows one device call returns (hx.h: HX_SCROLL_MAX_LIMIT)
DIRECTIONS = ("asc", "desc")
_EPOCH = _dt.datetime(1970, 1, 1, tzinfo=_dt.timezone.utc)
_RFC3339 = re.compile(r"^(\d{4})-(\d{2})-(\d{2})[Tt ](\d{2}):(\d{2}):(\d{2})(?:\.(\d+))?([Zz]|[+-]\d{2}:\d{2})?$")


def datetime_micros(v) -> Optional[int]:
    """The integer microseconds since the epoch of a `datetime.datetime` or of a `str` that parses as RFC 3339; None for
    anything else (an unparsable string, a date no datetime holds)."""
    if isinstance(v, str):
        m = _RFC3339.match(v)
        if m is None:
            return None
        y, mo, d, h, mi, s, frac, off = m.groups()
        tz = _dt.timezone.utc
        if off and off not in "Zz":
            minutes = int(off[1:3]) * 60 + int(off[4:6])
            tz = _dt.timezone(_dt.timedelta(minutes=-minutes if off[0] == "-" else minutes))
        try:
            v = _dt.datetime(int(y), int(mo), int(d), int(h), int(mi), int(s), int(((frac or "") + "000000")[:6]), tz)
        except (ValueError, OverflowError):
            return None
    if not isinstance(v, _dt.datetime):
        return None
    if v.tzinfo is None or v.tzinfo.utcoffset(v) is None:
        v = v.replace(tzinfo=_dt.timezone.utc)
    try:
        delta = v - _EPOCH
    except OverflowError:
        return None
    return (delta.days * 86400 + delta.seconds) * 1000000 + delta.microseconds


def order_value(v):
    """The order value of a payload value (an int or a float), None when the value is not orderable."""
    if isinstance(v, bool):
        return None
    if isinstance(v, int):
        return v
    if isinstance(v, float):
        return None if v != v else v
    if isinstance(v, (str, _dt.datetime)):
        return datetime_micros(v)
    return None


def check_limit(limit, most: Optional[int] = None) -> None:
    if isinstance(limit, bool) or not isinstance(limit, int) or limit < 1 or (most is not None and limit > most):
        raise ValueError(f"limit must be an integer in [1, {most}]" if most else "limit must be a positive integer")


def check_order_by(order_by) -> Tuple[str, bool, Any]:
    """(key, descending, start_from as an order value or None) of an order_by; ValueError for one no scroll can serve.
    A bare string is the key, ascending."""
    if isinstance(order_by, str):
        order_by = {"key": order_by}
    if not isinstance(order_by, dict) or set(order_by) - {"key", "direction", "start_from"}:
        raise ValueError('order_by must be {"key": ..., "direction": "asc" | "desc", "start_from": ...}')
    key = order_by.get("key")
    if not isinstance(key, str) or not key:
        raise ValueError("order_by: key must be a non-empty string (a payload key, dotted paths allowed)")
    direction = order_by.get("direction") or "asc"
    if direction not in DIRECTIONS:
        raise ValueError(f"order_by: direction must be one of {DIRECTIONS}, got {direction!r}")
    start = order_by.get("start_from")
    if start is not None:
        start = order_value(start)
        if start is None:
            raise ValueError("order_by: start_from must be a number that is not a NaN, a datetime or an RFC 3339 string")
    return key, direction == "desc", start


def scroll_rows(n: int, keep, start_row: int, limit: int) -> List[int]:
    """hx_scroll_rows: the first `limit` rows r in [start_row, n) that `keep` keeps (see faceting.keep_rows), ascending."""
    check_limit(limit)
    rows = _faceting.keep_rows(keep, n)
    out: List[int] = []
    for r in range(max(int(start_row), 0), n):
        if rows is None or rows[r]:
            out.append(r)
            if len(out) == limit:
                break
    return out


def ordered_rows(payloads: Sequence[Any], key: str, desc: bool, keep=None, start_from=None,
                 after: Optional[Tuple[Any, int]] = None, limit: Optional[int] = None) -> List[Tuple[int, Any]]:
    """hx_payload_order over the payloads: [(row, order value)] of the orderable rows `keep` keeps that lie within
    start_from (an order value; inclusive) and strictly after the cursor `after` = (order value, row), in the order
    (value in the direction, row ascending); the first `limit` of them (None: all)."""
    if limit is not None:
        check_limit(limit)
    rows = _faceting.keep_rows(keep, len(payloads))
    hits: List[Tuple[int, Any]] = []
    for r, p in enumerate(payloads):
        if rows is not None and not rows[r]:
            continue
        v = _filters._get(p, key)
        if v is _filters._MISSING or v is None:
            continue
        x = order_value(v)
        if x is None:
            continue
        if start_from is not None and (x > start_from if desc else x < start_from):
            continue
        if after is not None:
            av, ar = after
            if (x > av if desc else x < av) or (x == av and r <= ar):
                continue
        hits.append((r, x))
    # a stable sort by the value alone keeps the rows ascending inside a value in both directions (reverse=True keeps
    # equal keys in their original order) and never negates a value
    hits.sort(key=lambda h: h[1], reverse=desc)
    return hits if limit is None else hits[:limit]
