"""Payload index: indexed payload fields as engine columns, filters as predicate programs.

Qdrant's `create_payload_index(collection, field_name, field_schema)`, the engine's way.  A `PayloadIndex` belongs to
one collection.  It knows the indexed keys (dotted paths as `filters._get` reads them), each key's schema
("keyword" | "number" | "bool" | "datetime"), the keyword dictionaries (str -> code) and the ids of the engine columns
(hx.h: hx_payload_*).  It does two things:

  encode(key, payloads)   the cells of some rows of one key -- or None when a value POISONS the key;
  compile(filter)         the postfix program hx_payload_mask evaluates -- or None when the filter is DECLINED.

The oracle is `filters.matches`: whatever compiles gives exactly its mask; everything else goes the Python way
(`filters.row_mask`), which is always right and only slow.

A row's value: missing -> MISSING, None -> NULL, a value of the key's schema -> its cell.  Values of the schema are a
`str` (keyword), a `bool` (bool), an `int` / `float` that is not a bool, not a NaN and -- an int -- at most 2^53 in
magnitude (number: every stored number is then an exact double, and Python's exact int / float comparison is IEEE's).
Anything else (a list, a dict, a value of another type, NaN, an oversized int) poisons the key: its column is
dropped and every filter that mentions the key is declined until the index on it is created again.

List schemas ("keyword_list" | "number_list" | "bool_list") are opt-in: a row's value is then
missing, None, or a `list` of values of the element schema ([] included); a bare scalar of the element schema is stored
as the one-element list (filters._values makes the two equivalent in every clause).  A tuple (() is not [] to
is_empty), a nested list or dict, a None element, a NaN, an oversized int or an element of another type poisons the
key.  The clauses compile to the list ops: one element has to meet a whole `range`, as filters._range asks.

The text schema ("text") is opt-in too: a row's value is missing, None, or a `str`, stored as the
UTF-8 bytes of `value.lower()`; anything else (a number, a bool, a list, a dict, a string with a lone surrogate) poisons
the key.  `match text` on such a key compiles to one TEXT_ALL over the distinct words of `str(text).lower().split()`,
each as UTF-8 bytes: UTF-8 is self-synchronising, so a byte-substring test on the two encodings is Python's `w in hay`
on the code points.  Lower-casing and splitting stay Python's; the engine only sees bytes.

The datetime schema ("datetime") exists for ordered scrolls: a row's value is missing, None, a
`datetime.datetime` or a `str` that parses as RFC 3339 (scrolling.datetime_micros), stored as an F64 cell holding the
integer microseconds since the epoch -- exact while |us| <= 2^53; anything else (a number, an unparsable string, a value
outside that range) poisons the key.  The compiler DECLINES every condition on such a key: `filters.matches` compares the
payload's own value, not its microseconds, and the masks stay what it gives.

Array keys ("A[].f" with schema "keyword" | "number" | "bool") index one field of the objects of an
array of objects: exactly one "[]", `A` and `f` dotted paths without one.  The key is stored as an ordinary list column
that holds ONE element per object of `A`, so every key "A[].*" of one parent has the same heads and offsets (they are
"element-aligned").  A row's head: `A` missing or not a list -> MISSING, None -> NULL, a list -> len(A).  Element i is the
cell of A[i][f] when that value is of the schema; for a keyword or bool key it is the reserved code ABSENT when A[i] is
not a dict, lacks `f` or holds None there (no string maps to it: such a key's dictionary holds one code fewer); a value
of another type, a list or a dict poisons the key.  For a NUMBER key an absent or None field poisons the key too: the
engine refuses NaN elements, so there is no spare double.  A payload whose dict holds the literal key "A[]" (which
filters._get prefers) poisons the key.
A plain condition on "A[].f" compiles to the list ops (ABSENT lies in no set); is_empty / is_null on it are declined
(aligned storage cannot tell "no object has f" from []), and so is a None among the constants of its match.
{"nested": {"key": A, "filter": F}} compiles to ONE nested block (hx.h: HX_PAY_NESTED) when every leaf of F is a match
value / any / except or a range on a key f whose "A[].f" is live, joined by must / should / must_not and sub-filters; at
element level `except` is "not ABSENT and not in the set".  Everything else declines: is_empty, is_null, match text, a
nested inside, an unindexed or poisoned f, more than 64 element ops or 8 distinct columns, and a parent in which some
stored array held an element that is not a dict (the oracle skips such an element, a position cannot)."""
from __future__ import annotations

import math
import struct
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np

from . import filters as _filters
from . import scrolling as _scrolling

# hx.h
PAY_U32, PAY_F64, PAY_LIST_U32, PAY_LIST_F64, PAY_TEXT = 1, 2, 3, 4, 5
U32_MISSING, U32_NULL = 0xFFFFFFFF, 0xFFFFFFFE
F64_MISSING, F64_NULL = 0x7FF80000FFFFFFFF, 0x7FF80000FFFFFFFE
MAX_STACK, MAX_OPS, MAX_COLUMNS = 32, 4096, 64
(TRUE, FALSE, IS_MISSING, IS_NULL, PRESENT, EQ, IN, LT, LE, GT, GE, ROW_IN, AND, OR, NOT, ANY_EQ, ANY_IN, ANY_RANGE,
 IS_EMPTY_LIST, TEXT_ALL) = range(20)
NESTED, EL_EQ, EL_IN, EL_RANGE = 20, 21, 22, 23
NESTED_MAX_OPS, NESTED_MAX_COLS = 64, 8
ABSENT = 0xFFFFFFFD                     # host-side: the element of an array key whose object lacks the field
TEXT_MAX_WORDS, TEXT_MAX_WORD_BYTES = 32, 64
TEXT_MAX_COLUMN_WORDS = 0x7FFFFFFF      # a text column holds fewer than 2^31 32-bit words

SCHEMAS = {"keyword": "keyword", "number": "number", "integer": "number", "float": "number", "bool": "bool",
           "keyword_list": "keyword_list", "number_list": "number_list", "integer_list": "number_list",
           "float_list": "number_list", "bool_list": "bool_list", "text": "text", "datetime": "datetime"}
_CLAUSES = ("must", "should", "must_not")
_MAX_KEYWORDS = U32_NULL            # codes 0 .. 0xFFFFFFFD


def schema_of(field_schema) -> str:
    s = SCHEMAS.get(str(field_schema).lower()) if isinstance(field_schema, str) else None
    if s is None:
        raise ValueError(f"field_schema must be one of {sorted(SCHEMAS)}, got {field_schema!r}")
    return s


def f64_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def exact_double(v) -> Optional[float]:
    """The double equal to the int / float v (Python compares the two kinds exactly), None when there is none: a
    bool, another type, a NaN, an int no double holds."""
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        return None
    if isinstance(v, float):
        return None if v != v else v
    try:
        f = float(v)
    except OverflowError:
        return None
    return f if f == v else None


def split_array_key(key) -> Optional[Tuple[str, str]]:
    """(A, f) of an array key "A[].f", None for a key without "[]"; ValueError for any other use of "[]"."""
    if not isinstance(key, str) or "[]" not in key:
        return None
    a, sep, f = key.partition("[].")
    if not sep or "[]" in a or "[]" in f or not all(a.split(".")) or not all(f.split(".")):
        raise ValueError(f'an array key is "A[].f" with exactly one "[]", A and f dotted paths, got {key!r}')
    return a, f


class _Decline(Exception):
    pass


class _Key:
    def __init__(self, schema: str, key: Optional[str] = None):
        self.schema = schema
        self.array = split_array_key(key)  # (A, f) of an array key "A[].f": stored as a list column, one element per object
        if self.array and schema not in ("keyword", "number", "bool"):
            raise ValueError(f"an array key takes the schema keyword, number (integer, float) or bool, got {schema!r}")
        self.nondict = False               # an array key: some stored array held an element that is not a dict
        self.col: Optional[int] = None     # the engine column; None = not live (poisoned, or its column was lost)
        self.codes: Dict[str, int] = {}    # keyword -> code
        self._names: List[str] = []        # code -> keyword, built when a grouped search asks (value_of)
        self._ranks: Optional[np.ndarray] = None   # code -> position of its keyword in sorted order (ranks)
        self._sorted: List[str] = []       # position -> keyword

    def value_of(self, code: int):
        """The stored value a cell of a "keyword" or "bool" column stands for: what a grouped search names a group by."""
        if self.schema == "bool":
            return bool(code)
        if len(self._names) != len(self.codes):           # codes are handed out in order and never taken back
            self._names = list(self.codes)
        return self._names[code]

    def ranks(self) -> Optional[np.ndarray]:
        """np.uint32 [len(codes)]: the position of each code's keyword in sorted order (Python's order on `str`) -- the
        rank array of hx_facet_top, which carries the tie order "value ascending" onto the device.  Cached; built again
        when the dictionary has grown (codes are never taken back).  None for a bool key: False = 0 < True = 1, a code
        ranks as itself."""
        if self.elem != "keyword":
            return None
        if self._ranks is None or self._ranks.shape[0] != len(self.codes):
            names = list(self.codes)                          # (in code order: dicts keep insertion order)
            order = sorted(range(len(names)), key=names.__getitem__)
            r = np.empty(len(names), np.uint32)
            r[order] = np.arange(len(names), dtype=np.uint32)
            self._ranks, self._sorted = r, [names[i] for i in order]
        return self._ranks

    def value_at(self, rank: int):
        """The keyword at a position of the sorted order `ranks` describes (a bool key: the code's value)."""
        if self.elem != "keyword":
            return bool(rank)
        self.ranks()
        return self._sorted[rank]

    @property
    def is_list(self) -> bool:
        return self.schema.endswith("_list") or self.array is not None

    @property
    def elem(self) -> str:             # the schema of a cell, or of a list's elements
        return self.schema[:-5] if self.schema.endswith("_list") else self.schema

    @property
    def is_text(self) -> bool:
        return self.schema == "text"

    @property
    def kind(self) -> int:
        if self.is_text:
            return PAY_TEXT
        if self.is_list:
            return PAY_LIST_F64 if self.elem == "number" else PAY_LIST_U32
        return PAY_F64 if self.schema in ("number", "datetime") else PAY_U32


class PayloadIndex:
    def __init__(self):
        self.keys: Dict[str, _Key] = {}
        self.device_evals = 0              # masks evaluated by hx_payload_mask
        self.python_evals = 0              # masks evaluated by the Python loop
        self.declined: Dict[str, int] = {}  # reason -> filters that did not compile
        self.group_device_calls = 0        # grouped searches served by hx_hybrid_query_groups_host
        self.facet_device_calls = 0        # facets served by hx_payload_facet_host
        self.facet_python_calls = 0        # facets counted by faceting.py over the payloads
        self.scroll_device_calls = 0       # scrolls served by hx_scroll_rows_host / hx_payload_order_host
        self.scroll_python_calls = 0       # scrolls walked by scrolling.py over the payloads
        self.boost_device_calls = 0        # boosted searches served by hx_hybrid_query_formula_host

    # -- definitions -----------------------------------------------------------------------------------------------
    def definitions(self) -> Dict[str, str]:
        return {k: v.schema for k, v in self.keys.items()}

    def live(self, key: str) -> bool:
        return key in self.keys and self.keys[key].col is not None

    def live_keys(self) -> List[str]:
        return [k for k, v in self.keys.items() if v.col is not None]

    # -- encoder ---------------------------------------------------------------------------------------------------
    def encode(self, key: str, payloads, heads_of: Optional[Dict[str, np.ndarray]] = None) -> Optional[np.ndarray]:
        """The cells of `payloads` for `key` (np.uint32 codes or np.uint64 bit patterns of doubles), or None when a
        value poisons the key.  Keywords met for the first time get the next code; a poisoned call leaves the
        dictionary with codes no row uses, which is harmless.  heads_of: parent -> heads, shared by the array keys of
        one parent over one batch."""
        k = self.keys[key]
        get, missing = _filters._get, _filters._MISSING
        n = len(payloads)
        if k.array:
            return self._encode_array(k, payloads, heads_of)
        if k.is_list:
            return self._encode_lists(k, key, payloads)
        if k.is_text:
            return self._encode_text(key, payloads)
        if k.schema == "datetime":
            vals = np.zeros(n, np.float64)
            special = []
            for r, p in enumerate(payloads):
                v = get(p, key)
                if v is missing:
                    special.append((r, F64_MISSING))
                elif v is None:
                    special.append((r, F64_NULL))
                else:
                    us = _scrolling.datetime_micros(v)
                    if us is None or abs(us) > 2 ** 53:
                        return None
                    vals[r] = float(us)
            cells = vals.view(np.uint64).copy()
            for r, bits in special:
                cells[r] = bits
            return cells
        if k.schema == "number":
            vals = np.zeros(n, np.float64)
            special: List[Tuple[int, int]] = []
            for r, p in enumerate(payloads):
                v = get(p, key)
                if v is missing:
                    special.append((r, F64_MISSING))
                elif v is None:
                    special.append((r, F64_NULL))
                elif isinstance(v, bool) or not isinstance(v, (int, float)):
                    return None
                elif isinstance(v, float):
                    if v != v:
                        return None
                    vals[r] = v
                else:
                    if abs(v) > 2 ** 53:
                        return None
                    vals[r] = float(v)
            cells = vals.view(np.uint64).copy()
            for r, bits in special:
                cells[r] = bits
            return cells
        cells = np.empty(n, np.uint32)
        if k.schema == "bool":
            for r, p in enumerate(payloads):
                v = get(p, key)
                if v is missing:
                    cells[r] = U32_MISSING
                elif v is None:
                    cells[r] = U32_NULL
                elif isinstance(v, bool):
                    cells[r] = 1 if v else 0
                else:
                    return None
            return cells
        codes = k.codes
        for r, p in enumerate(payloads):
            v = get(p, key)
            if v is missing:
                cells[r] = U32_MISSING
            elif v is None:
                cells[r] = U32_NULL
            elif type(v) is str:
                c = codes.get(v)
                if c is None:
                    if len(codes) >= _MAX_KEYWORDS:
                        return None
                    c = codes[v] = len(codes)
                cells[r] = c
            else:
                return None
        return cells

    def _encode_lists(self, k: _Key, key: str, payloads):
        """(heads, values) of a list key for hx_payload_append_lists -- heads: np.uint32, MISSING / NULL / the row's
        element count; values: the rows' elements one after another, np.uint32 codes or np.float64 -- or None when a
        value poisons the key.  The element rules are the scalar encoder's."""
        get, missing = _filters._get, _filters._MISSING
        elem, codes = k.elem, k.codes
        heads = np.empty(len(payloads), np.uint32)
        vals: List[Any] = []
        for r, p in enumerate(payloads):
            v = get(p, key)
            if v is missing:
                heads[r] = U32_MISSING
                continue
            if v is None:
                heads[r] = U32_NULL
                continue
            row = v if type(v) is list else (v,)          # (a tuple inside the 1-tuple fails the element test below)
            for x in row:
                if elem == "keyword":
                    if type(x) is not str:
                        return None
                    c = codes.get(x)
                    if c is None:
                        if len(codes) >= _MAX_KEYWORDS:
                            return None
                        c = codes[x] = len(codes)
                    vals.append(c)
                elif elem == "bool":
                    if not isinstance(x, bool):
                        return None
                    vals.append(1 if x else 0)
                else:
                    if isinstance(x, bool) or not isinstance(x, (int, float)) or x != x:
                        return None
                    if isinstance(x, int) and abs(x) > 2 ** 53:
                        return None
                    vals.append(float(x))
            heads[r] = len(row)
        return heads, np.array(vals, np.float64 if elem == "number" else np.uint32)

    @staticmethod
    def array_heads(parent: str, payloads) -> Optional[np.ndarray]:
        """The heads of an array parent `A` over a batch: MISSING (missing or not a list), NULL (None) or len(A); None
        when a payload holds the literal key "A[]", which filters._get reads instead."""
        get, missing = _filters._get, _filters._MISSING
        up, _, last = parent.rpartition(".")
        heads = np.empty(len(payloads), np.uint32)
        for r, p in enumerate(payloads):
            holder = get(p, up) if up else p
            if isinstance(holder, dict) and (last + "[]") in holder:
                return None
            v = get(p, parent)
            heads[r] = U32_NULL if v is None else len(v) if type(v) is list else U32_MISSING
        return heads

    def _encode_array(self, k: _Key, payloads, heads_of):
        """(heads, values) of an array key "A[].f" for hx_payload_append_lists: ONE element per object of A (the module
        docstring states the rules), or None when a value poisons the key."""
        get, missing = _filters._get, _filters._MISSING
        parent, field = k.array
        heads = heads_of.get(parent) if heads_of is not None else None
        if heads is None:
            heads = self.array_heads(parent, payloads)
            if heads is None:
                return None
            if heads_of is not None:
                heads_of[parent] = heads
        elem, codes = k.elem, k.codes
        vals: List[Any] = []
        for r, p in enumerate(payloads):
            if heads[r] >= U32_NULL:
                continue
            for el in get(p, parent):
                x = get(el, field) if isinstance(el, dict) else missing
                if not isinstance(el, dict):
                    k.nondict = True
                if x is missing or x is None:
                    if elem == "number":
                        return None
                    vals.append(ABSENT)
                elif elem == "keyword":
                    if type(x) is not str:
                        return None
                    c = codes.get(x)
                    if c is None:
                        if len(codes) >= ABSENT:          # codes 0 .. ABSENT - 1
                            return None
                        c = codes[x] = len(codes)
                    vals.append(c)
                elif elem == "bool":
                    if not isinstance(x, bool):
                        return None
                    vals.append(1 if x else 0)
                else:
                    if isinstance(x, bool) or not isinstance(x, (int, float)) or x != x:
                        return None
                    if isinstance(x, int) and abs(x) > 2 ** 53:
                        return None
                    vals.append(float(x))
        return heads, np.array(vals, np.float64 if elem == "number" else np.uint32)

    @staticmethod
    def _encode_text(key: str, payloads):
        """(heads, data) of a text key for hx_payload_append_text -- heads: np.uint32, MISSING / NULL / the row's byte
        length; data: the rows' bytes one after another (bytes) -- or None when a value poisons the key: anything that is
        not a `str` (a `str` is never == [], which keeps is_empty exact), a string with a lone surrogate, or rows whose
        bytes, each padded to a 32-bit word, would pass the column limit."""
        get, missing = _filters._get, _filters._MISSING
        heads = np.empty(len(payloads), np.uint32)
        parts: List[bytes] = []
        words = 0
        for r, p in enumerate(payloads):
            v = get(p, key)
            if v is missing:
                heads[r] = U32_MISSING
            elif v is None:
                heads[r] = U32_NULL
            elif type(v) is str:
                try:
                    b = v.lower().encode("utf-8")
                except UnicodeEncodeError:
                    return None
                words += (len(b) + 3) // 4
                if words > TEXT_MAX_COLUMN_WORDS:
                    return None
                heads[r] = len(b)
                parts.append(b)
            else:
                return None
        return heads, b"".join(parts)

    @staticmethod
    def text_blob(words: List[bytes]) -> bytes:
        """The pattern blob of TEXT_ALL (hx.h): uint32 P, uint32 len[P], the patterns' bytes one after another."""
        return struct.pack(f"<{1 + len(words)}I", len(words), *[len(w) for w in words]) + b"".join(words)

    # -- compiler --------------------------------------------------------------------------------------------------
    def compile(self, flt, id_rows: Optional[Callable[[], Dict[Any, int]]] = None):
        """(ops, sets) for hx_payload_mask -- ops: (op, column, imm) triples, sets: sorted np.uint32 / np.float64
        arrays, or the pattern blob (bytes) of a TEXT_ALL -- or None when the filter is declined (the reason is counted in `declined`).  Unknown clause names of
        the filter itself raise ValueError, as filters.matches does.  id_rows: gives the collection's id -> row
        dictionary (for has_id)."""
        if flt and isinstance(flt, dict):
            unknown = set(flt) - set(_CLAUSES)
            if unknown:
                raise ValueError(f"unsupported filter clause(s): {sorted(unknown, key=str)}")
        ops: List[Tuple[int, int, int]] = []
        sets: List[np.ndarray] = []
        try:
            self._filter(flt, ops, sets, id_rows)
            if len(ops) > MAX_OPS:
                raise _Decline("program too long")
            depth, skip = 0, 0
            for op, _, imm in ops:
                if skip:                              # (the element ops of a nested block: counted by _nested)
                    skip -= 1
                    continue
                skip = imm if op == NESTED else 0
                depth += -1 if op in (AND, OR) else 0 if op == NOT else 1
                if depth > MAX_STACK:
                    raise _Decline("stack deeper than 32")
        except _Decline as d:
            reason = str(d)
            self.declined[reason] = self.declined.get(reason, 0) + 1
            return None
        return ops, sets

    def _filter(self, flt, ops, sets, id_rows, cond=None):
        cond = cond or self._condition
        if not flt:
            ops.append((TRUE, 0, 0))
            return
        if not isinstance(flt, dict):
            raise _Decline("filter is not a dict")
        if set(flt) - set(_CLAUSES):
            raise _Decline("unknown clause in a nested filter")      # (matches raises only where evaluation reaches it)
        terms = 0
        for c in _filters._as_list(flt.get("must")):
            cond(c, ops, sets, id_rows)
            if terms:
                ops.append((AND, 0, 0))
            terms += 1
        for c in _filters._as_list(flt.get("must_not")):
            cond(c, ops, sets, id_rows)
            ops.append((NOT, 0, 0))
            if terms:
                ops.append((AND, 0, 0))
            terms += 1
        should = _filters._as_list(flt.get("should"))
        for i, c in enumerate(should):
            cond(c, ops, sets, id_rows)
            if i:
                ops.append((OR, 0, 0))
        if should:
            if terms:
                ops.append((AND, 0, 0))
            terms += 1
        if not terms:
            ops.append((TRUE, 0, 0))

    def _key(self, key) -> _Key:
        if not isinstance(key, str):
            raise _Decline("key is not a string")
        k = self.keys.get(key)
        if k is None:
            raise _Decline("unindexed key")
        if k.col is None:
            raise _Decline("poisoned key")
        if k.schema == "datetime":
            raise _Decline("datetime key")
        return k

    def _condition(self, c, ops, sets, id_rows):
        if not isinstance(c, dict):
            raise _Decline("condition is not a dict")
        if any(k in c for k in _CLAUSES):
            return self._filter(c, ops, sets, id_rows)
        if "nested" in c:
            return self._nested(c["nested"], ops, sets)
        if "has_id" in c:
            listed = c["has_id"]
            if not isinstance(listed, (list, tuple)) or id_rows is None:
                raise _Decline("has_id form")
            rows = id_rows()
            if rows is None:
                raise _Decline("has_id over duplicate ids")
            found = set()
            for i in listed:
                try:
                    r = rows.get(i)
                except TypeError:                     # unhashable: equal to no id
                    r = None
                if r is not None and type(i) is str:
                    found.add(r)
            sets.append(np.array(sorted(found), np.uint32))
            ops.append((ROW_IN, 0, len(sets) - 1))
            return
        if "is_empty" in c or "is_null" in c:
            what = "is_empty" if "is_empty" in c else "is_null"
            if not isinstance(c[what], dict) or "key" not in c[what]:
                raise _Decline(what + " form")
            k = self._key(c[what]["key"])
            if k.array:
                raise _Decline(what + " on an array key")
            if what == "is_empty":
                ops.extend([(IS_MISSING, k.col, 0), (IS_NULL, k.col, 0), (OR, 0, 0)])
                if k.is_list:
                    ops.extend([(IS_EMPTY_LIST, k.col, 0), (OR, 0, 0)])
            else:
                ops.append((IS_NULL, k.col, 0))
            return
        if "key" in c:
            if "match" in c:
                return self._match(self._key(c["key"]), c["match"], ops, sets)
            if "range" in c:
                return self._range(self._key(c["key"]), c["range"], ops, sets)
        raise _Decline("unsupported condition")

    @staticmethod
    def _cell_of(k: _Key, v) -> Optional[int]:
        """The cell a stored value equal to the constant v has (filters._match's rule for `value`: equal, and of the
        same type or neither a bool), None when no stored value of the key's schema can equal it."""
        if k.elem == "keyword":
            return k.codes.get(v) if isinstance(v, str) else None
        if k.elem == "bool":
            return (1 if v else 0) if isinstance(v, bool) else None
        d = exact_double(v)
        return None if d is None else f64_bits(d)

    def _set_of(self, k: _Key, listed) -> np.ndarray:
        """The cells equal (Python's ==, as `in` compares) to an entry of the list."""
        if not isinstance(listed, (list, tuple)):
            raise _Decline("match list is not a list")
        has_bool = any(isinstance(e, bool) for e in listed)
        has_num = any(isinstance(e, (int, float)) and not isinstance(e, bool) for e in listed)
        if has_bool and has_num:
            raise _Decline("list mixes bools and numbers")
        out = set()
        for e in listed:
            if k.elem == "keyword":
                if isinstance(e, str) and e in k.codes:
                    out.add(k.codes[e])
            elif k.elem == "bool":                  # True == 1 and False == 0 under `in`
                if isinstance(e, (bool, int, float)) and e == 0:
                    out.add(0)
                elif isinstance(e, (bool, int, float)) and e == 1:
                    out.add(1)
            else:
                d = float(e) if isinstance(e, bool) else exact_double(e)
                if d is not None:
                    out.add(d + 0.0)                  # (-0.0 and 0.0 are one entry: -0.0 + 0.0 = 0.0)
        if k.elem == "number":
            return np.array(sorted(out), np.float64)
        return np.array(sorted(out), np.uint32)

    def _match(self, k: _Key, m, ops, sets):
        if not isinstance(m, dict):
            raise _Decline("match is not a dict")
        if k.is_text:
            return self._match_text(k, m, ops, sets)
        if k.array:                                   # (a None field is collected by the projection, and stored as ABSENT)
            form = next((f for f in ("value", "any", "except") if f in m), None)
            if form and (m[form] is None or (form != "value" and isinstance(m[form], (list, tuple))
                                             and any(e is None for e in m[form]))):
                raise _Decline("None in a match on an array key")
        if "value" in m:
            v = m["value"]
            if v is not None and not isinstance(v, (str, bool, int, float)):
                raise _Decline("match value of an unsupported type")
            cell = self._cell_of(k, v)
            ops.append((FALSE, 0, 0) if cell is None else (ANY_EQ if k.is_list else EQ, k.col, cell))
        elif "any" in m:
            sets.append(self._set_of(k, m["any"]))
            ops.append((ANY_IN if k.is_list else IN, k.col, len(sets) - 1))
        elif "except" in m:                           # (a list: no element is listed -- [] passes, as all() of nothing)
            sets.append(self._set_of(k, m["except"]))
            ops.extend([(PRESENT, k.col, 0), (ANY_IN if k.is_list else IN, k.col, len(sets) - 1), (NOT, 0, 0), (AND, 0, 0)])
        elif "text" in m:
            raise _Decline("match text")
        else:
            raise _Decline("unsupported match")

    def _match_text(self, k: _Key, m, ops, sets):
        """A match on a text key.  `text` is filters._match's rule on bytes: every distinct word of
        str(text).lower().split() is a byte substring of the stored lower-cased UTF-8; no word = the value is present."""
        for form in ("value", "any", "except"):      # (the order filters._match tests them in)
            if form in m:
                raise _Decline(f"match {form} on a text key")
        if "text" not in m:
            raise _Decline("unsupported match")
        words: List[bytes] = []
        for w in dict.fromkeys(str(m["text"]).lower().split()):
            try:
                b = w.encode("utf-8")
            except UnicodeEncodeError:
                raise _Decline("match text word with a lone surrogate")
            if len(b) > TEXT_MAX_WORD_BYTES:
                raise _Decline("match text word over 64 bytes")
            words.append(b)
        if len(words) > TEXT_MAX_WORDS:
            raise _Decline("match text with more than 32 words")
        if not words:
            ops.append((PRESENT, k.col, 0))
            return
        sets.append(self.text_blob(words))
        ops.append((TEXT_ALL, k.col, len(sets) - 1))

    def _range(self, k: _Key, r, ops, sets):
        if not isinstance(r, dict):
            raise _Decline("range is not a dict")
        if k.is_text:
            raise _Decline("range on a text key")
        if k.elem != "number":                        # (filters._range: only numbers that are not bools are in a range)
            ops.append((FALSE, 0, 0))
            return
        if k.is_list:
            return self._range_any(k, r, ops, sets)
        terms = 0
        for name, op in (("gt", GT), ("gte", GE), ("lt", LT), ("lte", LE)):
            b = r.get(name)
            if b is None:
                continue
            if isinstance(b, bool) or not isinstance(b, (int, float)):
                raise _Decline("range bound is not a number")
            if b != b:
                ops.append((FALSE, 0, 0))             # nothing is ordered against a NaN
            else:
                d = exact_double(b)
                if d is None:
                    raise _Decline("range bound is not an exact double")
                ops.append((op, k.col, f64_bits(d)))
            if terms:
                ops.append((AND, 0, 0))
            terms += 1
        if not terms:
            ops.append((PRESENT, k.col, 0))

    # -- nested blocks -------------------------------------------------------------------------
    def _nested(self, nd, ops, sets):
        """{"key": A, "filter": F} as one nested block: NESTED anchor m, then the m element ops of F."""
        if not isinstance(nd, dict) or not isinstance(nd.get("key"), str):
            raise _Decline("nested form")
        parent = nd["key"][:-2] if nd["key"].endswith("[]") else nd["key"]
        if "[]" in parent:
            raise _Decline("nested key with an inner []")
        siblings = [k for name, k in self.keys.items() if k.array and k.array[0] == parent and k.col is not None]
        if not siblings:
            raise _Decline("unindexed key")
        if any(k.nondict for k in siblings):
            raise _Decline("nested over an array that holds a non-object element")
        eops: List[Tuple[int, int, int]] = []

        def cond(c, o, s, id_rows):
            if not isinstance(c, dict):
                raise _Decline("condition is not a dict")
            if any(name in c for name in _CLAUSES):
                return self._filter(c, o, s, None, cond)
            if "nested" in c:
                raise _Decline("nested inside a nested filter")
            if "has_id" in c:
                raise _Decline("has_id inside a nested filter")      # (filters.matches raises)
            if "is_empty" in c or "is_null" in c:
                raise _Decline(("is_empty" if "is_empty" in c else "is_null") + " inside a nested filter")
            if "key" in c and isinstance(c["key"], str) and "[]" not in c["key"]:
                k = self._key(parent + "[]." + c["key"])
                if "match" in c:
                    return self._el_match(k, c["match"], o, s)
                if "range" in c:
                    return self._el_range(k, c["range"], o, s)
            raise _Decline("unsupported condition")

        self._filter(nd.get("filter"), eops, sets, None, cond)
        if len(eops) > NESTED_MAX_OPS:
            raise _Decline("nested filter with more than 64 element ops")
        cols = {col for op, col, _ in eops if op in (EL_EQ, EL_IN, EL_RANGE)}
        if len(cols) > NESTED_MAX_COLS:
            raise _Decline("nested filter over more than 8 columns")
        depth = 0
        for op, _, _ in eops:
            depth += -1 if op in (AND, OR) else 0 if op == NOT else 1
            if depth > MAX_STACK:
                raise _Decline("stack deeper than 32")
        anchor = next((k.col for k in siblings if k.col in cols), siblings[0].col)
        ops.append((NESTED, anchor, len(eops)))
        ops.extend(eops)

    def _el_match(self, k: _Key, m, ops, sets):
        """filters._match on ONE element: a missing or None field (ABSENT) matches nothing, `except` included."""
        if not isinstance(m, dict):
            raise _Decline("match is not a dict")
        if "value" in m:
            v = m["value"]
            if v is not None and not isinstance(v, (str, bool, int, float)):
                raise _Decline("match value of an unsupported type")
            cell = self._cell_of(k, v)
            ops.append((FALSE, 0, 0) if cell is None else (EL_EQ, k.col, cell))
        elif "any" in m:
            sets.append(self._set_of(k, m["any"]))
            ops.append((EL_IN, k.col, len(sets) - 1))
        elif "except" in m:
            sets.append(self._set_of(k, m["except"]))
            ops.extend([(EL_IN, k.col, len(sets) - 1), (NOT, 0, 0)])
            if k.elem != "number":                    # (a number key holds no ABSENT)
                ops.extend([(EL_EQ, k.col, ABSENT), (NOT, 0, 0), (AND, 0, 0)])
        elif "text" in m:
            raise _Decline("match text inside a nested filter")
        else:
            raise _Decline("unsupported match")

    def _el_range(self, k: _Key, r, ops, sets):
        if not isinstance(r, dict):
            raise _Decline("range is not a dict")
        if k.elem != "number":                        # (filters._range: only numbers that are not bools are in a range)
            ops.append((FALSE, 0, 0))
            return
        self._range_any(k, r, ops, sets, EL_RANGE)

    def _range_any(self, k: _Key, r, ops, sets, op=ANY_RANGE):
        """filters._range over a list: ONE element meets every bound, so the bounds become one closed interval [lo, hi]
        and one ANY_RANGE op (EL_RANGE inside a nested block).  A strict bound moves to the neighbouring double (every
        stored number is a double, so x > b is x >= nextafter(b, +inf) exactly; +-0 and the subnormals included)."""
        lo, hi = -math.inf, math.inf
        for name in ("gt", "gte", "lt", "lte"):
            b = r.get(name)
            if b is None:
                continue
            if isinstance(b, bool) or not isinstance(b, (int, float)):
                raise _Decline("range bound is not a number")
            if b != b:
                ops.append((FALSE, 0, 0))             # nothing is ordered against a NaN
                return
            d = exact_double(b)
            if d is None:
                raise _Decline("range bound is not an exact double")
            if name == "gt":
                if d == math.inf:
                    ops.append((FALSE, 0, 0))
                    return
                d = math.nextafter(d, math.inf)
            elif name == "lt":
                if d == -math.inf:
                    ops.append((FALSE, 0, 0))
                    return
                d = math.nextafter(d, -math.inf)
            if name in ("gt", "gte"):
                lo = max(lo, d)
            else:
                hi = min(hi, d)
        if lo > hi:
            ops.append((FALSE, 0, 0))
            return
        sets.append(np.array([lo, hi], np.float64))
        ops.append((op, k.col, len(sets) - 1))
