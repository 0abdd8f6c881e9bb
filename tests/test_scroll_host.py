"""CPU: scroll on the host -- rag_application_amd/scrolling.py against a brute-force sorted(), the
`datetime` payload schema, the handler's argument checks over a stub index, and the four entries of the C ABI.  No GPU
needed."""
import asyncio
import datetime
import functools
import math
import os
import re

import numpy as np
import pytest

from rag_application_amd import _lib
from rag_application_amd import filters as F
from rag_application_amd import payload_index as PI
from rag_application_amd import scrolling as SC
from rag_application_amd.handler import QdrantHandler, Record, _Collection
from tests import scroll_helpers as SH

UTC = datetime.timezone.utc
T0 = datetime.datetime(2024, 5, 1, 12, 0, 0, 250000, tzinfo=UTC)
T0_US = 1714564800250000


# ---- the brute force --------------------------------------------------------------------------------------------------------
def brute_value(v):
    """the order value, restated: numbers that are no bool and no NaN, datetimes and RFC 3339 strings as microseconds"""
    if type(v) in (int, float) and v == v:
        return v
    if isinstance(v, datetime.datetime):
        if v.tzinfo is None:
            v = v.replace(tzinfo=UTC)
        return round((v - datetime.datetime(1970, 1, 1, tzinfo=UTC)) / datetime.timedelta(microseconds=1))
    if isinstance(v, str):
        try:
            d = datetime.datetime.strptime(v.replace("Z", "+0000").replace("+01:00", "+0100"),
                                           "%Y-%m-%dT%H:%M:%S.%f%z" if "." in v else "%Y-%m-%dT%H:%M:%S%z")
        except ValueError:
            return None
        return brute_value(d)
    return None


def brute(payloads, key, desc, keep=None, start=None, after=None):
    hits = []
    for r, p in enumerate(payloads):
        if keep is not None and not keep[r]:
            continue
        x = brute_value(p.get(key)) if isinstance(p, dict) else None
        if x is None:
            continue
        if start is not None and not (x <= start if desc else x >= start):
            continue
        hits.append((r, x))

    def cmp(a, b):                                         # value in the direction, then the row ascending
        if a[1] != b[1]:
            return -1 if ((a[1] > b[1]) if desc else (a[1] < b[1])) else 1
        return a[0] - b[0]
    hits = sorted(hits, key=functools.cmp_to_key(cmp))
    if after is not None:
        hits = [h for h in hits if cmp(h, (after[1], after[0])) > 0]
    return hits


VALUES = [0, 1, -1, 2.5, -2.5, 3, 3.0, True, False, float("nan"), None, [1, 2], [], {"a": 1}, -0.0, 0.0, 2 ** 53 + 1,
          -(2 ** 53) - 1, 1e300, float("inf"), -float("inf"), T0, T0.isoformat().replace("+00:00", "Z"),
          "2024-05-01T13:00:00.250000+01:00", T0.replace(tzinfo=None), T0 + datetime.timedelta(microseconds=1),
          "not a date", "2024-13-01T00:00:00Z", "", T0_US, float(T0_US)]


def table(n, rng):
    pays = []
    for _ in range(n):
        c = int(rng.integers(0, len(VALUES) + 2))
        pays.append({"other": 1} if c >= len(VALUES) else {"k": VALUES[c], "other": 2})
    return pays


@pytest.mark.parametrize("n", [0, 1, 2, 17, 100, 300])
def test_ordered_rows_equal_a_brute_force_sort(n):
    rng = np.random.default_rng(n)
    pays = table(n, rng)
    for keep in (None, rng.random(n) < 0.5):
        for desc in (False, True):
            want = brute(pays, "k", desc, keep)
            assert SC.ordered_rows(pays, "k", desc, keep=keep) == want
            assert SC.ordered_rows(pays, "k", desc, keep=None if keep is None else F.pack_rows(keep)) == want
            for limit in (1, 3, 7):
                assert SC.ordered_rows(pays, "k", desc, keep=keep, limit=limit) == want[:limit]
            for start in (0, -0.0, 2.5, 2.7, 3, T0_US, T0_US + 0.5, 1e301, -1e301, 2 ** 53 + 1):
                assert SC.ordered_rows(pays, "k", desc, keep=keep, start_from=start) == brute(pays, "k", desc, keep, start)
            for r, x in want[::5]:
                assert SC.ordered_rows(pays, "k", desc, keep=keep, after=(x, r)) == brute(pays, "k", desc, keep, after=(x, r))
    if n >= 100:
        tied = [r for r, x in brute(pays, "k", False) if x == T0_US]
        assert len(tied) >= 5 and tied == sorted(tied)              # five spellings of one instant: the row decides


def test_what_is_orderable():
    assert SC.order_value(True) is None and SC.order_value(False) is None and SC.order_value(float("nan")) is None
    assert SC.order_value(None) is None and SC.order_value([1]) is None and SC.order_value({"a": 1}) is None
    assert SC.order_value(2 ** 53 + 1) == 2 ** 53 + 1 and SC.order_value(-0.0) == 0 and SC.order_value(2.5) == 2.5
    for v in (T0, T0.replace(tzinfo=None), "2024-05-01T12:00:00.25Z", "2024-05-01T12:00:00.250000z",
              "2024-05-01t14:00:00.25+02:00", "2024-05-01T06:30:00.250-05:30", "2024-05-01 12:00:00.2500001"):
        assert SC.order_value(v) == T0_US, v
    assert SC.order_value("2024-05-01T12:00:00") == T0_US - 250000          # naive: UTC
    assert SC.order_value(datetime.datetime(1969, 12, 31, 23, 59, 59, 999999)) == -1
    for v in ("", "2024-05-01", "12:00:00", "2024-05-01T25:00:00Z", "2024-02-30T00:00:00Z", "yesterday", "2024-05-01T12:00Z"):
        assert SC.order_value(v) is None, v


@pytest.mark.parametrize("column", ["constant", "distinct", "runs"])
@pytest.mark.parametrize("limit", [1, 3, 7])
def test_chained_pages_concatenate_to_the_full_list(column, limit):
    n = 41
    vals = {"constant": [5] * n, "distinct": [(r * 17) % n for r in range(n)], "runs": [r // 6 for r in range(n)]}[column]
    pays = [{"k": v} for v in vals]
    for desc in (False, True):
        full = SC.ordered_rows(pays, "k", desc)
        assert len(full) == n
        got, after, pages = [], None, 0
        while True:
            hits = SC.ordered_rows(pays, "k", desc, after=after, limit=limit + 1)
            got += hits[:limit]
            pages += 1
            if len(hits) <= limit:
                break
            after = (hits[limit - 1][1], hits[limit - 1][0])
        assert got == full and pages == math.ceil(n / limit)


def test_plain_rows():
    keep = np.array([r % 3 == 0 for r in range(100)])
    assert SC.scroll_rows(100, None, 95, 10) == [95, 96, 97, 98, 99]
    assert SC.scroll_rows(100, keep, 4, 3) == [6, 9, 12] and SC.scroll_rows(100, F.pack_rows(keep), 99, 3) == [99]
    assert SC.scroll_rows(100, keep, 100, 3) == [] and SC.scroll_rows(0, None, 0, 3) == []
    for n in (0, 1, 33, 100):
        k = np.random.default_rng(n).random(n) < 0.4
        for start in (0, n // 2, n):
            for limit in (1, 5, 200):
                want, cnt = SH.ref_scroll_rows(n, k, start, limit)
                assert SC.scroll_rows(n, k, start, limit) == want[:cnt].tolist()


def test_the_helpers_and_the_model_agree_on_exact_doubles():
    """the numpy restatement of hx.h (bits) and scrolling.py (Python's comparison) order the same cells the same way"""
    rng = np.random.default_rng(5)
    vals = np.concatenate([rng.integers(-4, 4, 200).astype(np.float64), [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324,
                                                                             2.0 ** 53, -2.0 ** 53, 1.7e15, 1.7e15 + 1]])
    cells = SH.bits_of(vals)
    cells[::13] = SH.MISSING
    cells[5::17] = SH.NULL
    pays = [{} if c == SH.MISSING else {"k": None} if c == SH.NULL else {"k": float(v)} for c, v in zip(cells.tolist(), vals)]
    keep = rng.random(len(pays)) < 0.6
    for desc in (False, True):
        for start, after in ((None, None), (0.0, None), (-0.0, (0.0, 100)), (None, (1.0, 50)), (2.0, (3.0, 7))):
            rows, bits, cnt = SH.ref_payload_order(cells, keep, desc, start, after, 2048)
            assert rows[:cnt].tolist() == [r for r, _ in SC.ordered_rows(pays, "k", desc, keep=keep, start_from=start, after=after)]


# ---- the datetime schema ---------------------------------------------------------------------------------------------------
def dt_index():
    pi = PI.PayloadIndex()
    pi.keys["t"] = PI._Key(PI.schema_of("datetime"))
    pi.keys["n"] = PI._Key(PI.schema_of("integer"))
    return pi


def test_datetime_cells_hold_exact_microseconds():
    pi = dt_index()
    assert pi.keys["t"].kind == PI.PAY_F64 and "datetime" in PI.SCHEMAS
    pays = [{"t": T0}, {"t": "2024-05-01T12:00:00.250000Z"}, {}, {"t": None}, {"t": T0.replace(tzinfo=None)},
            {"t": datetime.datetime(1969, 12, 31, 23, 59, 59, 999999, tzinfo=UTC)}]
    cells = pi.encode("t", pays)
    assert cells.dtype == np.uint64
    assert cells.tolist() == [PI.f64_bits(float(T0_US))] * 2 + [PI.F64_MISSING, PI.F64_NULL, PI.f64_bits(float(T0_US)),
                                                                  PI.f64_bits(-1.0)]
    assert float(T0_US) == T0_US


def test_what_poisons_a_datetime_key(monkeypatch):
    pi = dt_index()
    for bad in (5, 5.0, True, "not a date", [T0], {"a": 1}, datetime.date(2024, 5, 1)):
        assert pi.encode("t", [{"t": T0}, {"t": bad}]) is None, bad
    # the 2^53 boundary: no datetime reaches it, so the parse is stood in for
    monkeypatch.setattr(SC, "datetime_micros", lambda v: v if isinstance(v, int) else None)
    assert pi.encode("t", [{"t": 2 ** 53}, {"t": -(2 ** 53)}]).tolist() == [PI.f64_bits(2.0 ** 53), PI.f64_bits(-(2.0 ** 53))]
    assert pi.encode("t", [{"t": 2 ** 53 + 1}]) is None and pi.encode("t", [{"t": -(2 ** 53) - 1}]) is None


def test_the_compiler_declines_every_condition_on_a_datetime_key():
    pi = dt_index()
    pi.keys["t"].col, pi.keys["n"].col = 0, 1
    for cond in ({"key": "t", "range": {"gte": 0}}, {"key": "t", "match": {"value": "2024-05-01T12:00:00Z"}},
                 {"is_empty": {"key": "t"}}, {"is_null": {"key": "t"}}, {"key": "t", "match": {"any": [1]}}):
        assert pi.compile({"must": [cond]}) is None
        assert pi.compile({"must": [{"key": "n", "range": {"gte": 0}}], "must_not": [cond]}) is None
    assert pi.declined == {"datetime key": 10}
    assert pi.compile({"must": [{"key": "n", "range": {"gte": 0}}]}) is not None


# ---- the handler over a stub index -------------------------------------------------------------------------------------------
class StubIndex:
    """no scroll entries: every scroll goes the Python way"""

    def count(self):
        return 16


class DeviceStub(StubIndex):
    """the two host entries, answered by tests/scroll_helpers.py over cells the test hands in"""

    def __init__(self, cells):
        self.cells, self.calls = cells, []

    def _keep(self, mask):
        return None if mask is None else np.unpackbits(np.asarray(mask, np.uint32).view(np.uint8), bitorder="little")[:16].astype(bool)

    def scroll_rows_host(self, limit, start_row=0, mask=None):
        self.calls.append(("rows", limit, start_row))
        rows, cnt = SH.ref_scroll_rows(16, self._keep(mask), start_row, limit)
        return rows[:cnt]

    def payload_order_host(self, col, limit, desc=False, start_from=None, after=None, mask=None):
        self.calls.append(("order", col, limit, desc, start_from, after))
        rows, bits, cnt = SH.ref_payload_order(self.cells, self._keep(mask), desc, start_from, after, limit)
        return rows[:cnt], bits[:cnt]


def stub_handler(index=None):
    h = QdrantHandler()
    col = _Collection.__new__(_Collection)
    col.dim, col.msizes, col.sparse_enabled = 4, (), True
    col.index = index if index is not None else StubIndex()
    col.ids = [f"p{r}" for r in range(16)]
    col.payloads = [{"page": r // 3, "even": r % 2 == 0, "w": None if r == 4 else (16 - r) / 2} for r in range(16)]
    col._masks, col.pindex, col.tokens = {}, None, None
    h._collections["u"] = col
    return h, col


EVEN = {"must": [{"key": "even", "match": {"value": True}}]}


def scan(h, **kw):
    out, offset = [], None
    while True:
        recs, nxt = asyncio.run(h.scroll("u", offset=offset, **kw))
        out.append(([r.id for r in recs], [r.order_value for r in recs]))
        if nxt is None:
            return out
        offset = nxt


def test_handler_pages_on_the_python_path():
    h, col = stub_handler()
    recs, nxt = asyncio.run(h.scroll("u", limit=5))
    assert [r.id for r in recs] == ["p0", "p1", "p2", "p3", "p4"] and nxt == "p5"
    assert all(isinstance(r, Record) and r.order_value is None for r in recs) and recs[2].payload is col.payloads[2]
    assert recs[0].dict() == {"id": "p0", "payload": col.payloads[0], "vector": None, "shard_key": None, "order_value": None}
    assert [ids for ids, _ in scan(h, limit=3, filters=EVEN)] == [["p0", "p2", "p4"], ["p6", "p8", "p10"], ["p12", "p14"]]
    assert asyncio.run(h.scroll("u", limit=16)) [1] is None and asyncio.run(h.scroll("u", limit=15))[1] == "p15"
    pages = scan(h, limit=4, order_by={"key": "page", "direction": "desc"}, filters=EVEN)
    assert [i for ids, _ in pages for i in ids] == ["p12", "p14", "p10", "p6", "p8", "p4", "p0", "p2"]
    assert [v for _, vs in pages for v in vs] == [4, 4, 3, 2, 2, 1, 0, 0]
    recs, nxt = asyncio.run(h.scroll("u", limit=2, order_by="w", with_payload=False))
    assert [(r.id, r.order_value, r.payload) for r in recs] == [("p15", 0.5, None), ("p14", 1.0, None)]
    assert nxt == {"value": 1.0, "id": "p14"}
    assert sum(len(ids) for ids, _ in scan(h, limit=4, order_by={"key": "w", "start_from": 2})) == 12      # p4 has no value
    assert asyncio.run(h.scroll("u", order_by={"key": "no such key"})) == ([], None)


def test_handler_takes_the_device_path_for_a_live_number_or_datetime_key():
    cells = SH.bits_of([(16 - r) / 2 for r in range(16)])
    cells[4] = SH.NULL
    h, col = stub_handler(DeviceStub(cells))
    col.pindex = PI.PayloadIndex()
    col.pindex.keys["w"] = PI._Key("number")
    col.pindex.keys["w"].col = 7
    want = scan(stub_handler()[0], limit=4, order_by={"key": "w", "direction": "desc", "start_from": 6})
    assert scan(h, limit=4, order_by={"key": "w", "direction": "desc", "start_from": 6}) == want
    assert col.index.calls[0] == ("order", 7, 5, True, 6.0, None) and col.index.calls[1][5] == (4.0, 8)      # (p4 holds None)
    assert col.pindex.scroll_device_calls == len(want) and col.pindex.scroll_python_calls == 0
    assert scan(h, limit=5) == scan(stub_handler()[0], limit=5) and col.index.calls[-1] == ("rows", 6, 15)
    # a bound no double holds, an unindexed key and a poisoned key go the Python way
    before = col.pindex.scroll_device_calls
    asyncio.run(h.scroll("u", order_by={"key": "w", "start_from": 2 ** 53 + 1}))
    asyncio.run(h.scroll("u", order_by={"key": "page"}))
    col.pindex.keys["w"].col = None
    asyncio.run(h.scroll("u", order_by={"key": "w"}))
    assert col.pindex.scroll_device_calls == before and col.pindex.scroll_python_calls == 3


def test_handler_refusals():
    h, col = stub_handler()

    def scroll(**kw):
        return asyncio.run(h.scroll("u", **kw))
    for limit in (0, -1, 2048, 2.0, True, None):
        with pytest.raises(ValueError, match="limit"):
            scroll(limit=limit)
    assert len(scroll(limit=2047)[0]) == 16
    for order_by in ({}, {"key": ""}, {"key": 5}, {"key": "w", "direction": "up"}, {"key": "w", "extra": 1}, 5,
                     {"key": "w", "start_from": float("nan")}, {"key": "w", "start_from": True}, {"key": "w", "start_from": "soon"}):
        with pytest.raises(ValueError, match="order_by"):
            scroll(order_by=order_by)
    with pytest.raises(ValueError, match="no point with id"):
        scroll(offset="nobody")
    with pytest.raises(ValueError, match="no point with id"):
        scroll(order_by="w", offset={"value": 1.0, "id": "nobody"})
    for offset in ("p3", {"value": 1.0}, {"value": float("nan"), "id": "p3"}, {"value": None, "id": "p3"}):
        with pytest.raises(ValueError, match="offset"):
            scroll(order_by="w", offset=offset)
    with pytest.raises(ValueError, match="clause"):
        scroll(filters={"mustnt": []})
    assert asyncio.run(h.scroll("nobody")) == ([], None) and asyncio.run(h.retrieve("nobody", ["p1"])) == []
    got = asyncio.run(h.retrieve("u", ["p9", "nobody", "p1", "p9", 5]))
    assert got == [Record(id=f"p{r}", payload=col.payloads[r]) for r in (9, 1, 9)]
    assert asyncio.run(h.retrieve("u", ("p2",), with_payload=False)) == [Record(id="p2")]
    with pytest.raises(ValueError, match="point_ids"):
        asyncio.run(h.retrieve("u", "p1"))


def test_a_sharded_collection_is_refused():
    from rag_application_amd.sharded import ShardedHandler
    h = ShardedHandler.__new__(ShardedHandler)                      # (no process group: the refusal comes first)
    h._collections, h._lock = {}, None
    assert ShardedHandler._scroll is False and QdrantHandler._scroll is True
    with pytest.raises(ValueError, match="sharded"):
        asyncio.run(h.scroll("u"))
    with pytest.raises(ValueError, match="sharded"):
        asyncio.run(h.retrieve("u", ["p1"]))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
ENTRIES = ("hx_scroll_rows", "hx_payload_order", "hx_scroll_rows_host", "hx_payload_order_host")


def test_the_entries_are_declared_bound_and_exported():
    import ctypes as C
    from rag_application_amd import build, engine
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hx.h")).read()
    cdll = C.CDLL(build.build())
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.EXPORTS and name in _lib._SIGS and getattr(cdll, name) is not None
        assert hasattr(engine.HxIndex, name[3:])
    for name, value in (("HX_ORDER_ASC", 0), ("HX_ORDER_DESC", 1), ("HX_ORDER_HAS_START", 1), ("HX_ORDER_HAS_AFTER", 2),
                        ("HX_SCROLL_MAX_LIMIT", 2048), ("HX_ABI_VERSION", 3)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1)) == value
    assert len(_lib._SIGS["hx_payload_order"]) == 14 and len(_lib._SIGS["hx_payload_order_host"]) == 13
    assert SC.MAX_LIMIT == 2048
    # a NULL index is refused with a message before anything touches a device
    lib = _lib.lib()
    assert lib.hx_scroll_rows(None, None, 0, 0, 5, None, None, None) != 0 and lib.hx_last_error()
    assert lib.hx_payload_order_host(None, 0, None, 0, 0, 0, 0.0, 0.0, 0, 5, None, None, None) != 0
