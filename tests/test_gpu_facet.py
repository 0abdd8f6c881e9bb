"""GPU: payload facets (hx_payload_facet, hx_facet_top, hx_payload_facet_host, QdrantHandler.facet).

Every count and every ranking comes out of the engine through the C ABI and is compared, exactly, with faceting.py over
the same cells and the same mask -- never with another device result.  A cell of code c is the payload value int(c) (the
model counts ints), a missing cell no key, a null cell None; a stray code is a value at or above n_codes, which the
expectation sets apart.  The index is 64-dimensional and filled by synth_fill; the columns go in through the engine's
wrappers."""
import asyncio
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from rag_application_amd import faceting as FC
from rag_application_amd import filters as F
from rag_application_amd import payload_index as PI

pytestmark = pytest.mark.gpu

MISSING, NULL = PI.U32_MISSING, PI.U32_NULL
SIZES = [1, 63, 64, 65, 255, 256, 257, 4096]


def _lds_codes():
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hx.h")
    return int(re.search(r"#define\s+HX_FACET_LDS_CODES\s+(\d+)", open(hdr).read()).group(1))


LDS = _lds_codes()


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from rag_application_amd import engine
    return engine


def index_of(eng, n):
    ix = eng.HxIndex(64, (64,))
    ix.synth_fill(n, O.SEED_CORPUS)
    return ix


def dev_i32(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).cuda()


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def masks_of(n, rng):
    """None, all zero, all one, a random half -- as bool arrays"""
    return [None, np.zeros(n, bool), np.ones(n, bool), rng.random(n) < 0.5]


# ---- the model's side ------------------------------------------------------------------------------------------------------
def scalar_pays(cells):
    return [{} if c == MISSING else {"k": None} if c == NULL else {"k": int(c)} for c in cells.tolist()]


def list_pays(rows):
    """rows[r] = "missing", None or a list of codes"""
    return [{} if v == "missing" else {"k": None if v is None else [int(x) for x in v]} for v in rows]


def expect(pays, keep, n_codes):
    """(counts [n_codes] uint32 from faceting.facet_counts, the values at or above n_codes it counted)"""
    counts = np.zeros(n_codes, np.uint32)
    beyond = 0
    for (tag, v), c in FC.facet_counts(pays, "k", keep).items():
        assert tag == "int"
        if v < n_codes:
            counts[v] = c
        else:
            beyond += c
    return counts, beyond


def check_counts(ix, col, pays, n_codes, keep, stray_want=None):
    import torch
    mask = None if keep is None else dev_i32(F.pack_rows(keep))
    counts, stray = ix.payload_facet(col, n_codes, mask=mask)
    torch.cuda.synchronize()
    want, beyond = expect(pays, keep, n_codes)
    np.testing.assert_array_equal(host_u32(counts), want)
    assert int(stray.item()) == (beyond if stray_want is None else stray_want)
    return want


# ---- cell patterns of a scalar column ---------------------------------------------------------------------------------------
def patterns(n, rng):
    """name -> (cells, n_codes)"""
    r = np.arange(n, dtype=np.int64)
    out = {
        "every_row_one_code": (np.full(n, 3, np.uint32), 64),
        "one_code_in_all": (np.zeros(n, np.uint32), 1),
        "runs_of_50": ((r // 50 % 64).astype(np.uint32), 64),
        # runs of 300 from row 37 on: they cross the 64-row groups, the 256-row passes of a wave and, under a two-workgroup
        # grid (8192 rows per pass), the grid-stride edge in the middle of a run
        "runs_that_straddle": (((r + 263) // 300 % 7).astype(np.uint32), 7),
        "uniform_random": (rng.integers(0, 64, n).astype(np.uint32), 64),
        "all_distinct": (rng.permutation(n).astype(np.uint32), n),
        "all_missing_or_null": (np.where(r % 3 == 0, NULL, MISSING).astype(np.uint32), 64),
    }
    holes = rng.integers(0, 2, n).astype(np.uint32)
    h = rng.random(n) < 0.1
    holes[h] = np.where(rng.random(int(h.sum())) < 0.5, NULL, MISSING)
    out["ten_percent_holes"] = (holes, 2)
    return out


@pytest.mark.parametrize("n,grid", [(n, None) for n in SIZES] + [(20_000, 2)])
def test_scalar_counts_equal_the_model_at_every_row_count(eng, monkeypatch, n, grid):
    if grid:
        monkeypatch.setenv("HX_DEBUG_PAY_GRID", str(grid))     # two workgroups: the stride loop is crossed
    rng = np.random.default_rng(n)
    ix = index_of(eng, n)
    try:
        seen = 0
        for name, (cells, n_codes) in patterns(n, rng).items():
            col = ix.payload_create(PI.PAY_U32)
            ix.payload_append(col, cells)
            pays = scalar_pays(cells)
            for keep in masks_of(n, rng):
                seen += int(check_counts(ix, col, pays, n_codes, keep).sum())
            ix.payload_drop(col)
        assert seen > 0
    finally:
        ix.close()


@pytest.mark.parametrize("n_codes", [1, 2, 64, LDS - 1, LDS, LDS + 1, 1 << 20])
def test_scalar_counts_at_every_tier_of_n_codes(eng, n_codes):
    n = 4097
    rng = np.random.default_rng(n_codes)
    ix = index_of(eng, n)
    try:
        uniform = rng.integers(0, n_codes, n).astype(np.uint32)
        uniform[:2] = [n_codes - 1, 0]                                  # the two ends of the histogram are hit
        runs = (np.arange(n) // 50 * 2654435761 % n_codes).astype(np.uint32)
        holes = uniform.copy()
        holes[rng.random(n) < 0.1] = MISSING
        for cells in (uniform, runs, holes):
            col = ix.payload_create(PI.PAY_U32)
            ix.payload_append(col, cells)
            pays = scalar_pays(cells)
            for keep in (None, rng.random(n) < 0.5):
                assert check_counts(ix, col, pays, n_codes, keep).sum() > 0
            ix.payload_drop(col)
    finally:
        ix.close()


def test_stray_codes_count_only_where_the_row_is_kept(eng):
    n, n_codes = 1000, 100
    rng = np.random.default_rng(3)
    ix = index_of(eng, n)
    try:
        cells = rng.integers(0, 150, n).astype(np.uint32)               # a third of the rows hold a code past the dictionary
        cells[[5, 500, 999]] = 0xFFFFFFFD                               # the largest code a column takes
        cells[[6, 501]] = [MISSING, NULL]
        keep = rng.random(n) < 0.5
        keep[[5, 999]], keep[500] = True, False
        col = ix.payload_create(PI.PAY_U32)
        ix.payload_append(col, cells)
        pays = scalar_pays(cells)
        for k in (None, keep, ~keep, np.zeros(n, bool)):
            live = np.ones(n, bool) if k is None else k
            stray = int((live & (cells >= n_codes) & (cells < NULL)).sum())
            check_counts(ix, col, pays, n_codes, k, stray_want=stray)   # (the model's count of the same values agrees)
            assert (stray > 0) == (k is None or bool(k.any()))
    finally:
        ix.close()
    # a list column: every kept stray ELEMENT counts, a repeated one twice
    rows = [[1, 120, 120, 2], [130], [], None, "missing", [3, 3, 0xFFFFFFFD], [99, 100]] * 40
    heads, values = list_cells(rows)
    ix = index_of(eng, len(rows))
    try:
        lcol = ix.payload_create(PI.PAY_LIST_U32)
        ix.payload_append_lists(lcol, heads, values)
        pays = list_pays(rows)
        for k, stray in ((None, 200), (np.arange(280) % 7 < 2, 120), (np.arange(280) % 7 >= 2, 80)):
            assert check_list(ix, lcol, rows, pays, n_codes, k) == stray
    finally:
        ix.close()


# ---- list columns ------------------------------------------------------------------------------------------------------------
def list_cells(rows):
    heads = np.array([MISSING if v == "missing" else NULL if v is None else len(v) for v in rows], np.uint32)
    values = np.array([x for v in rows if isinstance(v, list) for x in v], np.uint32)
    return heads, values


def check_list(ix, col, rows, pays, n_codes, keep):
    """check_counts for a list column: the stray ELEMENTS of the kept rows are counted here, one by one (the model
    counts a repeated value once); returns their number"""
    live = np.ones(len(rows), bool) if keep is None else keep
    stray = sum(sum(1 for x in v if n_codes <= x < NULL) for v, on in zip(rows, live) if on and isinstance(v, list))
    check_counts(ix, col, pays, n_codes, keep, stray_want=stray)
    return stray


def _list_shapes():
    rng = np.random.default_rng(17)
    out = {}
    lens = np.tile([0, 1, 2, 63, 64, 65, 300, 1], 40)
    out["lengths_0_1_2_63_64_65_300"] = [rng.integers(0, 40, k).tolist() for k in lens]      # 40 values: repeats abound
    rows = [[] for _ in range(300)]
    rows[0] = list(range(100, 160))                                      # 60 elements: row 1 starts at element 60
    rows[1] = [1, 2, 3, 7, 4, 7, 5]                                      # the pair of 7s sits on elements 63 and 65
    rows[2] = [9, 9, 9, 8, 8]                                            # adjacent repeats
    rows[3] = [7] + list(range(200, 349)) + [7] + list(range(400, 449)) + [7]     # repeats 150 and 50 positions apart
    rows[130] = [5, 6] * 40
    out["repeats_adjacent_far_apart_and_across_a_chunk"] = rows
    rows = [rng.integers(0, 6, int(k)).tolist() for k in rng.integers(0, 4, 600)]
    rows[255] = rng.integers(0, 30, 70).tolist()                         # the last row of the first wave's pass
    rows[256] = rng.integers(0, 30, 70).tolist()                         # ... and the first of the second wave's
    out["lists_on_either_side_of_a_wave_edge"] = rows
    rows = [[] for _ in range(400)]
    rows[200] = rng.integers(10, 13, 5000).tolist()
    rows[399] = [12, 3]
    out["one_row_of_5000_elements_with_3_values"] = rows
    out["empty_lists_only"] = [[] for _ in range(300)]
    rows = [rng.integers(0, 9, int(k)).tolist() for k in rng.integers(0, 5, 700)]
    for r in range(0, 700, 5):
        rows[r] = None if r % 2 else "missing"
    rows[256:512] = [None] * 256                                         # a wave whose run is empty
    out["null_and_missing_heads"] = rows
    return out


LIST_SHAPES = _list_shapes()


@pytest.mark.parametrize("shape", sorted(LIST_SHAPES))
def test_list_counts_equal_the_model(eng, shape):
    rows = LIST_SHAPES[shape]
    n = len(rows)
    rng = np.random.default_rng(n)
    heads, values = list_cells(rows)
    top_code = int(values.max()) + 1 if values.size else 1
    ix = index_of(eng, n)
    try:
        col = ix.payload_create(PI.PAY_LIST_U32)
        ix.payload_append_lists(col, heads, values)
        pays = list_pays(rows)
        for n_codes in (top_code, LDS + 1):                              # the LDS tier and the global tier
            for keep in masks_of(n, rng):
                assert check_list(ix, col, rows, pays, n_codes, keep) == 0
        if top_code > 4:                                                 # a dictionary that ends inside the values
            assert check_list(ix, col, rows, pays, top_code - 3, None) > 0
    finally:
        ix.close()


@pytest.mark.parametrize("n,grid", [(1, None), (65, None), (257, None), (4096, None), (20_000, 2)])
def test_list_counts_at_several_row_counts(eng, monkeypatch, n, grid):
    if grid:
        monkeypatch.setenv("HX_DEBUG_PAY_GRID", str(grid))
    rng = np.random.default_rng(1000 + n)
    lens = np.minimum(rng.geometric(0.3, n) - 1, 64)                     # mean 2.3, a few long rows
    rows = [rng.integers(0, 50, int(k)).tolist() for k in lens]
    for r in range(3, n, 11):
        rows[r] = None if r % 2 else "missing"
    heads, values = list_cells(rows)
    ix = index_of(eng, n)
    try:
        col = ix.payload_create(PI.PAY_LIST_U32)
        ix.payload_append_lists(col, heads, values)
        pays = list_pays(rows)
        for n_codes in (50, LDS + 1):
            for keep in (None, rng.random(n) < 0.5):
                check_list(ix, col, rows, pays, n_codes, keep)
        if n > 1:
            assert check_list(ix, col, rows, pays, 30, rng.random(n) < 0.5) > 0
    finally:
        ix.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_a_refused_call_leaves_its_outputs_untouched(eng):
    import torch
    from rag_application_amd import _lib
    n = 100
    ix = index_of(eng, n)
    try:
        col = ix.payload_create(PI.PAY_U32)
        ix.payload_append(col, np.arange(n, dtype=np.uint32) % 5)
        f64 = ix.payload_create(PI.PAY_F64)
        ix.payload_append(f64, np.zeros(n, np.float64))
        short = ix.payload_create(PI.PAY_U32)
        ix.payload_append(short, np.zeros(n - 1, np.uint32))
        counts = torch.full((8,), -1, dtype=torch.int32, device="cuda")
        stray = torch.full((1,), 77, dtype=torch.int64, device="cuda")
        mask = dev_i32(np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32))
        lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
        pc, ps, pm = counts.data_ptr(), stray.data_ptr(), mask.data_ptr()
        refused = {
            "n_codes 0": lambda: lib.hx_payload_facet(ix._h, col, None, 0, 0, pc, ps, st),
            "n_codes above 0xFFFFFFFE": lambda: lib.hx_payload_facet(ix._h, col, None, 0, 0xFFFFFFFF, pc, ps, st),
            "unknown column": lambda: lib.hx_payload_facet(ix._h, 999, None, 0, 8, pc, ps, st),
            "kind": lambda: lib.hx_payload_facet(ix._h, f64, None, 0, 8, pc, ps, st),
            "not filled": lambda: lib.hx_payload_facet(ix._h, short, None, 0, 8, pc, ps, st),
            "mask_rows": lambda: lib.hx_payload_facet(ix._h, col, pm, n + 1, 8, pc, ps, st),
            "mask_rows short": lambda: lib.hx_payload_facet(ix._h, col, pm, n - 1, 8, pc, ps, st),
            "NULL counts": lambda: lib.hx_payload_facet(ix._h, col, None, 0, 8, None, ps, st),
            "NULL stray": lambda: lib.hx_payload_facet(ix._h, col, None, 0, 8, pc, None, st),
        }
        for what, f in refused.items():
            assert f() != 0, what
            msg = lib.hx_last_error().decode()
            assert msg, what
            if what == "kind":
                assert "kind" in msg
        out = torch.full((16,), -1, dtype=torch.int64, device="cuda")
        cnt = torch.full((1,), -5, dtype=torch.int32, device="cuda")
        good = dev_i32(np.arange(8))
        for what, f in {
            "limit 0": lambda: lib.hx_facet_top(ix._h, good.data_ptr(), 8, None, 0, out.data_ptr(), cnt.data_ptr(), st),
            "limit 2049": lambda: lib.hx_facet_top(ix._h, good.data_ptr(), 8, None, 2049, out.data_ptr(), cnt.data_ptr(), st),
            "n_codes 0": lambda: lib.hx_facet_top(ix._h, good.data_ptr(), 0, None, 4, out.data_ptr(), cnt.data_ptr(), st),
            "NULL counts": lambda: lib.hx_facet_top(ix._h, None, 8, None, 4, out.data_ptr(), cnt.data_ptr(), st),
            "NULL out": lambda: lib.hx_facet_top(ix._h, good.data_ptr(), 8, None, 4, None, cnt.data_ptr(), st),
        }.items():
            assert f() != 0, what
            assert lib.hx_last_error(), what
        torch.cuda.synchronize()
        assert (counts == -1).all() and stray.item() == 77 and (out == -1).all() and cnt.item() == -5
        with pytest.raises(Exception):
            ix.payload_facet_host(f64, 8, 4)
        with pytest.raises(Exception):
            ix.payload_facet_host(col, 8, 4, mask=np.zeros(n + 1, bool))
        # and the same call goes through once its arguments are right: the sentinels are overwritten everywhere
        ix.payload_facet(col, 8, mask=mask, counts=counts, stray=stray)
        torch.cuda.synchronize()
        assert host_u32(counts).tolist() == [20] * 5 + [0] * 3 and stray.item() == 0
    finally:
        ix.close()


# ---- the top stage -----------------------------------------------------------------------------------------------------------
def check_top(ix, counts, rank, limit):
    import torch
    n_codes = counts.shape[0]
    out = torch.full((limit,), -1, dtype=torch.int64, device="cuda")            # every slot must be written
    keys, hits = ix.facet_top(dev_i32(counts), limit, rank=None if rank is None else dev_i32(rank), out=out)
    torch.cuda.synchronize()
    keys = keys.cpu().numpy().view(np.uint64)
    r = np.arange(n_codes) if rank is None else rank
    nz = np.flatnonzero(counts)
    want = FC.facet_top({("int", int(r[c])): int(counts[c]) for c in nz}, limit)   # ranks stand for the values
    k = int(hits.item())
    assert k == len(want) == min(limit, nz.size)
    got = [(0xFFFFFFFF - int(x & np.uint64(0xFFFFFFFF)), int(x >> np.uint64(32))) for x in keys[:k]]
    assert got == want
    assert not keys[k:].any()


@pytest.fixture(scope="module")
def tiny(eng):
    ix = index_of(eng, 1)
    yield ix
    ix.close()


@pytest.mark.parametrize("n_codes", [1, 8192, 8193, 100_000])
@pytest.mark.parametrize("limit", [1, 10, 2048])
def test_top_with_all_counts_equal_is_cut_by_rank_alone(tiny, n_codes, limit):
    counts = np.full(n_codes, 5, np.uint32)
    check_top(tiny, counts, None, limit)
    check_top(tiny, counts, np.random.default_rng(n_codes).permutation(n_codes).astype(np.uint32), limit)


@pytest.mark.parametrize("limit", [1, 10, 512, 513, 2048])
def test_top_of_mixed_counts_and_zero_counters(tiny, limit):
    rng = np.random.default_rng(limit)
    for n_codes, live in ((5, 3), (300, 7), (2049, 2049), (LDS + 1, 600), (1 << 20, 3000), (1 << 20, 1)):
        counts = np.zeros(n_codes, np.uint32)
        at = rng.choice(n_codes, size=live, replace=False)
        counts[at] = rng.integers(1, 40, live)                           # many ties, zero counters in between
        counts[at[0]] = 0xFFFFFFFF                                       # the largest count a counter holds
        rank = rng.permutation(n_codes).astype(np.uint32)
        check_top(tiny, counts, rank, limit)
        check_top(tiny, counts, None, limit)
    check_top(tiny, np.zeros(70_000, np.uint32), None, limit)            # nothing to return


def test_the_host_entry_counts_and_ranks_in_one_call(eng):
    n, n_codes = 5000, 300
    rng = np.random.default_rng(9)
    ix = index_of(eng, n)
    try:
        cells = (np.arange(n) // 17 % n_codes).astype(np.uint32)
        cells[rng.random(n) < 0.05] = NULL
        col = ix.payload_create(PI.PAY_U32)
        ix.payload_append(col, cells)
        pays = scalar_pays(cells)
        rank = rng.permutation(n_codes).astype(np.uint32)
        code_of = np.argsort(rank)
        for keep in (None, rng.random(n) < 0.5, np.zeros(n, bool)):
            counts, _ = expect(pays, keep, n_codes)
            for limit in (1, 10, 2048):
                first, cnt, stray = ix.payload_facet_host(col, n_codes, limit, rank=rank, mask=keep)
                want = FC.facet_top({("int", int(rank[c])): int(counts[c]) for c in np.flatnonzero(counts)}, limit)
                assert stray == 0 and list(zip(first.tolist(), cnt.tolist())) == want
                assert [int(counts[code_of[r]]) for r in first.tolist()] == cnt.tolist()
                first, cnt, stray = ix.payload_facet_host(col, n_codes, limit, mask=keep)      # no ranks: codes come back
                assert stray == 0 and list(zip(first.tolist(), cnt.tolist())) == FC.facet_top(FC.facet_counts(pays, "k", keep), limit)
        first, cnt, stray = ix.payload_facet_host(col, 100, 10)                               # a dictionary out of step
        assert stray == int(((cells >= 100) & (cells < NULL)).sum()) > 0
    finally:
        ix.close()


# ---- the handler -------------------------------------------------------------------------------------------------------------
LANGS = ["en", "de", "fr", "es", "it", "nl"]


def _chunks(n, seed, doc0=0):
    rng = np.random.default_rng(seed)
    X = O.synth_dense(O.SEED_CORPUS, seed * 10_000, n, 64)
    out = []
    for r in range(n):
        doc = doc0 + r // 9
        meta = {"document_id": f"doc{doc:03d}", "user_id": "u", "file_name": f"f{doc}.txt", "mime_type": ("text/plain", "application/pdf")[doc % 2],
                "file_size": 1, "description": "", "file_path": "/x", "context_version": 1, "chunk_number": r % 9, "doc_summary": "s",
                "page_number": int(r % 13) if r % 4 else None,
                "languages": None if r % 17 == 0 else [LANGS[int(i)] for i in rng.integers(0, 6, int(rng.integers(0, 4)))]}
        out.append({"dense_embedding": X[r].tolist(), "sparse_embedding": {"indices": [1 + r % 5, 40], "values": [1.0, 0.5]},
                    "content": f"chunk {r}", "chunk_metadata": meta})
    return out


def test_handler_facet_equals_the_model_on_both_paths(eng):
    from rag_application_amd.handler import FacetHit, QdrantHandler
    h = QdrantHandler()
    asyncio.run(h.create_collection("u", dense_vector_size=64, matryoshka_sizes=[64], quantized_size=64))
    asyncio.run(h.store_document_vectors(_chunks(400, 1), "u"))
    for key, schema in (("document_id", "keyword"), ("languages", "keyword_list"), ("page_number", "integer")):
        assert asyncio.run(h.create_payload_index("u", key, schema)) is True
    col = h._collections["u"]
    pi = col.pindex
    flts = [None, {"must": [{"key": "page_number", "range": {"gte": 3}}]},
            {"must_not": [{"key": "languages", "match": {"any": ["en", "de"]}}]},
            {"must": [{"key": "document_id", "match": {"value": "no such document"}}]}]

    def want(key, flt, limit):
        keep = F.row_mask(col.ids, col.payloads, flt) if flt else None
        return [FacetHit(v, c) for v, c in FC.facet_top(FC.facet_counts(col.payloads, key, keep), limit)]

    def check_device(keys=("document_id", "languages")):
        calls = 0
        for key in keys:
            for flt in flts:
                for limit in (3, 10, 1000):
                    got = asyncio.run(h.facet("u", key, filters=flt, limit=limit, exact=(limit == 3)))
                    assert got == want(key, flt, limit), (key, flt, limit)
                    calls += 1
        return calls

    dev = check_device()
    assert pi.facet_device_calls == dev and pi.facet_python_calls == 0
    assert len(want("document_id", None, 1000)) == 45 and want("languages", None, 3)[0].count > 50
    # an unindexed key, ints included, and a number key take the Python path
    for key in ("mime_type", "chunk_number", "page_number", "no_such_key"):
        for flt in flts[:2]:
            assert asyncio.run(h.facet("u", key, filters=flt, limit=5)) == want(key, flt, 5), key
    assert pi.facet_device_calls == dev and pi.facet_python_calls == 8
    assert asyncio.run(h.facet("u", "document_id", limit=5000)) == want("document_id", None, 5000)    # above the device's limit
    assert pi.facet_python_calls == 9
    # after a delete
    assert asyncio.run(h.delete_points("u", filters={"must": [{"key": "document_id", "match": {"any": ["doc003", "doc010"]}}]})) == 18
    dev += check_device()
    assert len(want("document_id", None, 1000)) == 43
    # after an upsert of existing ids with changed values
    moved = _chunks(5, 2)
    for c in moved:
        c["chunk_metadata"]["document_id"] = "doc020"
        c["chunk_metadata"]["languages"] = ["nl", "nl", "en"]
    assert asyncio.run(h.upsert_points("u", moved, [col.ids[r] for r in (0, 1, 2, 200, 381)])) == 5
    dev += check_device()
    # after new keywords enlarge the dictionaries: "aaa" sorts in front of every other value, its code is the largest
    fresh = _chunks(14, 3)                                               # as many chunks as the largest document: a tie
    for c in fresh:
        c["chunk_metadata"]["document_id"] = "aaa"
        c["chunk_metadata"]["languages"] = ["aa", "zz"]
    asyncio.run(h.store_document_vectors(fresh, "u"))
    dev += check_device()
    assert want("document_id", None, 2) == [FacetHit("aaa", 14), FacetHit("doc020", 14)]
    assert pi.facet_device_calls == dev and pi.facet_python_calls == 9
    # a read call: an unknown collection or a bad argument gives []
    assert asyncio.run(h.facet("nobody", "document_id")) == []
    assert asyncio.run(h.facet("u", "document_id", limit=0)) == []
    assert asyncio.run(h.facet("u", "document_id", filters={"bogus": []})) == []
    asyncio.run(h.delete_collection("u"))
