"""Host: the late-interaction rerank's host side (rag_application_amd/late_interaction.py, the handler's arguments;
DESIGN.md section 23) against tests/maxsim_helpers.py, the independent model written from include/hx.h.  No GPU needed."""
from __future__ import annotations

import asyncio

import numpy as np
import pytest

from rag_application_amd import late_interaction as LI
from rag_application_amd.handler import QdrantHandler, RerankedPoint, ScoredPoint, _Collection
from tests import maxsim_helpers as MH

F32 = np.float32
P = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, dense_limit=40,
         quantized_limit=40, sparse_limit=50, final_limit=30, hnsw_ef=128)


def random_tokens(rng, t, dim, spread=1.0):
    x8 = rng.integers(-127, 128, (t, dim)).astype(np.int8)
    sc = (rng.random(t) * spread).astype(F32)
    return x8, sc


@pytest.mark.parametrize("dim", [64, 128, 192, 1024])
def test_maxsim_scores_equals_the_helper_bit_for_bit(dim):
    rng = np.random.default_rng(dim)
    for tq in (1, 2, 15, 16, 17, 32, 33, 63, 64):
        q8, sq = random_tokens(rng, tq, dim, 0.01)
        rows = [random_tokens(rng, td, dim, 0.02) for td in (1, 15, 16, 17, 33, 65)]
        rows.append((np.zeros((3, dim), np.int8), np.zeros(3, F32)))               # scale-0 tokens: +0
        rows.append((-np.abs(q8[:1]).repeat(17, 0), np.full(17, 0.5, F32)))         # every product is <= 0
        got = LI.maxsim_scores(q8, sq, rows)
        want = np.asarray([MH.maxsim(q8, sq, d8, sd) for d8, sd in rows], F32)
        assert got.dtype == F32
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"dim={dim} tq={tq}")


def test_the_tree_is_not_a_running_sum():
    """slots whose balanced pairwise sum differs from the left-to-right sum: the model must give the tree's"""
    slots = [F32(0.0)] * 64
    slots[0], slots[1], slots[2], slots[3] = F32(2.0 ** 24), F32(1.0), F32(1.0), F32(1.0)
    assert MH.tree_sum(slots) == F32(2.0 ** 24 + 2.0)                # (2^24 + 1 -> 2^24) + (1 + 1)
    run = F32(0.0)
    for v in slots:
        run = F32(run + v)
    assert run == F32(2.0 ** 24)                                      # the running sum loses all three
    q8 = np.zeros((4, 64), np.int8)
    q8[:, 0] = 1
    d8 = np.zeros((1, 64), np.int8)
    d8[0, 0] = 1
    sq = np.asarray([2.0 ** 24, 1.0, 1.0, 1.0], F32)
    got = LI.maxsim_scores(q8, sq, [(d8, np.ones(1, F32))])
    assert got[0] == F32(2.0 ** 24 + 2.0) == MH.maxsim(q8, sq, d8, np.ones(1, F32))


def test_quantiser_cases():
    x = np.zeros((3, 64), F32)
    x[1, 5] = -3.0                                                    # a single amax element
    x[2, :7] = [127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5]              # amax = 127: the multiplier is 1, exact ties at .5
    x8, sc = LI.quantize_tokens(x)
    assert x8.dtype == np.int8 and sc.dtype == F32
    assert not x8[0].any() and sc[0] == 0 and np.signbit(sc[0]) == False   # noqa: E712  an all-zero token
    assert x8[1, 5] == -127 and np.count_nonzero(x8[1]) == 1 and sc[1] == F32(F32(3.0) / F32(127.0))
    assert x8[2, :7].tolist() == [127, 0, 2, 2, 0, -2, -2] and sc[2] == F32(1.0)   # rint is half-to-even
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[0, 3] = bad
        with pytest.raises(ValueError, match="finite"):
            LI.quantize_tokens(y)
    rng = np.random.default_rng(5)
    z = (rng.standard_normal((9, 128)) * 10.0 ** rng.integers(-20, 20, (9, 1))).astype(F32)
    a8, asc = LI.quantize_tokens(z)
    b8, bsc = MH.quantize(z)
    np.testing.assert_array_equal(a8, b8)
    np.testing.assert_array_equal(asc.view(np.uint32), bsc.view(np.uint32))
    assert np.abs(a8).max(axis=1).tolist() == [127] * 9


@pytest.mark.parametrize("dim,tq,td", [(64, 1, 1), (128, 32, 100), (192, 17, 33), (1024, 64, 20)])
def test_the_model_is_close_to_float64_maxsim(dim, tq, td):
    """Bound, from the rounding rule.  A token is x = s * x8 + e with s = amax / 127 and |e_k| <= s / 2 (rint) -- the
    float32 product x * (127 / amax) in front of rint moves a value by at most 127 * 2^-23, so |e_k| <= s * (1/2 + 2^-16).
    For a query token q (scale sq, amax aq) and a row token d (sd, ad):
        |<q, d> - sq * sd * I| = |<eq, d> + <sq * q8, ed>| <= dim * (sq / 2) * ad + dim * aq * (sd / 2) = dim * aq * ad / 127.
    max_j is 1-Lipschitz in the sup norm and the score sums Tq of them: Tq * dim * aq * ad / 127, aq / ad the largest amax
    of the query's / the row's tokens; the factor (1 + 2^-12) covers the 2^-16 above and the rounding of the two scales.
    The model's own float32 arithmetic adds at most 8 roundings (one product by sd, one by sq, six tree levels) of
    relative size 2^-24 on partial sums bounded by Tq * dim * aq * ad: 16 * 2^-24 * Tq * dim * aq * ad bounds it twice over."""
    rng = np.random.default_rng(dim + tq)
    q = rng.standard_normal((tq, dim)).astype(F32)
    d = rng.standard_normal((td, dim)).astype(F32)
    q8, sq = LI.quantize_tokens(q)
    d8, sd = LI.quantize_tokens(d)
    got = float(LI.maxsim_scores(q8, sq, [(d8, sd)])[0])
    want = MH.float64_maxsim(q, d)
    aq, ad = float(np.abs(q).max()), float(np.abs(d).max())
    bound = tq * dim * aq * ad / 127.0 * (1 + 2.0 ** -12) + 16 * 2.0 ** -24 * tq * dim * aq * ad
    print(f"dim={dim} tq={tq} td={td}: model {got:.6f} float64 {want:.6f} |diff| {abs(got - want):.6f} bound {bound:.6f}")
    assert abs(got - want) <= bound


def test_ragged_packing():
    rng = np.random.default_rng(1)
    cells = [random_tokens(rng, 3, 64), None, random_tokens(rng, 0, 64), random_tokens(rng, 5, 64), None]
    heads, x8, sc, indptr = LI.pack_tokens(cells, 64)
    assert heads.dtype == np.uint32 and heads.tolist() == [3, LI.MISSING, 0, 5, LI.MISSING]
    assert indptr.tolist() == [0, 3, 3, 3, 8, 8] and x8.shape == (8, 64) and sc.shape == (8,)
    np.testing.assert_array_equal(x8[3:8], cells[3][0])
    np.testing.assert_array_equal(sc[:3], cells[0][1])
    assert LI.pack_tokens([None], 64, absent=LI.NULL)[0].tolist() == [LI.NULL]
    empty = LI.pack_tokens([], 128)
    assert empty[1].shape == (0, 128) and empty[3].tolist() == [0]
    with pytest.raises(ValueError, match="cell 0"):
        LI.pack_tokens([random_tokens(rng, 2, 128)], 64)
    # queries: padded to the width, quantised as stored tokens are
    qs = [rng.standard_normal((2, 48)).astype(F32), rng.standard_normal((64, 64)).astype(F32)]
    q8, qsc, qip = LI.pack_queries(qs, 64)
    assert qip.tolist() == [0, 2, 66] and not q8[:2, 48:].any()
    np.testing.assert_array_equal(q8[:2, :48], MH.quantize(qs[0])[0])
    for bad, word in (([np.zeros((0, 64), F32)], "1 to 64"), ([np.zeros((65, 64), F32)], "1 to 64"),
                      ([np.zeros((1, 65), F32)], "width"), ([np.full((1, 64), np.nan, F32)], "finite")):
        with pytest.raises(ValueError, match=word):
            LI.pack_queries(bad, 64)
    for dim in (0, 32, 65, 1088, 64.0, True, None):
        with pytest.raises(ValueError, match="multiple of 64"):
            LI.check_dim(dim)
    assert [LI.check_dim(d) for d in (64, 128, 1024)] == [64, 128, 1024]


# ---- the handler over a stub index -------------------------------------------------------------------------------------------
class StubIndex:
    """the token entries of HxIndex, recording what they are given"""

    def __init__(self):
        self.calls, self.cols, self.next = [], {}, 0

    def count(self):
        return 16

    def payload_create_tokens(self, dim_t):
        self.next += 1
        self.cols[self.next] = {"dim": dim_t, "heads": []}
        return self.next

    def payload_drop(self, col):
        del self.cols[col]

    def payload_rows(self, col):
        return len(self.cols[col]["heads"])

    def payload_append_tokens(self, col, heads, x8, scales):
        assert x8.shape == (scales.shape[0], self.cols[col]["dim"]) and x8.dtype == np.int8
        self.cols[col]["heads"].extend(heads.tolist())

    def hybrid_query_rerank_host(self, q, indptr, idx, val, hp, col, q8, qscale, qtip, limit, candidates_limit=0, mask=None,
                                 mask_root_only=False):
        B = q.shape[0]
        self.calls.append((int(hp.mode), col, q8.shape, qtip.tolist(), limit, candidates_limit, mask is not None,
                           bool(mask_root_only)))
        n = min(limit, 2)
        scores = np.full((B, limit), -np.inf, F32)
        ids = np.full((B, limit), -1, np.int64)
        first = np.full((B, limit), -np.inf, F32)
        scores[:, :n], ids[:, :n], first[:, :n] = [7.5, 3.25][:n], [4, 11][:n], [0.5, 0.75][:n]
        return scores, ids, first, np.full(B, n, np.int32)


def stub_handler():
    h = QdrantHandler()
    col = _Collection.__new__(_Collection)
    col.dim, col.msizes, col.sparse_enabled = 4, (), True
    col.index = StubIndex()
    col.ids = [f"p{r}" for r in range(16)]
    col.payloads, col._masks, col.pindex, col.tokens = [{"chunk": r, "even": r % 2 == 0} for r in range(16)], {}, None, None
    h._collections["u"] = col
    return h, col


def search(h, B=2, tokens=None, **kw):
    qs = [[0.1, 0.2, 0.3, 0.4]] * B
    sv = [{"indices": [1, 5], "values": [1.0, 0.5]}] * B
    kw.setdefault("search_params", P)
    toks = tokens if tokens is not None else [np.ones((3, 100), F32)] * B
    return asyncio.run(h.hybrid_search_rerank("u", qs, sv, toks, **kw))


EVEN = {"must": [{"key": "even", "match": {"value": True}}]}


def test_handler_passes_the_call_on_and_shapes_the_hits():
    h, col = stub_handler()
    asyncio.run(h.create_token_index("u", 128))
    assert col.tokens["dim"] == 128 and col.tokens["cells"] == [None] * 16
    assert col.index.cols[col.tokens["col"]]["heads"] == [LI.MISSING] * 16     # the stored points hold no tokens
    asyncio.run(h.create_token_index("u", 128))                                # again, the same width: nothing happens
    assert len(col.index.cols) == 1
    res = search(h)
    assert col.index.calls == [(0, col.tokens["col"], (6, 128), [0, 3, 6], 10, 50, False, False)]
    for hits in res:
        assert all(isinstance(p, RerankedPoint) and isinstance(p, ScoredPoint) for p in hits)
        assert [(p.id, p.score, p.first_score) for p in hits] == [("p4", 7.5, 0.5), ("p11", 3.25, 0.75)]
        assert hits[0].payload is col.payloads[4]
    search(h, B=1, mode="h1", limit=2048, candidates_limit=None)
    assert col.index.calls[-1][0] == 1 and col.index.calls[-1][4:] == (2048, 90, False, False)
    search(h, B=1, candidates_limit=7, filters=EVEN)
    assert col.index.calls[-1][4:] == (10, 7, True, True)                      # a root filter: the eligibility plane
    search(h, B=1, filters=EVEN, filter_stages="all", mode="h1")
    assert col.index.calls[-1][4:] == (10, 90, True, False)


def test_handler_refusals():
    h, col = stub_handler()
    with pytest.raises(ValueError, match="create_token_index"):                # no token index yet
        search(h)
    for dim in (0, 100, 2048, "128"):
        with pytest.raises(ValueError, match="multiple of 64"):
            asyncio.run(h.create_token_index("u", dim))
    with pytest.raises(KeyError):
        asyncio.run(h.create_token_index("nobody", 128))
    asyncio.run(h.create_token_index("u", 128))
    with pytest.raises(ValueError, match="width"):
        asyncio.run(h.create_token_index("u", 256))
    for limit in (0, -1, 2049, 2.0, True, None):
        with pytest.raises(ValueError, match="limit"):
            search(h, limit=limit)
    for cl in (0, -5, 1.5, True):
        with pytest.raises(ValueError, match="candidates_limit"):
            search(h, candidates_limit=cl)
    for toks, word in (([np.zeros((0, 128), F32)] * 2, "1 to 64"), ([np.zeros((65, 128), F32)] * 2, "1 to 64"),
                       ([np.zeros((2, 129), F32)] * 2, "width"), ([np.full((1, 8), np.inf, F32)] * 2, "finite"),
                       ([np.zeros((2, 128), F32)], "token lists")):
        with pytest.raises(ValueError, match=word):
            search(h, tokens=toks)
    with pytest.raises(ValueError, match="root"):
        search(h, mode="h1", filters=EVEN)
    with pytest.raises(ValueError, match="mode"):
        search(h, mode="flat")
    with pytest.raises(ValueError, match="filter_stages"):
        search(h, filter_stages="none")
    with pytest.raises(ValueError, match="clause"):
        search(h, filters={"mustnt": []})
    assert col.index.calls == []                                               # refused before the engine is asked
    assert search(h, search_params=None) == []                                 # any other failure: logged, []
    assert asyncio.run(h.hybrid_search_rerank("nobody", [[0.1] * 4], [{"indices": [1], "values": [1.0]}],
                                              [np.ones((1, 8), F32)], search_params=P)) == []
    # a chunk that brings tokens to a collection without a token index is refused before anything is stored
    h2, col2 = stub_handler()
    with pytest.raises(ValueError, match="create_token_index"):
        col2.token_cells_of([{"token_embeddings": np.ones((2, 8), F32)}])
    assert col2.token_cells_of([{}, {"token_embeddings": None}]) is None


def test_a_sharded_collection_is_refused():
    from rag_application_amd.sharded import ShardedHandler
    h = ShardedHandler.__new__(ShardedHandler)                                 # (no process group: the refusal comes first)
    h._collections, h._lock = {}, None
    assert ShardedHandler._late_rerank is False and QdrantHandler._late_rerank is True
    with pytest.raises(ValueError, match="sharded"):
        QdrantHandler._rerank_sync(h, "u", [[0.0]], [{"indices": [], "values": []}], [np.ones((1, 64), F32)], 10, 100, P,
                                   None, "tree", "root")
    with pytest.raises(ValueError, match="sharded"):
        asyncio.run(QdrantHandler.create_token_index(h, "u", 128))
