"""CPU: the host model of the discovery and context search (tests/discover_helpers.py) against a
naive per-row restatement, its edge properties, the precondition of the GPU ties test, and QdrantHandler.discover's
refusals over a stub index.  No GPU needed."""
import asyncio

import numpy as np
import pytest

from oracle import oracle as O
from rag_application_amd.handler import QdrantHandler, ScoredPoint, _Collection
from tests import discover_helpers as DH

F32 = np.float32
EPS = F32(2.0 ** -23)
ENTRIES = (QdrantHandler.discover, QdrantHandler.discover_batch)   # what the model below is the oracle of: bound at import


def bits(a):
    return np.asarray(a, F32).view(np.uint32)


def sig(v):
    v = F32(v)
    return F32(v / F32(F32(1.0) + F32(abs(v))))


def brute(rows, target, pairs, limit, excluded):
    """the definition, literally: one similarity matrix, the score of every row in a Python loop over the pairs in the
    order given, then a sort by (score descending, id ascending)"""
    n = len(rows)
    if n == 0:
        return []
    ex = ([target] if target is not None else []) + [e for pq in pairs for e in pq]
    S = O.spec_dot_matrix(rows, np.stack(ex))               # [E, n]
    t = 0 if target is None else 1
    sc = []
    for i in range(n):
        v = F32(0.0)
        for k in range(len(pairs)):
            sp, sn = S[t + 2 * k, i], S[t + 2 * k + 1, i]
            if target is not None:
                v = F32(v + (F32(1.0) if sp > sn else F32(-1.0) if sp < sn else F32(0.0)))
            else:
                d = F32(F32(sp - sn) - EPS)
                v = F32(v + sig(min(d, F32(0.0))))
        if target is not None:
            v = F32(v + F32(F32(0.5) * F32(sig(S[0, i]) + F32(1.0))))
        sc.append(F32(v + F32(0.0)))
    order = sorted((i for i in range(n) if not excluded[i]), key=lambda i: (-float(sc[i]), i))[:limit]
    return [(i, int(bits(sc[i]))) for i in order]


def case(seed, n, dim, with_target, n_pairs):
    rng = np.random.default_rng(seed)
    rows = O.cosine_preprocess(rng.standard_normal((max(n, 1), dim)).astype(F32))[:n]
    ex = O.cosine_preprocess(rng.standard_normal((1 + 2 * n_pairs, dim)).astype(F32))
    target = ex[0] if with_target else None
    pairs = [(ex[1 + 2 * k], ex[2 + 2 * k]) for k in range(n_pairs)]
    return rows, target, pairs, rng


def model(rows, target, pairs, limit, excluded):
    sc, ids = DH.discover(rows, target, pairs, limit, excluded)
    return [(int(i), int(b)) for i, b in zip(ids, bits(sc))]


@pytest.mark.parametrize("n", (0, 1, 2, 63, 300))
def test_model_equals_the_naive_restatement(n):
    for seed, (with_target, n_pairs, dim) in enumerate(((True, 0, 64), (True, 1, 64), (True, 3, 100), (True, 15, 130),
                                                        (False, 1, 64), (False, 16, 100))):
        rows, target, pairs, rng = case(seed, n, dim, with_target, n_pairs)
        excluded = rng.random(n) < 0.2
        for limit in (1, 10, n + 1):
            assert model(rows, target, pairs, limit, excluded) == brute(rows, target, pairs, limit, excluded), \
                (n, with_target, n_pairs, limit)


def test_target_only_is_the_cosine_order_with_ids_ascending_among_merged_scores():
    rows, target, _, _ = case(3, 300, 64, True, 0)
    sc, ids = DH.discover(rows, target, [], 300, np.zeros(300, bool))
    sim = DH.spec_dot(rows, target)
    assert (np.diff(sim[ids]) <= 0).all()                    # never against the cosine order
    assert (np.diff(sc) <= 0).all()
    tied = np.diff(sc) == 0                                  # the sigmoid may merge neighbours: then ids ascend
    assert (np.diff(ids)[tied] > 0).all()
    np.testing.assert_array_equal(bits(sc), bits(F32(0.5) * (DH.fast_sigmoid(sim[ids]) + F32(1.0))))
    # a merged pair, constructed: two sims one ulp apart whose scores are the same float
    a = F32(0.75)
    b = np.nextafter(a, F32(1.0))
    sa, sb = (F32(0.5) * (DH.fast_sigmoid(np.asarray([a, b], F32)) + F32(1.0))).astype(F32)
    assert a != b and sa == sb


def test_one_pair_with_pos_equal_to_neg():
    rows, target, pairs, _ = case(4, 50, 64, True, 1)
    same = [(pairs[0][0], pairs[0][0])]
    none = np.zeros(50, bool)
    with_pair, ids = DH.discover(rows, target, same, 50, none)           # rank 0: the target-only list
    alone, ids0 = DH.discover(rows, target, [], 50, none)
    np.testing.assert_array_equal(ids, ids0)
    np.testing.assert_array_equal(bits(with_pair), bits(alone))
    ctx = DH.scores(rows, None, same)                                    # context: fast_sigmoid(-eps) for every row
    want = F32(-EPS / F32(F32(1.0) + EPS))
    assert want < 0 and (bits(ctx) == bits(want)).all()
    assert DH.discover(rows, None, same, 5, none)[1].tolist() == [0, 1, 2, 3, 4]


def test_the_three_branches_of_a_pair():
    e = np.zeros((3, 64), F32)
    e[0, 0] = e[1, 1] = 1.0
    e[2, 0] = e[2, 1] = F32(np.sqrt(0.5))
    rows = np.stack([e[0], e[1], e[2]])                                   # nearer pos, nearer neg, equally near
    target = e[2]
    sc = DH.scores(rows, target, [(e[0], e[1])])
    base = DH.scores(rows, target, [])
    np.testing.assert_array_equal(bits(sc), bits((np.asarray([1, -1, 0], F32) + base).astype(F32)))
    ctx = DH.scores(rows, None, [(e[0], e[1])])
    assert ctx[0] == 0 and bits(ctx[0]) == 0                              # the positive side: exactly +0
    assert bits(ctx[1]) == bits(sig(F32(F32(-1.0) - EPS)))                # the negative side: fast_sigmoid(-1 - eps)
    assert bits(ctx[2]) == bits(sig(-EPS))                                # on the border: the epsilon still counts


def test_minus_zero_becomes_plus_zero():
    rows = np.zeros((2, 64), F32)
    rows[0, 0], rows[1, 1] = 1.0, 1.0
    neg = -rows[0]
    sc = DH.scores(rows, rows[1], [(rows[0], neg), (neg, rows[0])])       # rank +1 - 1 on row 0, 0 on row 1
    assert bits(F32(-0.0)) != 0 and (np.signbit(sc) == False).all()       # noqa: E712
    ctx = DH.scores(rows, None, [(rows[0], rows[1])])
    assert bits(ctx[0]) == 0


def test_exclusion_and_exhaustion():
    rows, target, pairs, _ = case(6, 40, 100, True, 3)
    excluded = np.zeros(40, bool)
    excluded[[0, 5, 39]] = True
    for t in (target, None):
        sc, ids = DH.discover(rows, t, pairs, 100, excluded)
        assert len(ids) == 37 and not set(ids.tolist()) & {0, 5, 39}
        full, fids = DH.discover(rows, t, pairs, 100, np.zeros(40, bool))
        assert [i for i in fids.tolist() if i not in (0, 5, 39)] == ids.tolist()      # exclusion moves nobody else
        assert DH.discover(rows, t, pairs, 5, excluded)[1].tolist() == ids[:5].tolist()
        assert len(DH.discover(rows, t, pairs, 5, np.ones(40, bool))[1]) == 0


def test_request_model_excludes_stored_examples():
    rows, _, _, rng = case(10, 30, 64, True, 0)
    raw = rng.standard_normal(64).astype(F32) * 3
    keys, cnt = DH.request_model(rows, (3, [(raw, 4), (3, 7)]), 40)
    assert cnt == 27 and (keys[27:] == 0).all()
    ids = 0xFFFFFFFF - (keys[:cnt] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert not set(ids.tolist()) & {3, 4, 7}
    assert (np.diff(keys[:cnt].astype(np.float64)) <= 0).all()


def test_corpus_b_with_one_pair_scores_exactly_zero_for_a_quarter_of_the_rows_and_more():
    """the precondition of the GPU ties test (tests/test_gpu_discover.py): context search with the pair (row 0, row 1)"""
    Xn = O.cosine_preprocess(O.synth_dense(O.SEED_CORPUS, 0, 4096, 64))
    sc = DH.scores(Xn, None, [(Xn[0], Xn[1])])
    zeros = int((bits(sc) == 0).sum())
    assert zeros >= 1024, zeros
    assert (sc <= 0).all()


# ---- the handler over a stub index -------------------------------------------------------------------------------------------
class StubIndex:
    """discover_host that records its arguments and returns the first rows"""

    def __init__(self):
        self.calls = []

    def discover_host(self, requests, limit, mask=None):
        self.calls.append((requests, limit, mask is not None))
        R = len(requests)
        n = min(limit, 3)
        scores = np.full((R, limit), -np.inf, np.float32)
        ids = np.full((R, limit), -1, np.int64)
        scores[:, :n] = [0.9, 0.8, 0.7][:n]
        ids[:, :n] = [5, 1, 9][:n]
        return scores, ids, np.full(R, n, np.int32)

    def count(self):
        return 16


def stub_handler():
    h = QdrantHandler()
    col = _Collection.__new__(_Collection)
    col.dim, col.msizes, col.sparse_enabled = 4, (), True
    col.index = StubIndex()
    col.ids = [f"p{r}" for r in range(16)]
    col.payloads, col._masks, col.pindex = [{"chunk": r, "even": r % 2 == 0} for r in range(16)], {}, None
    h._collections["u"] = col
    return h, col


EVEN = {"must": [{"key": "even", "match": {"value": True}}]}
V = [0.1, 0.2, 0.3, 0.4]


def pair(p, n):
    return {"positive": p, "negative": n}


def test_handler_passes_the_call_on_and_shapes_the_hits():
    h, col = stub_handler()
    hits = asyncio.run(h.discover("u", target="p3", context=[pair(V, "p7"), pair("p2", "p4")], limit=5))
    (reqs, limit, masked), = col.index.calls
    assert (limit, masked) == (5, False)
    (target, pairs), = reqs
    assert target == 3 and pairs[1] == (2, 4) and pairs[0][1] == 7
    np.testing.assert_array_equal(pairs[0][0], np.asarray(V, np.float32))
    assert all(isinstance(p, ScoredPoint) for p in hits) and [p.id for p in hits] == ["p5", "p1", "p9"]
    assert hits[0].payload is col.payloads[5] and np.float32(hits[0].score) == np.float32(0.9)
    res = asyncio.run(h.discover_batch("u", [{"target": V}, {"context": [pair("p1", V)]}], limit=2, filters=EVEN))
    assert len(res) == 2 and all(len(r) == 2 for r in res)
    reqs, limit, masked = col.index.calls[-1]
    assert (limit, masked) == (2, True) and reqs[0][1] == [] and reqs[1][0] is None
    assert asyncio.run(h.discover("u", context=[pair("p1", "p2")])) and col.index.calls[-1][1:] == (10, False)


def test_handler_refusals():
    h, col = stub_handler()

    def disc(*a, **kw):
        return asyncio.run(h.discover("u", *a, **kw))
    with pytest.raises(ValueError, match="unknown point id"):
        disc("nobody")
    with pytest.raises(ValueError, match="unknown point id"):
        disc("p1", [pair("p2", "nobody")])
    with pytest.raises(ValueError, match="target or a context pair"):
        disc()
    with pytest.raises(ValueError, match="target or a context pair"):
        disc(None, [])
    for bad in ({"positive": "p1"}, {"positive": "p1", "negative": None}, ("p1", "p2"), "p1",
                {"positive": "p1", "negative": "p2", "extra": 1}):
        with pytest.raises(ValueError, match="context pair"):
            disc("p3", [bad])
    with pytest.raises(ValueError, match="list of pairs"):
        disc("p3", {"positive": "p1", "negative": "p2"})
    with pytest.raises(ValueError, match="too many examples"):
        disc("p0", [pair("p1", "p2")] * 16)                         # 33 examples
    with pytest.raises(ValueError, match="too many examples"):
        disc(None, [pair("p1", "p2")] * 17)                         # 34
    for limit in (0, -1, 1025, 2.0, True, None):
        with pytest.raises(ValueError, match="limit"):
            disc("p1", limit=limit)
    with pytest.raises(ValueError, match="dimension"):
        disc([0.1, 0.2])
    with pytest.raises(ValueError, match="dimension"):
        disc("p1", [pair("p2", [0.1] * 5)])
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            disc([0.1, bad, 0.3, 0.4])
    with pytest.raises(ValueError, match="clause"):
        disc("p1", filters={"mustnt": []})
    with pytest.raises(ValueError, match="requests"):
        asyncio.run(h.discover_batch("u", []))
    with pytest.raises(ValueError, match="requests"):
        asyncio.run(h.discover_batch("u", [{"target": "p1"}] * 17))
    assert col.index.calls == []                                    # refused before the engine is asked
    assert asyncio.run(h.discover("nobody", "p1")) == []            # any other failure: logged, [] -- as every search
    assert disc("p0", [pair("p1", "p2")] * 15, limit=1024)          # the most examples and the largest limit pass
    assert disc(None, [pair("p1", "p2")] * 16)


def test_wide_rows_take_fewer_examples():
    h, col = stub_handler()
    col.dim = 4096                                                  # 32768 / 4096 = 8 examples
    with pytest.raises(ValueError, match="too many examples"):
        asyncio.run(h.discover("u", "p0", [pair("p1", "p2")] * 4))
    assert asyncio.run(h.discover("u", None, [pair("p1", "p2")] * 4))


def test_a_sharded_collection_is_refused():
    from rag_application_amd.sharded import ShardedHandler
    h = ShardedHandler.__new__(ShardedHandler)                      # (no process group: the refusal comes first)
    h._collections, h._lock = {}, None
    assert ShardedHandler._discover is False and QdrantHandler._discover is True
    with pytest.raises(ValueError, match="sharded"):
        QdrantHandler._discover_sync(h, "u", [{"target": "p1"}], 10, None)
