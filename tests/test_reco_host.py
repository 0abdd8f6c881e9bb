"""CPU: the host model of the recommend search (tests/reco_helpers.py) against a brute-force
restatement with a full similarity matrix, its edge properties, and QdrantHandler.recommend's refusals over a stub index.
No GPU needed."""
import asyncio

import numpy as np
import pytest

from oracle import oracle as O
from rag_application_amd.handler import QdrantHandler, ScoredPoint, _Collection
from tests import reco_helpers as RH

F32 = np.float32
STRATEGIES = (RH.AVERAGE, RH.BEST_SCORE, RH.SUM_SCORES)


def bits(a):
    return np.asarray(a, F32).view(np.uint32)


def brute(rows, examples, signs, strategy, limit, excluded):
    """the definition, literally: one similarity matrix, the score of every row in a Python loop over the examples in the
    order given, then a sort by (score descending, id ascending)"""
    n = len(rows)
    if n == 0:
        return []
    if strategy == RH.AVERAGE:
        P = [e for e, s in zip(examples, signs) if s == 1]
        N = [e for e, s in zip(examples, signs) if s == -1]
        q = np.zeros(examples.shape[1], F32)
        for k in range(examples.shape[1]):
            p = P[0][k]
            for e in P[1:]:
                p = F32(p + e[k])
            p = F32(p / F32(len(P)))
            if N:
                m = N[0][k]
                for e in N[1:]:
                    m = F32(m + e[k])
                m = F32(m / F32(len(N)))
                q[k] = F32(p + F32(p - m))
            else:
                q[k] = p
        S = O.spec_dot_matrix(rows, O.cosine_preprocess(q)[None, :])
        sc = [S[0, i] for i in range(n)]
    else:
        S = O.spec_dot_matrix(rows, examples)           # [E, n]
        sc = []
        for i in range(n):
            if strategy == RH.BEST_SCORE:
                sp = max([S[e, i] for e in range(len(signs)) if signs[e] == 1], default=F32(-np.inf))
                sm = max([S[e, i] for e in range(len(signs)) if signs[e] == -1], default=F32(-np.inf))
                v = sp if sp > sm else F32(-F32(sm * sm))
            else:
                v = F32(0.0)
                for e in range(len(signs)):
                    if signs[e] == 1:
                        v = F32(v + S[e, i])
                for e in range(len(signs)):
                    if signs[e] == -1:
                        v = F32(v - S[e, i])
            sc.append(F32(v + F32(0.0)))
    order = sorted((i for i in range(n) if not excluded[i]), key=lambda i: (-float(sc[i]), i))[:limit]
    return [(i, int(bits(sc[i]))) for i in order]


def case(seed, n, dim, n_pos, n_neg):
    rng = np.random.default_rng(seed)
    rows = O.cosine_preprocess(rng.standard_normal((max(n, 1), dim)).astype(F32))[:n]
    examples = O.cosine_preprocess(rng.standard_normal((n_pos + n_neg, dim)).astype(F32))
    signs = [1] * n_pos + [-1] * n_neg
    perm = rng.permutation(n_pos + n_neg)                # the signs interleaved: order matters inside each group only
    return rows, examples[perm], [signs[i] for i in perm], rng


@pytest.mark.parametrize("n", (0, 1, 2, 63, 300))
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_model_equals_the_brute_force_restatement(n, strategy):
    for seed, (n_pos, n_neg, dim) in enumerate(((1, 0, 64), (3, 2, 100), (5, 4, 130), (0, 3, 64))):
        if strategy == RH.AVERAGE and n_pos == 0:
            continue
        rows, ex, signs, rng = case(seed, n, dim, n_pos, n_neg)
        excluded = rng.random(n) < 0.2
        for limit in (1, 10, n + 1):
            sc, ids = RH.recommend(rows, ex, signs, strategy, limit, excluded)
            assert [(int(i), int(b)) for i, b in zip(ids, bits(sc))] == brute(rows, ex, signs, strategy, limit, excluded)


@pytest.mark.parametrize("strategy", (RH.BEST_SCORE, RH.SUM_SCORES))
def test_one_positive_is_the_plain_cosine_list_without_the_example(strategy):
    rows, _, _, _ = case(11, 200, 100, 1, 0)
    e = 17
    excluded = np.zeros(200, bool)
    excluded[e] = True
    sc, ids = RH.recommend(rows, rows[e][None, :], [1], strategy, 20, excluded)
    ws, wi = O.topk(O.spec_dot(rows, rows[e]), np.arange(200), 21)
    assert wi[0] == e                                     # the example is its own nearest row
    np.testing.assert_array_equal(ids, wi[1:])
    np.testing.assert_array_equal(bits(sc), bits(ws[1:]))


def test_best_score_without_negatives_and_without_positives():
    rows, ex, _, _ = case(5, 120, 64, 3, 0)
    none = np.zeros(120, bool)
    S = O.spec_dot_matrix(rows, ex)
    sc, ids = RH.recommend(rows, ex, [1, 1, 1], RH.BEST_SCORE, 120, none)
    best = S.max(axis=0)
    np.testing.assert_array_equal(bits(sc), bits(best[ids]))           # N = 0: the largest positive similarity
    sc, ids = RH.recommend(rows, ex, [-1, -1, -1], RH.BEST_SCORE, 120, none)
    np.testing.assert_array_equal(bits(sc), bits((-(best * best) + F32(0.0))[ids]))   # P = 0: -(s-)^2
    assert (sc <= 0).all()


def test_the_boundary_s_plus_equal_to_s_minus_takes_the_negative_branch():
    rows, _, _, _ = case(6, 50, 64, 1, 0)
    v = rows[7]                                           # given as RAW vectors: the row itself stays in the list
    sc, ids = RH.recommend(rows, np.stack([v, v]), [1, -1], RH.BEST_SCORE, 50, np.zeros(50, bool))
    s = O.spec_dot(rows, v)
    want = (-(s * s) + F32(0.0)).astype(F32)              # s+ == s- on EVERY row: never "greater"
    np.testing.assert_array_equal(bits(sc), bits(want[ids]))
    assert ids[-1] == 7 and sc[-1] < 0                    # the row equal to both examples: the most negative score


def test_minus_zero_is_canonicalised():
    rows = np.zeros((4, 64), F32)
    rows[:, 0] = 1.0                                      # orthogonal to the example
    e = np.zeros((1, 64), F32)
    e[0, 1] = 1.0
    for strategy, signs in ((RH.BEST_SCORE, [-1]), (RH.SUM_SCORES, [-1]), (RH.SUM_SCORES, [1])):
        sc, ids = RH.recommend(rows, e, signs, strategy, 4, np.zeros(4, bool))
        assert (bits(sc) == 0).all(), (strategy, signs)   # +0.0f, never 0x80000000
        assert ids.tolist() == [0, 1, 2, 3]


def test_ties_go_to_the_smaller_id_and_ids_are_the_global_ones():
    base, ex, signs, _ = case(8, 16, 100, 2, 1)
    rows = base[np.arange(96) % 16]                       # every row six times
    gids = np.arange(96) * 3 + 1000
    for strategy in STRATEGIES:
        sc, ids = RH.recommend(rows, ex, signs, strategy, 96, np.zeros(96, bool), ids=gids)
        for k in range(0, 96, 6):
            assert len(set(bits(sc[k:k + 6]).tolist())) == 1
            assert ids[k:k + 6].tolist() == sorted(ids[k:k + 6].tolist())
            assert len({(int(i) - 1000) // 3 % 16 for i in ids[k:k + 6]}) == 1


def test_exclusion_and_exhaustion():
    rows, ex, signs, rng = case(9, 40, 64, 2, 2)
    excluded = np.zeros(40, bool)
    excluded[[0, 5, 39]] = True
    for strategy in STRATEGIES:
        sc, ids = RH.recommend(rows, ex, signs, strategy, 100, excluded)
        assert len(ids) == 37 and not set(ids.tolist()) & {0, 5, 39}
        full, fids = RH.recommend(rows, ex, signs, strategy, 100, np.zeros(40, bool))
        assert [i for i in fids.tolist() if i not in (0, 5, 39)] == ids.tolist()      # exclusion moves nobody else
        short, sids = RH.recommend(rows, ex, signs, strategy, 5, excluded)
        assert sids.tolist() == ids[:5].tolist()
        assert len(RH.recommend(rows, ex, signs, strategy, 5, np.ones(40, bool))[1]) == 0


def test_request_model_excludes_stored_examples_of_either_sign():
    rows, _, _, rng = case(10, 30, 64, 1, 0)
    raw = rng.standard_normal(64).astype(F32) * 3
    keys, cnt = RH.request_model(rows, [(3, 1), (raw, 1), (4, -1), (3, -1)], RH.SUM_SCORES, 40)
    assert cnt == 28 and (keys[28:] == 0).all()
    ids = 0xFFFFFFFF - (keys[:cnt] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert not set(ids.tolist()) & {3, 4}
    assert (np.diff(keys[:cnt].astype(np.float64)) <= 0).all()


# ---- the handler over a stub index -------------------------------------------------------------------------------------------
class StubIndex:
    """recommend_host that records its arguments and returns the first rows"""

    def __init__(self):
        self.calls = []

    def recommend_host(self, requests, strategy, limit, mask=None):
        self.calls.append((requests, strategy, limit, mask is not None))
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


def test_handler_passes_the_call_on_and_shapes_the_hits():
    h, col = stub_handler()
    hits = asyncio.run(h.recommend("u", ["p3", V], negative=["p7"], strategy="best_score", limit=5))
    (reqs, strategy, limit, masked), = col.index.calls
    assert (strategy, limit, masked) == (1, 5, False)
    (r0,) = reqs
    assert [(e if isinstance(e, int) else None, s) for e, s in r0] == [(3, 1), (None, 1), (7, -1)]
    np.testing.assert_array_equal(r0[1][0], np.asarray(V, np.float32))
    assert all(isinstance(p, ScoredPoint) for p in hits) and [p.id for p in hits] == ["p5", "p1", "p9"]
    assert hits[0].payload is col.payloads[5] and np.float32(hits[0].score) == np.float32(0.9)
    res = asyncio.run(h.recommend_batch("u", [{"positive": ["p1"], "strategy": "sum_scores"},
                                              {"negative": [V], "strategy": "sum_scores"}], limit=2, filters=EVEN))
    assert len(res) == 2 and all(len(r) == 2 for r in res)
    assert col.index.calls[-1][1:] == (2, 2, True)
    assert asyncio.run(h.recommend("u", ["p1"])) and col.index.calls[-1][1:] == (0, 10, False)   # average_vector, 10


def test_handler_refusals():
    h, col = stub_handler()

    def reco(*a, **kw):
        return asyncio.run(h.recommend("u", *a, **kw))
    with pytest.raises(ValueError, match="unknown point id"):
        reco(["nobody"])
    with pytest.raises(ValueError, match="strategy"):
        reco(["p1"], strategy="nearest")
    with pytest.raises(ValueError, match="at least one example"):
        reco([], negative=[])
    with pytest.raises(ValueError, match="at least one example"):
        reco(None)
    with pytest.raises(ValueError, match="positive"):
        reco([], negative=["p1"], strategy="average_vector")
    with pytest.raises(ValueError, match="too many examples"):
        reco([f"p{r % 16}" for r in range(33)], strategy="sum_scores")
    for limit in (0, -1, 1025, 2.0, True, None):
        with pytest.raises(ValueError, match="limit"):
            reco(["p1"], limit=limit)
    with pytest.raises(ValueError, match="dimension"):
        reco([[0.1, 0.2]])
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            reco([[0.1, bad, 0.3, 0.4]])
    with pytest.raises(ValueError, match="clause"):
        reco(["p1"], filters={"mustnt": []})
    with pytest.raises(ValueError, match="requests"):
        asyncio.run(h.recommend_batch("u", []))
    with pytest.raises(ValueError, match="requests"):
        asyncio.run(h.recommend_batch("u", [{"positive": ["p1"]}] * 17))
    with pytest.raises(ValueError, match="one strategy"):
        asyncio.run(h.recommend_batch("u", [{"positive": ["p1"]}, {"positive": ["p1"], "strategy": "best_score"}]))
    assert col.index.calls == []                                    # refused before the engine is asked
    assert asyncio.run(h.recommend("nobody", ["p1"])) == []         # any other failure: logged, [] -- as every search
    assert reco(["p1", "p2"], negative=[V], strategy="best_score", limit=1024)        # the largest limit passes


def test_wide_rows_take_fewer_examples():
    h, col = stub_handler()
    col.dim = 4096                                                  # 32768 / 4096 = 8 examples
    with pytest.raises(ValueError, match="too many examples"):
        asyncio.run(h.recommend("u", [f"p{r}" for r in range(9)], strategy="sum_scores"))
    assert asyncio.run(h.recommend("u", [f"p{r}" for r in range(8)], strategy="sum_scores"))


def test_a_sharded_collection_is_refused():
    from rag_application_amd.sharded import ShardedHandler
    h = ShardedHandler.__new__(ShardedHandler)                      # (no process group: the refusal comes first)
    h._collections, h._lock = {}, None
    assert ShardedHandler._recommend is False and QdrantHandler._recommend is True
    with pytest.raises(ValueError, match="sharded"):
        QdrantHandler._recommend_sync(h, "u", [{"positive": ["p1"]}], 10, None)
