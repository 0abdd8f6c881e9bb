"""GPU: node filters and thresholds of the query trees through QdrantHandler.query_points(filter_stages=...) (DESIGN.md
section 32) on the corpus of tests/golden/corpus_a_2048x768.npz, payloads page_number = r % 2 and document_id = doc{r // 64}
as tests/test_gpu_query_tree.py stores them.  A filtered nearest-neighbour search equals the brute-force ranking of the kept
rows; the reference's tree and the H1 tree under "all" equal hybrid_search_batch(filter_stages="all"); a root-only filter
on an input of at most 2048 is the same under "node" and "root"; wider unions, different filters on two prefetches,
thresholds below the root and a dozen random trees with random node filters equal the oracle interpreter
(tests/query_tree_filter_helpers.py), the random ones node by node; a batch comes back in request order; a cached mask
follows an upsert and a delete."""
from __future__ import annotations

import asyncio

import numpy as np
import pytest

from oracle import oracle as O
from rag_application_amd import filters as FL
from rag_application_amd import query_tree as QT
from tests import fusion_helpers as H
from tests import query_tree_helpers as T
from tests.query_tree_filter_helpers import FilteredOracleStages, FilterRecorder
from tests.test_gpu_query_tree import (DIM, DOC5, HALF, MS, N, P, as_rows, bits, chunk, flat, h1_tree, reference_tree,
                                       wide_fusion, wide_rescore)

pytestmark = pytest.mark.gpu

B = 4
NOTHING = {"must": [{"key": "document_id", "match": {"value": "no such document"}}]}
DOC9 = {"must": [{"key": "document_id", "match": {"any": ["doc9", "doc10", "doc31"]}}]}
KH, K5, K9, KN = (FL.filter_key(f) for f in (HALF, DOC5, DOC9, NOTHING))


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from rag_application_amd import engine
    return engine


@pytest.fixture(scope="module")
def corpus(synth_tables):
    X = O.synth_dense(O.SEED_CORPUS, 0, N, DIM)
    ip, si, sv = O.synth_sparse_docs(O.SEED_SPDOC, 0, N, synth_tables)
    Q = O.synth_dense(O.SEED_QUERY, 0, B, DIM)
    qip, qsi, qsv = O.synth_sparse_queries(O.SEED_SPQUERY, 0, B, synth_tables)
    sparse = [{"indices": qsi[qip[b]:qip[b + 1]].tolist(), "values": qsv[qip[b]:qip[b + 1]].tolist()} for b in range(B)]
    return X, ip, si, sv, Q, sparse, (qip, qsi, qsv)


@pytest.fixture(scope="module")
def handler(eng, corpus):
    from rag_application_amd.handler import QdrantHandler
    X, ip, si, sv = corpus[:4]
    h = QdrantHandler()
    asyncio.run(h.store_document_vectors([chunk(r, X, ip, si, sv) for r in range(N)], "u"))
    yield h
    asyncio.run(h.delete_collection("u"))


@pytest.fixture(scope="module")
def masks():
    r = np.arange(N)
    return {KH: r % 2 == 0, K5: r // 64 == 5, K9: np.isin(r // 64, (9, 10, 31)), KN: np.zeros(N, bool)}


@pytest.fixture(scope="module")
def oracle(corpus, masks):
    """the oracle's stages with every mask of this file: an OracleIndex of the kept rows each; fusion by fusion_helpers"""
    return FilteredOracleStages(corpus[:4], DIM, MS, masks, fuse=H)


def queries(corpus, n=B):
    return [corpus[4][b].tolist() for b in range(n)], corpus[5][:n]


def ask(handler, reqs, how):
    return asyncio.run(handler.query_points_batch("u", [dict(r, filter_stages=how) for r in reqs]))


def oracle_lists(oracle, reqs, how="node"):
    """the oracle interpreter over node-mode requests of ONE shape: per request [(row, score bits)], best first"""
    parsed = [QT.parse_nodes(r, DIM, MS, prefetch_filters=how == "node") for r in reqs]
    shapes = {QT.push_to_leaves(p[0]) if how == "all" else p[0] for p in parsed}
    assert len(shapes) == 1
    keys, cnt = QT.run(shapes.pop(), QT.batch_vectors([p[1] for p in parsed]), oracle,
                       thresholds=QT.batch_thresholds([p[2] for p in parsed]))
    return [[(H.key_id(int(x)), bits(H.key_score(int(x)))) for x in keys[b, :int(cnt[b])]] for b in range(len(reqs))]


def test_the_payloads_give_the_masks_of_this_file(handler, masks):
    col = handler._collections["u"]
    for flt, key in ((HALF, KH), (DOC5, K5), (DOC9, K9), (NOTHING, KN)):
        assert [FL.matches(col.payloads[r], flt, col.ids[r]) for r in range(N)] == masks[key].tolist()


@pytest.mark.parametrize("using, prefix", [("dense", 0), ("matryoshka_128", 128), ("quantized", 0), ("sparse", 0)])
@pytest.mark.parametrize("flt, key", [(HALF, KH), (DOC5, K5), (NOTHING, KN)], ids=["half", "one-in-32", "nothing"])
def test_a_filtered_nearest_neighbour_search_is_the_brute_force_ranking_of_the_kept_rows(handler, corpus, oracle, masks,
                                                                                         using, prefix, flt, key):
    qs, sps = queries(corpus)
    ora = oracle.ix
    for b in range(B):
        q = sps[b] if using == "sparse" else qs[b]
        got = asyncio.run(handler.query_points("u", query=q, using=using, limit=15, filters=flt, filter_stages="node"))
        if using == "sparse":
            sc, ids = ora.search_sparse(np.asarray(q["indices"]), np.asarray(q["values"], np.float32), N)
        elif using == "quantized":
            sc, ids = ora.search_i8(corpus[4][b], N)
        else:
            sc, ids = ora.search_dense(corpus[4][b], N, prefix)
        ok = masks[key][ids]
        want = [(int(i), bits(s)) for s, i in zip(sc[ok][:15], ids[ok][:15])]
        assert as_rows(handler, [got]) == [want], (using, b)
        assert all(FL.matches(p.payload, flt, p.id) for p in got)
    # "all" on a root without prefetch is the same search
    one = asyncio.run(handler.query_points("u", query=q, using=using, limit=15, filters=flt, filter_stages="all"))
    assert flat([one]) == flat([got])


def test_the_default_still_refuses_a_filter_on_a_root_without_prefetch(handler, corpus):
    qs, _ = queries(corpus, 1)
    with pytest.raises(ValueError, match="without prefetch"):
        asyncio.run(handler.query_points("u", query=qs[0], filters=HALF))
    with pytest.raises(ValueError, match="without prefetch"):
        asyncio.run(handler.query_points_batch("u", [{"query": qs[0], "filters": HALF, "filter_stages": "root"}]))
    with pytest.raises(ValueError, match="take no mask"):
        asyncio.run(handler.query_points("u", query=qs[0], prefetch=[{"query": qs[0], "filter": HALF}]))
    with pytest.raises(ValueError, match="filter_stages='node'"):
        asyncio.run(handler.query_points("u", query=qs[0], filters=HALF, prefetch=[{"query": qs[0], "filter": DOC5}],
                                         filter_stages="all"))


@pytest.mark.parametrize("flt", [HALF, DOC5], ids=["half", "one-in-32"])
def test_the_two_fixed_trees_under_all_equal_hybrid_search_all(handler, corpus, flt):
    qs, sps = queries(corpus)
    for mode, tree in (("tree", reference_tree), ("h1", h1_tree)):
        want = asyncio.run(handler.hybrid_search_batch("u", qs, sps, top_k=P["final_limit"], search_params=P, filters=flt,
                                                       filter_stages="all", mode=mode))
        got = ask(handler, [dict(tree(q, sp), filters=flt) for q, sp in zip(qs, sps)], "all")
        assert len(want) == B and all(len(w) > 0 for w in want)
        assert flat(got) == flat(want), mode


@pytest.mark.parametrize("tree", [wide_fusion, wide_rescore, reference_tree], ids=["fusion", "rescore", "reference"])
@pytest.mark.parametrize("flt", [HALF, DOC5], ids=["half", "one-in-32"])
def test_a_root_only_filter_on_an_input_of_at_most_2048_is_the_same_under_node_and_root(handler, corpus, tree, flt):
    qs, sps = queries(corpus)
    reqs = [tree(q, sp, filters=flt, score_threshold=0.01) for q, sp in zip(qs, sps)]
    assert QT.input_width(QT.parse(reqs[0], DIM, MS)[0]) <= 2048
    root = ask(handler, reqs, "root")
    assert len(root) == B and any(len(r) > 0 for r in root)
    assert flat(ask(handler, reqs, "node")) == flat(root)


def test_a_union_wider_than_2048_is_filtered_whole_before_the_rescore(handler, corpus, oracle, masks):
    """The 2048 + 2048 + 300 root of tests/test_gpu_query_tree.py's wide-input test, and one of 3 x 2048 + 2024: under
    "node" the whole union meets the filter and the kept ids are re-scored -- the oracle filters the full union, then
    re-scores.  (On 2048 rows a union holds at most 2048 distinct ids, so "root" loses nothing HERE and must agree;
    what "node" adds is that this no longer depends on the number of distinct ids.)"""
    qs, sps = queries(corpus, 3)
    trees = (lambda q, sp, **kw: dict({"prefetch": [{"query": q, "limit": 2048},
                                                    {"query": q[:64], "using": "matryoshka_64", "limit": 2048},
                                                    {"query": sp, "using": "sparse", "limit": 300}],
                                       "query": q[:128], "using": "matryoshka_128", "limit": 10}, **kw),
             lambda q, sp, **kw: dict({"prefetch": [{"query": q, "limit": 2048},
                                                    {"query": q[:64], "using": "matryoshka_64", "limit": 2048},
                                                    {"query": q, "using": "quantized", "limit": 2048},
                                                    {"query": sp, "using": "sparse", "limit": 2024}],
                                       "query": q, "using": "dense", "limit": 10}, **kw))
    ora = oracle.ix
    for tree, prefix in zip(trees, (128, 0)):
        reqs = [tree(q, sp, filters=DOC5) for q, sp in zip(qs, sps)]
        width = QT.input_width(QT.parse(reqs[0], DIM, MS)[0])
        assert width > 2048
        got = as_rows(handler, ask(handler, reqs, "node"))
        assert got == oracle_lists(oracle, reqs)
        for b in range(3):                                   # ... and stated without the interpreter
            lists = [ora.search_dense(corpus[4][b], 2048, 0)[1], ora.search_dense(corpus[4][b], 2048, 64)[1]]
            if width > 8000:
                lists.append(ora.search_i8(corpus[4][b], 2048)[1])
            lists.append(ora.search_sparse(np.asarray(sps[b]["indices"]), np.asarray(sps[b]["values"], np.float32),
                                           width - 2048 * len(lists))[1])
            union = np.concatenate(lists)
            sc, ids = ora.rescore(corpus[4][b], union[masks[K5][union]], 10, prefix)
            assert got[b] == [(int(i), bits(s)) for s, i in zip(sc, ids)] and len(got[b]) == 10
        assert got == as_rows(handler, ask(handler, reqs, "root"))


def test_different_filters_on_the_two_prefetches_of_one_fusion_and_thresholds_below_the_root(handler, corpus, oracle, masks):
    qs, sps = queries(corpus)
    reqs = [{"query": {"fusion": "rrf"}, "limit": 20,
             "prefetch": [{"query": q, "limit": 60, "filter": HALF},
                          {"query": sp, "using": "sparse", "limit": 50, "filter": DOC9}]}
            for q, sp in zip(qs, sps)]
    got = as_rows(handler, ask(handler, reqs, "node"))
    assert got == oracle_lists(oracle, reqs)
    rows = {r for l in got for r, _ in l}
    assert any(masks[KH][r] and not masks[K9][r] for r in rows) and any(masks[K9][r] and not masks[KH][r] for r in rows)
    assert all(masks[KH][r] or masks[K9][r] for r in rows)
    # thresholds on a leaf, on a re-scoring node and on a fusion node below a dense root; one per query
    thr = [0.02, 0.05, 0.0, 0.3]
    reqs = [{"query": q, "limit": 12, "filters": HALF,
             "prefetch": [{"query": q[:128], "using": "matryoshka_128", "limit": 40, "score_threshold": 2 * t,
                           "prefetch": [{"query": q, "using": "quantized", "limit": 200, "score_threshold": t,
                                         "filter": DOC9}]},
                          {"query": {"fusion": "dbsf"}, "limit": 30, "score_threshold": 0.5 + t, "filter": HALF,
                           "prefetch": [{"query": q, "limit": 100}, {"query": sp, "using": "sparse", "limit": 100}]}]}
            for q, sp, t in zip(qs, sps, thr)]
    got = as_rows(handler, ask(handler, reqs, "node"))
    want = oracle_lists(oracle, reqs)
    assert got == want and any(len(l) > 0 for l in got)


def test_a_batch_interleaving_three_filters_and_two_shapes_comes_back_in_request_order(handler, corpus):
    qs, sps = queries(corpus)
    flts = (HALF, DOC5, DOC9)
    makers = (lambda b, f: dict(h1_tree(qs[b], sps[b]), filters=f),
              lambda b, f: {"query": qs[b], "limit": 9, "prefetch": [{"query": qs[b], "using": "quantized", "limit": 80,
                                                                      "filter": f}]})
    reqs = [makers[i % 2](i % B, flts[i % 3]) for i in range(12)]
    reqs[5] = dict(reqs[5], filter_stages="root")            # a batch may mix the switch too
    for i, r in enumerate(reqs):
        r.setdefault("filter_stages", "node")
    reqs[5]["prefetch"][0].pop("filter")
    batch = asyncio.run(handler.query_points_batch("u", reqs))
    assert len(batch) == 12 and sum(len(x) > 0 for x in batch) >= 8
    for i, r in enumerate(reqs):
        assert flat(asyncio.run(handler.query_points_batch("u", [r]))) == flat([batch[i]]), i
        flt = flts[i % 3]
        if i % 2 == 0:
            assert all(FL.matches(p.payload, flt, p.id) for p in batch[i])


def with_random_filters(rng, node, depth=1):
    """a copy of the request with node filters drawn from {none, HALF, DOC9, a filter keeping nothing} and thresholds"""
    node = dict(node)
    flt = [None, None, HALF, DOC9, NOTHING][int(rng.integers(5))] if depth > 1 or rng.random() < 0.5 else None
    if flt is not None and not (flt is NOTHING and rng.random() < 0.5):
        node["filters" if depth == 1 else "filter"] = flt
    if rng.random() < 0.3:
        node["score_threshold"] = float(rng.choice([-0.1, 0.0, 0.02, 0.3]))
    if node.get("prefetch"):
        node["prefetch"] = [with_random_filters(rng, c, depth + 1) for c in node["prefetch"]]
    return node


def test_a_dozen_random_trees_with_random_node_filters_equal_the_oracle_node_by_node(eng, handler, corpus, oracle):
    assert not np.isin(T.ABSENT_TERMS, corpus[2]).any()
    col = handler._collections["u"]
    pools = [T.sparse_pool(*corpus[1:4], *corpus[6], b) for b in range(2)]
    flts = {KH: HALF, K9: DOC9, KN: NOTHING}
    reqs, kinds = [], set()
    for seed in range(101, 113):
        def dense(width, count=[0], seed=seed):
            count[0] += 1
            return O.synth_dense(O.SEED_QUERY, 16 * count[0] + seed, 1, DIM)[0, :width].tolist()
        tree = T.random_tree(np.random.default_rng(seed), DIM, MS, dense, lambda kind, s=seed: pools[s % 2][kind],
                             max_nodes=8)
        reqs.append(with_random_filters(np.random.default_rng(1000 + seed), tree))
    for i, req in enumerate(reqs):
        shape, vecs, thrs, _ = QT.parse_nodes(req, DIM, MS)
        vectors, thresholds = QT.batch_vectors([vecs]), QT.batch_thresholds([thrs])
        dev = FilterRecorder(QT.DeviceStages(col.index, eng, masks=lambda key: col.row_mask(flts[key])),
                             to_host=QT.DeviceStages.to_host)
        ora = FilterRecorder(oracle)
        QT.run(shape, vectors, dev, thresholds=thresholds)
        QT.run(shape, vectors, ora, thresholds=thresholds)
        T.assert_same_nodes(dev.nodes, ora.nodes, f"request {i}")
        kinds |= {(k, "mask" in a and a["mask"] is not None) for k, a, _, _ in dev.nodes}
    assert {("keep", True), ("keep", False)} <= kinds and any(m for k, m in kinds if k != "keep"), sorted(kinds)
    got = as_rows(handler, ask(handler, reqs, "node"))
    for i, req in enumerate(reqs):
        assert got[i] == oracle_lists(oracle, [req])[0], i


def test_a_cached_mask_follows_an_upsert_and_a_delete(eng, corpus):
    from rag_application_amd.handler import QdrantHandler
    X, ip, si, sv = corpus[:4]
    n = 256
    h = QdrantHandler()
    try:
        asyncio.run(h.store_document_vectors([chunk(r, X, ip, si, sv) for r in range(n)], "m"))
        flt = {"must": [{"key": "document_id", "match": {"value": "doc1"}}]}
        q = X[300].tolist()                                  # a row the collection does not hold yet
        ask1 = lambda: asyncio.run(h.query_points("m", query=q, limit=5, filters=flt, filter_stages="node",
                                                  prefetch=[{"query": q, "using": "quantized", "limit": 30, "filter": flt}]))
        first = ask1()
        assert len(first) == 5 and all(p.payload["document_id"] == "doc1" for p in first)
        assert FL.filter_key(flt) in h._collections["m"]._masks
        new = chunk(300, X, ip, si, sv)
        new["chunk_metadata"]["document_id"] = "doc1"
        moved = chunk(70, X, ip, si, sv)                     # an existing doc1 row leaves the filter, in place
        moved["chunk_metadata"]["document_id"] = "doc9"
        old70 = h._collections["m"].ids[70]
        assert asyncio.run(h.upsert_points("m", [new, moved], ["new-point", old70])) == 1
        second = ask1()
        assert second[0].id == "new-point" and second[0].score > first[0].score
        assert old70 not in [p.id for p in second]
        assert asyncio.run(h.delete_points("m", point_ids=["new-point"])) == 1
        third = ask1()
        assert "new-point" not in [p.id for p in third] and len(third) == 5
        assert flat([third[:4]]) == flat([second[1:]])       # the ranking of the rows doc1 still holds
    finally:
        asyncio.run(h.delete_collection("m"))
