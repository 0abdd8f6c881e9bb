"""GPU: the using="binary" leaf of the query trees and QdrantHandler.search_binary on a collection
created with binary_quantization=True.  Trees with a binary leaf -- under a dense re-score, under an RRF and a DBSF fusion
beside a sparse leaf, with a node filter and with a score_threshold on the leaf -- equal query_tree.run over the host stage
set whose `bin` is the numpy model (tests/binary_helpers.py) and whose other stages are the oracle's.  search_binary equals
the tree written by hand, its rescore=False form the leaf's list, and with an oversampling that covers every row the exact
dense list.  The flag survives save_collection and a reopen; a collection without it and a sharded handler refuse."""
from __future__ import annotations

import asyncio

import numpy as np
import pytest

from oracle import oracle as O
from rag_application_amd import filters as FL
from rag_application_amd import query_tree as QT
from tests import binary_helpers as BH
from tests import fusion_helpers as H
from tests.test_gpu_query_tree import HALF, bits, chunk, flat

pytestmark = pytest.mark.gpu

N, DIM, MS, B = 1500, 768, (64, 128, 256), 4
KH = FL.filter_key(HALF)


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
    return X, ip, si, sv, Q, sparse


@pytest.fixture(scope="module")
def handler(eng, corpus):
    from rag_application_amd.handler import QdrantHandler
    X, ip, si, sv = corpus[:4]
    h = QdrantHandler()
    asyncio.run(h.create_collection("u", DIM, list(MS), DIM, binary_quantization=True))
    asyncio.run(h.store_document_vectors([chunk(r, X, ip, si, sv) for r in range(N)], "u"))
    yield h
    asyncio.run(h.delete_collection("u"))


@pytest.fixture(scope="module")
def model(corpus):
    return BH.BinaryOracleStages(corpus[:4], DIM, MS, {KH: np.arange(N) % 2 == 0}, fuse=H)


def as_rows(handler, res):
    row_of = {pid: r for r, pid in enumerate(handler._collections["u"].ids)}
    return [[(row_of[p.id], bits(p.score)) for p in pts] for pts in res]


def model_lists(model, reqs):
    """query_tree.run over the host stage set, for node-mode requests of ONE shape: per request [(row, score bits)]"""
    parsed = [QT.parse_nodes(r, DIM, MS) for r in reqs]
    assert len({p[0] for p in parsed}) == 1
    keys, cnt = QT.run(parsed[0][0], QT.batch_vectors([p[1] for p in parsed]), model,
                       thresholds=QT.batch_thresholds([p[2] for p in parsed]))
    return [[(H.key_id(int(x)), bits(H.key_score(int(x)))) for x in keys[b, :int(cnt[b])]] for b in range(len(reqs))]


def leaf(q, limit, **kw):
    return dict({"using": "binary", "query": q, "limit": limit}, **kw)


TREES = {
    "under a dense re-score": lambda q, sp: {"using": "dense", "query": q, "limit": 12, "prefetch": [leaf(q, 200)]},
    "under an rrf fusion": lambda q, sp: {"query": {"fusion": "rrf"}, "limit": 30,
                                          "prefetch": [leaf(q, 100), {"using": "sparse", "query": sp, "limit": 50}]},
    "under a dbsf fusion": lambda q, sp: {"query": {"fusion": "dbsf", "weights": [1.0, 0.5]}, "limit": 30,
                                          "prefetch": [leaf(q, 100), {"using": "sparse", "query": sp, "limit": 50}]},
    "a node filter on the leaf": lambda q, sp: {"using": "dense", "query": q, "limit": 12,
                                                "prefetch": [leaf(q, 100, filter=HALF)]},
    "a score_threshold on the leaf": lambda q, sp: {"using": "dense", "query": q, "limit": 2048,
                                                    "prefetch": [leaf(q, 300, score_threshold=56.0)]},
    "the leaf alone": lambda q, sp: leaf(q, 40),
}


@pytest.mark.parametrize("name", list(TREES))
def test_a_tree_with_a_binary_leaf_equals_the_host_stages(handler, corpus, model, name):
    Q, sps = corpus[4], corpus[5]
    reqs = [TREES[name](Q[b].tolist(), sps[b]) for b in range(B)]
    want = model_lists(model, reqs)
    assert any(c[0] == "bin" for c in model.calls) and all(len(w) > 0 for w in want)
    if name == "a score_threshold on the leaf":                    # the threshold cuts inside the leaf's list
        assert all(0 < len(w) < 300 for w in want)
    got = asyncio.run(handler.query_points_batch("u", [dict(r, filter_stages="node") for r in reqs]))
    assert as_rows(handler, got) == want
    if "filter" not in name and "threshold" not in name:           # the default path serves the same tree
        root = asyncio.run(handler.query_points_batch("u", reqs))
        assert as_rows(handler, root) == want
    if "filter" in name:
        assert all(p.payload["page_number"] == 0 for pts in got for p in pts)


def test_search_binary_is_the_two_level_tree(handler, corpus, model):
    Q = corpus[4]
    qs = [Q[b].tolist() for b in range(B)]
    got = asyncio.run(handler.search_binary_batch("u", qs, limit=10, oversampling=4.0))
    hand = asyncio.run(handler.query_points_batch(
        "u", [{"using": "dense", "query": q, "limit": 10, "prefetch": [leaf(q, 40)]} for q in qs]))
    assert flat(got) == flat(hand) and all(len(g) == 10 for g in got)
    want = model_lists(model, [{"using": "dense", "query": q, "limit": 10, "prefetch": [leaf(q, 40)]} for q in qs])
    assert as_rows(handler, got) == want
    one = asyncio.run(handler.search_binary("u", qs[2], limit=10, oversampling=4.0))
    assert flat([one]) == flat([got[2]])
    # ceil(limit * oversampling): 10 * 2.05 -> 21 candidates
    got21 = asyncio.run(handler.search_binary_batch("u", qs, limit=10, oversampling=2.05))
    assert as_rows(handler, got21) == model_lists(
        model, [{"using": "dense", "query": q, "limit": 10, "prefetch": [leaf(q, 21)]} for q in qs])


def test_search_binary_without_rescore_is_the_leafs_list(handler, corpus):
    Q = corpus[4]
    got = asyncio.run(handler.search_binary_batch("u", [Q[b].tolist() for b in range(B)], limit=25, rescore=False))
    keys, cnt = BH.search(BH.row_bits(corpus[0]), Q, 25)
    want = [[(H.key_id(int(x)), bits(H.key_score(int(x)))) for x in keys[b, :int(cnt[b])]] for b in range(B)]
    assert as_rows(handler, got) == want
    assert all(float(p.score) == int(p.score) and -DIM <= p.score <= DIM for pts in got for p in pts)


def test_an_oversampling_that_covers_every_row_gives_the_exact_dense_list(handler, corpus):
    """N <= 2048, so ceil(limit * oversampling) reaches every row: the re-scored result is hx_search_dense's list."""
    Q = corpus[4]
    qs = [Q[b].tolist() for b in range(B)]
    got = asyncio.run(handler.search_binary_batch("u", qs, limit=10, oversampling=N / 10))
    exact = asyncio.run(handler.query_points_batch("u", [{"using": "dense", "query": q, "limit": 10} for q in qs]))
    assert flat(got) == flat(exact) and all(len(g) == 10 for g in got)


def test_search_binary_refuses_bad_arguments(handler, corpus):
    q = corpus[4][0].tolist()
    for bad in (0.5, float("nan"), float("inf"), "4", None, True):
        with pytest.raises(ValueError, match="oversampling"):
            asyncio.run(handler.search_binary("u", q, oversampling=bad))
    for bad in (0, 2049, 2.5):
        with pytest.raises(ValueError, match="limit"):
            asyncio.run(handler.search_binary("u", q, limit=bad))


def test_the_flag_survives_save_and_reopen(eng, corpus, tmp_path):
    from rag_application_amd.handler import QdrantHandler
    X, ip, si, sv, Q = corpus[:5]
    n = 300
    h = QdrantHandler(persist_dir=str(tmp_path))
    asyncio.run(h.create_collection("s", DIM, list(MS), DIM, binary_quantization=True))
    asyncio.run(h.store_document_vectors([chunk(r, X, ip, si, sv) for r in range(n)], "s"))
    before = asyncio.run(h.search_binary("s", Q[0].tolist(), limit=5, rescore=False))
    asyncio.run(h.save_collection("s"))
    with pytest.raises(ValueError, match="binary_quantization"):
        asyncio.run(h.create_collection("s", DIM, list(MS), DIM))          # live: the flag cannot change
    h._collections.pop("s").close()                                        # (delete_collection would remove the files)
    h2 = QdrantHandler(persist_dir=str(tmp_path))
    with pytest.raises(ValueError, match="stored collection"):
        asyncio.run(h2.create_collection("s", DIM, list(MS), DIM))         # stored: neither
    asyncio.run(h2.create_collection("s", DIM, list(MS), DIM, binary_quantization=True))
    col = h2._collections["s"]
    assert col.binary_quantization and col.index.binary_enabled() and col.index.count() == n
    assert np.array_equal(np.stack([col.index.binary_row(r) for r in range(n)]), BH.words(BH.row_bits(X[:n])))
    after = asyncio.run(h2.search_binary("s", Q[0].tolist(), limit=5, rescore=False))
    assert flat([after]) == flat([before]) and len(after) == 5
    col.close()


def test_a_collection_without_the_flag_refuses_a_binary_node(eng, corpus):
    from rag_application_amd.handler import QdrantHandler
    X, ip, si, sv, Q = corpus[:5]
    h = QdrantHandler()
    asyncio.run(h.store_document_vectors([chunk(r, X, ip, si, sv) for r in range(40)], "p"))
    try:
        assert not h._collections["p"].index.binary_enabled()
        q = Q[0].tolist()
        for how in ("root", "node", "all"):
            with pytest.raises(ValueError, match="binary_quantization=True"):
                asyncio.run(h.query_points("p", query=q, using="binary", filter_stages=how))
        with pytest.raises(ValueError, match="binary_quantization=True"):
            asyncio.run(h.query_points("p", query=q, prefetch=[leaf(q, 20)]))
        with pytest.raises(ValueError, match="binary_quantization=True"):
            asyncio.run(h.search_binary("p", q))
        assert len(asyncio.run(h.query_points("p", query=q, limit=5))) == 5
    finally:
        asyncio.run(h.delete_collection("p"))


def test_a_sharded_handler_refuses_the_flag():
    from rag_application_amd.handler import QdrantHandler
    from rag_application_amd.sharded import ShardedHandler
    h = ShardedHandler.__new__(ShardedHandler)          # (no process group: the refusal comes before any command)
    QdrantHandler.__init__(h)
    h.dim, h.msizes = 4, ()
    with pytest.raises(ValueError, match="not supported on a sharded collection"):
        asyncio.run(h.create_collection("u", binary_quantization=True))
    assert h._collections == {}
