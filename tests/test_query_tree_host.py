"""CPU: rag_application_amd/query_tree.py -- parsing, defaults and every refusal of a caller-defined query tree; grouping
by shape; and the interpreter end to end over a stub whose stages are OracleIndex's (fusion by fusion.py): the
reference's tree written as a request equals oracle.hybrid_tree, the H1 tree equals oracle.hybrid_h1, in ids and
scores, on the rows of tests/golden/corpus_b_4096x64.npz."""
from __future__ import annotations

import os
from types import SimpleNamespace as NS

import numpy as np
import pytest

from oracle import oracle as O
from rag_application_amd import fusion as F
from rag_application_amd import query_tree as QT
from tests.query_tree_helpers import OracleStages

DIM, MS = 64, (16, 32)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corpus_b_4096x64.npz")
V = [0.5] * DIM
SP = {"indices": [3, 9], "values": [1.0, 0.5]}


def parse(req):
    return QT.parse(req, DIM, MS)


# ---- parsing and defaults ---------------------------------------------------------------------------------------------------
def test_a_leaf_its_defaults_and_the_attribute_form():
    shape, vecs = parse({"query": V})
    assert shape == ("nearest", "dense", 0, QT.PREFETCH_DEFAULT_LIMIT, ()) and QT.PREFETCH_DEFAULT_LIMIT == 10
    assert vecs[0].dtype == np.float32 and vecs[0].shape == (DIM,)
    assert parse(NS(query=V, using="quantized", limit=7, prefetch=None))[0] == ("nearest", "quantized", 0, 7, ())
    shape, vecs = parse({"query": NS(indices=[1, 2], values=[0.5, 2.0]), "using": "sparse", "limit": 5})
    assert shape == ("nearest", "sparse", 0, 5, ()) and vecs[0][0].tolist() == [1, 2] and vecs[0][1].dtype == np.float32
    assert parse({"query": {"nearest": V}, "limit": 3})[0] == ("nearest", "dense", 0, 3, ())


def test_a_matryoshka_vector_is_padded_to_the_full_width():
    shape, vecs = parse({"query": [1.0] * 16, "using": "matryoshka_16", "limit": 4})
    assert shape == ("nearest", "matryoshka_16", 16, 4, ())
    assert vecs[0].shape == (DIM,) and vecs[0][:16].tolist() == [1.0] * 16 and not vecs[0][16:].any()
    assert parse({"query": V, "using": "matryoshka_32"})[0][2] == 32            # the full vector is taken as it is


def test_a_fusion_node_its_defaults_and_the_order_of_the_vectors():
    req = {"prefetch": [{"query": V, "limit": 20, "prefetch": {"query": [2.0] * 16, "using": "matryoshka_16", "limit": 50}},
                        {"query": SP, "using": "sparse", "limit": 30}],
           "query": {"fusion": "dbsf", "weights": [1, 0.5]}}
    shape, vecs = parse(req)
    assert shape == ("fusion", F.DBSF, (1.0, 0.5), 2.0, 0, 10,
                     (("nearest", "dense", 0, 20, (("nearest", "matryoshka_16", 16, 50, ()),)),
                      ("nearest", "sparse", 0, 30, ())))
    assert len(vecs) == 3 and vecs[0][0] == 0.5 and vecs[1][0] == 2.0 and isinstance(vecs[2], tuple)   # pre-order
    s = parse({"prefetch": [{"query": V}], "query": NS(fusion=NS(value="rrf"))})[0]                   # Fusion.RRF-like
    assert s[:6] == ("fusion", F.RRF, None, 2.0, 0, 10)
    s = parse({"prefetch": [{"query": V}], "query": {"fusion": "rrf", "rrf_k": 60, "rank_base": 1}, "limit": 5})[0]
    assert s[:6] == ("fusion", F.RRF, None, 60.0, 1, 5)
    assert QT.shape_limit(shape) == 10 and QT.input_width(shape) == 50


def nest(depth):
    node = {"query": V}
    for _ in range(depth - 1):
        node = {"query": V, "prefetch": [node]}
    return node


REFUSED = {
    "no query": {"prefetch": [{"query": V}]},
    "not a node": [1, 2, 3],
    "unknown field": {"query": V, "offset": 3},
    "unknown using": {"query": V, "using": "image"},
    "matryoshka size the collection lacks": {"query": V, "using": "matryoshka_64"},
    "wrong width": {"query": [1.0] * 5},
    "wrong prefix width": {"query": [1.0] * 8, "using": "matryoshka_16"},
    "non-finite": {"query": [float("nan")] * DIM},
    "sparse query under dense": {"query": SP},
    "dense query under sparse": {"query": V, "using": "sparse"},
    "sparse lengths": {"query": {"indices": [1], "values": [1.0, 2.0]}, "using": "sparse"},
    "limit 0": {"query": V, "limit": 0},
    "limit above 2048": {"query": V, "limit": 2049},
    "limit not an integer": {"query": V, "limit": 2.5},
    "quantized re-scoring": {"query": V, "using": "quantized", "prefetch": [{"query": V}]},
    "sparse re-scoring": {"query": SP, "using": "sparse", "prefetch": [{"query": V}]},
    "union too wide": {"query": V, "prefetch": [{"query": V, "limit": 2048}] * 5},
    "fusion without prefetch": {"query": {"fusion": "rrf"}},
    "fusion of nine": {"query": {"fusion": "rrf"}, "prefetch": [{"query": V}] * 9},
    "fusion too wide": {"query": {"fusion": "rrf"}, "prefetch": [{"query": V, "limit": 2048}] * 3},
    "unknown fusion": {"query": {"fusion": "max"}, "prefetch": [{"query": V}]},
    "unknown fusion field": {"query": {"fusion": "rrf", "k": 3}, "prefetch": [{"query": V}]},
    "weights count": {"query": {"fusion": "rrf", "weights": [1]}, "prefetch": [{"query": V}] * 2},
    "negative weight": {"query": {"fusion": "dbsf", "weights": [1, -1]}, "prefetch": [{"query": V}] * 2},
    "nan weight": {"query": {"fusion": "dbsf", "weights": [1, float("nan")]}, "prefetch": [{"query": V}] * 2},
    "rrf_k 0": {"query": {"fusion": "rrf", "rrf_k": 0}, "prefetch": [{"query": V}]},
    "rank_base negative": {"query": {"fusion": "rrf", "rank_base": -1}, "prefetch": [{"query": V}]},
    "order_by": {"query": {"order_by": "page_number"}},
    "recommend": {"query": {"recommend": {"positive": [1]}}},
    "discover": {"query": {"discover": {"target": 1}}},
    "context": {"query": {"context": []}},
    "formula": {"query": {"formula": {"sum": []}}, "prefetch": [{"query": V}]},
    "mmr": {"query": {"nearest": V, "mmr": {"diversity": 0.5}}},
    "sample": {"query": {"sample": "random"}},
    "point id": {"query": 17},
    "prefetch filter": {"query": V, "prefetch": [{"query": V, "filter": {"must": []}}]},
    "prefetch filters": {"query": V, "prefetch": [{"query": V, "filters": {"must": [{"key": "a", "match": {"value": 1}}]}}]},
    "inner score_threshold": {"query": V, "prefetch": [{"query": V, "score_threshold": 0.5}]},
    "lookup_from": {"query": V, "lookup_from": {"collection": "x"}},
    "nine levels": nest(9),
    "object with a recommend query": NS(query=NS(recommend=NS(positive=[1])), prefetch=None, using=None, limit=None),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_every_refusal_is_a_value_error_with_a_reason(name):
    with pytest.raises(ValueError) as e:
        parse(REFUSED[name])
    assert len(str(e.value)) > 10


def test_eight_levels_and_the_root_fields_pass():
    assert parse(nest(8))[0][0] == "nearest"
    parse({"query": V, "prefetch": [{"query": V}], "filters": {"must": []}, "score_threshold": 0.1, "with_payload": False})
    assert parse({"query": {"fusion": "dbsf", "rrf_k": float("nan")}, "prefetch": [{"query": V}]})   # DBSF ignores rrf_k


def test_grouping_by_shape_keeps_request_order():
    a, b, c = {"query": V}, {"query": V, "limit": 3}, {"query": SP, "using": "sparse"}
    shapes = [parse(r)[0] for r in (a, b, c, b, a, a, c)]
    groups = QT.group_by_shape(shapes)
    assert list(groups.values()) == [[0, 4, 5], [1, 3], [2, 6]]
    vecs = QT.batch_vectors([parse(r)[1] for r in (a, a, a)])
    assert vecs[0].shape == (3, DIM)
    vecs = QT.batch_vectors([parse(r)[1] for r in (c, c)])
    assert len(vecs[0]) == 2 and vecs[0][0][0].tolist() == [3, 9]


def test_a_sharded_collection_refuses_both_calls():
    import asyncio
    from rag_application_amd.handler import QdrantHandler
    from rag_application_amd.sharded import ShardedHandler
    assert QdrantHandler._query_tree is True and ShardedHandler._query_tree is False
    h = QdrantHandler()
    h._query_tree = False                                   # what ShardedHandler sets
    with pytest.raises(ValueError, match="sharded"):
        asyncio.run(h.query_points("u", query=V))
    with pytest.raises(ValueError, match="sharded"):
        asyncio.run(h.query_points_batch("u", [{"query": V}]))


# ---- the interpreter over the oracle's stages --------------------------------------------------------------------------------
# OracleStages (tests/query_tree_helpers.py): query_tree's stage interface over an OracleIndex, fusion by fusion.py


B = 4
P = dict(matryoshka_16_limit=120, matryoshka_32_limit=80, dense_limit=40, quantized_limit=60, sparse_limit=50,
         final_limit=12, hnsw_ef=128)


@pytest.fixture(scope="module")
def world(synth_tables):
    n = 4096
    ix = O.OracleIndex(DIM, MS)
    ip, si, sv = O.synth_sparse_docs(O.SEED_SPDOC, 0, n, synth_tables)
    ix.add(O.synth_dense(O.SEED_CORPUS, 0, n, DIM), ip, si, sv)
    ix.finalize()
    Q = O.synth_dense(O.SEED_QUERY, 0, B, DIM)
    qip, qsi, qsv = O.synth_sparse_queries(O.SEED_SPQUERY, 0, B, synth_tables)
    sparse = [{"indices": qsi[qip[b]:qip[b + 1]].tolist(), "values": qsv[qip[b]:qip[b + 1]].tolist()} for b in range(B)]
    return ix, Q, sparse


def reference_tree(q, sp, p=P):
    """qdrant_handler.py:305-372 as a request: the matryoshka cascade under a dense stage, the quantized list refined by
    dense and the sparse list fused by RRF (no limit: 10), the union re-scored by dense at the root"""
    q = list(map(float, q))
    cascade = {"query": q[:16], "using": "matryoshka_16", "limit": p["matryoshka_16_limit"]}
    cascade = {"prefetch": [cascade], "query": q[:32], "using": "matryoshka_32", "limit": p["matryoshka_32_limit"]}
    cascade = {"prefetch": [cascade], "query": q, "using": "dense", "limit": p["dense_limit"]}
    quant = {"prefetch": [{"query": q, "using": "quantized", "limit": p["quantized_limit"]}], "query": q, "using": "dense",
             "limit": p["dense_limit"]}
    sparse = {"query": sp, "using": "sparse", "limit": p["sparse_limit"]}
    fusion = {"prefetch": [quant, sparse], "query": {"fusion": "rrf"}}
    return {"prefetch": [cascade, fusion], "query": q, "using": "dense", "limit": p["final_limit"]}


def h1_tree(q, sp, dense_limit=100, sparse_limit=100, limit=10):
    return {"prefetch": [{"query": list(map(float, q)), "using": "dense", "limit": dense_limit},
                         {"query": sp, "using": "sparse", "limit": sparse_limit}],
            "query": {"fusion": "rrf"}, "limit": limit}


def run_batch(ix, requests):
    parsed = [QT.parse(r, DIM, MS) for r in requests]
    groups = QT.group_by_shape([s for s, _ in parsed])
    assert len(groups) == 1
    st = OracleStages(ix)
    keys, cnt = QT.run(parsed[0][0], QT.batch_vectors([v for _, v in parsed]), st)
    return keys, cnt, st


def test_the_reference_tree_as_a_request_is_the_oracles_hybrid_tree(world):
    ix, Q, sparse = world
    keys, cnt, st = run_batch(ix, [reference_tree(Q[b], sparse[b]) for b in range(B)])
    assert all(c[1] == B for c in st.calls) and len(st.calls) == 8           # one batch per stage, no stage twice
    for b in range(B):
        sc, ids = O.hybrid_tree(ix, Q[b], sparse[b]["indices"], sparse[b]["values"], P)
        assert cnt[b] == len(ids) == P["final_limit"]
        assert F.key_ids(keys[b, :cnt[b]]).tolist() == ids.tolist()
        assert F.key_scores(keys[b, :cnt[b]]).view(np.uint32).tolist() == sc.view(np.uint32).tolist()


def test_the_h1_tree_is_the_oracles_hybrid_h1(world):
    ix, Q, sparse = world
    keys, cnt, _ = run_batch(ix, [h1_tree(Q[b], sparse[b]) for b in range(B)])
    for b in range(B):
        sc, ids = O.hybrid_h1(ix, Q[b], sparse[b]["indices"], sparse[b]["values"])
        assert cnt[b] == len(ids)
        assert F.key_ids(keys[b, :cnt[b]]).tolist() == ids.tolist()
        assert F.key_scores(keys[b, :cnt[b]]).view(np.uint32).tolist() == sc.view(np.uint32).tolist()


def test_a_dense_leaf_gives_the_golden_lists_and_root_limit_overrides_the_roots(world):
    ix, Q, _ = world
    gold = np.load(GOLD)
    parsed = [QT.parse({"query": Q[b].tolist(), "limit": 10}, DIM, MS) for b in range(B)]
    vecs = QT.batch_vectors([v for _, v in parsed])
    keys, cnt = QT.run(parsed[0][0], vecs, OracleStages(ix))
    for b in range(B):
        n = int(gold["dense_cnt"][b])
        assert cnt[b] == n and F.key_ids(keys[b, :n]).tolist() == gold["dense_ids"][b, :n].tolist()
        assert F.key_scores(keys[b, :n]).view(np.uint32).tolist() == gold["dense_bits"][b, :n].tolist()
    wide, wcnt = QT.run(parsed[0][0], vecs, OracleStages(ix), root_limit=25)
    assert wide.shape == (B, 25) and (wcnt == 25).all() and np.array_equal(wide[:, :10], keys)
