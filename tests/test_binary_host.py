"""Binary quantization without a GPU: query_tree.parse takes using="binary" as a leaf and nowhere
else, query_tree.run hands the leaf to stages.bin -- checked over the host stage set whose `bin` is the numpy model
(tests/binary_helpers.py) -- DeviceStages.bin calls the engine's search_bin, query_tree.binary_request builds the tree of
search_binary and refuses what it must, and the handlers refuse what they cannot serve."""
from __future__ import annotations

import asyncio

import numpy as np
import pytest

from oracle import oracle as O
from rag_application_amd import query_tree as QT
from rag_application_amd.handler import QdrantHandler, _Collection
from tests import binary_helpers as BH
from tests import query_tree_helpers as T

DIM, MS, N, B = 64, (64,), 300, 3


def vec(seed=0, dim=DIM):
    return np.random.default_rng(seed).standard_normal(dim).astype(np.float32).tolist()


# ---- parsing --------------------------------------------------------------------------------------------------------------
def test_binary_is_a_leaf():
    shape, vecs = QT.parse({"using": "binary", "query": vec(), "limit": 50}, DIM, MS)
    assert shape == ("nearest", "binary", 0, 50, ()) and len(vecs) == 1 and vecs[0].shape == (DIM,)
    assert QT.uses_binary(shape)
    shape, vecs = QT.parse({"using": "dense", "query": vec(1), "prefetch": [{"using": "binary", "query": vec(2), "limit": 40}]},
                           DIM, MS)
    assert shape == ("nearest", "dense", 0, 10, (("nearest", "binary", 0, 40, ()),)) and len(vecs) == 2
    assert QT.uses_binary(shape)
    fused, _ = QT.parse({"query": {"fusion": "dbsf"}, "prefetch": [{"using": "binary", "query": vec()},
                                                                   {"using": "quantized", "query": vec()}]}, DIM, MS)
    assert fused[0] == "fusion" and QT.uses_binary(fused)
    plain, _ = QT.parse({"using": "dense", "query": vec(), "prefetch": [{"using": "quantized", "query": vec()}]}, DIM, MS)
    assert not QT.uses_binary(plain)
    assert "binary" in QT.USINGS


def test_binary_cannot_rescore_and_takes_a_dense_query_of_dim_values():
    with pytest.raises(ValueError, match="using='binary' cannot re-score a prefetch"):
        QT.parse({"using": "binary", "query": vec(), "prefetch": [{"using": "dense", "query": vec()}]}, DIM, MS)
    with pytest.raises(ValueError, match="'quantized', 'sparse' or 'binary'"):
        QT.parse({"using": "ternary", "query": vec()}, DIM, MS)
    with pytest.raises(ValueError, match="needs using='sparse'"):
        QT.parse({"using": "binary", "query": {"indices": [1], "values": [1.0]}}, DIM, MS)
    with pytest.raises(ValueError, match="a query of 32 values under using='binary', want 64"):
        QT.parse({"using": "binary", "query": vec(dim=32)}, DIM, MS)
    bad = vec()
    bad[5] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        QT.parse({"using": "binary", "query": bad}, DIM, MS)


def test_a_binary_leaf_takes_node_filters_and_thresholds():
    flt = {"must": [{"key": "k", "match": {"value": 1}}]}
    shape, vecs, thrs, flts = QT.parse_nodes(
        {"using": "dense", "query": vec(), "prefetch": [{"using": "binary", "query": vec(), "limit": 30, "filter": flt,
                                                         "score_threshold": 12}]}, DIM, MS)
    (key,) = flts
    assert shape[-1] == (("keep", key, True, 30, (("nearest", "binary", 0, 30, ()),)),) and thrs == [np.float32(12)]
    assert QT.uses_binary(shape)
    pushed = QT.push_to_leaves(QT.parse_nodes({"using": "dense", "query": vec(), "filters": flt,
                                               "prefetch": [{"using": "binary", "query": vec(), "limit": 30}]}, DIM, MS,
                                              prefetch_filters=False)[0])
    assert pushed == ("nearest", "dense", 0, 10, (("keep", key, False, 30, (("nearest", "binary", 0, 30, ()),)),))


# ---- run() over the host stages ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(synth_tables):
    rows = T.synth_rows(N, DIM, synth_tables)
    masks = {"even": np.arange(N) % 2 == 0}
    Q = O.synth_dense(O.SEED_QUERY, 0, B, DIM)
    return rows, BH.BinaryOracleStages(rows, DIM, MS, masks), Q


def test_run_hands_the_leaf_to_bin_and_its_list_to_the_node_above(world):
    rows, stages, Q = world
    xb = BH.row_bits(rows[0])
    stages.calls.clear()
    leaf, _ = QT.parse({"using": "binary", "query": Q[0].tolist(), "limit": 25}, DIM, MS)
    BH.assert_same_lists(QT.run(leaf, [Q], stages), BH.search(xb, Q, 25), "the leaf alone")
    assert stages.calls == [("bin", B, 25)]
    # under a dense re-score: the leaf's ids, re-scored by the oracle
    tree, _ = QT.parse({"using": "dense", "query": Q[0].tolist(), "limit": 7,
                        "prefetch": [{"using": "binary", "query": Q[0].tolist(), "limit": 60}]}, DIM, MS)
    keys, cnt = QT.run(tree, [Q, Q], stages)
    lk, lc = BH.search(xb, Q, 60)
    for b in range(B):
        sc, ids = stages.ix.rescore(Q[b], T.key_ids(lk[b, :lc[b]]), 7)
        assert cnt[b] == 7 and keys[b].tolist() == O.order_key(sc, ids).tolist()
    # a root_limit overrides the leaf's
    BH.assert_same_lists(QT.run(leaf, [Q], stages, root_limit=40), BH.search(xb, Q, 40), "root_limit")


def test_run_passes_masks_and_thresholds_of_a_binary_leaf(world):
    rows, stages, Q = world
    xb = BH.row_bits(rows[0])
    even = np.arange(N) % 2 == 0
    shape = ("keep", "even", True, 20, (("nearest", "binary", 0, 20, ()),))
    thr = np.array([4.0, 8.0, -64.0], np.float32)
    stages.calls.clear()
    keys, cnt = QT.run(shape, [Q], stages, thresholds=[thr])
    assert stages.calls[0] == ("bin", B, 20, "even")
    mk, mc = BH.search(xb, Q, 20, even)
    from tests.query_tree_filter_helpers import key_scores
    for b in range(B):
        ok = ~(key_scores(mk[b, :mc[b]]) < thr[b])
        assert keys[b, :cnt[b]].tolist() == mk[b, :mc[b]][ok].tolist() and cnt[b] == int(ok.sum())
    assert cnt[2] == 20                                  # every score is at least -dim
    # a fusion reads the list like any other: ranks for RRF, the integer scores for DBSF
    from rag_application_amd import fusion as F
    for method in ("rrf", "dbsf"):
        tree, _ = QT.parse({"query": {"fusion": method}, "limit": 15,
                            "prefetch": [{"using": "binary", "query": Q[0].tolist(), "limit": 30},
                                         {"using": "quantized", "query": Q[0].tolist(), "limit": 30}]}, DIM, MS)
        got = QT.run(tree, [Q, Q], stages)
        want = F.fuse_keys([BH.search(xb, Q, 30)[0], stages.i8(Q, 30)[0]], [BH.search(xb, Q, 30)[1], stages.i8(Q, 30)[1]],
                           tree[1], None, 15, tree[3], tree[4])
        BH.assert_same_lists(got, want, method)


def test_device_stages_bin_calls_search_bin():
    import torch

    class Index:
        _tdev = torch.device("cpu")

        def __init__(self):
            self.calls = []

        def search_bin(self, q, limit, **kw):
            self.calls.append((tuple(q.shape), q.dtype, limit, sorted(kw)))
            return torch.zeros((q.shape[0], limit), dtype=torch.int64), torch.zeros(q.shape[0], dtype=torch.int32)

    ix = Index()
    stages = QT.DeviceStages(ix, None, masks=lambda key: np.array([0xFFFFFFFF], np.uint32))
    Q = np.zeros((2, DIM), np.float64)
    QT.run(("nearest", "binary", 0, 9, ()), [Q], stages)
    QT.run(("keep", "k", False, 9, (("nearest", "binary", 0, 9, ()),)), [Q], stages)
    assert ix.calls == [((2, DIM), torch.float32, 9, []), ((2, DIM), torch.float32, 9, ["mask"])]


# ---- search_binary's request ------------------------------------------------------------------------------------------------
def test_binary_request_builds_the_two_level_tree():
    q = vec()
    assert QT.binary_request(q) == {"using": "dense", "query": q, "limit": 10,
                                    "prefetch": [{"using": "binary", "query": q, "limit": 40}]}
    assert QT.binary_request(q, 10, 2.05)["prefetch"][0]["limit"] == 21           # ceil
    assert QT.binary_request(q, 7, 1)["prefetch"][0]["limit"] == 7
    assert QT.binary_request(q, 1000, 4.0)["prefetch"][0]["limit"] == 2048        # the widest list a stage keeps
    assert QT.binary_request(q, 2048, 8.0)["prefetch"][0]["limit"] == 2048
    assert QT.binary_request(q, 25, 4.0, rescore=False) == {"using": "binary", "query": q, "limit": 25}
    flt = {"must": [{"key": "k", "match": {"value": 1}}]}
    assert QT.binary_request(q, 5, 2.0, filters=flt)["filters"] == flt
    assert "filters" not in QT.binary_request(q, 5, 2.0, filters=None)
    shape, vecs = QT.parse(QT.binary_request(q, 10, np.float32(3.0)), DIM, MS)
    assert shape == ("nearest", "dense", 0, 10, (("nearest", "binary", 0, 30, ()),)) and len(vecs) == 2


@pytest.mark.parametrize("bad", [0.99, 0, -1.0, float("nan"), float("inf"), -float("inf"), "4", None, True, [4.0]])
def test_binary_request_refuses_an_oversampling_below_one_or_not_finite(bad):
    with pytest.raises(ValueError, match="oversampling"):
        QT.binary_request(vec(), 10, bad)


@pytest.mark.parametrize("bad", [0, -3, 2049, 2.0, "10", None, True])
def test_binary_request_refuses_a_limit_out_of_range(bad):
    with pytest.raises(ValueError, match="limit must be an integer in \\[1, 2048\\]"):
        QT.binary_request(vec(), bad)


# ---- the handlers -----------------------------------------------------------------------------------------------------------
def test_a_collection_without_the_flag_refuses_a_binary_shape():
    col = _Collection.__new__(_Collection)               # made by hand, as older tests make them: no such attribute
    shape, _ = QT.parse({"using": "binary", "query": vec()}, DIM, MS)
    with pytest.raises(ValueError, match="binary_quantization=True"):
        QdrantHandler._check_binary(col, shape)
    col.binary_quantization = True
    QdrantHandler._check_binary(col, shape)
    col.binary_quantization = False
    QdrantHandler._check_binary(col, QT.parse({"using": "dense", "query": vec()}, DIM, MS)[0])


def test_search_binary_checks_its_arguments_before_the_collection():
    h = QdrantHandler()
    with pytest.raises(ValueError, match="filter_stages"):
        asyncio.run(h.search_binary("nobody", vec(), filter_stages="leaf"))
    with pytest.raises(ValueError, match="oversampling"):
        asyncio.run(h.search_binary("nobody", vec(), oversampling=0.5))
    with pytest.raises(ValueError, match="binary_quantization must be True or False"):
        asyncio.run(h.create_collection("u", 4, [], 4, binary_quantization="yes"))


def test_a_sharded_handler_refuses_binary_quantization():
    from rag_application_amd.sharded import ShardedHandler
    h = ShardedHandler.__new__(ShardedHandler)           # (no process group: the refusal comes before any command)
    QdrantHandler.__init__(h)
    h.dim, h.msizes = 4, ()
    with pytest.raises(ValueError, match="binary_quantization=True is not supported on a sharded collection"):
        asyncio.run(h.create_collection("u", binary_quantization=True))
    assert h._collections == {}
