"""CPU: node filters of the query trees -- query_tree.parse_nodes, its refusals and the shape it
gives; the default parse unchanged; grouping (filters split groups, thresholds do not); and the interpreter's node rules
over FilteredOracleStages (tests/query_tree_filter_helpers.py) on 300 rows of dim 192 with prefixes (64, 128), each checked
against an independent statement: the oracle's FULL ranking filtered and cut, the union filtered before the re-score, the
fusion filtered behind its ranks."""
from __future__ import annotations

import asyncio

import numpy as np
import pytest

from oracle import oracle as O
from rag_application_amd import filters as FL
from rag_application_amd import fusion as F
from rag_application_amd import query_tree as QT
from tests.query_tree_filter_helpers import FilteredOracleStages, key_scores, list_keep_model
from tests.query_tree_helpers import key_ids, oracle_index, synth_rows
from tests.test_query_tree_host import REFUSED

N, DIM, MS = 300, 192, (64, 128)
V = [0.25] * DIM
SP = {"indices": [3, 9], "values": [1.0, 0.5]}
HALF = {"must": [{"key": "page_number", "match": {"value": 0}}]}
DOC2 = {"must": [{"key": "document_id", "match": {"value": "doc2"}}]}
NONE = {"must": [{"key": "document_id", "match": {"value": "no such document"}}]}
KH, KD, KN = FL.filter_key(HALF), FL.filter_key(DOC2), FL.filter_key(NONE)


def nodes(req, **kw):
    return QT.parse_nodes(req, DIM, MS, **kw)


# ---- parsing ----------------------------------------------------------------------------------------------------------------
def test_a_tree_without_filters_or_thresholds_has_todays_shape():
    req = {"query": {"fusion": "rrf"}, "prefetch": [{"query": V, "limit": 20}, {"query": SP, "using": "sparse"}]}
    shape, vecs, thrs, flts = nodes(req)
    assert shape == QT.parse(req, DIM, MS)[0] and thrs == [] and flts == {} and len(vecs) == 2
    assert nodes({"query": V, "filters": {}, "filter": None})[0] == ("nearest", "dense", 0, 10, ())   # an empty filter is none


def test_filters_and_thresholds_at_any_depth_wrap_their_node():
    req = {"query": V, "limit": 5, "filters": HALF, "score_threshold": 0.5,
           "prefetch": [{"query": V[:128], "using": "matryoshka_128", "limit": 20, "filter": DOC2},
                        {"query": {"fusion": "dbsf"}, "limit": 9, "filters": HALF, "score_threshold": 2,
                         "prefetch": [{"query": SP, "using": "sparse", "limit": 7, "score_threshold": -1.5}]}]}
    shape, vecs, thrs, flts = nodes(req)
    leaf_m = ("keep", KD, False, 20, (("nearest", "matryoshka_128", 128, 20, ()),))
    leaf_s = ("keep", None, True, 7, (("nearest", "sparse", 0, 7, ()),))
    fus = ("keep", KH, True, 9, (("fusion", F.DBSF, None, 2.0, 0, 9, (leaf_s,)),))
    assert shape == ("keep", KH, True, 5, (("nearest", "dense", 0, 5, (leaf_m, fus)),))
    assert [float(t) for t in thrs] == [0.5, 2.0, -1.5] and all(t.dtype == np.float32 for t in thrs)      # pre-order
    assert flts == {KH: HALF, KD: DOC2} and len(vecs) == 3
    assert QT.shape_limit(shape) == 5 and QT.shape_limit(fus) == 9


REFUSED_NODES = {
    "a bad clause at the root": ({"query": V, "filters": {"musst": []}}, {}),
    "a bad condition in a prefetch": ({"query": V, "prefetch": [{"query": V, "filter": {"must": [{"keyy": "a"}]}}]}, {}),
    "a filter that is no dict": ({"query": V, "prefetch": [{"query": V, "filter": [1]}]}, {}),
    "a threshold that is a string": ({"query": V, "prefetch": [{"query": V, "score_threshold": "0.5"}]}, {}),
    "a threshold that is a bool": ({"query": V, "score_threshold": True}, {}),
    "a NaN threshold": ({"query": V, "score_threshold": float("nan")}, {}),
    "a prefetch filter under 'all'": ({"query": V, "filters": HALF, "prefetch": [{"query": V, "filter": DOC2}]},
                                      {"prefetch_filters": False}),
}


@pytest.mark.parametrize("name", list(REFUSED_NODES))
def test_node_mode_refusals_are_value_errors_with_a_reason(name):
    req, kw = REFUSED_NODES[name]
    with pytest.raises(ValueError) as e:
        nodes(req, **kw)
    assert len(str(e.value)) > 10


def test_node_mode_still_refuses_what_parse_refuses_for_other_reasons():
    for name, req in REFUSED.items():
        if name in ("prefetch filter", "prefetch filters", "inner score_threshold"):
            QT.parse_nodes(req, 64, (16, 32))                # ... and takes exactly these three
            continue
        with pytest.raises(ValueError):
            QT.parse_nodes(req, 64, (16, 32))


@pytest.mark.parametrize("name", list(REFUSED))
def test_the_default_parse_refuses_what_it_refused(name):
    with pytest.raises(ValueError):
        QT.parse(REFUSED[name], 64, (16, 32))


def test_the_default_parse_names_the_mask_for_a_prefetch_filter():
    with pytest.raises(ValueError, match="take no mask"):
        QT.parse(REFUSED["prefetch filter"], 64, (16, 32))
    with pytest.raises(ValueError, match="belongs to the root"):
        QT.parse(REFUSED["inner score_threshold"], 64, (16, 32))


def test_unknown_filter_stages_and_mask_with_flag_are_value_errors():
    from rag_application_amd import engine
    from rag_application_amd.handler import QdrantHandler
    h = QdrantHandler()
    with pytest.raises(ValueError, match="filter_stages"):
        asyncio.run(h.query_points("u", query=V, filter_stages="leaf"))
    with pytest.raises(ValueError, match="filter_stages"):
        asyncio.run(h.query_points_batch("u", [{"query": V, "filter_stages": "every"}]))
    for call in (lambda: engine.HxIndex.search_dense(None, None, 10, 0, flag=object(), mask=object()),
                 lambda: engine.HxIndex.search_i8(None, None, 10, flag=object(), mask=object()),
                 lambda: engine.HxIndex.search_sparse(None, None, None, None, 10, flag=object(), mask=object())):
        with pytest.raises(ValueError, match="mask and flag"):
            call()


def test_all_pushes_the_roots_filter_into_every_leaf_and_keeps_the_roots_threshold():
    req = {"query": {"fusion": "rrf"}, "filters": HALF, "score_threshold": 0.1, "limit": 4,
           "prefetch": [{"query": V, "limit": 20, "score_threshold": 3},
                        {"query": V, "limit": 6, "prefetch": [{"query": V, "using": "quantized"}]}]}
    shape = QT.push_to_leaves(nodes(req, prefetch_filters=False)[0])
    a = ("keep", KH, True, 20, (("nearest", "dense", 0, 20, ()),))
    b = ("nearest", "dense", 0, 6, (("keep", KH, False, 10, (("nearest", "quantized", 0, 10, ()),)),))
    assert shape == ("keep", None, True, 4, (("fusion", F.RRF, None, 2.0, 0, 4, (a, b)),))
    leaf = QT.push_to_leaves(nodes({"query": V, "filters": DOC2, "score_threshold": 1}, prefetch_filters=False)[0])
    assert leaf == ("keep", KD, True, 10, (("nearest", "dense", 0, 10, ()),))
    plain = nodes({"query": V, "prefetch": [{"query": V}]})[0]
    assert QT.push_to_leaves(plain) is plain


def test_filters_split_groups_and_thresholds_do_not():
    def req(flt, thr):
        return {"query": V, "prefetch": [{"query": V, "filter": flt, "score_threshold": thr, "limit": 30}]}
    parsed = [nodes(req(f, t)) for f, t in ((HALF, 0.1), (DOC2, 0.1), (HALF, 0.7), (HALF, -3), (DOC2, 9))]
    groups = QT.group_by_shape([p[0] for p in parsed])
    assert list(groups.values()) == [[0, 2, 3], [1, 4]]
    thr = QT.batch_thresholds([parsed[i][2] for i in (0, 2, 3)])
    assert len(thr) == 1 and thr[0].dtype == np.float32 and thr[0].tolist() == [np.float32(0.1), np.float32(0.7), -3.0]
    assert QT.batch_thresholds([[], []]) == []


# ---- the interpreter --------------------------------------------------------------------------------------------------------
B = 3


@pytest.fixture(scope="module")
def world(synth_tables):
    rows = synth_rows(N, DIM, synth_tables)
    r = np.arange(N)
    masks = {KH: r % 2 == 0, KD: r // 64 == 2, KN: np.zeros(N, bool)}
    ora = oracle_index(rows, DIM, MS)
    Q = O.synth_dense(O.SEED_QUERY, 0, B, DIM)
    qip, qsi, qsv = O.synth_sparse_queries(O.SEED_SPQUERY, 0, B, synth_tables)
    sparse = [{"indices": qsi[qip[b]:qip[b + 1]].tolist(), "values": qsv[qip[b]:qip[b + 1]].tolist()} for b in range(B)]
    return rows, masks, ora, Q, sparse


def run(world, requests, how="node"):
    rows, masks, ora, _, _ = world
    parsed = [nodes(r, prefetch_filters=how == "node") for r in requests]
    shapes = [QT.push_to_leaves(p[0]) if how == "all" else p[0] for p in parsed]
    assert len(set(shapes)) == 1
    st = FilteredOracleStages(rows, DIM, MS, masks, ix=ora)
    keys, cnt = QT.run(shapes[0], QT.batch_vectors([p[1] for p in parsed]), st,
                       thresholds=QT.batch_thresholds([p[2] for p in parsed]))
    return keys, cnt, st


def same(keys, cnt, b, scores, ids):
    m = len(ids)
    assert cnt[b] == m, (b, int(cnt[b]), m)
    assert key_ids(keys[b, :m]).tolist() == np.asarray(ids).tolist()
    assert key_scores(keys[b, :m]).view(np.uint32).tolist() == np.asarray(scores, np.float32).view(np.uint32).tolist()
    assert not keys[b, m:].any()


LEAVES = (("dense", 0), ("matryoshka_64", 64), ("matryoshka_128", 128), ("quantized", 0), ("sparse", 0))


@pytest.mark.parametrize("using, prefix", LEAVES)
@pytest.mark.parametrize("fkey, flt", [(KH, HALF), (KD, DOC2), (KN, NONE)])
def test_a_masked_leaf_is_the_full_ranking_filtered_and_cut(world, using, prefix, fkey, flt):
    _, masks, ora, Q, sparse = world
    limit = 17
    reqs = [{"query": sparse[b] if using == "sparse" else Q[b].tolist(), "using": using, "limit": limit, "filters": flt}
            for b in range(B)]
    keys, cnt, st = run(world, reqs)
    assert len(st.calls) == 1 and st.calls[0][-1] == fkey and st.calls[0][1:3] == (B, limit)   # one masked stage call
    for b in range(B):
        if using == "sparse":
            sc, ids = ora.search_sparse(np.asarray(sparse[b]["indices"]), np.asarray(sparse[b]["values"], np.float32), N)
        elif using == "quantized":
            sc, ids = ora.search_i8(Q[b], N)
        else:
            sc, ids = ora.search_dense(Q[b], N, prefix)
        ok = masks[fkey][ids]
        same(keys, cnt, b, sc[ok][:limit], ids[ok][:limit])


def test_a_rescoring_nodes_filter_is_applied_to_the_whole_union_before_the_rescore(world):
    _, masks, ora, Q, sparse = world
    reqs = [{"query": Q[b].tolist(), "using": "matryoshka_128", "limit": 12, "filters": DOC2, "score_threshold": 0.05,
             "prefetch": [{"query": Q[b].tolist(), "using": "quantized", "limit": 150},
                          {"query": sparse[b], "using": "sparse", "limit": 120}]} for b in range(B)]
    keys, cnt, st = run(world, reqs)
    assert [c[0] for c in st.calls] == ["i8", "sparse", "keep", "rescore", "keep"]
    assert st.calls[2] == ("keep", B, 270, KD, False) and st.calls[4] == ("keep", B, 12, None, True)
    for b in range(B):
        _, a = ora.search_i8(Q[b], 150)
        _, s = ora.search_sparse(np.asarray(sparse[b]["indices"]), np.asarray(sparse[b]["values"], np.float32), 120)
        union = np.concatenate([a, s])
        sc, ids = ora.rescore(Q[b], union[masks[KD][union]], 12, 128)
        ok = ~(sc < np.float32(0.05))
        same(keys, cnt, b, sc[ok], ids[ok])


def test_a_fusion_nodes_filter_follows_the_fusion_and_shares_its_keep_with_the_threshold(world):
    _, masks, ora, Q, sparse = world
    thr = [0.4, 0.0, 9.0]
    reqs = [{"query": {"fusion": "rrf"}, "limit": 8, "filters": HALF, "score_threshold": thr[b],
             "prefetch": [{"query": Q[b].tolist(), "limit": 40}, {"query": sparse[b], "using": "sparse", "limit": 30}]}
            for b in range(B)]
    keys, cnt, st = run(world, reqs)
    assert [c[0] for c in st.calls] == ["dense", "sparse", "fuse", "keep"]
    assert st.calls[2][2] == 70 and st.calls[3] == ("keep", B, 8, KH, True)
    for b in range(B):
        fs, fi = O.hybrid_h1(ora, Q[b], sparse[b]["indices"], sparse[b]["values"], 40, 30, 70)
        ok = masks[KH][fi] & ~(fs < np.float32(thr[b]))
        same(keys, cnt, b, fs[ok][:8], fi[ok][:8])
    assert cnt[2] == 0                                       # no fused score reaches 9


def test_all_equals_the_whole_tree_on_an_index_of_the_kept_rows(world):
    rows, masks, ora, Q, sparse = world
    def tree(b, **root):
        q = Q[b].tolist()
        return dict({"query": q, "limit": 9, "prefetch": [
            {"query": q, "using": "matryoshka_128", "limit": 30, "prefetch": [{"query": q, "using": "matryoshka_64", "limit": 60}]},
            {"query": {"fusion": "rrf"}, "prefetch": [{"query": q, "using": "quantized", "limit": 25},
                                                      {"query": sparse[b], "using": "sparse", "limit": 25}]}]}, **root)
    keys, cnt, _ = run(world, [tree(b, filters=HALF) for b in range(B)], how="all")
    kept = np.flatnonzero(masks[KH])
    from tests.query_tree_filter_helpers import sub_oracle
    from tests.query_tree_helpers import OracleStages
    parsed = [QT.parse(tree(b), DIM, MS) for b in range(B)]
    wk, wc = QT.run(parsed[0][0], QT.batch_vectors([p[1] for p in parsed]), OracleStages(sub_oracle(rows, DIM, MS, kept)))
    for b in range(B):
        same(keys, cnt, b, key_scores(wk[b, :wc[b]]), kept[key_ids(wk[b, :wc[b]])])


def test_the_scalar_model_of_list_keep():
    k = O.order_key(np.array([5.0, 4.0, 4.0, 3.0, 2.0], np.float32), np.array([7, 3, 9, 7, 1]))
    keys = np.zeros((1, 8), np.uint64)
    keys[0, [0, 1, 3, 4, 5]] = k                            # a 0 slot inside the list
    keep = np.zeros(10, bool)
    keep[[7, 9, 1]] = True
    out, cnt = list_keep_model(keys, None, 8, keep, np.array([3.0], np.float32))
    assert cnt.tolist() == [3] and key_ids(out[0, :3]).tolist() == [7, 9, 7] and not out[0, 3:].any()   # 3.0 stays
    out, cnt = list_keep_model(keys, np.array([4]), 1, keep, None)
    assert cnt.tolist() == [1] and key_ids(out[0, :1]).tolist() == [7]
    out, cnt = list_keep_model(keys, None, 8, None, np.array([np.nan], np.float32))
    assert cnt.tolist() == [5]                               # a NaN threshold keeps everything
