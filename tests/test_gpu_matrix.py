"""GPU: distance matrix search (hx_search_matrix, hx_search_matrix_host, QdrantHandler.search_matrix_pairs / _offsets;
DESIGN.md section 28).

Every device result is compared with tests/matrix_helpers.py over the same rows -- never with another device result, the
one stated cross-check against hx_recommend_host aside -- and exactly: ids and fp32 score bits (as keys), counts, and the
zeros of the slots past them.  The model builds the sims of a sample once; every limit and threshold is cut from them."""
import asyncio
import os

import numpy as np
import pytest

from oracle import oracle as O
from rag_application_amd import filters as FL
from rag_application_amd import matrix as MX
from tests import matrix_helpers as MH
from tests import reco_helpers as RH

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from rag_application_amd import engine
    return engine


def corpus(name):
    if name == "b64":
        return O.synth_dense(O.SEED_CORPUS, 0, 4096, 64)          # golden corpus B
    if name == "a768":
        return O.synth_dense(O.SEED_CORPUS, 0, 2048, 768)         # golden corpus A's dense rows
    dim = {"w100": 100, "wide1088": 1088}[name]                   # padding inside the last 64 / the one-row-per-wave form
    return np.random.default_rng(dim).standard_normal((512, dim)).astype(F32)


@pytest.fixture(scope="module")
def staged(eng):
    out = {}
    for name in ("b64", "a768", "w100", "wide1088"):
        X = corpus(name)
        ix = eng.HxIndex(X.shape[1], ())
        ix.add(X)
        out[name] = (ix, O.cosine_preprocess(X))
    yield out
    for ix, _ in out.values():
        ix.close()


def run(ix, rows, limit, threshold=None):
    keys, cnt = ix.search_matrix(rows, limit, threshold)
    return keys.cpu().numpy().view(np.uint64), cnt.cpu().numpy()


def check(ix, Xn, rows, limits, threshold=None, ids=None, what=""):
    """the device against the model at every limit; returns (M, the model's keys and counts at the last limit)"""
    rows = np.asarray(rows, np.int64)
    gid = rows if ids is None else np.asarray(ids, np.int64)[rows]
    M = MH.sim_matrix(Xn[rows])
    out = None
    for limit in limits:
        wk, wc = MH.neighbours(M, gid, limit, threshold)
        gk, gc = run(ix, rows, limit, threshold)
        assert gk.shape == (len(rows), limit) and gc.shape == (len(rows),)
        np.testing.assert_array_equal(gc, wc, err_msg=f"{what} limit {limit}: counts")
        np.testing.assert_array_equal(gk, wk, err_msg=f"{what} limit {limit}: keys")
        out = (wk, wc)
    return M, out


def sample_of(n, S, seed):
    return np.random.default_rng(seed).permutation(n)[:S]          # out of order


@pytest.mark.parametrize("S", (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257))
def test_sample_sizes_at_width_64(staged, S):
    ix, Xn = staged["b64"]
    _, (wk, wc) = check(ix, Xn, sample_of(4096, S, S), (3, max(S - 1, 1)), what=f"S{S}")
    assert (wc == S - 1).all()


@pytest.mark.parametrize("name", ("b64", "w100", "a768", "wide1088"))
def test_widths(staged, name):
    ix, Xn = staged[name]
    check(ix, Xn, sample_of(len(Xn), 67, 67), (10, 66), what=name)


def test_a_sample_of_4096_at_width_64(staged):
    ix, Xn = staged["b64"]
    check(ix, Xn, sample_of(4096, 4096, 1), (3,), what="S4096")


def test_a_sample_of_300_at_width_768(staged):
    ix, Xn = staged["a768"]
    check(ix, Xn, sample_of(2048, 300, 2), (3, 64), what="S300")


def test_limits(staged):
    ix, Xn = staged["b64"]
    _, (wk, wc) = check(ix, Xn, sample_of(4096, 33, 3), (1, 3, 31, 32, 33, 38), what="S33")
    assert (wc == 32).all() and (wk[:, 32:] == 0).all()
    check(ix, Xn, sample_of(4096, 1100, 4), (1024,), what="S1100")


def test_thresholds(staged):
    ix, Xn = staged["b64"]
    rows = sample_of(4096, 67, 5)
    M, _ = check(ix, Xn, rows, (10,), what="no threshold")
    check(ix, Xn, rows, (10,), threshold=-np.inf, what="-inf")
    off = M[~np.eye(67, dtype=bool)]
    median = np.sort(off)[len(off) // 2]                           # the exact bits of a score: inclusive
    _, (wk, wc) = check(ix, Xn, rows, (10, 66), threshold=median, what="median")
    assert wc.sum() == (off >= median).sum() and (wc < 66).any()
    _, (wk, wc) = check(ix, Xn, rows, (10,), threshold=np.nextafter(off.max(), F32(np.inf)), what="above the maximum")
    assert (wc == 0).all() and (wk == 0).all()


def test_duplicates_above_a_threshold(eng):
    """the near-duplicate use: five stored copies of one vector, a threshold just below their sim"""
    X = O.synth_dense(O.SEED_CORPUS, 0, 300, 64).copy()
    copies = [10, 57, 123, 124, 290]
    X[copies] = X[10]
    Xn = O.cosine_preprocess(X)
    ix = eng.HxIndex(64, ())
    ix.add(X)
    rows = sample_of(300, 300, 6)
    same = MH.sim_matrix(Xn[copies])
    assert len(set(same.view(np.uint32).reshape(-1).tolist())) == 1
    thr = np.nextafter(same[0, 0], F32(-np.inf))
    _, (wk, wc) = check(ix, Xn, rows, (8,), threshold=thr, what="duplicates")
    for i, r in enumerate(rows):
        if r in copies:
            assert wc[i] == 4 and MH.key_ids(wk[i, :4]).tolist() == [c for c in copies if c != r]
        else:
            assert wc[i] == 0
    ix.close()


def test_copies_tie_and_the_smaller_id_comes_first(eng):
    """the corpus of tests/golden/ties_512x128.npz: 16 distinct rows repeated 32 times"""
    g = np.load(os.path.join(GOLD, "ties_512x128.npz"))
    assert g["dense_ids"].shape[1] >= 1
    X = O.synth_dense(77, 0, 16, 128)[np.arange(512) % 16]
    Xn = O.cosine_preprocess(X)
    ix = eng.HxIndex(128, ())
    ix.add(X)
    rows = sample_of(512, 512, 7)
    _, (wk, wc) = check(ix, Xn, rows, (1, 40, 511), what="ties")
    for i in (0, 100, 511):
        ids = MH.key_ids(wk[i])
        first = ids[:31]                                           # the 31 other copies of the row, ids ascending
        assert (first % 16 == rows[i] % 16).all() and (np.diff(first) > 0).all() and rows[i] not in first
        assert len(set((wk[i, :31] >> np.uint64(32)).tolist())) == 1
    ix.close()


@pytest.mark.parametrize("name", ("b64", "a768", "wide1088"))
def test_symmetry_of_the_bits(staged, name):
    """from the device's own lists: the score of (a, b) in a's row and of (b, a) in b's row"""
    ix, Xn = staged[name]
    rows = sample_of(len(Xn), 65, 8)
    gk, gc = run(ix, rows, 64)
    assert (gc == 64).all()
    score = {}
    for i, a in enumerate(rows):
        for k in gk[i]:
            score[(int(a), int(MH.key_ids(k)))] = int(k >> np.uint64(32))
    assert len(score) == 65 * 64
    for (a, b), s in score.items():
        assert score[(b, a)] == s, (a, b)
    gk3, _ = run(ix, rows, 3)                                      # a short limit: whenever both appear
    short = {(int(a), int(MH.key_ids(k))): int(k >> np.uint64(32)) for i, a in enumerate(rows) for k in gk3[i]}
    both = [(a, b) for (a, b) in short if (b, a) in short]
    assert both and all(short[(a, b)] == short[(b, a)] for a, b in both)


@pytest.mark.parametrize("name", ("b64", "a768", "wide1088"))
def test_a_row_equals_recommend_best_score_under_the_sample_mask(staged, name):
    """the cross-check against existing code: hx_recommend_host(BEST_SCORE, one stored positive a) under the packed mask of
    the sample scores sim(x, a) over the sample's rows and leaves a out"""
    ix, Xn = staged[name]
    rows = sample_of(len(Xn), 70, 9)
    keep = np.zeros(len(Xn), bool)
    keep[rows] = True
    for limit in (5, 80):
        sc, ids, cnt = ix.search_matrix_host(rows, limit)
        for i in (0, 1, 33, 69):
            rs, ri, rc = ix.recommend_host([[(int(rows[i]), 1)]], RH.BEST_SCORE, limit, mask=keep)
            assert rc[0] == cnt[i] == min(limit, 69)
            np.testing.assert_array_equal(ri[0], ids[i])
            np.testing.assert_array_equal(rs[0].view(np.uint32), sc[i].view(np.uint32))
            assert (ids[i, cnt[i]:] == -1).all() and np.isneginf(sc[i, cnt[i]:]).all()


def test_moved_and_rewritten_rows(eng):
    X = corpus("b64")[:600].copy()
    ix = eng.HxIndex(64, ())
    ix.add(X)
    keep = np.ones(600, bool)
    keep[[0, 5, 64, 299, 300, 599]] = False
    assert ix.retain(keep) == 6                                    # every later row moves down
    X = X[keep]
    rng = np.random.default_rng(10)
    rewritten = rng.permutation(594)[:40]
    fresh = rng.standard_normal((40, 64)).astype(F32)
    ix.replace(rewritten, fresh)
    X[rewritten] = fresh
    Xn = O.cosine_preprocess(X)
    rows = np.concatenate([rewritten[:20], sample_of(594, 594, 11)[:80]])
    rows = rows[np.sort(np.unique(rows, return_index=True)[1])]
    assert len(set(rows.tolist()) & set(rewritten.tolist())) >= 20
    check(ix, Xn, rows, (3, 50), what="moved")
    ix.close()


def test_global_ids(eng):
    X = O.synth_dense(O.SEED_CORPUS, 0, 700, 64)
    Xn = O.cosine_preprocess(X)
    based = eng.HxIndex(64, (), id_base=1 << 20)
    based.add(X)
    rows = sample_of(700, 90, 12)
    _, (wk, _) = check(based, Xn, rows, (4, 89), ids=np.arange(700) + (1 << 20), what="id_base")
    assert MH.key_ids(wk[:, 0]).min() >= 1 << 20
    based.close()
    ix = eng.HxIndex(64, ())
    gids = []
    for first, (a, b) in ((1000, (0, 100)), (5000, (100, 450)), (5350, (450, 700))):
        ix.set_next_id(first)
        ix.add(X[a:b])
        gids.extend(range(first, first + b - a))
    _, (wk, _) = check(ix, Xn, rows, (4, 89), ids=np.asarray(gids), what="named ids")
    ids = MH.key_ids(wk)
    assert ids.min() >= 1000 and ids.max() >= 5350
    ix.close()


def test_refusals_leave_the_outputs_untouched(staged):
    import torch
    from rag_application_amd import _lib
    ix, Xn = staged["b64"]
    keys = torch.full((8, 10), -7, dtype=torch.int64, device="cuda")
    counts = torch.full((8,), -9, dtype=torch.int32, device="cuda")
    good = [3, 1, 2]
    cases = [
        ([], 10, None, "sample"),
        (list(range(4097)), 10, None, "sample"),
        (good, 0, None, "limit"),
        (good, 1025, None, "limit"),
        (good, -1, None, "limit"),
        ([3, 4096], 10, None, "row"),
        ([-1, 3], 10, None, "row"),
        ([3, 1, 3], 10, None, "twice"),
        (good, 10, float("nan"), "NaN"),
    ]
    for rows, limit, thr, word in cases:
        with pytest.raises(_lib.HxError, match=word):
            ix.search_matrix(rows, limit, thr, keys=keys, counts=counts)
        torch.cuda.synchronize()
        assert (keys == -7).all() and (counts == -9).all(), word
    with pytest.raises(_lib.HxError, match="NULL"):
        ix.search_matrix(good, 10, keys=keys, counts=torch.empty(0, dtype=torch.int32))   # (a NULL output)
    sc, ids, cnt = np.full((3, 10), 5, F32), np.full((3, 10), 5, np.int64), np.full(3, 5, np.int32)
    rows = np.asarray([3, 1, 3], np.int64)
    rc = _lib.lib().hx_search_matrix_host(ix._h, rows.ctypes.data, 3, 10, float("-inf"), sc.ctypes.data, ids.ctypes.data,
                                          cnt.ctypes.data)
    assert rc != 0 and (sc == 5).all() and (ids == 5).all() and (cnt == 5).all()
    rc = _lib.lib().hx_search_matrix_host(ix._h, None, 3, 10, float("-inf"), sc.ctypes.data, ids.ctypes.data, cnt.ctypes.data)
    assert rc != 0 and (sc == 5).all() and (ids == 5).all() and (cnt == 5).all()
    wk, wc = MH.model(Xn, good, 10)                                # (and the host entry works: empty slots aside)
    sc, ids, cnt = ix.search_matrix_host(good, 10, float("-inf"))
    assert cnt.tolist() == [2, 2, 2] and (ids[:, 2:] == -1).all() and np.isneginf(sc[:, 2:]).all()
    np.testing.assert_array_equal(RH.make_keys(sc[:, :2], ids[:, :2]), wk[:, :2])
    gk, gc = run(ix, [77], 4)                                      # S = 1: one row, count 0
    assert gk.tolist() == [[0, 0, 0, 0]] and gc.tolist() == [0]


def test_the_collection_around_the_sample_does_not_matter(eng):
    """the same 48 vectors inside a 512-row index and inside a 65536-row index, in the same relative order"""
    rng = np.random.default_rng(13)
    V = rng.standard_normal((48, 64)).astype(F32)
    order = rng.permutation(48)
    lists = []
    for n in (512, 65536):
        X = O.synth_dense(O.SEED_CORPUS, 0, n, 64).copy()
        at = np.sort(rng.permutation(n)[:48])
        X[at] = V
        ix = eng.HxIndex(64, ())
        ix.add(X)
        rows = at[order]
        _, (wk, wc) = check(ix, O.cosine_preprocess(X), rows, (5, 47), what=f"n{n}")
        pos = {int(r): i for i, r in enumerate(rows)}
        lists.append([[(pos[int(MH.key_ids(k))], int(k >> np.uint64(32))) for k in wk[i]] for i in range(48)])
        ix.close()
    assert lists[0] == lists[1]


# ---- through the handler, on corpus A ------------------------------------------------------------------------------------------
N, DIM = 2048, 768
P = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, dense_limit=40,
         quantized_limit=40, sparse_limit=50, final_limit=30, hnsw_ef=128)
HALF = {"must": [{"key": "page_number", "match": {"value": 0}}]}       # keeps half the rows
DOC3 = {"must": [{"key": "document_id", "match": {"value": "doc3"}}]}  # keeps 64 rows


def chunk(r, X, ip, si, sv):
    meta = {"document_id": f"doc{r // 64}", "user_id": "u", "file_name": "f", "mime_type": "text/plain", "file_size": 1,
            "description": "", "file_path": "/x", "context_version": 1, "chunk_number": r, "doc_summary": "s",
            "page_number": r % 2}
    return {"dense_embedding": X[r].tolist(), "content": f"chunk {r}", "chunk_metadata": meta,
            "sparse_embedding": {"indices": si[ip[r]:ip[r + 1]].tolist(), "values": sv[ip[r]:ip[r + 1]].tolist()}}


@pytest.fixture(scope="module")
def corpus_a(synth_tables):
    X = O.synth_dense(O.SEED_CORPUS, 0, N, DIM)
    ip, si, sv = O.synth_sparse_docs(O.SEED_SPDOC, 0, N, synth_tables)
    Q = O.synth_dense(O.SEED_QUERY, 0, 5, DIM)
    qip, qsi, qsv = O.synth_sparse_queries(O.SEED_SPQUERY, 0, 5, synth_tables)
    sparse = [{"indices": qsi[qip[b]:qip[b + 1]].tolist(), "values": qsv[qip[b]:qip[b + 1]].tolist()} for b in range(5)]
    return X, ip, si, sv, Q, sparse, O.cosine_preprocess(X)


@pytest.fixture(scope="module")
def handler(eng, corpus_a):
    from rag_application_amd.handler import QdrantHandler
    X, ip, si, sv = corpus_a[:4]
    h = QdrantHandler()
    asyncio.run(h.store_document_vectors([chunk(r, X, ip, si, sv) for r in range(N)], "u"))
    yield h
    asyncio.run(h.delete_collection("u"))


def bits(x):
    return int(np.float32(x).view(np.uint32))


def plain(h, corpus_a):
    res = asyncio.run(h.hybrid_search_batch("u", corpus_a[4].tolist(), corpus_a[5], top_k=30, search_params=P))
    assert len(res) == 5
    return [[(p.id, bits(p.score)) for p in r] for r in res]


def handler_model(h, corpus_a, rows, limit, threshold=None):
    """the two shapes of the model's lists for the sample `rows` of the collection as it stands"""
    col = h._collections["u"]
    Xn = corpus_a[6][[int(p["chunk_number"]) for p in col.payloads]]
    keys, counts = MH.model(Xn, rows, limit, threshold)
    ids = [col.ids[r] for r in rows]
    id_of = dict(enumerate(col.ids))
    return MH.shape_pairs(ids, keys, counts, id_of), MH.shape_offsets(ids, keys, counts, id_of)


def both_forms(h, **kw):
    ps = asyncio.run(h.search_matrix_pairs("u", **kw))
    of = asyncio.run(h.search_matrix_offsets("u", **kw))
    return [(p.a, p.b, bits(p.score)) for p in ps], (of.offsets_row, of.offsets_col, [bits(s) for s in of.scores], of.ids)


def filtered_rows(h, flt, sample, seed):
    col = h._collections["u"]
    keep = np.asarray([FL.matches(p, flt, i) for i, p in zip(col.ids, col.payloads)], bool) if flt else np.ones(len(col.ids), bool)
    return keep, MX.choose_rows(FL.pack_rows(keep), len(col.ids), sample, seed).tolist()


def check_handler(h, corpus_a):
    for flt, sample, seed, limit, thr in ((None, 10, 1, 3, None), (HALF, 40, 7, 3, None), (HALF, 33, 8, 5, 0.02),
                                          (DOC3, 100, 9, 4, None)):
        keep, rows = filtered_rows(h, flt, sample, seed)
        assert len(rows) == min(sample, int(keep.sum())) >= 2 and keep[rows].all()
        got = both_forms(h, sample=sample, limit=limit, filters=flt, seed=seed, score_threshold=thr)
        assert got == handler_model(h, corpus_a, rows, limit, thr), (flt, sample)
        assert got == both_forms(h, sample=sample, limit=limit, filters=flt, seed=seed, score_threshold=thr)   # repeatable
        assert got[1][3] == [h._collections["u"].ids[r] for r in rows]
    keep, rows = filtered_rows(h, DOC3, 100, 9)
    assert len(rows) == 64 < 100                                   # a filter keeping fewer than `sample` points: all of them
    a = both_forms(h, sample=40, limit=3, filters=HALF, seed=1)
    b = both_forms(h, sample=40, limit=3, filters=HALF, seed=2)
    assert a[1][3] != b[1][3]                                      # another seed, another sample
    fresh = asyncio.run(h.search_matrix_offsets("u", sample=40, limit=3, filters=HALF))
    assert len(fresh.ids) == 40 and len(fresh.scores) == 120       # seed None: fresh entropy, the same shape


def test_handler_by_filter_with_and_without_a_payload_index(handler, corpus_a):
    before = plain(handler, corpus_a)
    check_handler(handler, corpus_a)
    assert plain(handler, corpus_a) == before                      # the plain search is what it was
    col = handler._collections["u"]
    assert col.pindex is None
    assert asyncio.run(handler.create_payload_index("u", "page_number", "integer")) is True
    evals = col.pindex.device_evals
    col._masks.clear()
    check_handler(handler, corpus_a)                               # the same lists through the payload index
    assert col.pindex.device_evals > evals
    assert plain(handler, corpus_a) == before


def test_handler_by_point_ids(handler, corpus_a):
    col = handler._collections["u"]
    rows = sample_of(len(col.ids), 25, 14).tolist()                # the order given, not ascending
    pids = [col.ids[r] for r in rows]
    got = both_forms(handler, limit=4, point_ids=pids)
    assert got == handler_model(handler, corpus_a, rows, 4)
    assert got[1][3] == pids and len(got[0]) == 100
    kept = [r for r in rows if col.payloads[r]["page_number"] == 0]
    assert 2 <= len(kept) < 25
    got = both_forms(handler, limit=4, point_ids=pids, filters=HALF)       # the filter drops the ones it does not keep
    assert got == handler_model(handler, corpus_a, kept, 4)
    with pytest.raises(ValueError, match="unknown"):
        asyncio.run(handler.search_matrix_pairs("u", point_ids=pids + ["nobody"]))
    with pytest.raises(ValueError, match="twice"):
        asyncio.run(handler.search_matrix_offsets("u", point_ids=pids + pids[:1]))
    assert asyncio.run(handler.search_matrix_pairs("u", point_ids=pids[:1])) == []
