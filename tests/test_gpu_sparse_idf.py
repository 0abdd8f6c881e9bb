"""GPU: the sparse IDF modifier (spstats.hip, hx_sparse_df / hx_sparse_idf_apply / hx_sparse_idf_host; DESIGN.md section
31).  df, N and the scaled weights are compared EXACTLY with tests/sparse_idf_helpers.py, the restatement of the header's
contract: over a small index with empty rows (every kind of term, every nnz around the wave width, repeated ids, out
aliasing in), over a base plus a tail, over a three-segment index, through every refusal; through the handler's life
cycle (appends, deletes, upserts, a truncate, save and load) against the surviving rows and a fresh index of them; and
through every search entry that takes sparse queries, where a collection with the modifier must answer as a plain one
fed weights pre-scaled by the helpers."""
import asyncio
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import sparse_idf_helpers as H

pytestmark = pytest.mark.gpu

F32 = np.float32
EVERY, ONCE = 1000000, 2000000000            # a term of every row that holds a vector; a term of one row
VOCAB = 3 + 7 * np.arange(400)               # live terms lie 7 apart: t - 1 and t + 1 are absent
TAIL_VOCAB = 5 + 7 * np.arange(60)           # terms only later appends use


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from rag_application_amd import engine
    return engine


def make_rows(n, seed, vocab=VOCAB, empty_every=10, once_at=None):
    """n sparse rows: every empty_every-th empty, the others 1..12 vocabulary terms plus EVERY (ascending ids)"""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(n):
        if empty_every and r % empty_every == 4:
            rows.append((np.zeros(0, np.int64), np.zeros(0, F32)))
            continue
        t = np.sort(rng.choice(vocab, int(rng.integers(1, 13)), replace=False))
        t = np.append(t, EVERY)
        if once_at is not None and r == once_at:
            t = np.append(t, ONCE)
        rows.append((t.astype(np.int64), (rng.random(len(t)) * 2 + 0.25).astype(F32)))
    return rows


def csr(rows):
    ip = np.concatenate([[0], np.cumsum([len(i) for i, _ in rows])]).astype(np.int64)
    si = np.concatenate([i for i, _ in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    sv = np.concatenate([v for _, v in rows] + [np.zeros(0, F32)]).astype(F32)
    return ip, si, sv


def dense_rows(n, dim, seed):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(F32)


def probe_terms(si, rng, n):
    """n term ids: live ones, their absent neighbours, ids nobody holds, negative ones -- with repeats"""
    live = np.unique(si)
    pool = np.concatenate([live, live - 1, live + 1, [0, 1, 2, 2 ** 31 - 1, -1, -7, -2 ** 31, EVERY, ONCE, ONCE + 1, ONCE - 1,
                                                     int(live.min()), int(live.max())]])
    return rng.choice(pool, n, replace=True).astype(np.int32)


def check_stats(eng, ix, rows, terms, vals=None):
    """df, N and the weights of `terms` through the device entries and the host entry, against the helpers"""
    import torch
    ip, si, _ = csr(rows)
    terms = np.asarray(terms, np.int32)
    vals = (np.random.default_rng(len(terms)).random(len(terms)) * 3 + 0.01).astype(F32) if vals is None else vals
    want_df, want_n = H.stats(ip, si, terms)
    want_w = H.weights(vals, want_df, want_n)
    dev = ix._tdev
    t_idx, t_val = torch.from_numpy(terms).to(dev), torch.from_numpy(vals).to(dev)
    df, nd = ix.sparse_df(t_idx)
    assert df.dtype == torch.int64 and nd.shape == (1,)
    assert df.cpu().tolist() == want_df and int(nd.cpu()[0]) == want_n
    w = ix.sparse_idf(t_idx, t_val)
    assert (w.data_ptr() != t_val.data_ptr() or len(terms) == 0) and H.same_bits(w.cpu().numpy(), want_w)
    assert np.array_equal(t_val.cpu().numpy(), vals)                         # the input is left alone
    same = eng.sparse_idf_apply(t_val, df, nd, out=t_val)                    # out aliasing in
    assert same.data_ptr() == t_val.data_ptr() and H.same_bits(t_val.cpu().numpy(), want_w)
    hw, hdf, hn = ix.sparse_idf_host(terms, vals, want_stats=True)
    assert H.same_bits(hw, want_w) and hdf.tolist() == want_df and hn == want_n
    assert H.same_bits(ix.sparse_idf_host(terms, vals), want_w)              # both optional outputs NULL
    return want_df, want_n


# ---- statistics ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(eng):
    rows = make_rows(300, 11, once_at=123)
    ix = eng.HxIndex(64, ())
    ix.add(dense_rows(300, 64, 1), *csr(rows))
    yield ix, rows
    ix.close()


def test_every_kind_of_term(eng, small):
    ix, rows = small
    _, si, _ = csr(rows)
    live = np.unique(si)
    lo, hi = int(live.min()), int(live.max())
    assert hi == ONCE and lo == int(VOCAB[VOCAB >= lo][0])
    t = int(VOCAB[17])
    terms = [EVERY, ONCE, 999, -1, -2 ** 31, t, t - 1, t + 1, lo, hi, lo - 1, hi + 1, 2 ** 31 - 1, 0, t, t, EVERY]
    df, n = check_stats(eng, ix, rows, terms)
    assert n == 270 and df[0] == 270 and df[1] == 1 and df[2] == 0 and df[3] == 0 and df[6] == 0 and df[7] == 0
    assert df[5] > 0 and df[8] > 0 and df[9] == 1 and df[14] == df[5]
    # a non-finite weight stays non-finite, the sign survives, and so does a zero
    vals = np.array([np.inf, -np.inf, np.nan, -1.5, 0.0, 1e-44, 3e38], F32)
    check_w = ix.sparse_idf_host(np.array([EVERY, ONCE, t, t, t, EVERY, ONCE], np.int32), vals)
    assert np.isposinf(check_w[0]) and np.isneginf(check_w[1]) and np.isnan(check_w[2]) and check_w[3] < 0
    assert check_w[4] == 0 and check_w[5] == 0 and np.isposinf(check_w[6])  # (underflow and overflow of the one multiply)
    assert H.same_bits(check_w[[0, 1, 3, 4, 5, 6]], H.weights(vals, [270, 1, df[5], df[5], df[5], 270, 1], 270)[[0, 1, 3, 4, 5, 6]])


@pytest.mark.parametrize("nnz", [0, 1, 63, 64, 65, 5000])
def test_every_nnz_around_the_wave_width(eng, small, nnz):
    ix, rows = small
    terms = probe_terms(csr(rows)[1], np.random.default_rng(nnz), nnz)
    df, n = check_stats(eng, ix, rows, terms)
    assert n == 270
    if nnz == 5000:                                           # live and absent ids, and repeated ones
        assert any(d > 0 for d in df) and any(d == 0 for d in df) and len(set(terms.tolist())) < nnz


def test_an_index_without_sparse_vectors_and_an_empty_one(eng):
    ix = eng.HxIndex(64, ())
    try:
        check_stats(eng, ix, [], [3, EVERY, -1])                              # no row at all: N = 0, idf = ln 2
        ix.add(dense_rows(5, 64, 2))
        df, n = check_stats(eng, ix, [(np.zeros(0, np.int64), np.zeros(0, F32))] * 5, [3, EVERY])
        assert n == 0 and df == [0, 0]
        assert H.same_bits(ix.sparse_idf_host([3], [1.0]), [F32(0.6931472)])
    finally:
        ix.close()


def test_a_base_plus_a_tail(eng, monkeypatch):
    monkeypatch.setenv("HX_DEBUG_TAIL_MIN", "1000000")       # appends after a finalize go to the tail view
    base = make_rows(200, 21, once_at=50)
    tail = make_rows(100, 22, vocab=np.concatenate([VOCAB[:80], TAIL_VOCAB]), empty_every=7)
    ix = eng.HxIndex(64, ())
    try:
        ix.add(dense_rows(200, 64, 3), *csr(base))
        ix.finalize()
        assert ix.stats()["n_segments"] == 1
        ix.add(dense_rows(100, 64, 4), *csr(tail))
        rows = base + tail
        _, si, _ = csr(rows)
        _, tsi, _ = csr(tail)
        tail_only = np.setdiff1d(np.unique(tsi), np.unique(csr(base)[1]))
        both = np.intersect1d(np.unique(tsi), np.unique(csr(base)[1]))
        assert len(tail_only) > 10 and len(both) > 10
        terms = np.concatenate([tail_only, both, [ONCE, EVERY, -1], tail_only - 1, probe_terms(si, np.random.default_rng(5), 300)])
        df, n = check_stats(eng, ix, rows, terms)
        assert ix.stats()["n_segments"] == 2                 # a base and a tail: df is a sum over the two views
        assert all(d > 0 for d in df[:len(tail_only)]) and df[len(tail_only) + len(both) + 1] == n
    finally:
        ix.close()


def test_a_directory_row_that_spans_three_segments(eng, monkeypatch):
    monkeypatch.setenv("HX_DEBUG_SEG_DOCS", "32768")
    n = 70000
    rng = np.random.default_rng(31)
    lens = rng.integers(0, 9, n)
    lens[::11] = 0
    ip = np.concatenate([[0], np.cumsum(lens + (lens > 0))]).astype(np.int64)      # (+ EVERY in every row with a vector)
    row = np.repeat(np.arange(n), lens + (lens > 0))
    pos = np.arange(int(ip[-1])) - ip[row]
    start = rng.integers(0, len(VOCAB) - 8, n)               # a row holds lens[r] consecutive vocabulary terms, then EVERY
    si = np.where(pos < lens[row], VOCAB[np.minimum(start[row] + pos, len(VOCAB) - 1)], EVERY).astype(np.int32)
    sv = (rng.random(len(si)) + 0.5).astype(F32)
    ix = eng.HxIndex(64, ())
    try:
        ix.add(dense_rows(n, 64, 6), ip, si, sv)
        terms = np.concatenate([[EVERY, -1, EVERY + 1], VOCAB[::3], VOCAB[::5] + 1]).astype(np.int32)
        want_df, want_n = H.stats(ip, si, terms)
        assert want_n == int((lens > 0).sum()) and want_df[0] == want_n
        vals = (rng.random(len(terms)) + 0.1).astype(F32)
        w, df, nd = ix.sparse_idf_host(terms, vals, want_stats=True)
        assert ix.stats()["n_segments"] == 3
        assert df.tolist() == want_df and nd == want_n and H.same_bits(w, H.weights(vals, want_df, want_n))
    finally:
        ix.close()


def test_every_refusal_leaves_the_outputs_alone(eng, small):
    import torch
    from rag_application_amd import _lib
    ix, _ = small
    L = _lib.lib()
    dev = ix._tdev
    idx = torch.tensor([3, 10, EVERY], dtype=torch.int32, device=dev)
    val = torch.full((3,), 2.0, dtype=torch.float32, device=dev)
    df = torch.full((3,), -7, dtype=torch.int64, device=dev)
    nd = torch.full((1,), -7, dtype=torch.int64, device=dev)
    out = torch.full((3,), -7.0, dtype=torch.float32, device=dev)
    p = lambda t: t.data_ptr()
    h = ix._h

    def refused(rc, word):
        assert rc == 1 and word in L.hx_last_error().decode(), L.hx_last_error()

    refused(L.hx_sparse_df(None, p(idx), 3, p(df), p(nd), None), "NULL")
    refused(L.hx_sparse_df(h, p(idx), -1, p(df), p(nd), None), "nnz < 0")
    refused(L.hx_sparse_df(h, None, 3, p(df), p(nd), None), "NULL")
    refused(L.hx_sparse_df(h, p(idx), 3, None, p(nd), None), "NULL")
    refused(L.hx_sparse_df(h, p(idx), 3, p(df), None, None), "NULL")
    refused(L.hx_sparse_idf_apply(0, p(val), p(df), p(nd), -1, p(out), None), "nnz < 0")
    refused(L.hx_sparse_idf_apply(0, None, p(df), p(nd), 3, p(out), None), "NULL")
    refused(L.hx_sparse_idf_apply(0, p(val), None, p(nd), 3, p(out), None), "NULL")
    refused(L.hx_sparse_idf_apply(0, p(val), p(df), None, 3, p(out), None), "NULL")
    refused(L.hx_sparse_idf_apply(0, p(val), p(df), p(nd), 3, None, None), "NULL")
    hi, hv = np.array([3, 10, EVERY], np.int32), np.full(3, 2.0, F32)
    ho, hdf, hn = np.full(3, -7.0, F32), np.full(3, -7, np.int64), C.c_int64(-7)
    q = lambda a: a.ctypes.data
    refused(L.hx_sparse_idf_host(None, q(hi), q(hv), 3, q(ho), q(hdf), C.byref(hn)), "NULL")
    refused(L.hx_sparse_idf_host(h, q(hi), q(hv), -1, q(ho), q(hdf), C.byref(hn)), "nnz < 0")
    refused(L.hx_sparse_idf_host(h, None, q(hv), 3, q(ho), q(hdf), C.byref(hn)), "NULL")
    refused(L.hx_sparse_idf_host(h, q(hi), None, 3, q(ho), q(hdf), C.byref(hn)), "NULL")
    refused(L.hx_sparse_idf_host(h, q(hi), q(hv), 3, None, q(hdf), C.byref(hn)), "NULL")
    torch.cuda.synchronize()
    assert df.cpu().tolist() == [-7] * 3 and nd.cpu().tolist() == [-7] and out.cpu().tolist() == [-7.0] * 3
    assert ho.tolist() == [-7.0] * 3 and hdf.tolist() == [-7] * 3 and hn.value == -7
    # nnz = 0 still writes N, through NULL term and df pointers; the host entry's stats alone
    assert L.hx_sparse_df(h, None, 0, None, p(nd), None) == 0
    torch.cuda.synchronize()
    assert nd.cpu().tolist() == [270]
    assert L.hx_sparse_idf_host(h, q(hi), q(hv), 3, q(ho), None, C.byref(hn)) == 0 and hn.value == 270
    assert L.hx_sparse_idf_host(h, None, None, 0, None, None, C.byref(hn)) == 0 and hn.value == 270
    with pytest.raises(eng.HxError):
        ix.sparse_df(torch.zeros(3, dtype=torch.int64, device=dev))
    with pytest.raises(eng.HxError):
        eng.sparse_idf_apply(val, df[:2], nd)


# ---- the life cycle through the handler ---------------------------------------------------------------------------------------
def chunk(r, dense, idx, val, doc=None):
    meta = {"document_id": doc or f"doc{r // 16}", "user_id": "u", "file_name": "f", "mime_type": "text/plain", "file_size": 1,
            "description": "", "file_path": "/x", "context_version": 1, "chunk_number": r, "doc_summary": "s",
            "page_number": r % 2}
    return {"dense_embedding": np.asarray(dense, F32).tolist(), "content": f"chunk {r}", "chunk_metadata": meta,
            "sparse_embedding": {"indices": [int(i) for i in idx], "values": [float(v) for v in val]}}


def test_term_stats_follow_the_life_cycle(eng, monkeypatch, tmp_path):
    from rag_application_amd.handler import QdrantHandler
    monkeypatch.setenv("HX_DEBUG_TAIL_MIN", "1000000")       # the second and third append live in the tail
    run = asyncio.run
    h = QdrantHandler(persist_dir=str(tmp_path))
    run(h.create_collection("u", 64, [], 64, sparse_modifier="idf"))
    col = h._collections["u"]
    model = []                                               # the surviving rows: [dense, idx, val], in row order
    terms = np.concatenate([VOCAB[:150], TAIL_VOCAB, [EVERY, ONCE, -1, 4, int(VOCAB[3]) + 1]]).astype(np.int32)

    def check(step):
        rows = [(m[1], m[2]) for m in model]
        ip, si, sv = csr(rows)
        want_df, want_n = H.stats(ip, si, terms)
        got = run(h.term_stats("u", terms.tolist()))
        assert got == {"n_docs": want_n, "df": want_df}, step
        vals = np.linspace(0.5, 2.0, len(terms)).astype(F32)
        w = h._collections["u"].index.sparse_idf_host(terms, vals)
        assert H.same_bits(w, H.weights(vals, want_df, want_n)), step
        fresh = eng.HxIndex(64, ())
        try:
            if model:
                fresh.add(np.stack([m[0] for m in model]), ip, si, sv)
            fw, fdf, fn = fresh.sparse_idf_host(terms, vals, want_stats=True)
            assert fdf.tolist() == want_df and fn == want_n and H.same_bits(fw, w), step
        finally:
            fresh.close()
        assert len(h._collections["u"].ids) == len(model) == h._collections["u"].index.count()

    check("empty")
    r0 = 0
    for k, (n, vocab) in enumerate(((100, VOCAB), (57, np.concatenate([VOCAB[:50], TAIL_VOCAB])), (80, TAIL_VOCAB))):
        rows = make_rows(n, 40 + k, vocab=vocab, once_at=5 if k == 1 else None)
        X = dense_rows(n, 64, 50 + k)
        run(h.store_document_vectors([chunk(r0 + j, X[j], *rows[j]) for j in range(n)], "u"))
        model += [[X[j], rows[j][0], rows[j][1]] for j in range(n)]
        r0 += n
        check(f"append {k}")
    # delete: the row that held ONCE, rows of the base and of the tail
    gone = [105, 0, 1, 2, 50, 99, 100, 156, 157, 236] + list(range(20, 40))
    assert ONCE in model[105][1]
    assert run(h.delete_points("u", point_ids=[col.ids[r] for r in gone])) == len(gone)
    model = [m for r, m in enumerate(model) if r not in set(gone)]
    check("delete")
    # upsert by id: a longer, a shorter and an empty sparse vector; one new point; ONCE comes back elsewhere
    X = dense_rows(5, 64, 60)
    long_ = (np.append(np.sort(VOCAB[100:130]), [EVERY, ONCE]), np.full(32, 0.75, F32))
    short = (np.array([int(VOCAB[2])]), np.array([1.25], F32))
    none = (np.zeros(0, np.int64), np.zeros(0, F32))
    new = (np.array([int(TAIL_VOCAB[1]), EVERY]), np.array([0.5, 0.5], F32))
    was_empty = next(r for r, m in enumerate(model) if len(m[1]) == 0)
    targets = [3, 60, 150, was_empty]
    vecs = [long_, short, none, short]
    replaced = run(h.upsert_points("u", [chunk(900 + j, X[j], *vecs[j]) for j in range(4)] + [chunk(999, X[4], *new)],
                                   [col.ids[r] for r in targets] + [None]))
    assert replaced == 4
    for j, r in enumerate(targets):
        model[r] = [X[j], vecs[j][0].astype(np.int64), vecs[j][1]]
    model.append([X[4], new[0].astype(np.int64), new[1]])
    check("upsert")
    # truncate, as a refused upsert rolls back
    n_keep = 170
    col.index.truncate(n_keep)
    del col.ids[n_keep:]
    del col.payloads[n_keep:]
    col._idrows = None
    col._masks.clear()
    model = model[:n_keep]
    check("truncate")
    # save, load onto a new handler: the modifier comes back with the statistics
    run(h.save_collection("u"))
    run(h.delete_collection("u"))
    h = QdrantHandler(persist_dir=str(tmp_path))
    with pytest.raises(ValueError, match="stored collection"):
        run(h.create_collection("u", 64, [], 64))
    run(h.create_collection("u", 64, [], 64, sparse_modifier="idf"))
    assert h._collections["u"].sparse_modifier == "idf"
    check("load")
    run(h.delete_collection("u"))


# ---- search --------------------------------------------------------------------------------------------------------------------
N, DIM, B = 2000, 256, 6
P = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, dense_limit=40,
         quantized_limit=40, sparse_limit=50, final_limit=30, hnsw_ef=128)
HALF = {"must": [{"key": "page_number", "match": {"value": 0}}]}


@pytest.fixture(scope="module")
def pair(eng, synth_tables):
    """one handler, the same 2 000 rows in a collection with the modifier and in a plain one; the queries raw and
    pre-scaled by the helpers with the corpus' statistics"""
    from rag_application_amd.handler import QdrantHandler
    X = O.synth_dense(O.SEED_CORPUS, 0, N, DIM)
    ip, si, sv = O.synth_sparse_docs(O.SEED_SPDOC, 0, N, synth_tables)
    Q = O.synth_dense(O.SEED_QUERY, 0, B, DIM)
    qip, qsi, qsv = O.synth_sparse_queries(O.SEED_SPQUERY, 0, B, synth_tables)
    df, n_docs = H.stats(ip, si, qsi)
    scaled = H.weights(qsv, df, n_docs)
    raw = [{"indices": qsi[qip[b]:qip[b + 1]].tolist(), "values": qsv[qip[b]:qip[b + 1]].tolist()} for b in range(B)]
    pre = [{"indices": qsi[qip[b]:qip[b + 1]].tolist(), "values": scaled[qip[b]:qip[b + 1]].tolist()} for b in range(B)]
    h = QdrantHandler()
    chunks = [chunk(r, X[r], si[ip[r]:ip[r + 1]], sv[ip[r]:ip[r + 1]]) for r in range(N)]
    asyncio.run(h.create_collection("idf", DIM, [64, 128, 256], DIM, sparse_modifier="idf"))
    asyncio.run(h.create_collection("plain", DIM, [64, 128, 256], DIM))
    for name in ("idf", "plain"):
        asyncio.run(h.store_document_vectors(chunks, name))
    yield h, [Q[b].tolist() for b in range(B)], raw, pre
    for name in ("idf", "plain"):
        asyncio.run(h.delete_collection(name))


def bits(x):
    return int(F32(x).view(np.uint32))


def flat(res):
    """a result without the point ids (every collection draws its own): chunk numbers, score bits, the extra score"""
    def point(p):
        extra = [bits(getattr(p, k)) for k in ("mmr_score", "base_score") if hasattr(p, k)]
        return (p.payload["chunk_number"], bits(p.score), *extra)
    return [[(g.id, [point(p) for p in g.hits]) if hasattr(g, "hits") else point(g) for g in hits] for hits in res]


def sparse_leaf(sp):
    return {"query": sp, "using": "sparse", "limit": P["sparse_limit"]}


def weighted_rrf(q, sp):
    return {"prefetch": [{"query": q, "using": "dense", "limit": P["dense_limit"]}, sparse_leaf(sp)],
            "query": {"fusion": "rrf", "weights": [1.0, 2.5]}, "limit": P["final_limit"]}


ENTRIES = {
    "batch-tree": lambda h, u, q, sp: h.hybrid_search_batch(u, q, sp, top_k=30, search_params=P),
    "batch-h1": lambda h, u, q, sp: h.hybrid_search_batch(u, q, sp, top_k=30, search_params=P, mode="h1"),
    "batch-tree-root": lambda h, u, q, sp: h.hybrid_search_batch(u, q, sp, top_k=30, search_params=P, filters=HALF),
    "batch-tree-all": lambda h, u, q, sp: h.hybrid_search_batch(u, q, sp, top_k=30, search_params=P, filters=HALF,
                                                                filter_stages="all"),
    "batch-h1-all": lambda h, u, q, sp: h.hybrid_search_batch(u, q, sp, top_k=30, search_params=P, filters=HALF, mode="h1",
                                                              filter_stages="all"),
    "groups": lambda h, u, q, sp: h.hybrid_search_groups(u, q, sp, group_by="document_id", limit=5, group_size=3,
                                                         search_params=P, mode="h1"),
    "mmr": lambda h, u, q, sp: h.hybrid_search_mmr(u, q, sp, limit=10, diversity=0.5, candidates_limit=60,
                                                   search_params=P, mode="h1"),
    "boost": lambda h, u, q, sp: h.hybrid_search_boost(u, q, sp, formula={"sum": ["$score", 1.0]}, limit=10,
                                                       search_params=P, mode="h1"),
    "tree-sparse-leaf": lambda h, u, q, sp: h.query_points_batch(u, [sparse_leaf(s) for s in sp]),
    "tree-weighted-rrf": lambda h, u, q, sp: h.query_points_batch(u, [weighted_rrf(a, s) for a, s in zip(q, sp)]),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_the_modifier_equals_a_plain_collection_fed_scaled_weights(pair, entry):
    h, q, raw, pre = pair
    call = ENTRIES[entry]
    got = flat(asyncio.run(call(h, "idf", q, raw)))
    want = flat(asyncio.run(call(h, "plain", q, pre)))
    assert len(got) == B and all(len(g) > 0 for g in got), entry
    assert got == want, entry
    if entry in ("batch-h1", "tree-sparse-leaf"):
        # ... and the modifier does something: the plain collection fed the RAW weights answers otherwise
        assert flat(asyncio.run(call(h, "plain", q, raw))) != got


def test_a_plain_collection_answers_as_the_oracle(pair, synth_tables):
    """the plain path is the one the build had before: bit for bit the numpy oracle's lists"""
    h, q, raw, _ = pair
    X = O.synth_dense(O.SEED_CORPUS, 0, N, DIM)
    ip, si, sv = O.synth_sparse_docs(O.SEED_SPDOC, 0, N, synth_tables)
    ora = O.OracleIndex(DIM, (64, 128, 256))
    ora.add(X, ip, si, sv)
    ora.finalize()
    assert h._collections["plain"].sparse_modifier is None
    for mode in ("tree", "h1"):
        got = flat(asyncio.run(h.hybrid_search_batch("plain", q, raw, top_k=30, search_params=P, mode=mode)))
        for b in range(B):
            sp = (np.asarray(raw[b]["indices"]), np.asarray(raw[b]["values"], F32))
            es, ei = (O.hybrid_tree(ora, np.asarray(q[b], F32), *sp, P) if mode == "tree" else
                      O.hybrid_h1(ora, np.asarray(q[b], F32), *sp, P["dense_limit"], P["sparse_limit"], P["final_limit"]))
            assert got[b] == [(int(i), bits(s)) for s, i in zip(es, ei)], (mode, b)
