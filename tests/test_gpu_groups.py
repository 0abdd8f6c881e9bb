"""GPU: grouped hybrid search (hx_group, hx_hybrid_query_groups_host, QdrantHandler.hybrid_search_groups; DESIGN.md
section 20).

Every device result is compared with rag_application_amd/grouping.py over the same pool -- never with another device
result -- and exactly: uint64 key for key, code for code, every slot of the output stride, the zeros included."""
import asyncio
import os

import numpy as np
import pytest

from oracle import oracle as O
from rag_application_amd import grouping as GR

pytestmark = pytest.mark.gpu

ROWS = 4096
MISSING, NULL = 0xFFFFFFFF, 0xFFFFFFFE
LENGTHS = [1, 2, 63, 64, 65, 74, 255, 256, 257, 1000, 2047, 2048]
BATCHES = [1, 3, 65]
SHAPES = [(1, 1), (1, 2048), (2048, 1), (10, 3), (3, 10), (64, 32)]
DISTINCT = [1, 7, 4096]


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from rag_application_amd import engine
    return engine


def column_cells(distinct, seed):
    """seeded codes with `distinct` values (the extremes 0 and 0xFFFFFFFD among them), about 10 % MISSING / NULL cells"""
    rng = np.random.default_rng(seed)
    table = np.unique(rng.integers(1, NULL - 1, distinct, dtype=np.uint64))
    if distinct > 1:
        table[0], table[-1] = 0, NULL - 1
    cells = table[rng.integers(0, len(table), ROWS)].astype(np.uint32)
    hole = rng.random(ROWS)
    cells[hole < 0.05] = MISSING
    cells[(hole >= 0.05) & (hole < 0.10)] = NULL
    return cells


@pytest.fixture(scope="module")
def staged(eng):
    """a 64-dim index of 4096 synthetic rows with one U32 column per entry of DISTINCT"""
    ix = eng.HxIndex(64, (64,))
    ix.synth_fill(ROWS, O.SEED_CORPUS)
    cols = {}
    for d in DISTINCT:
        cells = column_cells(d, 100 + d)
        col = ix.payload_create(eng.PAY_U32)
        ix.payload_append(col, cells)
        cols[d] = (col, cells)
    yield ix, cols
    ix.close()


def make_keys(scores, ids):
    """the engine's keys (hx.h): orderable(score) << 32 | (0xFFFFFFFF - id)"""
    u = np.asarray(scores, np.float32).view(np.uint32).astype(np.uint64)
    o = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return (o << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(ids, np.uint64))


def key_rows(keys, id_base=0):
    return (0xFFFFFFFF - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64) - id_base


def lists(rng, cells, n, B, with_counts):
    """B strictly descending key lists of n slots over rows < ROWS, some slots empty (0); query 1 of a batch holds only
    rows without a group, query 2 only rows of one group; with counts: a stride beyond n, the last query of a batch of
    more than three has counts = 0, query 0 a count below n"""
    stride = min(2048, n + 7) if with_counts else n
    keys = np.zeros((B, stride), np.uint64)
    counts = np.full(B, n, np.int32)
    eligible = np.flatnonzero(cells < NULL)
    holes = np.flatnonzero(cells >= NULL)
    one = np.flatnonzero(cells == cells[eligible[0]])
    for b in range(B):
        if B >= 3 and b == 1:
            rows = rng.choice(holes, n, replace=True)
        elif B >= 3 and b == 2:
            rows = rng.choice(one, n, replace=True)
        else:
            rows = rng.choice(ROWS, n, replace=False)
        scores = (2.0 - np.arange(stride) * 2.0 ** -12 - b * 2.0 ** -20).astype(np.float32)
        keys[b, :n] = make_keys(scores[:n], rows)
        if stride > n:                                    # what lies past counts must not be read as part of the list
            keys[b, n:] = make_keys(scores[n:], rng.choice(ROWS, stride - n))
        if n >= 3:
            keys[b, rng.choice(n, max(1, n // 20), replace=False)] = 0
        assert (np.diff(keys[b][keys[b] != 0].astype(object)) < 0).all()
    if not with_counts:
        return keys, None
    if B > 3:
        counts[B - 1] = 0
    counts[0] = max(n - 1, 1) if n > 1 else n
    return keys, counts


def model(keys, counts, cells, G, S, id_base=0, n_rows=ROWS):
    """grouping.group_ranked over every list: (out [B, G * S], codes [B, G], group counts [B])"""
    B, stride = keys.shape
    out = np.zeros((B, G * S), np.uint64)
    codes = np.full((B, G), MISSING, np.uint32)
    cnt = np.zeros(B, np.int32)
    for b in range(B):
        n = stride if counts is None else int(counts[b])
        k = keys[b, :n]
        rows = key_rows(k, id_base)
        inside = (k != 0) & (rows >= 0) & (rows < n_rows)
        cell = np.where(inside, cells[np.clip(rows, 0, n_rows - 1)], MISSING)
        per_rank = [None if c >= NULL else c for c in cell.tolist()]
        groups = GR.group_ranked(per_rank, G, S)
        cnt[b] = len(groups)
        for g, ranks in enumerate(groups):
            codes[b, g] = per_rank[ranks[0]]
            out[b, g * S:g * S + len(ranks)] = k[ranks]
    return out, codes, cnt


def run_stage(ix, col, keys, counts, G, S):
    import torch
    tk = torch.from_numpy(keys.view(np.int64)).cuda()
    tc = None if counts is None else torch.from_numpy(counts).cuda()
    out, codes, cnt = ix.group(col, tk, tc, G, S)
    torch.cuda.synchronize()
    return (out.cpu().numpy().view(np.uint64).reshape(keys.shape[0], G * S), codes.cpu().numpy().view(np.uint32),
            cnt.cpu().numpy())


@pytest.mark.parametrize("with_counts", [True, False], ids=["counts", "no-counts"])
@pytest.mark.parametrize("distinct", DISTINCT)
def test_stage_alone_equals_the_host_model(eng, staged, distinct, with_counts):
    ix, cols = staged
    col, cells = cols[distinct]
    rng = np.random.default_rng(7 * distinct + with_counts)
    seen = set()
    for n in LENGTHS:
        for B in BATCHES:
            keys, counts = lists(rng, cells, n, B, with_counts)
            for G, S in SHAPES:
                got = run_stage(ix, col, keys, counts, G, S)
                want = model(keys, counts, cells, G, S)
                for name, g, w in zip(("out keys", "group codes", "group counts"), got, want):
                    np.testing.assert_array_equal(g, w, err_msg=f"{name}: n={n} B={B} G={G} S={S}")
                if B >= 3:
                    assert want[2][1] == 0 and not want[0][1].any(), "the query without an eligible row"
                    assert want[2][2] == 1, "the query of one group"
                    seen.add("one group")
                    if with_counts and B > 3:
                        assert want[2][B - 1] == 0 and not got[0][B - 1].any() and (got[1][B - 1] == MISSING).all()
                        seen.add("counts = 0")
    assert "one group" in seen and (not with_counts or "counts = 0" in seen)


def test_stage_on_global_ids_and_rows_of_other_shards(eng):
    """ids named batch by batch (hx_set_next_id): the keys come and go with global ids, the rows are found through the
    map; a key of an id this index does not hold is skipped"""
    rng = np.random.default_rng(3)
    ix = eng.HxIndex(64, (), id_base=1000)
    gids = []
    for first, m in ((1000, 300), (5000, 200), (5200, 100), (90000, 77)):
        ix.set_next_id(first)
        ix.add(O.synth_dense(O.SEED_CORPUS, len(gids), m, 64))
        gids.extend(range(first, first + m))
    gids = np.asarray(gids, np.int64)
    n_rows = len(gids)
    cells = rng.integers(0, 9, n_rows).astype(np.uint32)
    cells[rng.random(n_rows) < 0.1] = NULL
    col = ix.payload_create(eng.PAY_U32)
    ix.payload_append(col, cells)
    B, n = 5, 500
    keys = np.zeros((B, n), np.uint64)
    row_of = {int(g): r for r, g in enumerate(gids)}
    foreign = np.asarray([0, 999, 1300, 4999, 5300, 89999, 90077, 2 ** 32 - 2], np.int64)
    for b in range(B):
        ids = np.concatenate([rng.choice(gids, n - len(foreign), replace=False), foreign])
        rng.shuffle(ids)
        keys[b] = make_keys((1.0 - np.arange(n) * 2.0 ** -14).astype(np.float32), ids)
    for G, S in ((4, 3), (9, 100), (2048, 1)):
        got = run_stage(ix, col, keys, None, G, S)
        # the model sees local rows: a foreign id has none
        out = np.zeros((B, G * S), np.uint64)
        codes = np.full((B, G), MISSING, np.uint32)
        cnt = np.zeros(B, np.int32)
        for b in range(B):
            ids = (0xFFFFFFFF - (keys[b] & np.uint64(0xFFFFFFFF))).astype(np.int64)
            per_rank = [None if row_of.get(int(i)) is None or cells[row_of[int(i)]] >= NULL else int(cells[row_of[int(i)]])
                        for i in ids]
            groups = GR.group_ranked(per_rank, G, S)
            cnt[b] = len(groups)
            for g, ranks in enumerate(groups):
                codes[b, g] = per_rank[ranks[0]]
                out[b, g * S:g * S + len(ranks)] = keys[b, ranks]
        for name, g, w in zip(("out keys", "group codes", "group counts"), got, (out, codes, cnt)):
            np.testing.assert_array_equal(g, w, err_msg=f"{name}: G={G} S={S}")
    ix.close()


def test_refusals_leave_the_outputs_untouched(eng, staged):
    import torch
    from rag_application_amd import _lib
    ix, cols = staged
    col = cols[7][0]
    f64 = ix.payload_create(eng.PAY_F64)
    ix.payload_append(f64, np.zeros(ROWS, np.float64))
    lst = ix.payload_create(eng.PAY_LIST_U32)
    lagging = ix.payload_create(eng.PAY_U32)
    ix.payload_append(lagging, np.zeros(ROWS - 1, np.uint32))
    B, stride = 3, 64
    keys_np = make_keys(np.tile(1.0 - np.arange(stride) * 1e-3, (B, 1)), np.tile(np.arange(stride), (B, 1)))
    keys = torch.from_numpy(keys_np.view(np.int64)).cuda()
    counts = torch.full((B,), stride, dtype=torch.int32).cuda()
    out = torch.full((B, 2048), 0x5A5A5A5A, dtype=torch.int64).cuda()
    codes = torch.full((B, 2048), 0x5B5B5B5B, dtype=torch.int32).cuda()
    cnt = torch.full((B,), 0x5C5C5C5C, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    L, st = _lib.lib(), eng._stream()
    p = lambda t: t.data_ptr()                            # noqa: E731
    good = dict(h=ix._h, col=col, keys=p(keys), stride=stride, counts=p(counts), B=B, G=4, S=3, out=p(out), codes=p(codes),
                cnt=p(cnt))
    cases = [
        (dict(h=None), "NULL"), (dict(keys=None), "NULL"), (dict(out=None), "NULL"), (dict(codes=None), "NULL"),
        (dict(cnt=None), "NULL"), (dict(B=0), "B < 1"), (dict(B=-2), "B < 1"),
        (dict(stride=0), "stride"), (dict(stride=2049), "stride"), (dict(stride=-1), "stride"),
        (dict(G=0), "n_groups"), (dict(S=0), "n_groups"), (dict(G=-1, S=-1), "n_groups"), (dict(G=2049, S=1), "2048"),
        (dict(G=64, S=33), "2048"), (dict(G=2 ** 20, S=2 ** 20), "2048"),
        (dict(col=12345), "unknown column"), (dict(col=-1), "unknown column"),
        (dict(col=f64), "kind"), (dict(col=lst), "kind"), (dict(col=lagging), "not filled"),
    ]
    for change, word in cases:
        a = dict(good, **change)
        rc = L.hx_group(a["h"], a["col"], a["keys"], a["stride"], a["counts"], a["B"], a["G"], a["S"], a["out"], a["codes"],
                        a["cnt"], st)
        assert rc != 0, change
        assert word in L.hx_last_error().decode(), (change, L.hx_last_error().decode())
    with pytest.raises(eng.HxError, match="kind"):        # the binding raises what the entry says
        ix.group(f64, keys, counts, 4, 3)
    with pytest.raises(eng.HxError, match="2048"):
        ix.group(col, keys, counts, 2049, 1)
    torch.cuda.synchronize()
    assert (out == 0x5A5A5A5A).all() and (codes == 0x5B5B5B5B).all() and (cnt == 0x5C5C5C5C).all()
    # the same arguments unchanged are served: the refusals left the index and its columns as they were
    g = good
    assert L.hx_group(g["h"], g["col"], g["keys"], g["stride"], None, g["B"], g["G"], g["S"], g["out"], g["codes"], g["cnt"],
                      st) == 0
    torch.cuda.synchronize()
    want = model(keys_np, None, cols[7][1], 4, 3)
    np.testing.assert_array_equal(out.view(-1)[:B * 12].cpu().numpy().view(np.uint64).reshape(B, 12), want[0])
    np.testing.assert_array_equal(cnt.cpu().numpy(), want[2])
    for c in (f64, lst, lagging):
        ix.payload_drop(c)


# ---- the whole query, through the handler --------------------------------------------------------------------------------------
N, DIM, RUN = 2048, 768, 64
P = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, dense_limit=40,
         quantized_limit=40, sparse_limit=50, final_limit=30, hnsw_ef=128)
POOL = {"tree": 50, "h1": 90}
HALF = {"must": [{"key": "page_number", "match": {"value": 0}}]}       # keeps about half the rows


def doc_of(r):
    return None if r % 13 == 5 else f"doc{r // RUN}"                    # runs of 64 rows: the groups of a pool collide


def chunk(r, X, ip, si, sv, doc):
    meta = {"document_id": doc, "user_id": "u", "file_name": doc, "mime_type": "text/plain", "file_size": 1,
            "description": "", "file_path": "/x", "context_version": 1, "chunk_number": r, "doc_summary": "s",
            "page_number": r % 2}
    return {"dense_embedding": X[r].tolist(), "content": f"chunk {r}", "chunk_metadata": meta,
            "sparse_embedding": {"indices": si[ip[r]:ip[r + 1]].tolist(), "values": sv[ip[r]:ip[r + 1]].tolist()}}


@pytest.fixture(scope="module")
def corpus_a(synth_tables):
    """the corpus and the queries of tests/golden/corpus_a_2048x768.npz"""
    X = O.synth_dense(O.SEED_CORPUS, 0, N, DIM)
    ip, si, sv = O.synth_sparse_docs(O.SEED_SPDOC, 0, N, synth_tables)
    Q = O.synth_dense(O.SEED_QUERY, 0, 5, DIM)
    qip, qsi, qsv = O.synth_sparse_queries(O.SEED_SPQUERY, 0, 5, synth_tables)
    sparse = [{"indices": qsi[qip[b]:qip[b + 1]].tolist(), "values": qsv[qip[b]:qip[b + 1]].tolist()} for b in range(5)]
    return X, ip, si, sv, [q.tolist() for q in Q], sparse


@pytest.fixture(scope="module")
def handler(eng, corpus_a):
    """corpus A in one collection: document chunks whose document_id comes in runs (file_name is an unindexed copy of
    it), every 13th with document_id None, the last 148 rows chat messages, which have no document_id at all"""
    from rag_application_amd.handler import QdrantHandler
    X, ip, si, sv, _, _ = corpus_a
    h = QdrantHandler()
    n_docs = 1900
    asyncio.run(h.store_document_vectors([chunk(r, X, ip, si, sv, doc_of(r)) for r in range(n_docs)], "u"))
    chats = [dict(chunk(r, X, ip, si, sv, None), chat_id=f"c{r % 7}", message_type="user", timestamp="2024-01-01T00:00:00",
                  entities=[], relationships=[], chat_summary="s", message=f"chat {r}") for r in range(n_docs, N)]
    asyncio.run(h.store_chat_vectors(chats, "u"))
    assert asyncio.run(h.create_payload_index("u", "document_id", "keyword")) is True
    assert asyncio.run(h.create_payload_index("u", "is_chat", "bool")) is True
    assert asyncio.run(h.create_payload_index("u", "page_number", "integer")) is True
    yield h
    asyncio.run(h.delete_collection("u"))


def bits(x):
    return int(np.float32(x).view(np.uint32))


def flat(groups):
    return [(g.id, [(p.id, bits(p.score)) for p in g.hits]) for g in groups]


def grouped(h, corpus_a, B, key, mode, flt, limit, size, pool=None):
    res = asyncio.run(h.hybrid_search_groups("u", corpus_a[4][:B], corpus_a[5][:B], key, limit=limit, group_size=size,
                                             search_params=P, filters=flt, mode=mode,
                                             filter_stages="all" if flt else "root", group_pool=pool))
    assert len(res) == B
    return [flat(r) for r in res]


def from_the_pool(h, corpus_a, B, key, mode, flt, limit, size, pool):
    """grouping.group_ranked over hybrid_search_batch's list at final_limit = the pool"""
    res = asyncio.run(h.hybrid_search_batch("u", corpus_a[4][:B], corpus_a[5][:B], top_k=pool,
                                            search_params=dict(P, final_limit=pool), filters=flt, mode=mode,
                                            filter_stages="all" if flt else "root"))
    assert len(res) == B
    out = []
    for pts in res:
        values = [GR.group_value(p.payload, key) for p in pts]
        out.append([(values[g[0]][1], [(pts[r].id, bits(pts[r].score)) for r in g])
                    for g in GR.group_ranked(values, limit, size)])
    return out


def check_both_paths(h, corpus_a, shapes=((5, 3), (64, 4)), modes=("tree", "h1"), filters=(None, HALF), batches=(1, 5)):
    pi = h._collections["u"].pindex
    for mode in modes:
        for flt in filters:
            for B in batches:
                for limit, size in shapes:
                    dev0, dec0 = pi.group_device_calls, dict(pi.declined)
                    dev = grouped(h, corpus_a, B, "document_id", mode, flt, limit, size)
                    assert pi.group_device_calls == dev0 + 1 and pi.declined == dec0, "the device path was not taken"
                    py = grouped(h, corpus_a, B, "file_name", mode, flt, limit, size)
                    assert pi.group_device_calls == dev0 + 1, "the Python path was not taken"
                    assert pi.declined.get("group by an unindexed key", 0) == dec0.get("group by an unindexed key", 0) + 1
                    what = (mode, flt is not None, B, limit, size)
                    assert dev == py, what
                    assert dev == from_the_pool(h, corpus_a, B, "document_id", mode, flt, limit, size, POOL[mode]), what
                    assert all(0 < len(g) <= limit and all(0 < len(hits) <= size for _, hits in g) for g in dev), what
                    assert all(isinstance(i, str) for g in dev for i, _ in g), what
    return dev


def test_whole_query_device_path_equals_python_path(handler, corpus_a):
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corpus_a_2048x768.npz"))
    col = handler._collections["u"]
    plain = asyncio.run(handler.hybrid_search_batch("u", corpus_a[4], corpus_a[5], top_k=30, search_params=P))
    row = {i: r for r, i in enumerate(col.ids)}
    for b in range(5):                                    # the collection is the golden corpus: its lists are the file's
        m = int(gold["tree_mcp_cnt"][b])
        assert [row[p.id] for p in plain[b]] == gold["tree_mcp_ids"][b, :m].tolist()
        assert [bits(p.score) for p in plain[b]] == gold["tree_mcp_bits"][b, :m].tolist()
    dev = check_both_paths(handler, corpus_a)
    assert any(len(hits) > 1 for g in dev for _, hits in g), "no two hits of a pool share a document: nothing collided"
    # a shorter pool, and a bool column: chats against documents
    for pool in (1, 7, 50):
        assert grouped(handler, corpus_a, 5, "document_id", "tree", None, 5, 3, pool) == \
            from_the_pool(handler, corpus_a, 5, "document_id", "tree", None, 5, 3, pool)
    chat = grouped(handler, corpus_a, 5, "is_chat", "h1", None, 4, 50)
    assert chat == from_the_pool(handler, corpus_a, 5, "is_chat", "h1", None, 4, 50, 90)
    assert all(i is True for g in chat for i, _ in g) and any(g for g in chat)      # documents have no is_chat at all


def test_existing_calls_are_unchanged_by_a_grouped_call(handler, corpus_a):
    def plain():
        out = []
        for mode in ("tree", "h1"):
            for flt in (None, HALF):
                res = asyncio.run(handler.hybrid_search_batch("u", corpus_a[4], corpus_a[5], top_k=30, search_params=P, mode=mode,
                                                              filters=flt, filter_stages="all" if flt else "root"))
                assert len(res) == 5
                out.append([[(p.id, bits(p.score)) for p in r] for r in res])
        return out
    before = plain()
    sp = dict(P)
    for mode in ("tree", "h1"):
        for flt in (None, HALF):
            asyncio.run(handler.hybrid_search_groups("u", corpus_a[4], corpus_a[5], "document_id", limit=7, group_size=2,
                                                     search_params=sp, filters=flt, mode=mode,
                                                     filter_stages="all" if flt else "root"))
    assert sp == P, "the caller's search_params were written"
    assert plain() == before


def test_groups_follow_deletes_and_upserts(handler, corpus_a):
    X, ip, si, sv, _, _ = corpus_a
    col = handler._collections["u"]
    pi = col.pindex
    before = grouped(handler, corpus_a, 5, "document_id", "tree", None, 5, 3)
    gone = before[0][0][0]                                # the best document of query 0
    n = asyncio.run(handler.delete_points("u", filters={"must": [{"key": "document_id", "match": {"value": gone}}]}))
    assert n > 0 and pi.live("document_id")
    after = check_both_paths(handler, corpus_a, shapes=((5, 3),), batches=(5,))
    assert all(i != gone for g in after for i, _ in g)
    now = grouped(handler, corpus_a, 5, "document_id", "tree", None, 5, 3)
    assert now != before and all(i != gone for i, _ in now[0])
    # the best hit of query 0 moves to a document of its own
    best_id = now[0][0][1][0][0]
    r = col.ids.index(best_id)
    src = int(col.payloads[r]["chunk_number"])
    assert asyncio.run(handler.upsert_points("u", [chunk(src, X, ip, si, sv, "moved")], [best_id])) == 1
    assert pi.live("document_id")
    moved = check_both_paths(handler, corpus_a, shapes=((5, 3),), filters=(None,), batches=(5,))
    moved = grouped(handler, corpus_a, 5, "document_id", "tree", None, 5, 3)
    assert moved[0][0][0] == "moved" and [i for i, _ in moved[0][0][1]] == [best_id]
