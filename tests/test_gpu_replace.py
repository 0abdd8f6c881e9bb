"""GPU: upsert by an existing id (hx_replace_rows, hx_payload_replace, hx_payload_replace_lists, HxIndex.replace,
QdrantHandler.upsert_points).

The contract is section 14's: after replace(rows, ...) the index IS the index one gets by creating a new one and adding
the final rows in their order.  Everything is checked bit-exact (ids, uint32 views of the scores, counts, the bytes of
the stored copies) against such a fresh index and, for the first queries, the numpy oracle on the final rows.  The
corpus holds 2N rows, the index rows 0..N-1; a replace of positions S takes corpus rows N + S."""
import asyncio

import numpy as np
import pytest

from oracle import oracle as O
from tests.payload_helpers import U32_MISSING, U32_NULL
from tests.payload_list_helpers import ALL_SCHEMA, list_corpus, list_table
from tests.test_gpu_delete import check_fresh, delete_and_check, run_modes, same, stored_rows
from tests.test_gpu_payload import check, gpu_collection
from tests.test_gpu_prefilter import DIM, MODES, MS, P, Corpus, _chunks, check_masked, csr_rows, make_mask, params, queries

pytestmark = pytest.mark.gpu

N = 20000


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from rag_application_amd import engine
    return engine


@pytest.fixture(scope="module")
def corpus(synth_tables):
    return Corpus(2 * N, synth_tables)


def new_rows(corpus, S, shift=N):
    """the arguments of HxIndex.replace for positions S: corpus rows shift + S"""
    S = np.asarray(S, np.int64)
    ip, si, sv = csr_rows(corpus.ip, corpus.si, corpus.sv, S + shift)
    return S, corpus.X[S + shift], ip, si.astype(np.int32), sv


def others(S, n, k=16, seed=0):
    """rows that are not replaced: both ends where they are free, the neighbours of replaced rows, a random few"""
    S = np.asarray(S, np.int64)
    rng = np.random.default_rng(seed)
    cand = np.unique(np.concatenate([[0, n - 1], S[:4] - 1, S[:4] + 1, S[-4:] + 1, rng.integers(0, n, k)]))
    cand = cand[(cand >= 0) & (cand < n)]
    return np.setdiff1d(cand, S)


def pick(S, k=16, seed=0):
    S = np.asarray(S, np.int64)
    if len(S) <= k:
        return S
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([[S.min(), S.max()], S[rng.integers(0, len(S), k)]]))


def replace_and_check(eng, corpus, S, qs, n=N, ix=None, rows_now=None, n_oracle=1, shift=N, stored_rows=stored_rows):
    """full cycle: a fresh index of corpus rows 0..n-1 (or `ix` holding rows_now), the replace, then stored bytes and
    every list against the fresh index of the final rows"""
    own = ix is None
    rows_now = np.arange(n) if rows_now is None else rows_now.copy()
    if own:
        ix = corpus.index(eng, rows_now)
    S = np.asarray(S, np.int64)
    keep = others(S, len(rows_now))
    old = stored_rows(ix, keep)
    count0 = ix.count()
    ix.replace(*new_rows(corpus, S, shift))
    rows_now[S] = shift + S
    assert ix.count() == count0
    sub = corpus.index(eng, rows_now)
    assert stored_rows(ix, keep) == old, "a stored copy of a row that was not replaced changed"
    assert stored_rows(sub, keep) == old
    took = pick(S)
    assert stored_rows(ix, took) == stored_rows(sub, took), "a replaced row is not the fresh index's"
    assert ix.sparse_wmax() == sub.sparse_wmax()
    check_fresh(eng, corpus, ix, rows_now, qs, sub=sub, n_oracle=n_oracle)
    sub.close()
    if own:
        ix.close()
    return rows_now


# ---- sets of replaced rows ---------------------------------------------------------------------------------------------
def row_set(kind):
    if kind == "row0":
        return np.array([0])
    if kind == "last":
        return np.array([N - 1])
    if kind == "every_second":
        return np.arange(0, N, 2)
    if kind == "block_250_520":                      # crosses a 256-document workgroup of the splice
        return np.arange(250, 520)
    if kind == "all":
        return np.arange(N)
    if kind == "rand10_shuffled":
        rng = np.random.default_rng(10)
        return rng.permutation(N)[:N // 10]
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["row0", "last", "every_second", "block_250_520", "all", "rand10_shuffled"])
def test_row_sets_both_modes(eng, synth_tables, corpus, kind):
    replace_and_check(eng, corpus, row_set(kind), queries(33, synth_tables))


# ---- sparse shapes -----------------------------------------------------------------------------------------------------
def with_rows(corpus, over):
    """the corpus with the sparse vectors of some rows overridden: row -> (term ids, weights)"""
    lens = (corpus.ip[1:] - corpus.ip[:-1]).copy()
    for r, (ti, _) in over.items():
        lens[r] = len(ti)
    ip = np.zeros(corpus.n + 1, np.int64)
    np.cumsum(lens, out=ip[1:])
    si, sv = np.zeros(ip[-1], corpus.si.dtype), np.zeros(ip[-1], np.float32)
    for r in range(corpus.n):
        if r in over:
            si[ip[r]:ip[r + 1]], sv[ip[r]:ip[r + 1]] = over[r]
        else:
            si[ip[r]:ip[r + 1]] = corpus.si[corpus.ip[r]:corpus.ip[r + 1]]
            sv[ip[r]:ip[r + 1]] = corpus.sv[corpus.ip[r]:corpus.ip[r + 1]]
    return Corpus(corpus.n, None, X=corpus.X, csr=(ip, si, sv))


def test_sparse_shapes_inside_a_workgroup_and_across_its_boundary(eng, synth_tables, corpus):
    """new empty over old non-empty, new non-empty over old empty, longer, shorter, identical -- at rows 10..14 (inside
    the splice's first workgroup, which starts at the first replaced row) and at rows 264..268 (documents 254..258 of
    the splice: across the boundary of its first two workgroups)"""
    n, shift = 3000, N
    row = lambda r: (corpus.si[corpus.ip[r]:corpus.ip[r + 1]], corpus.sv[corpus.ip[r]:corpus.ip[r + 1]])
    top = int(corpus.si.max()) + 1
    over = {}
    for b in (10, 264):
        for r in range(b, b + 5):
            assert corpus.ip[r + 1] - corpus.ip[r] >= 2
        over[shift + b] = (np.zeros(0, np.int64), np.zeros(0, np.float32))                       # empty over non-empty
        over[b + 1] = (np.zeros(0, np.int64), np.zeros(0, np.float32))                           # non-empty over empty
        ti, tv = row(b + 2)                                                                      # longer
        over[shift + b + 2] = (np.concatenate([ti, top + np.arange(40)]), np.concatenate([tv, np.full(40, 0.5, np.float32)]))
        ti, tv = row(b + 3)                                                                      # shorter
        over[shift + b + 3] = (ti[:len(ti) // 2], tv[:len(ti) // 2])
        over[shift + b + 4] = row(b + 4)                                                         # identical
    c = with_rows(corpus, over)
    S = np.concatenate([np.arange(264, 269), np.arange(10, 15)])
    replace_and_check(eng, c, S, queries(16, synth_tables), n=n)


def test_dense_only_form_keeps_the_sparse_vectors(eng, synth_tables, corpus):
    n = 5000
    S = np.array([0, 77, 255, 256, 4999, 1234])
    ix = corpus.index(eng, np.arange(n))
    qs = queries(16, synth_tables)
    run_modes(eng, ix, qs)
    st0 = ix.stats()
    assert st0["n_segments"] > 0
    ix.replace(S, corpus.X[N + S])
    st1 = ix.stats()
    assert st1["nnz"] == st0["nnz"] and st1["n_segments"] == st0["n_segments"]      # the inverted index stayed
    # the fresh index: the new dense rows with the OLD sparse vectors
    X = corpus.X[:n].copy()
    X[S] = corpus.X[N + S]
    now = Corpus(n, None, X=X, csr=csr_rows(corpus.ip, corpus.si, corpus.sv, np.arange(n)))
    sub = now.index(eng)
    assert stored_rows(ix, S) == stored_rows(sub, S)
    keep = others(S, n)
    assert stored_rows(ix, keep) == stored_rows(sub, keep)
    check_fresh(eng, now, ix, np.arange(n), qs, sub=sub, n_oracle=1)
    ix.close()
    sub.close()


# ---- the inverted index ------------------------------------------------------------------------------------------------
def test_rows_replaced_in_base_and_tail(eng, synth_tables, corpus, monkeypatch):
    monkeypatch.setenv("HX_DEBUG_TAIL_MIN", "1000000")
    n0, n = 6000, 7500
    ix = corpus.index(eng, np.arange(n), batches=[(0, n0)])
    ix.finalize()
    ip, si, sv = csr_rows(corpus.ip, corpus.si, corpus.sv, np.arange(n0, n))
    ix.add(corpus.X[n0:n], ip, si.astype(np.int32), sv)
    qs = queries(16, synth_tables)
    run_modes(eng, ix, qs)
    assert ix.stats()["n_segments"] >= 2                      # base + tail
    replace_and_check(eng, corpus, np.array([5, 3000, 5999, 6000, 7000, 7499]), qs, ix=ix, rows_now=np.arange(n))
    ix.close()


@pytest.mark.parametrize("seg_docs", [32768, 65536])
def test_forced_segment_sizes(eng, synth_tables, corpus, monkeypatch, seg_docs):
    monkeypatch.setenv("HX_DEBUG_SEG_DOCS", str(seg_docs))
    S = np.random.default_rng(seg_docs).permutation(8000)[:800]
    replace_and_check(eng, corpus, S, queries(16, synth_tables), n=8000)


@pytest.mark.parametrize("searched_first", [False, True])
def test_trailing_rows_without_sparse_vectors_get_them(eng, synth_tables, corpus, searched_first):
    """rows at or past sp_rows (hx_add_dense alone: the CSR ends in front of them) replaced with sparse vectors, before
    any search has padded the CSR and after one has"""
    from rag_application_amd import _lib
    n0, n = 5000, 6500
    ix = corpus.index(eng, np.arange(n0))
    tail = np.ascontiguousarray(corpus.X[n0:n], np.float32)
    _lib.check(_lib.lib().hx_add_dense(ix._h, tail.ctypes.data, n - n0))
    assert ix.count() == n
    qs = queries(16, synth_tables)
    if searched_first:
        run_modes(eng, ix, qs)
    S = np.array([6499, 17, 5000, 5600, 4999])
    old = stored_rows(ix, others(S, n))
    ix.replace(*new_rows(corpus, S))
    # the final rows: trailing rows that were not replaced are empty documents
    rows_now = np.arange(n)
    rows_now[S] = N + S
    over = {int(r): (np.zeros(0, np.int64), np.zeros(0, np.float32)) for r in range(n0, n)}
    now = with_rows(corpus, over)
    sub = now.index(eng, rows_now)
    assert stored_rows(ix, others(S, n)) == old
    assert stored_rows(ix, S) == stored_rows(sub, S)
    check_fresh(eng, now, ix, rows_now, qs, sub=sub, n_oracle=1)
    ix.close()
    sub.close()


# ---- the masked query reads the new rows -----------------------------------------------------------------------------------
def test_masked_query_before_and_after(eng, synth_tables, corpus):
    n = 8000
    first = Corpus(n, None, X=corpus.X[:n], csr=csr_rows(corpus.ip, corpus.si, corpus.sv, np.arange(n)))
    ix = first.index(eng)
    keep = make_mask("rand10", n, seed=6)
    qs = queries(16, synth_tables)
    check_masked(eng, first, ix, keep, qs, n_oracle=1)
    S = np.flatnonzero(keep)[::3]                                 # kept rows: the gathered copies hold their old bytes
    S = np.concatenate([S, np.flatnonzero(~keep)[:50]])
    ix.replace(*new_rows(corpus, S))
    rows_now = np.arange(n)
    rows_now[S] = N + S
    now = Corpus(n, None, X=corpus.X[rows_now], csr=csr_rows(corpus.ip, corpus.si, corpus.sv, rows_now))
    check_masked(eng, now, ix, keep, qs, n_oracle=1)
    check_masked(eng, now, ix, keep, qs, n_oracle=0, dev=True)
    ix.close()


# ---- other index forms ---------------------------------------------------------------------------------------------------
def stage_entries_equal(eng, ix, sub, tables, B):
    import torch
    Q, qip, qsi, qsv = queries(B, tables, q0=200)
    tq, tip, tsi, tsv = (torch.from_numpy(a).cuda() for a in (Q, qip, qsi, qsv))

    def eq(a, b, what):
        assert torch.equal(a[1], b[1]), f"{what}: counts"
        assert torch.equal(a[0], b[0]), f"{what}: keys"
    for cand in ("i8", "f16"):
        ix.set_dense_candidates(cand)
        sub.set_dense_candidates(cand)
        try:
            for prefix in (0, 64, 128, 256):
                eq(ix.search_dense(tq, 50, prefix), sub.search_dense(tq, 50, prefix), f"dense {cand} prefix {prefix}")
            eq(ix.search_i8(tq, 40), sub.search_i8(tq, 40), "i8")
            eq(ix.search_sparse(tip, tsi, tsv, 50), sub.search_sparse(tip, tsi, tsv, 50), "sparse")
            ck, cc = sub.search_dense(tq, 100, 64)
            for prefix in (0, 128):
                eq(ix.rescore(tq, ck, cc, 30, prefix), sub.rescore(tq, ck, cc, 30, prefix), f"rescore {prefix}")
            assert torch.equal(ix.h1_local(tq, tip, tsi, tsv, 40, 50), sub.h1_local(tq, tip, tsi, tsv, 40, 50)), cand
            for m in MODES:
                hp = params(eng, m)
                eq(ix.hybrid_query(tq, tip, tsi, tsv, hp), sub.hybrid_query(tq, tip, tsi, tsv, hp), f"hybrid {m} {cand}")
        finally:
            ix.set_dense_candidates("i8")
            sub.set_dense_candidates("i8")


@pytest.fixture(scope="module")
def replaced(eng, corpus):
    """an index after a replace and the fresh index of its rows"""
    S = np.random.default_rng(77).permutation(N)[:N // 4]
    ix = corpus.index(eng, np.arange(N))
    ix.replace(*new_rows(corpus, S))
    rows_now = np.arange(N)
    rows_now[S] = N + S
    sub = corpus.index(eng, rows_now)
    yield ix, sub, rows_now
    ix.close()
    sub.close()


@pytest.mark.parametrize("B", [1, 33, 130, 1024])
def test_every_stage_entry_equals_the_fresh_index_on_both_candidate_kinds(eng, synth_tables, replaced, B):
    ix, sub, _ = replaced
    stage_entries_equal(eng, ix, sub, synth_tables, B)


def test_index_built_with_fp16_candidates_only(eng, synth_tables, corpus, monkeypatch):
    monkeypatch.setenv("HX_DENSE_CAND", "f16")
    n = 6000
    S = np.random.default_rng(3).permutation(n)[:600]
    def five_copies(ix, rows):                                    # (such an index keeps no int8 candidate copy: 5 and 6)
        return [[ix.debug_row(w, int(r)).tobytes() for w in range(5)] for r in rows]
    rows_now = replace_and_check(eng, corpus, S, queries(33, synth_tables), n=n, stored_rows=five_copies)
    assert (rows_now[S] == N + S).all()


def test_a_width_whose_rows_are_padded(eng, synth_tables, corpus):
    """dim 600: dim_pad = dim_pad8 = 640 (tests/test_row_widths_host.py's class of a padded row with an odd int8 tile count)"""
    dim, ms, n = 600, (64, 128, 256), 3000
    X = O.synth_dense(O.SEED_CORPUS, 0, 2 * n, dim)
    S = np.concatenate([[0, n - 1], np.random.default_rng(5).permutation(np.arange(1, n - 1))[:300]])
    rows_now = np.arange(n)
    rows_now[S] = n + S
    ix, sub = eng.HxIndex(dim, ms), eng.HxIndex(dim, ms)
    ip, si, sv = csr_rows(corpus.ip, corpus.si, corpus.sv, np.arange(n))
    ix.add(X[:n], ip, si.astype(np.int32), sv)
    ip, si, sv = csr_rows(corpus.ip, corpus.si, corpus.sv, n + S)
    ix.replace(S, X[n + S], ip, si.astype(np.int32), sv)
    fin = np.arange(n)
    fin[S] = n + S
    ip, si, sv = csr_rows(corpus.ip, corpus.si, corpus.sv, fin)
    sub.add(X[rows_now], ip, si.astype(np.int32), sv)
    took = np.concatenate([pick(S), others(S, n)])
    assert stored_rows(ix, took) == stored_rows(sub, took)
    Q = O.synth_dense(O.SEED_QUERY, 0, 33, dim)
    _, qip, qsi, qsv = queries(33, synth_tables)
    got, want = run_modes(eng, ix, (Q, qip, qsi, qsv)), run_modes(eng, sub, (Q, qip, qsi, qsv))
    for m in MODES:
        same(got[m], want[m], m)
    ix.close()
    sub.close()


# ---- life after a replace ------------------------------------------------------------------------------------------------
def test_replace_then_retain_add_save_load(eng, synth_tables, corpus, tmp_path):
    n = 8000
    qs = queries(16, synth_tables)
    ix = corpus.index(eng, np.arange(n))
    S = np.random.default_rng(9).permutation(n)[:900]
    rows = replace_and_check(eng, corpus, S, qs, ix=ix, rows_now=np.arange(n))
    # ... then a delete
    rows = delete_and_check(eng, corpus, make_mask("rand50", n, seed=4) | (np.arange(n) < 50), qs, ix=ix, rows=rows,
                            n_oracle=1)
    # ... then an add
    new = np.arange(n, n + 1500)
    ip, si, sv = csr_rows(corpus.ip, corpus.si, corpus.sv, new)
    ix.add(corpus.X[new], ip, si.astype(np.int32), sv)
    rows = np.concatenate([rows, new])
    check_fresh(eng, corpus, ix, rows, qs, n_oracle=1)
    # ... a second replace over the compacted and grown index (new rows from another part of the corpus)
    S2 = np.array([0, 1, len(rows) - 1, len(rows) // 2])
    ip, si, sv = csr_rows(corpus.ip, corpus.si, corpus.sv, 30000 + S2)
    ix.replace(S2, corpus.X[30000 + S2], ip, si.astype(np.int32), sv)
    rows[S2] = 30000 + S2
    check_fresh(eng, corpus, ix, rows, qs, n_oracle=1)
    # ... save / load
    path = str(tmp_path / "after.hx")
    ix.save(path)
    back = eng.HxIndex.load(path)
    check_fresh(eng, corpus, back, rows, qs, n_oracle=1)
    back.close()
    # ... and a rollback
    ix.truncate(4000)
    check_fresh(eng, corpus, ix, rows[:4000], qs, n_oracle=0)
    ix.close()


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_stored_byte_and_every_list(eng, synth_tables, corpus):
    from rag_application_amd import _lib
    n = 3000
    qs = queries(8, synth_tables)
    ix = corpus.index(eng, np.arange(n))
    all_rows = np.concatenate([np.arange(0, n, 97), [1, 2, 3, n - 1]])
    bytes0, r0, nnz0, w0 = stored_rows(ix, all_rows), run_modes(eng, ix, qs), ix.stats()["nnz"], ix.sparse_wmax()
    S, X, ip, si, sv = new_rows(corpus, np.array([1, 2, 3, n - 1]))

    bad = X.copy()
    bad[3, 17] = np.nan                                           # the LAST row of the batch: the others were derived
    with pytest.raises(eng.HxError, match="finite"):
        ix.replace(S, bad, ip, si, sv)
    bad[3, 17] = np.inf
    with pytest.raises(eng.HxError, match="finite"):
        ix.replace(S, bad)                                        # the dense-only form
    with pytest.raises(ValueError, match="unique"):
        ix.replace(np.array([1, 2, 3, 2]), X, ip, si, sv)
    dup = np.array([1, 2, 3, 2], np.int64)                        # ... and the engine's own check, behind the binding's
    assert _lib.lib().hx_replace_rows(ix._h, dup.ctypes.data, 4, X.ctypes.data, ip.ctypes.data, si.ctypes.data,
                                      sv.ctypes.data) != 0
    assert b"unique" in _lib.lib().hx_last_error()
    with pytest.raises(eng.HxError, match="outside"):
        ix.replace(np.array([1, 2, 3, ix.count()]), X, ip, si, sv)
    with pytest.raises(eng.HxError, match="outside"):
        ix.replace(np.array([1, 2, 3, -1]), X, ip, si, sv)
    rep = si.copy()
    assert ip[4] - ip[3] >= 2
    rep[ip[3] + 1] = rep[ip[3]]                                   # a repeated term id in the last vector
    with pytest.raises(eng.HxError, match="unique within a vector"):
        ix.replace(S, X, ip, rep, sv)
    neg = si.copy()
    neg[0] = -4
    with pytest.raises(eng.HxError, match="out of range"):
        ix.replace(S, X, ip, neg, sv)
    for v in (np.inf, np.nan, 2e18):
        w = sv.copy()
        w[-1] = v
        with pytest.raises(eng.HxError, match="finite"):
            ix.replace(S, X, ip, si, w)
    down = ip.copy()
    down[2] = down[1] - 1
    with pytest.raises(eng.HxError, match="monotone"):
        ix.replace(S, X, down, si, sv)
    with pytest.raises(ValueError):
        ix.replace(S, X[:3], ip, si, sv)

    assert ix.count() == n and ix.stats()["nnz"] == nnz0 and ix.sparse_wmax() == w0
    assert stored_rows(ix, all_rows) == bytes0
    r1 = run_modes(eng, ix, qs)
    for m in MODES:
        same(r1[m], r0[m], m)
    ix.replace(np.zeros(0, np.int64), np.zeros((0, DIM), np.float32))               # m == 0: nothing happens
    assert stored_rows(ix, all_rows) == bytes0
    ix.close()
    # an index whose ids were named: a shard of a sharded collection
    sh = eng.HxIndex(DIM, MS)
    ip2, si2, sv2 = csr_rows(corpus.ip, corpus.si, corpus.sv, np.arange(1000))
    sh.add(corpus.X[:1000], ip2, si2.astype(np.int32), sv2)
    sh.set_next_id(5000)
    ip2, si2, sv2 = csr_rows(corpus.ip, corpus.si, corpus.sv, np.arange(1000, 2000))
    sh.add(corpus.X[1000:2000], ip2, si2.astype(np.int32), sv2)
    S2 = np.array([1, 2, 3, 1999])
    b0 = stored_rows(sh, S2)
    with pytest.raises(eng.HxError, match="hx_set_next_id"):
        sh.replace(S2, X, ip, si, sv)
    assert stored_rows(sh, S2) == b0
    sh.close()


# ---- payload columns -------------------------------------------------------------------------------------------------
def decoded(col, key, r):
    """one cell as the payload held it: (state, value) for a scalar key, (head, values) for a list key"""
    k = col.pindex.keys[key]
    words = {c: w for w, c in k.codes.items()}
    if k.is_list:
        head, vals = col.index.payload_list(k.col, r, k.kind)
        vals = [words[int(v)] for v in vals] if k.elem == "keyword" else vals.tolist()
        return head if head >= U32_NULL else len(vals), vals
    bits = col.index.payload_cell(k.col, r, k.kind)
    if k.schema == "keyword" and bits < U32_NULL:
        return "kw", words[bits]
    return "bits", bits


def test_payload_cells_and_lists_replaced_in_place(eng):
    """scalar and list columns of every schema: rows patched through hx_payload_replace / _replace_lists against a
    collection to which the final payloads were appended -- every cell of the replaced rows and of their neighbours, and
    the masks of the randomised filters (ANY_EQ, IN, ranges, IS_EMPTY_LIST among them) against filters.row_mask"""
    n = 2047
    ids, pays0 = list_table(n, seed=1)
    _, other = list_table(n, seed=2)
    rng = np.random.default_rng(4)
    S = np.concatenate([[0, n - 1], np.arange(250, 520), rng.permutation(np.arange(600, n - 1))[:200]])
    S = rng.permutation(S)                                        # (any order)
    final = list(pays0)
    for r in S:
        final[r] = other[r]
    col, live = gpu_collection(eng, ids, pays0, ALL_SCHEMA)
    ref, live_ref = gpu_collection(eng, ids, final, ALL_SCHEMA)
    try:
        assert all(live.values()) and all(live_ref.values())
        for r in S:
            col.payloads[r] = final[r]
        col.replace_payload_cells(S, [final[r] for r in S])
        assert sorted(col.pindex.live_keys()) == sorted(ALL_SCHEMA)
        look = np.unique(np.concatenate([S[:60], others(S, n, k=40)]))
        for key in ALL_SCHEMA:
            for r in look:
                assert decoded(col, key, int(r)) == decoded(ref, key, int(r)), (key, int(r))
        seen = [int(check(col, f).sum()) for f in list_corpus(25, n, seed=31) + [{}]]
        assert any(0 < s < n for s in seen) and col.pindex.declined == {}
    finally:
        col.close()
        ref.close()


def test_lists_growing_shrinking_and_changing_state(eng):
    n = 700
    ids = [f"id{r}" for r in range(n)]
    pays0 = [{"t": [f"w{r % 5}", "x"], "x": [float(r % 7), 2.5]} for r in range(n)]
    states = [{"t": [f"g{j}" for j in range(9)], "x": [float(j) for j in range(9)]},       # grows
              {"t": ["x"], "x": [2.5]},                                                    # shrinks
              {"t": [], "x": []},                                                          # empty
              {"t": None, "x": None},                                                      # NULL
              {},                                                                          # MISSING
              {"t": "bare", "x": 41}]                                                      # a bare scalar: one element
    S = np.concatenate([np.arange(0, 6), np.arange(253, 259), np.arange(n - 6, n)])
    final = list(pays0)
    for k, r in enumerate(S):
        final[r] = states[k % len(states)]
    schema = {"t": "keyword_list", "x": "number_list"}
    col, _ = gpu_collection(eng, ids, pays0, schema)
    ref, _ = gpu_collection(eng, ids, final, schema)
    flts = [{"must": [{"key": "t", "match": {"value": "g3"}}]}, {"must": [{"key": "t", "match": {"any": ["x", "bare"]}}]},
            {"must": [{"key": "x", "range": {"gt": 3, "lt": 50}}]}, {"must": [{"is_empty": {"key": "t"}}]},
            {"must": [{"is_null": {"key": "x"}}]}, {"must": [{"key": "x", "match": {"value": 41}}]},
            {"must_not": [{"key": "t", "match": {"any": ["x"]}}]}]
    try:
        for r in S:
            col.payloads[r] = final[r]
        col.replace_payload_cells(S, [final[r] for r in S])
        for key in schema:
            for r in range(n):
                assert decoded(col, key, r) == decoded(ref, key, r), (key, r)
        for f in flts:
            assert 0 < int(check(col, f).sum()) < n
        # once more over rows already replaced: the lists shrink back
        col.payloads[255], col.payloads[0] = pays0[255], pays0[0]
        col.replace_payload_cells([255, 0], [pays0[255], pays0[0]])
        assert decoded(col, "t", 255) == (2, ["w0", "x"]) and decoded(col, "x", 0) == (2, [0.0, 2.5])
        for f in flts:
            check(col, f)
    finally:
        col.close()
        ref.close()


def test_payload_replace_refusals(eng):
    ix = eng.HxIndex(64, (64,))
    ix.synth_fill(100, O.SEED_CORPUS)
    c = ix.payload_create(eng.PAY_U32)
    ix.payload_append(c, np.arange(60, dtype=np.uint32))
    l = ix.payload_create(eng.PAY_LIST_U32)
    ix.payload_append_lists(l, np.full(60, 1, np.uint32), np.arange(60, dtype=np.uint32))
    with pytest.raises(eng.HxError, match="outside"):
        ix.payload_replace(c, [60], np.zeros(1, np.uint32))           # at `filled`, below count()
    with pytest.raises(eng.HxError, match="kind"):
        ix.payload_replace(l, [1], np.zeros(1, np.uint32))
    with pytest.raises(eng.HxError, match="kind"):
        ix.payload_replace_lists(c, [1], np.zeros(1, np.uint32), np.zeros(0, np.uint32))
    with pytest.raises(eng.HxError, match="sum"):
        ix.payload_replace_lists(l, [1], np.full(1, 2, np.uint32), np.zeros(1, np.uint32))
    with pytest.raises(eng.HxError, match="reserved"):
        ix.payload_replace_lists(l, [1], np.full(1, 1, np.uint32), np.full(1, U32_MISSING, np.uint32))
    with pytest.raises(eng.HxError, match="outside"):
        ix.payload_replace_lists(l, [60], np.full(1, 1, np.uint32), np.zeros(1, np.uint32))
    assert [ix.payload_cell(c, r, eng.PAY_U32) for r in (0, 1, 59)] == [0, 1, 59]
    assert [ix.payload_list(l, r, eng.PAY_LIST_U32)[1].tolist() for r in (0, 1, 59)] == [[0], [1], [59]]
    ix.close()


# ---- the handler, end to end -----------------------------------------------------------------------------------------
def _lists(hh, Q, qi, qv, **kw):
    out = {}
    for mode in MODES:
        res = asyncio.run(hh.hybrid_search_batch("u", [q.tolist() for q in Q], [{"indices": qi, "values": qv}] * len(Q),
                                                 top_k=20, search_params=dict(P, final_limit=20), mode=mode, **kw))
        assert len(res) == len(Q) and all(len(r) > 0 for r in res), mode
        out[mode] = [([p.payload for p in r], np.array([p.score for p in r], np.float32).view(np.uint32).tolist())
                     for r in res]
    return out


def test_handler_upsert_points(eng):
    from rag_application_amd import bm25
    from rag_application_amd.handler import QdrantHandler
    n, dim = 800, 768
    X = O.synth_dense(O.SEED_CORPUS, 0, n, dim)
    X2 = O.synth_dense(O.SEED_CORPUS + 5, 0, n, dim)
    docs = np.random.default_rng(1).integers(0, 30, n)
    chunks, _ = _chunks(n, X, docs)

    def variant(r, doc="docNEW"):
        """chunk r re-embedded: another dense vector, another chunk's text and sparse vector, another document"""
        src = chunks[(r + 7) % n]
        meta = dict(chunks[r]["chunk_metadata"], document_id=doc, chunk_number=10_000 + r)
        return {"content": src["content"], "dense_embedding": X2[r].tolist(), "sparse_embedding": src["sparse_embedding"],
                "chunk_metadata": meta}
    h = QdrantHandler()
    asyncio.run(h.store_document_vectors(chunks[:500], "u"))
    asyncio.run(h.store_document_vectors(chunks[500:], "u"))
    assert asyncio.run(h.create_payload_index("u", "document_id", "keyword"))
    col = h._collections["u"]
    ids0 = list(col.ids)
    flt = {"must": [{"key": "document_id", "match": {"value": "docNEW"}}]}
    assert asyncio.run(h.get_collection_chunk_count("u", filters=flt)) == 0       # (and the filter's mask is cached)
    R = [799, 0, 255, 256, 31, 500]
    extra = [variant(r, doc="docEXTRA") for r in (1, 2, 3, 4, 5)]
    batch = [variant(r) for r in R[:3]] + extra[:2] + [variant(r) for r in R[3:]] + extra[2:]
    pids = [ids0[r] for r in R[:3]] + ["custom-a", None] + [ids0[r] for r in R[3:]] + [None, "custom-b", None]
    assert asyncio.run(h.upsert_points("u", batch, pids)) == len(R)
    assert col.ids[:n] == ids0 and len(col.ids) == n + 5 == col.index.count()
    assert col.ids[n] == "custom-a" and col.ids[n + 3] == "custom-b"
    assert all(len(i) == 36 for i in (col.ids[n + 1], col.ids[n + 2], col.ids[n + 4]))
    assert col._masks == {} and col.pindex.live("document_id")
    # a handler that stored the final chunks in order
    final = list(chunks)
    for r in R:
        final[r] = variant(r)
    final += extra
    h2 = QdrantHandler()
    asyncio.run(h2.store_document_vectors(final, "u"))
    assert asyncio.run(h2.create_payload_index("u", "document_id", "keyword"))
    assert col.payloads == h2._collections["u"].payloads
    qi, qv = bm25.embed("hybrid dense sparse retrieval")
    Q = np.concatenate([O.synth_dense(O.SEED_QUERY, 0, 3, dim), X2[[255]]])      # the last query IS a replaced row's vector
    got, want = _lists(h, Q, qi, qv), _lists(h2, Q, qi, qv)
    assert got == want
    # a filter on the indexed field sees the new payload, every stage
    evals = col.pindex.device_evals
    assert asyncio.run(h.get_collection_chunk_count("u", filters=flt)) == len(R)
    assert col.pindex.device_evals == evals + 1
    fa, fb = _lists(h, Q, qi, qv, filters=flt, filter_stages="all"), _lists(h2, Q, qi, qv, filters=flt, filter_stages="all")
    assert fa == fb
    assert all(p["document_id"] == "docNEW" for m in MODES for pays, _ in fa[m] for p in pays)

    # a refused call: new points first, then a replace the engine refuses -- ids, payloads, count, lists as they were
    ids1, pays1, lists1 = list(col.ids), list(col.payloads), got
    worse = variant(100)
    worse["dense_embedding"][5] = float("nan")
    with pytest.raises(Exception, match="finite"):
        asyncio.run(h.upsert_points("u", [variant(9, "docX"), worse, variant(10, "docX")], [None, ids0[100], "custom-c"]))
    assert col.ids == ids1 and col.payloads == pays1 and col.index.count() == len(ids1)
    assert col.index.payload_rows(col.pindex.keys["document_id"].col) == len(ids1)
    assert _lists(h, Q, qi, qv) == lists1
    assert asyncio.run(h.get_collection_chunk_count("u", filters=flt)) == len(R)
    for bad_ids in ([ids0[1], ids0[1]], [ids0[1]]):
        with pytest.raises(ValueError):
            asyncio.run(h.upsert_points("u", [variant(1), variant(2)], bad_ids))
    with pytest.raises(ValueError):
        asyncio.run(h.upsert_points("u", [dict(variant(1), dense_embedding=[0.0] * 5)], [ids0[1]]))
    with pytest.raises(ValueError):
        asyncio.run(h.upsert_points("", [variant(1)], [ids0[1]]))
    assert col.ids == ids1 and col.payloads == pays1
    for hh in (h, h2):
        asyncio.run(hh.delete_collection("u"))


def test_handler_replaced_point_keeps_its_place_among_ties(eng):
    """the ties corpus of tests/golden/ties_512x128.npz (16 distinct rows repeated, every document the same sparse
    weight): the sparse list of the fixture's query is ids 0..19, all scores equal.  A point re-upserted under its id
    keeps row 3 and with it rank 3; the delete + add route moves it behind the 511 others"""
    import torch
    from rag_application_amd.handler import QdrantHandler
    g = np.load("tests/golden/ties_512x128.npz")
    X = O.synth_dense(77, 0, 16, 128)[np.arange(512) % 16]

    def chunk(r, text):
        return {"content": text, "dense_embedding": X[r].tolist(), "sparse_embedding": {"indices": [5], "values": [1.0]},
                "chunk_metadata": {"document_id": "d", "user_id": "u", "file_name": "f", "mime_type": "text/plain",
                                   "file_size": 1, "description": "", "file_path": "/x", "context_version": 1,
                                   "chunk_number": r, "doc_summary": "s"}}
    chunks = [chunk(r, f"text {r}") for r in range(512)]
    tq = (torch.tensor([0, 1], dtype=torch.int64).cuda(), torch.tensor([5], dtype=torch.int32).cuda(),
          torch.tensor([2.0], dtype=torch.float32).cuda())

    def sparse_top(hh):
        col = hh._collections["u"]
        keys, cnt = col.index.search_sparse(*tq, 20)
        s, i = (t.cpu().numpy()[0] for t in eng.unpack(keys))
        return s.view(np.uint32), i, [col.payloads[r]["content"] for r in i]
    ha, hb = QdrantHandler(), QdrantHandler()
    for hh in (ha, hb):
        asyncio.run(hh.create_collection("u", dense_vector_size=128, matryoshka_sizes=[64], quantized_size=128))
        asyncio.run(hh.store_document_vectors(chunks, "u"))
        bits, ids, _ = sparse_top(hh)
        np.testing.assert_array_equal(ids, g["sparse_ids"][0])
        np.testing.assert_array_equal(bits, g["sparse_bits"][0])
    pid = ha._collections["u"].ids[3]
    assert asyncio.run(ha.upsert_points("u", [chunk(3, "corrected text")], [pid])) == 1
    bits, ids, texts = sparse_top(ha)
    np.testing.assert_array_equal(ids, g["sparse_ids"][0])            # rank 3 is still row 3 ...
    np.testing.assert_array_equal(bits, g["sparse_bits"][0])
    assert texts[3] == "corrected text" and ha._collections["u"].ids[3] == pid    # ... the same point, its new payload
    # the only other route to the same point
    assert asyncio.run(hb.delete_points("u", point_ids=[hb._collections["u"].ids[3]])) == 1
    asyncio.run(hb.store_document_vectors([chunk(3, "corrected text")], "u"))
    _, ids_b, texts_b = sparse_top(hb)
    assert "corrected text" not in texts_b and texts_b[3] == "text 4"  # it now ties behind every other point
    for hh in (ha, hb):
        asyncio.run(hh.delete_collection("u"))
