"""GPU: the sparse select pass (sparse2.hip, sprescore.hip, shardx.hip) against its integer model and its margin.

The corpora come from tests/sparse_bracket_helpers.py: per limit L one corpus that holds the (T, L) cells of every
T in T_GPU (both sides of each step of T / 16) on disjoint term ranges, so the T-cells of one L are ONE batch.  In every
cell with T >= 15 the exact top-L lies T - 6 .. T - 4 integer units under the L-th best integer score (measured on the CPU:
tests/test_sparse_bracket_host.py) -- the lists below are right only if the scores, the cut and the margin all are.
Each corpus exists unpadded (one segment; 2400 background documents per cell keep the 11 cells of L = 256 under 32768
rows) and padded to 70,000 rows with rows of one non-query term (three segments of 32768, two of 65536).

What each test must take, stated through the route counter `sparse_fallback_queries` read around every call:
  integer scores, exact lists, both H1 paths      the select pass: the counter does not move (every margin set, with the
                                                  histogram's 3 units of slack, is below lout = 2048: checked per cell)
  lout boundary                                   per query what select_model (the helper's restatement of sp_cut,
                                                  the union of the parts and k_sparse_rescore) says of its margin set
  plateau                                         0 at lout - 1 keys, 1 per query at lout and lout + 1

CPU-measured disagreement of the cells used here (seed 2, 2400 background documents; gap = a_L - lowest integer score
in the exact top-L, inverted = exact top-L documents of integer rank >= L, keep = |{a > a_L - M - 3}|), unpadded corpus:
      T   M |  L = 10: gap inverted keep |  L = 100: gap inverted keep |  L = 256: gap inverted keep
      1   5 |           0     0      93  |            0     0     268  |            0     0     584
      2   6 |           0     0      98  |            0     0     291  |            0     0     590
     15  19 |          12    10     186  |           11   100     389  |           10   256     744
     16  21 |          13    10     196  |           12   100     413  |           11   256     733
     17  22 |          14    10     218  |           12   100     429  |           12   256     770
     31  36 |          28    10     311  |           27   100     498  |           26   256     827
     32  38 |          29    10     342  |           27   100     521  |           27   256     829
     47  53 |          44    10     400  |           42   100     619  |           42   256     942
     48  55 |          45    10     453  |           44   100     637  |           43   256     931
     63  70 |          59    10     510  |           57   100     738  |           57   256    1048
     64  72 |          60    10     522  |           59   100     738  |           58   256    1075

Searched at other limits than they were made for (300 and 1000 as well) the same cells keep at most 1906 keys.  The
boundary corpus (one T = 64 cell made for L = 1000 with 3000 background documents) has margin sets of 2579 keys at
L = 1000 and 3376 at L = 1323 and 1324 -- over lout = 2048, under lout = 4096 -- and 3443 at L = 2047 and 2048."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import sparse_bracket_helpers as H
from tests.test_gpu_parity import assert_list_equal, unpack_np
from tests.test_gpu_shard_exchange import _cf_exchange

pytestmark = pytest.mark.gpu

SEED, N_BG, PAD_TO, DIM, LOUT = 2, 2400, 70000, 64, 2048
L_GEN = (10, 100, 256)                 # hx_h1_plan at world 1 takes sparse_limit <= 256
L_SEARCH = (10, 100, 300, 1000)
CAND_CAP = 8192
HSHIFT = {32768: 2, 65536: 1}          # sparse2.hip SP_HSHIFT: the histogram's bins hold 4 / 2 scores
U64 = np.uint64

@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def eng():
    from rag_application_amd import engine
    return engine


class Host:
    """A corpus with everything the CPU knows about it: the integer model and the exact scores of every query, computed
    once and shared (never changed)."""

    def __init__(self, corpus, queries=None):
        self.c = corpus
        self.queries = corpus.queries if queries is None else queries
        self.X = O.synth_dense(41, 0, corpus.n, DIM)
        self.ora = O.OracleIndex(DIM, ())
        self.ora.add(self.X, corpus.indptr, corpus.idx, corpus.val)
        self.models = [H.int_model(qi, qv, corpus.indptr, corpus.idx, corpus.val, H.W_SENTINEL) for qi, qv in self.queries]
        # the call test_sparse_select_paths makes (ora.search_sparse) is topk over these
        self.scores = [self.ora.sparse_scores(qi, qv) for qi, qv in self.queries]
        self.qip = np.cumsum([0] + [len(q[0]) for q in self.queries]).astype(np.int64)
        self.qix = np.concatenate([np.asarray(q[0], np.int32) for q in self.queries])
        self.qv = np.concatenate([np.asarray(q[1], np.float32) for q in self.queries])

    def top(self, b, L, rows_below=None):
        ids, s = self.scores[b]
        if rows_below is not None:
            sel = ids < rows_below
            ids, s = ids[sel], s[sel]
        return O.topk(s, ids, L)

    def tq(self, torch_mod):
        return (torch_mod.from_numpy(self.qip).cuda(), torch_mod.from_numpy(self.qix).cuda(), torch_mod.from_numpy(self.qv).cuda())


@functools.lru_cache(maxsize=None)
def host(L, padded):
    return Host(H.adversarial_corpus(H.T_GPU, L, SEED, n_bg=N_BG, pad_to=PAD_TO if padded else 0))


def make_index(eng, monkeypatch, seg_docs, hst, rows=None, tail_min=None):
    monkeypatch.setenv("HX_DEBUG_SEG_DOCS", str(seg_docs))
    if tail_min is not None:
        monkeypatch.setenv("HX_DEBUG_TAIL_MIN", str(tail_min))
    ix = eng.HxIndex(DIM, ())
    c = hst.c
    n = c.n if rows is None else rows
    ix.add(hst.X[:n], c.indptr[:n + 1], c.idx[:c.indptr[n]].astype(np.int32), c.val[:c.indptr[n]])
    return ix


def n_segments(n, seg_docs):
    return (n + seg_docs - 1) // seg_docs


def rows_of(keys):
    return (U64(0xFFFFFFFF) - (keys & U64(0xFFFFFFFF))).astype(np.int64)


def fallbacks(ix):
    return ix.stats()["sparse_fallback_queries"]


def assert_select_serves(hst, b, L, what):
    """precondition of a cell that must take the select pass: its margin set, with the histogram's slack, fits the list"""
    assert len(H.keep_rows(hst.models[b], L, slack=3)) < LOUT, what


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", L_GEN)
@pytest.mark.parametrize("padded", [False, True], ids=["one_segment", "padded_70000"])
@pytest.mark.parametrize("seg_docs", [32768, 65536])
def test_integer_scores_key_by_key(eng, torch_mod, monkeypatch, seg_docs, padded, L):
    """hx_h1_nominate_async leaves the shard's whole integer-score list in the private tail of its result (shardx.hip
    k_h1x_pack: query b's list at word B (k1 + k2 + 2) + b lout, its length at B (k1 + k2 + 2) + B lout + b, a key =
    a << 32 | 0xFFFFFFFF - row).  Every listed score equals the CPU restatement's as an integer; the list is strictly
    descending, holds {a > a_L - M} and -- on one segment, where one workgroup makes one cut -- is exactly
    {a >= sp_thr(lower edge of the bin of a_L, M)}, inside {a > a_L - M - 3}: a looser list would mean sp_cut lost its
    threshold.  The k2 public keys are the head of the list; meta1 carries no flag, the list's length and wmax = 4.0.
    Path: the select pass serves all 11 queries (flag bit 0, the fallback counter does not move)."""
    hst = host(L, padded)
    B = len(hst.queries)
    ix = make_index(eng, monkeypatch, seg_docs, hst)
    assert ix.sparse_wmax() == (H.W_SENTINEL, False)
    k1, k2, lp, k3, lout = eng.h1_plan(10, L, 1)
    assert lout == LOUT
    Qd = torch_mod.from_numpy(O.synth_dense(O.SEED_QUERY, 0, B, DIM)).cuda()
    f0 = fallbacks(ix)
    nom = ix.h1_nominate_async(Qd, *hst.tq(torch_mod), 10, L, k1, k2, lout)
    torch_mod.cuda.synchronize()
    st = ix.stats()
    assert hst.c.n == PAD_TO if padded else hst.c.n <= 32768
    assert st["n_segments"] == ((3 if seg_docs == 32768 else 2) if padded else 1)
    assert st["sparse_fallback_queries"] == f0
    w = nom.cpu().numpy().view(np.uint64)
    priv = B * (k1 + k2 + 2)
    for b in range(B):
        T = len(hst.queries[b][0])
        what = f"seg={seg_docs} padded={padded} L={L} T={T}"
        m = hst.models[b]
        assert_select_serves(hst, b, L, what)
        meta1 = int(w[B * (k1 + k2) + 2 * b + 1])
        n_list = int(w[priv + B * lout + b])
        assert (meta1 >> 31) & 1 == 0, what
        assert np.asarray([meta1 >> 32], np.uint32).view(np.float32)[0] == np.float32(H.W_SENTINEL), what
        assert meta1 & 0x7FFFFFFF == n_list and 0 < n_list < lout, what
        keys = w[priv + b * lout: priv + b * lout + n_list]
        assert (keys[1:] < keys[:-1]).all(), what + ": list not strictly descending"
        rows, a = rows_of(keys), (keys >> U64(32)).astype(np.int64)
        assert rows.max() < hst.c.n and (m["a_of"][rows] > 0).all(), what + ": a listed row shares no term with the query"
        diff = np.nonzero(a != m["a_of"][rows])[0]
        assert len(diff) == 0, (what, "integer scores differ", rows[diff][:8], a[diff][:8], m["a_of"][rows][diff][:8])
        listed = set(rows.tolist())
        assert set(H.keep_rows(m, L).tolist()) <= listed, what + ": a row of {a > a_L - M} is missing"
        if not padded:
            assert listed <= set(H.keep_rows(m, L, slack=3).tolist()), what + ": rows beyond a_L - M - 3"
            exp = H.part_list(m["a"], m["rows"], L, m["M"], HSHIFT[seg_docs])
            np.testing.assert_array_equal(keys, exp, err_msg=what + ": sp_cut's threshold")
        pub = w[B * k1 + b * k2: B * k1 + (b + 1) * k2]
        h = min(k2, n_list)
        np.testing.assert_array_equal(pub[:h], keys[:h], err_msg=what + ": public keys")
        assert (pub[h:] == 0).all(), what
    ix.close()


@pytest.mark.parametrize("L_gen", L_GEN)
@pytest.mark.parametrize("padded", [False, True], ids=["unpadded", "padded_70000"])
@pytest.mark.parametrize("seg_docs", [32768, 65536])
def test_exact_lists_under_disagreement(eng, torch_mod, monkeypatch, seg_docs, padded, L_gen):
    """hx_search_sparse over the same corpora and T-cells at L = 10, 100, 300, 1000: ids and fp32 score bits of the
    oracle (upstream arithmetic, the call test_sparse_select_paths makes), although rank L of the integer order is
    nowhere near rank L of the exact one.  Path: the select pass for every query of every batch -- the fallback counter
    does not move (these cells test the pass, not the document-at-a-time path behind it)."""
    hst = host(L_gen, padded)
    B = len(hst.queries)
    ix = make_index(eng, monkeypatch, seg_docs, hst)
    tq = hst.tq(torch_mod)
    for L in L_SEARCH:
        for b in range(B):
            assert_select_serves(hst, b, L, f"L_gen={L_gen} L={L} b={b}")
        f0 = fallbacks(ix)
        s, i, c = unpack_np(eng, *ix.search_sparse(*tq, L))
        assert fallbacks(ix) == f0, f"L_gen={L_gen} L={L}: a query left the select pass"
        for b in range(B):
            es, ei = hst.top(b, L)
            assert_list_equal(s[b], i[b], c[b], es, ei, f"seg={seg_docs} padded={padded} L_gen={L_gen} L={L} T={len(hst.queries[b][0])}")
    assert ix.stats()["n_segments"] == n_segments(hst.c.n, seg_docs)
    ix.close()


@pytest.mark.parametrize("padded", [False, True], ids=["unpadded", "padded_70000"])
@pytest.mark.parametrize("seg_docs", [32768, 65536])
def test_h1_paths_under_disagreement(eng, torch_mod, monkeypatch, seg_docs, padded):
    """The L = 100 cells through both H1 paths -- hx_hybrid_query in H1 mode, and the candidates-first exchange at world
    1 (nominate, k_h1x_cuts' global threshold a_L - M + 1 on the shard's own list, finish) -- against O.hybrid_h1 with
    dense_limit 100, sparse_limit 100, final 10.  Path: the select pass (the fallback counter does not move, and the
    exchange flags no query for the per-shard redo)."""
    dl = sl = 100
    hst = host(100, padded)
    B = len(hst.queries)
    ix = make_index(eng, monkeypatch, seg_docs, hst)
    Q = O.synth_dense(O.SEED_QUERY, 0, B, DIM)
    Qd = torch_mod.from_numpy(Q).cuda()
    tq = hst.tq(torch_mod)
    exp = [O.hybrid_h1(hst.ora, Q[b], *hst.queries[b], dl, sl, 10) for b in range(B)]
    hp = eng.make_params(dict(matryoshka_64_limit=1, matryoshka_128_limit=1, matryoshka_256_limit=1, dense_limit=dl,
                              quantized_limit=1, sparse_limit=sl, final_limit=10, hnsw_ef=1), mode=eng.HX_MODE_H1)
    f0 = fallbacks(ix)
    s, i, c = unpack_np(eng, *ix.hybrid_query(Qd, *tq, hp))
    assert fallbacks(ix) == f0
    for b in range(B):
        assert_list_equal(s[b], i[b], c[b], *exp[b], f"hybrid h1 seg={seg_docs} padded={padded} b={b}")
    k1, k2, lp, k3, lout = eng.h1_plan(dl, sl, 1)
    keys, cnt, nfail, flags = _cf_exchange(eng, torch_mod, [ix], Qd, tq, dl, sl, 10, k1, k2, lp, k3, lout, flags=True)
    assert (flags & (4 | 8 | 16 | 32) == 0).all(), flags          # no sparse flag, cut, list or scale complaint
    s, i, c = unpack_np(eng, keys, cnt)
    assert fallbacks(ix) == f0
    # a list the exchange reports as final is the oracle's (nfail counts the queries it hands back for the per-shard redo;
    # only the dense certificate can ask for one here)
    differ = sum(1 for b in range(B) if c[b] != len(exp[b][1]) or not np.array_equal(i[b, :c[b]], exp[b][1])
                 or not np.array_equal(s[b, :c[b]].view(np.uint32), exp[b][0].view(np.uint32)))
    assert differ <= nfail, f"candidates-first seg={seg_docs} padded={padded}: {differ} lists differ, {nfail} flagged"
    ix.close()


# ---------------------------------------------------------------------------------------------------------------------
N_BASE = 66000


@functools.lru_cache(maxsize=None)
def host_boundary():
    """One T = 64 cell made for L = 1000 (1050 inflated, 1000 deflated, 3000 background documents) in 70,000 rows, the
    sentinel among the first 66,000; the heavy query beside 15 one-term queries on the cell's first 15 terms."""
    c = H.adversarial_corpus([64], 1000, SEED, n_bg=3000, pad_to=PAD_TO, sentinel_below=N_BASE)
    qi, qv = c.queries[0]
    rng = np.random.default_rng(5)
    queries = [(qi, qv)] + [(qi[t:t + 1], rng.uniform(0.5, 2.0, 1).astype(np.float32)) for t in range(15)]
    return Host(c, queries)


def predicted_failures(hst, L, seg_docs, n_base, n_all):
    """Per query whether the select pass hands it to the exact path (H.select_model), for the parts the launch can cut
    it into: a part of the tail index beside 1 .. pt_max parts of the base (sparse_select_lists: pt_cap = 8192 / lout,
    one of them for the tail).  The verdict must not depend on the plan's choice, or the cell proves nothing."""
    lout = max(2048, 1 << int(np.ceil(np.log2(L + L // 2 + 64))))
    pt_max = max(1, min(CAND_CAP // lout - 1, n_segments(n_base, seg_docs)))
    out = []
    for b, m in enumerate(hst.models):
        verdicts = set()
        for qp in range(1, pt_max + 1):
            parts = H.base_parts(n_base, seg_docs, qp) + [(n_base, n_all)]
            verdicts.add(H.select_model(m, L, lout, HSHIFT[seg_docs], parts)[2])
        assert len(verdicts) == 1, f"L={L} b={b}: the verdict depends on the plan"
        out.append(verdicts.pop())
    return lout, out


@pytest.mark.parametrize("seg_docs", [32768, 65536])
def test_lout_boundary_with_parts_and_a_tail(eng, torch_mod, monkeypatch, seg_docs):
    """sparse_lout(L) goes from 2048 to 4096 between L = 1323 and 1324: pt_cap = 8192 / lout halves (4 -> 2), so the base
    index is walked by up to 3 workgroups per query beside the tail's one, then by a single workgroup over all its
    segments (cuts between visits) beside the tail's.  66,000 rows are added and searched (base index: 3 segments of
    32768 / 2 of 65536), then 4,000 more (a tail index of one segment: 4 / 3 segments in all), so the adversarial
    documents sit in base segments and in the tail.  One 64-term query beside 15 one-term queries: the heavy one holds
    most of the batch's postings and k_sparse_plan cuts it into the most parts it may.  L = 1000, 1323 (lout 2048) and
    1324, 2047, 2048 (lout 4096) against the oracle; which queries overflow into the exact path is decided per query from
    the CPU restatement and the counter must move by exactly that many."""
    hst = host_boundary()
    B, n = len(hst.queries), hst.c.n
    assert n == PAD_TO
    ix = make_index(eng, monkeypatch, seg_docs, hst, rows=N_BASE, tail_min=1000000)
    tq = hst.tq(torch_mod)
    s, i, c = unpack_np(eng, *ix.search_sparse(*tq, 100))
    for b in range(B):
        assert_list_equal(s[b], i[b], c[b], *hst.top(b, 100, rows_below=N_BASE), f"base only seg={seg_docs} b={b}")
    assert ix.stats()["n_segments"] == n_segments(N_BASE, seg_docs) == (3 if seg_docs == 32768 else 2)
    cc = hst.c
    ix.add(hst.X[N_BASE:], cc.indptr[N_BASE:] - cc.indptr[N_BASE], cc.idx[cc.indptr[N_BASE]:].astype(np.int32),
           cc.val[cc.indptr[N_BASE]:])
    assert ix.sparse_wmax() == (H.W_SENTINEL, False)
    louts, moved = set(), {}
    for L in (1000, 1323, 1324, 2047, 2048):
        lout, fails = predicted_failures(hst, L, seg_docs, N_BASE, n)
        louts.add(lout)
        f0 = fallbacks(ix)
        s, i, c = unpack_np(eng, *ix.search_sparse(*tq, L))
        moved[L] = (fallbacks(ix) - f0, sum(fails))
        for b in range(B):
            assert_list_equal(s[b], i[b], c[b], *hst.top(b, L), f"seg={seg_docs} L={L} b={b} (predicted fail: {fails[b]})")
    assert ix.stats()["n_segments"] == n_segments(N_BASE, seg_docs) + 1
    assert louts == {2048, 4096}
    assert all(got == want for got, want in moved.values()), f"fallbacks (observed, predicted) per L: {moved}"
    ix.close()


# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_plateau():
    """Three one-term cells (terms 1000, 2000, 3000) for L = 100: 99 documents with distinct higher weights
    (1.01 .. 1.99: a steps by 164), P documents at weight 1.0 (a = 16382), 400 documents at 0.1 .. 0.8 (more than 3000
    units below), P = lout - 1 - 99, lout - 99, lout + 1 - 99; plus the sentinel.  Rows shuffled."""
    rng = np.random.default_rng(6)
    idx, val = [], []
    for cell_, P in enumerate((LOUT - 100, LOUT - 99, LOUT - 98)):
        w = np.concatenate([1.0 + 0.01 * np.arange(1, 100), np.full(P, 1.0), rng.uniform(0.1, 0.8, 400)])
        idx.append(np.full(len(w), 1000 * (cell_ + 1), np.int64))
        val.append(w.astype(np.float32))
    idx = np.concatenate(idx + [np.asarray([H.SENT_TERM], np.int64)])
    val = np.concatenate(val + [np.asarray([H.W_SENTINEL], np.float32)])
    perm = rng.permutation(len(idx))
    c = H.Corpus(np.arange(len(idx) + 1, dtype=np.int64), idx[perm], val[perm], [], [])
    queries = [(np.asarray([1000 * (k + 1)], np.int64), np.asarray([1.5], np.float32)) for k in range(3)]
    return Host(c, queries)


@pytest.mark.parametrize("seg_docs", [32768, 65536])
def test_plateau_at_the_edge_of_the_list(eng, torch_mod, monkeypatch, seg_docs):
    """A one-term query, L = 100, whose rank 100 falls into a plateau of P documents with one weight: the margin set
    {a > a_L - M} is the 99 documents above plus the plateau (nothing else within 3000 units), lout - 1, lout and
    lout + 1 keys.  The lists equal the oracle's in all three cells (rank 100 on: the plateau by ascending id).
    By the code: k_sparse_select's final write fails a query only when its part kept MORE than lout keys (nk > a.lout),
    and k_sparse_rescore fails it when the candidate prefix fills the list (lo == a.stride) -- so lout - 1 keys are
    served by the select pass (the counter moves by 0), lout keys fail in the rescore step and lout + 1 in the select
    pass: 1 per query.  Each cell is searched as a batch of two equal queries: 0, 2, 2."""
    hst = host_plateau()
    ix = make_index(eng, monkeypatch, seg_docs, hst)
    assert n_segments(hst.c.n, seg_docs) == 1
    for k, want in enumerate((0, 2, 2)):
        m = hst.models[k]
        n_margin = len(H.keep_rows(m, 100))
        assert n_margin == len(H.keep_rows(m, 100, slack=3)) == LOUT - 1 + k
        assert H.select_model(m, 100, LOUT, HSHIFT[seg_docs], [(0, hst.c.n)])[2] == (want > 0)
        qi, qv = hst.queries[k]
        qip = torch_mod.tensor([0, 1, 2], dtype=torch_mod.int64).cuda()
        qix = torch_mod.from_numpy(np.concatenate([qi, qi]).astype(np.int32)).cuda()
        qvv = torch_mod.from_numpy(np.concatenate([qv, qv])).cuda()
        f0 = fallbacks(ix)
        s, i, c = unpack_np(eng, *ix.search_sparse(qip, qix, qvv, 100))
        moved = fallbacks(ix) - f0
        es, ei = hst.top(k, 100)
        assert len(np.unique(es.view(np.uint32)[:99])) == 99 and es[99] < es[98]      # the list ends inside the plateau
        for b in range(2):
            assert_list_equal(s[b], i[b], c[b], es, ei, f"plateau seg={seg_docs} margin set {n_margin} keys b={b}")
        assert moved == want, f"margin set of {n_margin} keys (lout = {LOUT}): sparse_fallback_queries moved by {moved}"
    assert ix.stats()["n_segments"] == 1
    ix.close()
