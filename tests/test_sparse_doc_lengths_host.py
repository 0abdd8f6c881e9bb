"""CPU: what tests/test_gpu_sparse_doc_lengths.py takes for granted about its inputs (tests/sparse_doc_helpers.py), and the
oracle's sparse score on three documents worked out by hand."""
import numpy as np

from oracle import oracle as O
from tests import sparse_doc_helpers as H

F32 = np.float32


def test_every_length_and_position_cell_is_present():
    """Per length class: one probe document per stated position with the probe term exactly there; multi-term documents
    for every k the length allows, holding the first k class terms at their stated positions -- length - 1 among them and
    one in every tier the document has."""
    c = H.length_corpus()
    assert c.n == len(c.docs) and 200 <= c.n <= 500 and len(c.idx) <= 300000
    for l in H.LENS:
        want = [p for p in (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 192, 193, l - 2, l - 1) if 0 <= p < l]
        got = []
        for r in c.rows("probe", l):
            terms, w = c.doc(r)
            (p,) = c.docs[r]["pos"]
            assert len(terms) == l and terms[p] == c.probe_term[l] and (terms == c.probe_term[l]).sum() == 1
            got.append(p)
        assert sorted(got) == sorted(set(want)), l
        ks = sorted(len(c.docs[r]["pos"]) for r in c.rows("multi", l))
        assert ks == sorted(k for k in H.K_MULTI if l >= 5 and k <= l for _ in range(H.DOCS_PER_K)), l
        for r in c.rows("multi", l):
            terms, w = c.doc(r)
            d = c.docs[r]
            k = len(d["pos"])
            assert len(terms) == l and l - 1 in d["pos"]
            assert set(terms[d["pos"]].tolist()) == set(c.class_terms[l][:k].tolist())
            tiers = {sum(p >= t for t in H.TIERS) for p in d["pos"]}
            assert tiers == {sum(p >= t for t in H.TIERS) for p in range(l)} or k < 4, (l, k, d["pos"])
            if k >= 8:       # placed in an order unrelated to the ids
                held = terms[d["pos"]]
                assert (np.diff(held) < 0).any() and (np.diff(held) > 0).any()


def test_ids_are_unique_and_filler_is_disjoint_from_the_queries():
    c = H.length_corpus()
    assert H.rows_unique(c.indptr, c.idx)
    query_terms = set(c.probe_term.values()) | {int(t) for l in H.LENS for t in c.class_terms[l]}
    query_terms |= set(c.absent.tolist()) | {c.tie_term}
    assert len(query_terms) == len(H.LENS) * 65 + H.N_ABSENT + 1
    assert not query_terms & set(c.filler.tolist())
    assert not (set(c.absent.tolist()) | {c.tie_term}) & set(c.idx.tolist())       # held by no document
    for r, d in enumerate(c.docs):
        terms, w = c.doc(r)
        mask = np.ones(len(terms), bool)
        mask[d["pos"]] = False
        assert np.isin(terms[mask], c.filler).all()
        if len(terms) >= 64:
            assert (np.diff(terms) < 0).any()                                      # not ascending
        assert (w >= 0.5).all() and (w < 1.5).all()
    for name, qs in c.queries.items():
        for cls, T, t, v in qs:
            assert (np.diff(t) > 0).all() and t.min() >= 0 and t.max() <= H.TERM_MAX
            extra = len(t) - T
            assert extra == dict(pos=0, neg=1, t70=6)[name]
            assert ((v > 0).all() and len(t) <= 64) if name == "pos" else ((v <= 0).sum() == 1 if name == "neg" else len(t) == 70)


def test_the_two_summation_orders_are_told_apart():
    """At least a quarter of the multi-term documents with k >= 5 get other fp32 bits when summed in document-position
    order: a kernel that adds the matches as it finds them cannot pass."""
    assert H.order_sensitive_fraction(H.length_corpus()) >= 0.25


def test_queries_touch_what_they_should():
    """Every query touches fewer than TOUCH_MAX documents (asserted by Expect); a single-term query touches exactly its
    class's probe documents, a multi-term query every multi-term document of its class; the twins score as the originals."""
    e = H.expect_lengths()
    c = e.c
    for b, (cls, T, t, v) in enumerate(c.queries["pos"]):
        ids, s = e.scores["pos"][b]
        kind = "probe" if (T == 1 and t[0] == c.probe_term[cls]) else "multi"
        assert ids.tolist() == c.rows(kind, cls), (cls, T)
        ids2, s2 = e.scores["neg"][b]
        assert np.array_equal(ids, ids2) and np.array_equal(s.view(np.uint32), s2.view(np.uint32))
    full = [b for b, q in enumerate(c.queries["pos"]) if q[1] == 64]
    assert len(full) == len(c.queries["t70"]) == 16
    for b70, b in enumerate(full):
        assert np.array_equal(e.scores["pos"][b][1].view(np.uint32), e.scores["t70"][b70][1].view(np.uint32))


def test_range_pass_model():
    """The first pass of sparse_exact_fallback at limit 10: 8182 rows, 8182 more (10 + 8182 keys fill the 8192 slots
    exactly), then the rest -- it overflows once more than 8182 tied rows lie behind row 16364."""
    n0 = H.length_corpus().n
    assert not H.range_pass_overflows(n0 + 20000, n0, 10)
    assert not H.range_pass_overflows(16364 + 8182, n0, 10)
    assert H.range_pass_overflows(16364 + 8183, n0, 10)
    assert H.range_pass_overflows(n0 + 25000, n0, 10)


def test_ingest_cells():
    """B's cells: every length has its pairs, every pair meets every index of the batch, both bad values meet every index;
    the refused batch repeats an id in exactly one row and its twin in none."""
    assert H.dup_pairs(2) == [(0, 1)] and H.dup_pairs(3) == [(0, 1), (0, 2), (1, 2)]
    assert H.dup_pairs(65) == [(0, 1), (0, 64), (63, 64)]
    assert H.dup_pairs(129) == [(0, 1), (0, 128), (127, 128), (63, 64), (0, 64), (63, 128), (64, 128)]
    assert H.dup_pairs(2048) == [(0, 1), (0, 2047), (2046, 2047), (63, 64), (0, 64), (63, 2047), (1024, 2047)]
    cells = H.dup_cells(H.DUP_LENS + H.DUP_LENS_HOST)
    assert {(c["at"], c["v"]) for c in cells} == {(a, v) for a in H.BATCH_AT for v in H.BAD_VALUES}
    assert {c["both"] for c in cells if c["length"] in (64, 128, 2048)} == {False, True}
    rng = np.random.default_rng(3)
    for k, cell in enumerate(cells[::7]):
        ip, ix, v = H.dup_batch(rng, cell, H.MARK0 + 1)
        a, b = ip[cell["at"]], ip[cell["at"] + 1]
        assert len(ip) == 10 and b - a == cell["length"] and ix[a + cell["i"]] == ix[a + cell["j"]] == cell["v"]
        bad = [r for r in range(9) if len(np.unique(ix[ip[r]:ip[r + 1]])) != ip[r + 1] - ip[r]]
        assert bad == [cell["at"]] and ix.min() >= 0
        ip, ix, v = H.dup_batch(rng, cell, H.MARK0 + 1, fresh=H.FRESH0 + k)
        assert H.rows_unique(ip, ix) and (ix == H.FRESH0 + k).sum() == 1 and ix[ip[cell["at"]] + cell["j"]] == H.FRESH0 + k
        if cell["both"] and cell["length"] >= 3:
            assert {0, H.TERM_MAX} <= set(ix[a:b].tolist())


def test_vocabularies():
    for n_live in H.N_LIVE:
        v = H.vocab_corpus(n_live)
        assert np.array_equal(np.unique(v.idx), v.terms) and len(v.terms) == n_live and H.rows_unique(v.indptr, v.idx)
        assert np.array_equal(np.unique(v.idx[v.indptr[100]:]), v.terms)             # the last 100 documents hold them all
        assert np.array_equal(np.unique(v.idx[:v.indptr[100]]), v.terms)
        want = {i for i in (0, 63, 64, 65, n_live - 2, n_live - 1) if 0 <= i < n_live}
        assert want <= {i for _, i in v.lookups}
        absent = [t for t, i in v.lookups if i < 0]
        assert len(absent) == (3 if n_live >= 2 else 2) and not np.isin(absent, v.terms).any()
        assert absent[0] < v.terms[0] and absent[1] > v.terms[-1] and (len(absent) < 3 or v.terms[0] < absent[2] < v.terms[-1])
        for t, i in v.lookups:
            assert i < 0 or v.terms[i] == t


def test_oracle_scores_three_documents_by_hand():
    """sparse_scores is the spec: terms in ascending id, acc = f32(acc + f32(q * d)) from +0.
    doc 0 holds terms 30, 10, 20 (in that order) with weights -1e8, 1e8, 1 under query weights 1, 1, 1: ascending id gives
        (0 + 1e8) + 1 = 1e8 (the 1 is below half an ulp of 8), then 1e8 - 1e8 = 0; document order would give 1.
    doc 1 holds term 20 with 4097 and term 10 with 1; query 10 -> 1, 20 -> 4097, 30 -> 1: 0 + 1 = 1, then
        4097 * 4097 = 2^24 + 2^13 + 1 rounds to 2^24 + 2^13 (tie, to even) and 1 + 16785408 = 16785409 rounds to 16785408
        again; in the other order the product comes first and the result is the same, so this one pins the rounding only.
    doc 2 holds only term 40 (not in the query): untouched.  doc 3 holds term 30 with 0.5 under weight 1.5: 0.75."""
    ora = O.OracleIndex(4, ())
    ip = np.asarray([0, 3, 5, 6, 7], np.int64)
    ora.add(np.ones((4, 4), F32), ip, np.asarray([30, 10, 20, 20, 10, 40, 30], np.int64),
            np.asarray([-1e8, 1e8, 1.0, 4097.0, 1.0, 9.0, 0.5], F32))
    ids, s = ora.sparse_scores([30, 10, 20], [1.0, 1.0, 1.0])            # given unsorted: the oracle sorts by id
    assert ids.tolist() == [0, 1, 3] and s.dtype == F32
    assert s[0] == F32(0.0) and s[1] == F32(4098.0) and s[2] == F32(0.5)
    ids, s = ora.sparse_scores([10, 20, 30], [1.0, 4097.0, 1.5])
    assert ids.tolist() == [0, 1, 3]
    assert s[1] == F32(16785408.0) and s[1].view(np.uint32) == 0x4B801000
    assert s[2] == F32(0.75)
    # doc 0 under these weights: 1e8, then 1e8 + 4097 = 100004097 -> the nearest fp32 (ulp 8) is 100004096,
    # then 100004096 - 1.5e8 = -49995904 exactly
    assert s[0] == F32(-49995904.0)
    es, ei = ora.search_sparse([10, 20, 30], [1.0, 4097.0, 1.5], 2)
    assert ei.tolist() == [1, 3]
