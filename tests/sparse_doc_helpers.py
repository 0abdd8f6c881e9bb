"""Builders for the tests of the document-major sparse kernels (rag_application_amd/csrc/sprescore.hip) at the document
lengths, row lengths and vocabulary sizes where their loops change tier.

length_corpus()       A: documents of LENS terms whose matches sit at stated positions (sp_exact_score: registers for terms
                      0..63 and 64..127, memory from term 128 on, a partial last chunk), and their queries
expect_lengths()      the oracle's scores of every query of A, computed once and shared (never changed)
tie_rows() / range_pass_overflows()   the rows that push a query into the slot-per-row pass of sparse_exact_fallback
dup_cells() / dup_batch() / plain_batch()   B: batches for hx_add_sparse's checks (k_csr_unique, k_csr_check, k_minmax_f32)
vocab_corpus()        C: an index of n_live live terms and its lookups (sp_find_term_wave gains a step at 65, 4097, ...)

Used by tests/test_sparse_doc_lengths_host.py (CPU) and tests/test_gpu_sparse_doc_lengths.py (GPU)."""
import functools

import numpy as np

from oracle import oracle as O

F32 = np.float32
DIM = 64
SEED = 20            # picked once and kept: order_sensitive_fraction() is 0.51 with it (64 of 126 documents)
TERM_MAX = 2 ** 31 - 1

# ---------------------------------------------------------------------------------------------------------------------
# A. document lengths and match positions
# ---------------------------------------------------------------------------------------------------------------------
LENS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1000, 2048, 2049, 3000)
POS_FIXED = (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 192, 193)
K_MULTI = (2, 5, 8, 16, 64)          # query terms a multi-term document holds; also the T of the multi-term queries
DOCS_PER_K = 2
TIERS = (0, 64, 128, 192)            # first position of: the first register pair, the second, the first memory chunk, the rest
N_FILLER = 6000
N_ABSENT = 7                         # [0]: the negative-weight companion; [1:7]: the six extra terms of the T = 70 queries
TOUCH_MAX = 1000                     # every query touches fewer documents: no candidate list (lout >= 2048) can overflow
TIE_WEIGHT = F32(0.75)


def probe_positions(length):
    """the positions of a length class's probe documents"""
    return sorted({p for p in POS_FIXED + (length - 2, length - 1) if 0 <= p < length})


def multi_positions(rng, length, k):
    """k positions of a document of `length` terms: length - 1, the rest dealt round-robin to the tiers the document has
    (below 64, 64..127, 128..191, from 192 on), drawn without replacement inside a tier"""
    assert 1 <= k <= length
    free = []
    for a, b in zip(TIERS, TIERS[1:] + (length,)):
        cand = [p for p in range(a, min(b, length)) if p != length - 1]
        free.append(list(rng.permutation(cand)) if cand else [])
    pos = [length - 1]
    t = 0
    while len(pos) < k:
        if free[t % 4]:
            pos.append(int(free[t % 4].pop()))
        t += 1
    return sorted(pos)


class LengthCorpus:
    """CSR (indptr, idx, val; int64 / int64 / float32) of the shuffled documents, what each document is (docs[row]) and
    the terms of every length class"""

    def __init__(self, seed=SEED):
        rng = np.random.default_rng(seed)
        n_ids = len(LENS) * 65 + N_ABSENT + 1 + N_FILLER
        ids = np.unique(rng.integers(1, TERM_MAX, size=2 * n_ids))      # ids spread over [1, 2^31 - 1), unique
        ids = rng.permutation(ids)[:n_ids].astype(np.int64)
        assert len(ids) == n_ids
        take = iter(ids.tolist())
        self.probe_term = {l: next(take) for l in LENS}
        # a class's 64 query terms in the order the nested queries take them (first T of them: the T-term query)
        self.class_terms = {l: np.asarray([next(take) for _ in range(64)], np.int64) for l in LENS}
        self.absent = np.sort(np.asarray([next(take) for _ in range(N_ABSENT)], np.int64))
        self.tie_term = next(take)
        self.filler = np.asarray(list(take), np.int64)
        assert len(self.filler) == N_FILLER
        self.class_qw = {l: rng.uniform(0.1, 2.0, 64).astype(F32) for l in LENS}
        self.probe_qw = {l: F32(rng.uniform(0.1, 2.0)) for l in LENS}
        docs = []
        for l in LENS:
            for p in probe_positions(l):
                docs.append(dict(kind="probe", length=l, pos=[p], terms=np.asarray([self.probe_term[l]], np.int64)))
            if l < 5:
                continue
            for k in K_MULTI:
                if k > l:
                    continue
                for _ in range(DOCS_PER_K):
                    # the first k class terms, dealt to the (sorted) positions in an order unrelated to their ids
                    docs.append(dict(kind="multi", length=l, pos=multi_positions(rng, l, k),
                                     terms=rng.permutation(self.class_terms[l][:k])))
        order = rng.permutation(len(docs))
        self.docs = [docs[i] for i in order]
        indptr, idx, val = [0], [], []
        for d in self.docs:
            l, k = d["length"], len(d["pos"])
            row = np.empty(l, np.int64)
            mask = np.zeros(l, bool)
            mask[d["pos"]] = True
            row[mask] = d["terms"]
            row[~mask] = rng.choice(self.filler, l - k, replace=False)       # unique inside the document, shuffled
            idx.append(row)
            val.append(rng.uniform(0.5, 1.5, l).astype(F32))
            indptr.append(indptr[-1] + l)
        self.indptr = np.asarray(indptr, np.int64)
        self.idx = np.concatenate(idx)
        self.val = np.concatenate(val)
        self.n = len(self.docs)
        self.X = O.synth_dense(43, 0, self.n, DIM)
        self.queries = self._queries(rng)
        frac = order_sensitive_fraction(self)
        assert frac >= 0.25, f"only {frac:.2f} of the multi-term documents tell the two summation orders apart"

    def _queries(self, rng):
        """name -> list of (class, T, q_idx ascending int64, q_val float32); the same position in every list is the same
        query: `pos` all weights positive, T <= 64 (select pass + k_sparse_rescore); `neg` the same plus one absent term
        of weight -1 (k_sparse_range, scores unchanged); `t70` the T = 64 queries plus six absent terms of positive weight
        (T = 70 > SP_TMAX: k_sparse_range)"""
        def q(cls, terms, w, extra_t=(), extra_w=()):
            t = np.concatenate([np.asarray(terms, np.int64), np.asarray(extra_t, np.int64)])
            v = np.concatenate([np.asarray(w, F32), np.asarray(extra_w, F32)])
            o = np.argsort(t)
            return (cls, len(terms), t[o], v[o])
        w6 = rng.uniform(0.1, 2.0, 6).astype(F32)
        pos, neg, t70 = [], [], []
        for l in LENS:
            base = [([self.probe_term[l]], [self.probe_qw[l]])]
            if l >= 5:
                base += [(self.class_terms[l][:T], self.class_qw[l][:T]) for T in K_MULTI]
            for t, w in base:
                pos.append(q(l, t, w))
                neg.append(q(l, t, w, self.absent[:1], [-1.0]))
                if len(t) == 64:
                    t70.append(q(l, t, w, self.absent[1:7], w6))
        return dict(pos=pos, neg=neg, t70=t70)

    def rows(self, kind, length):
        return [r for r, d in enumerate(self.docs) if d["kind"] == kind and d["length"] == length]

    def doc(self, r):
        return self.idx[self.indptr[r]:self.indptr[r + 1]], self.val[self.indptr[r]:self.indptr[r + 1]]


def running_sum(qw, dw):
    """acc = acc + q * d from +0 in the order given: one fp32 multiply and one fp32 add per term"""
    acc = F32(0.0)
    for a, b in zip(qw, dw):
        acc = F32(acc + F32(F32(a) * F32(b)))
    return acc


def order_sensitive_fraction(c):
    """Among the multi-term documents with k >= 5: the share whose score under their class's 64-term query has other
    fp32 bits when the terms are summed in document-position order instead of ascending term id."""
    differ = total = 0
    for r, d in enumerate(c.docs):
        if d["kind"] != "multi" or len(d["pos"]) < 5:
            continue
        terms, w = c.doc(r)
        qw_of = dict(zip(c.class_terms[d["length"]].tolist(), c.class_qw[d["length"]]))
        held = [(int(terms[p]), p) for p in d["pos"]]
        by_id = [p for _, p in sorted(held)]
        a = running_sum([qw_of[int(terms[p])] for p in by_id], w[by_id])
        b = running_sum([qw_of[int(terms[p])] for p in d["pos"]], w[d["pos"]])
        differ += a.view(np.uint32) != b.view(np.uint32)
        total += 1
    return differ / total


@functools.lru_cache(maxsize=None)
def length_corpus():
    return LengthCorpus()


class Expect:
    """The oracle over a LengthCorpus and its (ids, scores) for every query of every list"""

    def __init__(self, c):
        self.c = c
        self.ora = O.OracleIndex(DIM, ())
        self.ora.add(c.X, c.indptr, c.idx, c.val)
        self.scores = {name: [self.ora.sparse_scores(t, v) for _, _, t, v in qs] for name, qs in c.queries.items()}
        for name, sc in self.scores.items():
            for (cls, T, _, _), (ids, _) in zip(c.queries[name], sc):
                assert 0 < len(ids) < TOUCH_MAX, f"{name} query of class {cls}, T = {T}: touches {len(ids)} documents"

    def top(self, name, b, L):
        ids, s = self.scores[name][b]
        return O.topk(s, ids, L)


@functools.lru_cache(maxsize=None)
def expect_lengths():
    return Expect(length_corpus())


def csr_queries(queries):
    """(q_indptr int64, q_idx int32, q_val float32) of a list of (.., .., q_idx, q_val)"""
    qip = np.cumsum([0] + [len(q[2]) for q in queries]).astype(np.int64)
    return qip, np.concatenate([q[2] for q in queries]).astype(np.int32), np.concatenate([q[3] for q in queries]).astype(F32)


def tie_rows(term, n):
    """n one-term rows that all hold `term` with one weight"""
    return np.arange(n + 1, dtype=np.int64), np.full(n, term, np.int64), np.full(n, TIE_WEIGHT, F32)


def range_pass_overflows(n_rows, first_tie, L, cap=8192):
    """Whether the first pass of sparse_exact_fallback overflows for a query on which every row from `first_tie` on ties
    (and no earlier row matches): rows in chunks of cap - L, then doubling; a chunk appends its ties behind the L keys
    kept so far, and more than `cap` keys in the buffer send the query to the slot-per-row pass."""
    r0, r1, kept = 0, min(n_rows, cap - L), 0
    while r0 < n_rows:
        ties = max(0, r1 - max(r0, first_tie))
        if kept + ties > cap:
            return True
        kept = min(kept + ties, L)
        r0, r1 = r1, min(n_rows, r1 * 2)
    return False


# ---------------------------------------------------------------------------------------------------------------------
# B. ingest checks
# ---------------------------------------------------------------------------------------------------------------------
DUP_LENS = (2, 3, 63, 64, 65, 128, 129, 1000, 2047, 2048)      # k_csr_unique compares them on the device
DUP_LENS_HOST = (2049, 5000)                                   # above CSR_UNIQUE_WAVE_MAX: sorted on the host
BATCH_AT = (0, 1, 2, 3, 8)           # the bad row's index among the nine: every wave of a workgroup, and a second workgroup
BAD_VALUES = (0, TERM_MAX)
OTHER_LENS = (0, 1, 2, 5, 63, 64, 65, 128, 200)
PLAIN_MAX = 1_900_000_000            # ordinary term ids lie in [1, PLAIN_MAX); marks and fresh ids above
MARK0 = 1_950_000_000
FRESH0 = 2_000_000_000


def dup_pairs(length):
    """the duplicate pairs (i, j) of a row of `length` terms, where they exist"""
    cand = [(0, 1), (0, length - 1), (length - 2, length - 1), (63, 64), (0, 64), (63, length - 1),
            (length // 2 // 64 * 64, length - 1)]
    out = []
    for i, j in cand:
        if 0 <= i < j < length and (i, j) not in out:
            out.append((i, j))
    return out


def dup_cells(lengths):
    """One cell per (length, pair, index in the batch); the bad value alternates with the index and starts the other way
    round on every other pair, so both values meet every index; every other cell also holds the other extreme id once."""
    cells = []
    for l in lengths:
        for pi, (i, j) in enumerate(dup_pairs(l)):
            for ai, at in enumerate(BATCH_AT):
                cells.append(dict(length=l, i=i, j=j, at=at, v=BAD_VALUES[(ai + pi) % 2], both=(ai + pi // 2) % 2 == 1))
    return cells


def plain_row(rng, length, mark=None, keep_free=()):
    """`length` unique ordinary ids, shuffled; `mark` (if given) at a position outside keep_free when there is one"""
    row = (rng.choice(PLAIN_MAX - 1, length, replace=False) + 1).astype(np.int64)
    free = [p for p in range(length) if p not in keep_free]
    if mark is not None and free:
        row[free[int(rng.integers(len(free)))]] = mark
    return row


def dup_batch(rng, cell, mark, fresh=None, n_rows=9, others=None):
    """Nine rows of mixed lengths, all valid but row cell['at']: that one holds cell['v'] at positions i and j -- or, with
    `fresh` given (the accepting twin), cell['v'] at i and the id `fresh` at j.  Every row that has room holds `mark`.
    others: the lengths of the valid rows by index in the batch (default: a rotation of OTHER_LENS).
    Returns (indptr int64, idx int32, val float32)."""
    l = cell["length"]
    rows = []
    for r in range(n_rows):
        if r != cell["at"]:
            rows.append(plain_row(rng, others[r] if others else OTHER_LENS[(r + cell["at"] + cell["i"]) % len(OTHER_LENS)], mark))
            continue
        i, j = cell["i"], cell["j"]
        other = [p for p in range(l) if p not in (i, j)]
        k = other[int(rng.integers(len(other)))] if cell["both"] and other else None
        row = plain_row(rng, l, mark, keep_free=(i, j, k))
        row[i] = cell["v"]
        row[j] = cell["v"] if fresh is None else fresh
        if k is not None:
            row[k] = TERM_MAX - cell["v"]          # the other extreme: the row holds id 0 and id 2^31 - 1
        rows.append(row)
    return pack_rows(rng, rows)


def pack_rows(rng, rows):
    indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    idx = np.concatenate(rows).astype(np.int32)
    return indptr, idx, rng.uniform(0.5, 1.5, len(idx)).astype(F32)


def plain_batch(rng, lengths, mark=None):
    return pack_rows(rng, [plain_row(rng, l, mark) for l in lengths])


def rows_unique(indptr, idx):
    return all(len(np.unique(idx[a:b])) == b - a for a, b in zip(indptr[:-1], indptr[1:]))


# ---------------------------------------------------------------------------------------------------------------------
# C. term lookup
# ---------------------------------------------------------------------------------------------------------------------
N_LIVE = (1, 2, 63, 64, 65, 66, 4096, 4097, 4161)
VOCAB_DOCS = 200


class VocabCorpus:
    """VOCAB_DOCS documents of min(64, n_live) terms over exactly n_live live terms (document d holds the live indices
    64 d .. 64 d + 63 modulo n_live, shuffled: any 100 consecutive documents hold every term when n_live <= 6400), and
    one-term queries: (term, live index or -1)."""

    def __init__(self, n_live, seed=SEED):
        rng = np.random.default_rng([seed, n_live])
        t = np.unique(rng.integers(1000, TERM_MAX - 1000, size=2 * n_live + 16))
        t = np.sort(rng.permutation(t)[:n_live]).astype(np.int64)
        assert len(t) == n_live and 64 * 100 >= n_live
        self.terms, self.n_live, self.n = t, n_live, VOCAB_DOCS
        per = min(64, n_live)
        rows = [t[rng.permutation((64 * d + np.arange(per)) % n_live)] for d in range(self.n)]
        self.indptr = np.arange(self.n + 1, dtype=np.int64) * per
        self.idx = np.concatenate(rows)
        self.val = rng.uniform(0.5, 1.5, len(self.idx)).astype(F32)
        self.X = O.synth_dense(47, 0, self.n, DIM)
        live = [0, n_live - 1, 63, 64, 65, n_live - 2, n_live - 1]
        live += rng.choice(n_live, min(12, n_live), replace=False).tolist()
        lookups = [(int(t[i]), int(i)) for i in live if 0 <= i < n_live]
        lookups += [(int(t[0]) - 7, -1), (int(t[-1]) + 7, -1)]             # below the smallest, above the largest
        gaps = np.nonzero(np.diff(t) > 1)[0]
        if len(gaps):                                                        # between two neighbours
            m = int(gaps[len(gaps) // 2])
            lookups.append((int(t[m]) + 1, -1))
        self.lookups = lookups
        self.q_val = rng.uniform(0.5, 2.0, len(lookups)).astype(F32)
        self.queries = [(None, 1, np.asarray([term], np.int64), self.q_val[b:b + 1]) for b, (term, _) in enumerate(lookups)]


@functools.lru_cache(maxsize=None)
def vocab_corpus(n_live):
    return VocabCorpus(n_live)
