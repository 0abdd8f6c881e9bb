"""The chunked host reference (oracle/full_size.py) against the numpy oracle on a corpus that fits in memory: every stage
list, the reference tree under both parameter sets and H1, ids and fp32 score bits -- with chunk sizes that cut through
tie runs and top lists.  tests/test_gpu_full_size.py trusts this reference at 10M rows."""
import numpy as np
import pytest

from oracle import full_size as FS
from oracle import oracle as O

N, DIM, NQ = 30_011, 768, 16
MSIZES = (64, 128, 256)
P_MCP = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, dense_limit=40,
             quantized_limit=40, sparse_limit=50, final_limit=30, hnsw_ef=128)


def p_fallback(n):
    # app/services/agents/hybrid_search_workflow.py:97-106
    return dict(matryoshka_64_limit=min(500, n // 10), matryoshka_128_limit=min(400, n // 15),
                matryoshka_256_limit=min(300, n // 20), dense_limit=min(200, n // 25),
                quantized_limit=min(300, n // 30), sparse_limit=min(100, n // 50), hnsw_ef=256, final_limit=10)


LIMITS = dict(dense=300, m64=500, m128=120, m256=120, i8=300, sparse=300)
SPARSE_COPIES = (7, 7000, 7001, 21003, 30005)      # document 7's sparse vector, query 0 asks for its terms


def copies(b):
    """The rows a near neighbour of query b (0..3) is copied to: both sides of the 7001-row and 30000-row boundaries."""
    return np.array([100 + b, 7000 - b, 7001 + b, 14002 + b, 29999 - b, 30000 + b])




def _replace_docs(ip, si, sv, dst, src):
    """The CSR with documents `dst` holding document src's sparse vector."""
    lens = np.diff(ip)
    segs_i = [si[ip[d]:ip[d + 1]] for d in range(len(lens))]
    segs_v = [sv[ip[d]:ip[d + 1]] for d in range(len(lens))]
    for d in dst:
        segs_i[d], segs_v[d], lens[d] = segs_i[src], segs_v[src], lens[src]
    return (np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate(segs_i), np.concatenate(segs_v))


@pytest.fixture(scope="module")
def corpus(synth_tables):
    X = O.synth_dense(O.SEED_CORPUS, 0, N, DIM)
    Q = O.synth_dense(O.SEED_QUERY, 0, NQ, DIM)
    for b in range(4):                        # exact dense / int8 ties across chunks, near the top of query b's lists
        X[copies(b)] = Q[b] + np.float32(0.01) * X[100 + b]
    ip, si, sv = O.synth_sparse_docs(O.SEED_SPDOC, 0, N, synth_tables)
    ip, si, sv = _replace_docs(ip, si, sv, SPARSE_COPIES[1:], SPARSE_COPIES[0])
    qip, qix, qv = O.synth_sparse_queries(O.SEED_SPQUERY, 0, NQ, synth_tables)
    t7 = np.sort(si[ip[7]:ip[8]])[:6]          # query 0 = six terms of document 7 (equal sparse scores across chunks)
    qix = np.concatenate([t7, qix[qip[1]:]])
    qv = np.concatenate([np.full(len(t7), 0.75, np.float32), qv[qip[1]:]])
    qip = np.concatenate([[0], qip[1:] - qip[1] + len(t7)]).astype(np.int64)
    ora = O.OracleIndex(DIM, MSIZES)
    ora.add(X, ip, si, sv)
    ora.finalize()
    return dict(X=X, Q=Q, ip=ip, si=si.astype(np.int32), sv=sv, qip=qip, qix=qix.astype(np.int32), qv=qv, ora=ora)


@pytest.fixture(scope="module")
def expected(corpus):
    """The numpy oracle's lists of every cell compare() checks, computed once."""
    ora, Q, qip, qix, qv = corpus["ora"], corpus["Q"], corpus["qip"], corpus["qix"], corpus["qv"]
    out = {}
    for b in range(NQ):
        qs, qw = qix[qip[b]:qip[b + 1]], qv[qip[b]:qip[b + 1]]
        out[("dense", b)] = ora.search_dense(Q[b], LIMITS["dense"])
        for d in MSIZES:
            out[(f"m{d}", b)] = ora.search_dense(Q[b], LIMITS[f"m{d}"], prefix=d)
        out[("i8", b)] = ora.search_i8(Q[b], LIMITS["i8"])
        out[("sparse", b)] = ora.search_sparse(qs, qw, LIMITS["sparse"])
        out[("tree mcp", b)] = O.hybrid_tree(ora, Q[b], qs, qw, P_MCP)
        out[("tree fallback", b)] = O.hybrid_tree(ora, Q[b], qs, qw, p_fallback(N))
        out[("h1", b)] = O.hybrid_h1(ora, Q[b], qs, qw, 100, 100, 10)
    return out


def reference(corpus, chunk_rows, drop_chunk=None):
    src = FS.ArraySource(corpus["X"], corpus["ip"], corpus["si"], corpus["sv"])
    return FS.FullSizeReference(src, corpus["Q"], (corpus["qip"], corpus["qix"], corpus["qv"]), LIMITS,
                                chunk_rows=chunk_rows, drop_chunk=drop_chunk)


def compare(ref, expected):
    """The cells where the reference differs from the oracle (ids or score bits; shorter L as prefixes of the longer)."""
    bad = []

    def check(what, got, want):
        gs, gi = got
        ws, wi = want
        if not (len(gi) == len(wi) and np.array_equal(gi, wi)
                and np.array_equal(np.asarray(gs, np.float32).view(np.uint32), np.asarray(ws, np.float32).view(np.uint32))):
            bad.append(what)

    for b in range(NQ):
        for name in ("dense", "m64", "m128", "m256", "i8", "sparse"):
            ws, wi = expected[(name, b)]
            check((name, b), ref.stage(name, b, LIMITS[name]), (ws, wi))
            for L in (1, 10, 100):             # a top-L list is a prefix of the top-Lmax list
                check((name, b, L), ref.stage(name, b, L), (ws[:L], wi[:L]))
        check(("tree mcp", b), ref.tree(b, P_MCP), expected[("tree mcp", b)])
        check(("tree fallback", b), ref.tree(b, p_fallback(N)), expected[("tree fallback", b)])
        check(("h1", b), ref.h1(b, 100, 100, 10), expected[("h1", b)])
    return bad


@pytest.mark.parametrize("chunk_rows", [7001, 30000])
def test_chunked_reference_equals_the_oracle(corpus, expected, chunk_rows):
    ref = reference(corpus, chunk_rows)
    assert ref.chunks == -(-N // chunk_rows)
    bad = compare(ref, expected)
    assert not bad, f"chunk {chunk_rows}: {len(bad)} cells differ from the oracle, first {bad[:8]}"


def test_planted_ties_cross_the_chunk_boundaries(corpus, expected):
    """The copies are where the test wants them: query b's dense, int8 and prefix lists open with the six equal rows
    (ascending id, across both chunkings' boundaries), and query 0's sparse list holds document 7's copies tied."""
    for b in range(4):
        want = np.sort(copies(b))
        for name in ("dense", "m64", "i8"):
            s, i = expected[(name, b)]
            np.testing.assert_array_equal(i[:len(want)], want, err_msg=f"{name} b={b}")
            assert len(set(s[:len(want)].view(np.uint32).tolist())) == 1
    s, i = expected[("sparse", 0)]
    pos = np.isin(i, SPARSE_COPIES)
    assert pos.sum() == len(SPARSE_COPIES) and len(set(s[pos].view(np.uint32).tolist())) == 1
    np.testing.assert_array_equal(i[pos], np.array(SPARSE_COPIES))


def test_a_dropped_chunk_is_seen(corpus, expected):
    """The comparison can fail: the same pass without its second chunk (rows 7001..14001, one copy of every planted tie)
    must differ from the oracle -- in the stage lists, the tree and H1 alike."""
    bad = compare(reference(corpus, 7001, drop_chunk=1), expected)
    kinds = {c[0] for c in bad}
    assert {"dense", "m64", "i8", "sparse", "tree mcp", "h1"} <= kinds, kinds
