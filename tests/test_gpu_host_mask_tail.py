"""GPU: garbage bits in the last word of a host mask (hx_hybrid_query_host_masked, hx_recommend_host, hx_discover_host).

A host mask of n rows is ceil(n / 32) words; the bits past row n - 1 of the last word are not rows.  The *_host entries
count the kept rows from the host mask (no read-back), and that count decides the route: every row kept = the unmasked
call, none kept = empty lists.  So the count must not see those bits.  100 rows = 4 words, bits 100..127 are garbage.
Every comparison is between two calls on the same index and exact: fp32 score bits, ids, counts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM, VOCAB, LIMIT = 100, 64, 50, 8
P = dict(matryoshka_64_limit=8, matryoshka_128_limit=8, matryoshka_256_limit=8, dense_limit=8, quantized_limit=8,
         sparse_limit=8, final_limit=8, hnsw_ef=128)
TAIL = np.uint32(0xFFFFFFF0)                      # bits 100..127: word 3, bits 4..31


def words(keep, garbage):
    """the packed mask of the bool array `keep` (one entry per row), with or without the bits past the last row"""
    w = np.zeros((N + 31) // 32, np.uint32)
    for r in np.flatnonzero(keep):
        w[r >> 5] |= np.uint32(1) << np.uint32(r & 31)
    if garbage:
        w[-1] |= TAIL
    return w


@pytest.fixture(scope="module")
def staged():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from rag_application_amd import engine as eng
    rng = np.random.default_rng(100)
    X = rng.standard_normal((N, DIM)).astype(np.float32)
    ip = np.arange(N + 1, dtype=np.int64) * 3                                     # three terms a row
    si = np.concatenate([rng.choice(VOCAB, 3, replace=False) for _ in range(N)]).astype(np.int32)
    sv = rng.uniform(0.5, 2.0, 3 * N).astype(np.float32)
    ix = eng.HxIndex(DIM, ())
    ix.add(X, ip, si, sv)
    ix.finalize()
    B = 3
    Q = rng.standard_normal((B, DIM)).astype(np.float32)
    qip = np.arange(B + 1, dtype=np.int64) * 3
    qsi = np.concatenate([rng.choice(VOCAB, 3, replace=False) for _ in range(B)]).astype(np.int32)
    qsv = rng.uniform(0.5, 2.0, 3 * B).astype(np.float32)
    raw = rng.standard_normal(DIM).astype(np.float32)
    reco = [[(3, 1), (17, 1), (64, -1)], [(raw, 1), (99, -1)]]                     # stored and raw examples, row 99 among them
    disc = [(5, [(21, 40)]), (None, [(99, 2), (raw, 77)])]                        # a target with a pair; context pairs only
    calls = {
        "query_tree": lambda m: ix.hybrid_query_host(Q, qip, qsi, qsv, eng.make_params(P, mode=eng.HX_MODE_TREE), mask=m),
        "query_h1": lambda m: ix.hybrid_query_host(Q, qip, qsi, qsv, eng.make_params(P, mode=eng.HX_MODE_H1), mask=m),
        "recommend_best_score": lambda m: ix.recommend_host(reco, 1, LIMIT, mask=m),
        "recommend_average": lambda m: ix.recommend_host(reco, 0, LIMIT, mask=m),
        "discover": lambda m: ix.discover_host(disc, LIMIT, mask=m),
    }
    yield calls
    ix.close()


ENTRIES = ("query_tree", "query_h1", "recommend_best_score", "recommend_average", "discover")


def same(got, want, what):
    for g, w, name in zip(got, want, ("scores", "ids", "counts")):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        np.testing.assert_array_equal(g.view(np.uint8), w.view(np.uint8), err_msg=f"{what}: {name}")


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_row_kept_and_garbage_is_the_unmasked_call(staged, entry):
    call = staged[entry]
    want = call(None)
    assert (want[2] > 0).all()                                                     # (the lists are not empty)
    same(call(words(np.ones(N, bool), True)), want, entry)


@pytest.mark.parametrize("entry", ENTRIES)
def test_scattered_rows_and_garbage_is_the_clean_mask(staged, entry):
    call = staged[entry]
    keep = np.zeros(N, bool)
    keep[np.random.default_rng(37).choice(N - 1, 36, replace=False)] = True
    keep[N - 1] = True                                                             # 37 rows; the last one sits next to the garbage
    want = call(words(keep, False))
    assert (want[2] > 0).all()
    same(call(words(keep, True)), want, entry)


@pytest.mark.parametrize("entry", ENTRIES)
def test_garbage_alone_keeps_no_row(staged, entry):
    s, i, c = staged[entry](words(np.zeros(N, bool), True))
    assert (c == 0).all(), entry
