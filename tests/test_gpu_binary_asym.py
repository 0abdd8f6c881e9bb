"""GPU: the asymmetric binary stage (hx_search_bin_asym, k_asym_queries, k_asym_scan) against the
numpy model of tests/binary_asym_helpers.py, key for key: ids, fp32 score bits, counts, zero slots behind the count -- at 4
and at 8 query bits.  The query kernel is held to the model through hx_bin_asym_debug_query, plane by plane.  The shapes
are the smallest that reach each path: one row, the wave's and the tile's boundaries, several tiles, every (planes,
queries per walk) form with a partial last group and several groups over a resident tile, rows of two staging passes, the
grid-stride loop; a second index under HX_DEBUG_BIN_CHUNK0 / HX_DEBUG_BIN_CAP takes several chunks, compacts its buffers
more than once and reaches the overflow redo."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import binary_asym_helpers as AH
from tests import binary_helpers as BH
from tests.test_gpu_binary import KNOBS, dev, make_index, rows_of

pytestmark = pytest.mark.gpu

BITS = (4, 8)
BS = (1, 2, 3, 5, 9, 33)         # 8 planes: 1 or 2 queries per walk; 4 planes: 1, 2 or 4 -- every form, a partial last group
HALF8 = [127, .5, 1.5, 2.5, -.5, -1.5, -127, 63.5]           # codes 127, 0, 2, 2, 0, -2, -127, 64 at 8 bits
HALF4 = [7, .5, 1.5, 2.5, -3.5, -7, 3.4999, 0]               # codes 7, 0, 2, 2, -4, -7, 3, 0 at 4 bits


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from rag_application_amd import engine
    return engine


def run(ix, Q, limit, bits, mask=None):
    k, c = ix.search_bin_asym(dev(Q), limit, bits, mask=mask)
    return k.cpu().numpy(), c.cpu().numpy()


def key_ids(keys):
    return 0xFFFFFFFF - (keys.view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)


# ---- the query kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [32, 100, 768])
def test_the_query_planes_and_totals_are_the_models(eng, dim):
    """dim 32: inside one padded 64; dim 100: padded to 128, columns 100..127 zero in every plane; dim 768: twelve ballots.
    Queries: random ones; the two rounding-half vectors; all zero; all negative (every code's sign plane set: its weight
    is -2^(P-1)); one dominant element, every other code 0 or +-1; magnitudes of 1e-30 and 1e30 in one batch."""
    rng = np.random.default_rng(100 + dim)
    R = rows_of(3, dim, 101 + dim)
    half8, half4, zero = (np.zeros(dim, np.float32) for _ in range(3))
    half8[:8], half4[:8] = HALF8, HALF4
    dominant = rng.standard_normal(dim).astype(np.float32)
    dominant[dim // 2] = -1000.0
    negative = -(0.5 + 0.5 * rng.random(dim)).astype(np.float32)             # codes -4 .. -7 and -64 .. -127
    Q = np.stack([R[0], R[1], R[2], half8, half4, zero, negative, dominant,
                  R[1] * np.float32(1e-30), R[2] * np.float32(1e30)]).astype(np.float32)
    ix = make_index(eng, rows_of(1, dim, 5), enable=False)   # the hook needs no binary copy
    try:
        for bits in BITS:
            c = AH.codes(Q, AH.QMAX[bits])
            planes, totals = ix.binary_query_planes(dev(Q), bits)
            assert planes.shape == (len(Q), bits, (dim + 63) // 64 * 2) and planes.dtype == np.uint32
            assert np.array_equal(AH.unplanes(planes, dim), c), bits
            assert np.array_equal(planes, AH.planes(c, bits)), bits          # the padding columns too
            assert totals.tolist() == c.sum(axis=1).tolist(), bits
            assert not planes[5].any() and totals[5] == 0
            assert (c[6] < 0).all() and np.array_equal(planes[6, bits - 1], BH.words(np.ones((1, dim), bool))[0])
            assert np.abs(c[7]).max() == AH.QMAX[bits] and (np.abs(np.delete(c[7], dim // 2)) <= 1).all()
        assert AH.codes(Q[3:4], 127)[0, :8].tolist() == [127, 0, 2, 2, 0, -2, -127, 64]
        assert AH.codes(Q[4:5], 7)[0, :8].tolist() == [7, 0, 2, 2, -4, -7, 3, 0]
        for bad in (np.nan, np.inf):
            Qb = Q.copy()
            Qb[2, dim - 1] = bad
            with pytest.raises(eng.HxError, match="finite"):
                ix.binary_query_planes(dev(Qb), 8)
    finally:
        ix.close()


# ---- the stage ----------------------------------------------------------------------------------------------------------------
_BASE = {}                       # the model's lists of a corpus, computed once and shared by the cases that need them


def stage_cases(ix, X, Q, limits, what, Bs=BS):
    n = len(X)
    for bits in BITS:
        if (what, bits) not in _BASE:
            _BASE[what, bits] = AH.search(BH.row_bits(X), Q, min(n, 2048), bits)
        base = _BASE[what, bits]
        for B in Bs:
            for limit in limits:
                BH.assert_same_lists(run(ix, Q[:B], limit, bits), BH.cut(base, B, limit),
                                     f"{what}: bits {bits} B {B} limit {limit}")


@pytest.mark.parametrize("knobs", [None, KNOBS], ids=["default", "small-chunks"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_the_stage_at_the_row_boundaries(eng, n, knobs):
    X, Q = rows_of(n, 768, 120 + n), rows_of(max(BS), 768, 121)
    ix = make_index(eng, X, env=knobs)
    try:
        # a limit above n where the stage takes one (at most 2048)
        stage_cases(ix, X, Q, (1, 10, 2048) + ((n + 5,) if n + 5 <= 2048 else ()), f"n {n}")
    finally:
        ix.close()


@pytest.mark.parametrize("knobs", [None, KNOBS], ids=["default", "small-chunks"])
def test_the_stage_over_20000_rows_of_100_columns(eng, knobs):
    """padding inside a word (columns 100..127 of the last) and 79 tiles"""
    X, Q = rows_of(20000, 100, 130), rows_of(max(BS), 100, 131)
    ix = make_index(eng, X, env=knobs)
    try:
        stage_cases(ix, X, Q, (1, 10, 2048), "20000 x 100", Bs=(1, 9, 33))
    finally:
        ix.close()


def test_a_row_wider_than_one_staging_pass(eng):
    """dim 2048 = 16 slots of 16 bytes: two column passes (13 + 3); 9 queries are several groups, the tile staged again for
    each"""
    X, Q = rows_of(700, 2048, 140), rows_of(9, 2048, 141)
    ix = make_index(eng, X)
    try:
        for bits in BITS:
            want = AH.search(BH.row_bits(X), Q, 30, bits)
            BH.assert_same_lists(run(ix, Q, 30, bits), want, f"bits {bits} B 9")
            BH.assert_same_lists(run(ix, Q[:1], 30, bits), BH.cut(want, 1, 30), f"bits {bits} B 1")
    finally:
        ix.close()


@pytest.mark.parametrize("knobs", [None, KNOBS], ids=["default", "small-chunks"])
def test_a_workgroup_walks_several_tiles(eng, knobs):
    """HX_DEBUG_BIN_GRID=3 over 2561 rows = 11 tiles, the last of one row: the grid-stride loop.  The mask keeps rows of
    tiles 3, 5 and 9: workgroups 0 and 2 skip their first tile and take later ones behind it."""
    n, dim = 2561, 768
    X, Q = rows_of(n, dim, 150), rows_of(9, dim, 151)
    xb = BH.row_bits(X)
    tile = np.arange(n) // 256
    masks = {"unmasked": None, "tiles 3, 5, 9": np.isin(tile, (3, 5, 9)) & (np.random.default_rng(152).random(n) < 0.5)}
    ix = make_index(eng, X, env=dict(knobs or {}, HX_DEBUG_BIN_GRID="3"))
    try:
        for what, mask in masks.items():
            for bits in BITS:
                want = AH.search(xb, Q, 2048, bits, mask)
                for B in (1, 9):
                    for limit in (10, 300, 2048):
                        BH.assert_same_lists(run(ix, Q[:B], limit, bits, mask), BH.cut(want, B, limit),
                                             f"{what}: bits {bits} B {B} limit {limit}")
    finally:
        ix.close()


def test_a_corpus_ordered_worst_first_goes_through_the_redo(eng):
    """Row i agrees with the all-ones query in i * 65 // n columns, so its score QMAX * (2 agree - dim) grows with i: every
    chunk beats the threshold of the rows before it, the small buffer overflows, and the query is scanned again in fixed
    chunks -- the same list.  The second query sees the corpus best first, the third is random."""
    n, dim = 4000, 64
    q = np.ones((1, dim), np.float32)
    X = -np.ones((n, dim), np.float32)
    for i in range(n):
        X[i, :i * 65 // n] = 1.0
    Q = np.concatenate([q, -q, rows_of(1, dim, 160)])
    ix = make_index(eng, X, env=KNOBS)
    try:
        for bits in BITS:
            for limit in (10, 100):
                BH.assert_same_lists(run(ix, Q, limit, bits), AH.search(BH.row_bits(X), Q, limit, bits),
                                     f"bits {bits} limit {limit}")
    finally:
        ix.close()


# ---- ties, zero, +-v ----------------------------------------------------------------------------------------------------------
def test_identical_rows_come_back_in_id_order_and_a_zero_query_returns_the_first_ids(eng):
    X = np.tile(rows_of(1, 64, 170), (5000, 1))
    Q = np.concatenate([rows_of(2, 64, 171), np.zeros((1, 64), np.float32)])
    Y = rows_of(5000, 64, 172)                               # distinct rows: the zero query still ties them all at 0
    for rows in (X, Y):
        ix = make_index(eng, rows, env=KNOBS)
        try:
            for bits in BITS:
                keys, cnt = run(ix, Q, 100, bits)
                assert cnt.tolist() == [100, 100, 100]
                ids = key_ids(keys)
                assert ids[2].tolist() == list(range(100))
                assert (keys[2].view(np.uint64) >> np.uint64(32) == np.uint64(0x80000000)).all()     # score +0.0
                if rows is X:
                    assert ids[0].tolist() == list(range(100)) and ids[1].tolist() == list(range(100))
                BH.assert_same_lists((keys, cnt), AH.search(BH.row_bits(rows), Q, 100, bits), f"bits {bits}")
        finally:
            ix.close()


def test_queries_of_one_magnitude_score_qmax_times_the_symmetric_stage(eng):
    rng = np.random.default_rng(180)
    X = rows_of(3000, 100, 181)
    Q = (np.where(rng.random((5, 100)) < 0.5, -1, 1) * np.array([[0.3], [1.0], [7.5], [1e-20], [1e20]])).astype(np.float32)
    ix = make_index(eng, X)
    try:
        sk, sc = (a.cpu().numpy() for a in ix.search_bin(dev(Q), 200))
        sym_scores = BH.scores(BH.row_bits(X), BH.query_bits(Q))
        for bits in BITS:
            keys, cnt = run(ix, Q, 200, bits)
            assert cnt.tolist() == sc.tolist() == [200] * 5
            assert np.array_equal(key_ids(keys), key_ids(sk))
            for b in range(5):
                want = AH.QMAX[bits] * sym_scores[b, key_ids(sk)[b]]
                assert np.array_equal((keys[b].view(np.uint64) >> np.uint64(32)).astype(np.uint32),
                                      (O.order_key(want, key_ids(sk)[b]) >> np.uint64(32)).astype(np.uint32))
    finally:
        ix.close()


# ---- masks, refusals, ids -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(eng):
    X, Q = rows_of(3001, 100, 190), rows_of(9, 100, 191)
    ix = make_index(eng, X)
    yield ix, X, Q
    ix.close()


def test_masks(eng, small):
    ix, X, Q = small
    n, xb = len(X), BH.row_bits(X)
    none = np.zeros(n, bool)
    other = np.arange(n) % 2 == 0
    last = np.zeros(n, bool)
    last[n - 1] = True
    no_tile = np.ones(n, bool)
    no_tile[256:512] = False                                 # the second tile is never read
    for bits in BITS:
        BH.assert_same_lists(run(ix, Q, 10, bits, none), (np.zeros((9, 10), np.uint64), np.zeros(9, np.int32)), "no row kept")
        for limit in (10, 2048):
            BH.assert_same_lists(run(ix, Q, limit, bits, other), AH.search(xb, Q, limit, bits, other),
                                 f"every other row, bits {bits} limit {limit}")
        got = run(ix, Q, 4, bits, last)
        BH.assert_same_lists(got, AH.search(xb, Q, 4, bits, last), "one kept row")
        assert got[1].tolist() == [1] * 9
        got = run(ix, Q, 2048, bits, no_tile)
        BH.assert_same_lists(got, AH.search(xb, Q, 2048, bits, no_tile), "a whole tile masked out")
        assert not np.isin(key_ids(got[0]), np.arange(256, 512)).any()
    with pytest.raises(eng.HxError, match="mask_rows"):
        ix.search_bin_asym(dev(Q), 10, 8, mask=np.ones(n - 1, bool))


def test_refusals(eng, small):
    ix, X, Q = small
    plain = make_index(eng, X[:10], enable=False)
    try:
        with pytest.raises(eng.HxError, match="binary"):
            plain.search_bin_asym(dev(Q), 10, 8)
    finally:
        plain.close()
    for bits in (0, 1, 16):
        with pytest.raises(eng.HxError, match="query_bits"):
            ix.search_bin_asym(dev(Q), 10, bits)
        with pytest.raises(eng.HxError, match="query_bits"):
            ix.binary_query_planes(dev(Q), bits)
    with pytest.raises(eng.HxError, match="B must be positive"):
        ix.search_bin_asym(dev(Q[:0]), 10, 8)
    for limit in (0, 2049):
        with pytest.raises(eng.HxError, match="limit"):
            ix.search_bin_asym(dev(Q), limit, 4)
    for bad in (np.nan, np.inf, -np.inf):
        Qb = Q.copy()
        Qb[4, 99] = bad
        for bits in BITS:
            with pytest.raises(eng.HxError, match="query values must be finite"):
                ix.search_bin_asym(dev(Qb), 10, bits)
    tiny = Q * np.float32(1e-44)                             # subnormal magnitudes: outside the bit-exact contract, no error
    keys, cnt = run(ix, tiny, 10, 8)
    assert cnt.tolist() == [10] * 9
    BH.assert_same_lists(run(ix, Q, 10, 8), AH.search(BH.row_bits(X), Q, 10, 8), "the index still answers")


def test_an_id_base_gives_global_ids(eng):
    X, Q = rows_of(500, 64, 200), rows_of(4, 64, 201)
    ix = make_index(eng, X, id_base=1_000_000)
    try:
        for bits in BITS:
            got = run(ix, Q, 25, bits)
            BH.assert_same_lists(got, AH.search(BH.row_bits(X), Q, 25, bits, id_base=1_000_000), "id_base")
            assert key_ids(got[0]).min() >= 1_000_000
    finally:
        ix.close()
