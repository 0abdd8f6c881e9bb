"""GPU: binary quantization -- the 1-bit copy of the rows (hx_binary_enable, k_binarize_rows) through
every entry that moves rows, and the Hamming scan stage (hx_search_bin, k_bin_scan) -- against the numpy model of
tests/binary_helpers.py, key for key: ids, fp32 score bits, counts, zero slots behind the count.  The shapes are the
smallest that reach each path: one row, the wave's and the tile's boundaries, several tiles, rows of one 16-byte slot and
of six, every query-group size and one more; a second index under HX_DEBUG_BIN_CHUNK0 / HX_DEBUG_BIN_CAP takes several
chunks, compacts its buffers more than once and reaches the overflow redo."""
from __future__ import annotations

import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import binary_helpers as BH

pytestmark = pytest.mark.gpu

BS = (1, 8, 9, 33, 130)          # the kernel scores 1, 2, 4 or 8 queries per walk: every form, a partial and a 17th group
KNOBS = {"HX_DEBUG_BIN_CHUNK0": "96", "HX_DEBUG_BIN_CAP": "64"}


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from rag_application_amd import engine
    return engine


def rows_of(n, dim, seed):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


def make_index(eng, X, env=None, id_base=0, enable=True):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        ix = eng.HxIndex(X.shape[1], (), device=0, id_base=id_base)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if enable:
        ix.binary_enable()
    if len(X):
        ix.add(X)
    return ix


def dev(Q):
    import torch
    return torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).cuda()


def run(ix, Q, limit, mask=None):
    k, c = ix.search_bin(dev(Q), limit, mask=mask)
    return k.cpu().numpy(), c.cpu().numpy()


def stored_words(ix, n):
    return np.stack([ix.binary_row(r) for r in range(n)]) if n else np.zeros((0, 0), np.uint32)


# ---- the stored copy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [32, 100, 768])
def test_the_stored_bits_are_the_signs_of_the_stored_normalised_rows(eng, dim):
    """dim 32: the row inside one padded 64; dim 100: padded to 128, bits 100..127 zero; dim 768: six 16-byte slots.  Row 1
    holds planted +0.0 and -0.0, row 2 an element that underflows to exactly 0 in the normalisation, row 3 is all zero
    (ingest accepts it: it stays as it is)."""
    X = rows_of(70, dim, 7 + dim)
    X[1, 0], X[1, 1], X[1, 5] = 0.0, -0.0, 0.0
    X[2, :] = 1.0e10
    X[2, 3] = 2.0e-38
    X[3, :] = 0.0
    stored = O.cosine_preprocess(X)
    assert X[2, 3] > 0 and stored[2, 3] == 0.0 and stored[2, 4] > 0
    assert np.signbit(stored[1, 1]) and stored[1, 1] == 0.0
    ix = make_index(eng, X)
    try:
        assert ix.binary_enabled()
        want = BH.words(BH.row_bits(X))
        got = stored_words(ix, len(X))
        assert got.shape == want.shape == (70, (dim + 63) // 64 * 2)
        assert np.array_equal(got, want)
        assert not (got[1, 0] & 0b100011) and not (got[2, 0] >> 3) & 1 and not got[3].any()
        if dim == 100:
            assert not (got[:, 3] >> 4).any()                # bits 100..127
        if dim == 32:
            assert not got[:, 1].any()
    finally:
        ix.close()


def test_the_copy_follows_every_entry_that_moves_rows(eng, tmp_path, monkeypatch):
    """Enable before or after the adds, hx_retain_rows in several chunks, hx_replace_rows of the first, a middle and the
    last row, hx_truncate, an add past the reserved capacity, save / load / enable: after each the copy, read row by
    row, is the model's bits of the final rows, and the stage over it is the model's."""
    monkeypatch.setenv("HX_DEBUG_COMPACT_CHUNK", "16")
    dim = 100
    rng = np.random.default_rng(11)
    Q = rows_of(3, dim, 12)
    A, B2 = rows_of(150, dim, 13), rows_of(120, dim, 14)

    def check(ix, X, what):
        assert ix.count() == len(X), what
        assert np.array_equal(stored_words(ix, len(X)), BH.words(BH.row_bits(X))), what
        BH.assert_same_lists(run(ix, Q, 20), BH.search(BH.row_bits(X), Q, 20), what)

    first = make_index(eng, np.zeros((0, dim), np.float32))
    later = make_index(eng, np.zeros((0, dim), np.float32), enable=False)
    try:
        BH.assert_same_lists(run(first, Q, 5), (np.zeros((3, 5), np.uint64), np.zeros(3, np.int32)), "an empty index")
        for ix in (first, later):
            ix.add(A)
            ix.add(B2)
        assert not later.binary_enabled()
        later.binary_enable()
        later.binary_enable()                                # idempotent
        X = np.concatenate([A, B2])
        check(first, X, "enable, then two adds")
        check(later, X, "two adds, then enable")
        assert np.array_equal(stored_words(first, len(X)), stored_words(later, len(X)))
        ix = first
        keep = rng.random(len(X)) < 0.6
        keep[[0, 17, len(X) - 1]] = [False, True, False]
        assert ix.retain(keep) == int((~keep).sum())
        X = X[keep]
        check(ix, X, "retain_rows")
        rows = np.array([len(X) - 1, 0, len(X) // 2])
        new = rows_of(3, dim, 15)
        ix.replace(rows, new)
        X[rows] = new
        check(ix, X, "replace_rows")
        ix.truncate(100)
        X = X[:100]
        check(ix, X, "truncate")
        more = rows_of(700, dim, 16)                         # past the capacity the first adds reserved: a grow
        ix.add(more)
        X = np.concatenate([X, more])
        check(ix, X, "an add past the capacity")
        path = str(tmp_path / "b.hx")
        ix.save(path)
        back = eng.HxIndex.load(path, device=0)
        try:
            assert not back.binary_enabled()
            with pytest.raises(eng.HxError, match="binary"):
                back.search_bin(dev(Q), 5)
            back.binary_enable()
            check(back, X, "save, load, enable")
        finally:
            back.close()
    finally:
        first.close()
        later.close()


# ---- the stage ----------------------------------------------------------------------------------------------------------------
_BASE = {}                       # the model's lists of a corpus, computed once and shared by the cases that need them


def stage_cases(ix, X, Q, limits, what):
    n = len(X)
    if what not in _BASE:
        _BASE[what] = BH.search(BH.row_bits(X), Q, min(n, 2048))
    base = _BASE[what]
    for B in BS:
        for limit in limits:
            BH.assert_same_lists(run(ix, Q[:B], limit), BH.cut(base, B, limit), f"{what}: B {B} limit {limit}")


@pytest.mark.parametrize("knobs", [None, KNOBS], ids=["default", "small-chunks"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_the_stage_at_the_row_boundaries(eng, n, knobs):
    X, Q = rows_of(n, 64, 20 + n), rows_of(max(BS), 64, 21)
    ix = make_index(eng, X, env=knobs)
    try:
        # a limit above n where the stage takes one (at most 2048)
        stage_cases(ix, X, Q, (1, 10, 2048) + ((n + 5,) if n + 5 <= 2048 else ()), f"n {n}")
    finally:
        ix.close()


@pytest.mark.parametrize("knobs", [None, KNOBS], ids=["default", "small-chunks"])
@pytest.mark.parametrize("dim", [768, 100])
def test_the_stage_over_20000_rows(eng, dim, knobs):
    n = 20000
    X, Q = rows_of(n, dim, 30 + dim), rows_of(max(BS), dim, 31)
    ix = make_index(eng, X, env=knobs)
    try:
        stage_cases(ix, X, Q, (1, 10, 2048), f"dim {dim}")
    finally:
        ix.close()


def test_a_row_wider_than_one_staging_pass(eng):
    """dim 2048 = 16 slots of 16 bytes: two column passes (13 + 3), and with 9 queries two groups over them"""
    X, Q = rows_of(700, 2048, 40), rows_of(9, 2048, 41)
    ix = make_index(eng, X)
    try:
        want = BH.search(BH.row_bits(X), Q, 30)
        BH.assert_same_lists(run(ix, Q, 30), want, "B 9")
        BH.assert_same_lists(run(ix, Q[:1], 30), BH.cut(want, 1, 30), "B 1")
    finally:
        ix.close()


@pytest.mark.parametrize("knobs", [None, KNOBS], ids=["default", "small-chunks"])
@pytest.mark.parametrize("dim", [64, 768, 2048])
def test_a_workgroup_walks_several_tiles(eng, dim, knobs):
    """HX_DEBUG_BIN_GRID=3 over 2561 rows = 11 tiles, the last of one row: k_bin_scan's grid-stride loop, which the launch's
    own grid (one workgroup per tile up to 256 per CU share) never takes below 65 000 rows.  At limit 2048 the first chunk
    holds every row: workgroup w walks tiles w, w + 3, ...; at the small limits the chunks are shorter launches (8 + 3 tiles
    by default, unaligned ones under the small-chunk knobs).  dim 64: one slot, one pass; 768: six slots; 2048: two passes,
    the tile staged again per group (B 9 = two groups).  The masks keep rows of tiles 1, 4 and 10 (workgroups 0 and 2 skip
    every tile, workgroup 1 skips its third between kept ones), of tiles 3, 5 and 9 (workgroups 0 and 2 skip their FIRST
    tile and take later ones behind it) and one single row: a skipped tile leaves the LDS tile and s_q of the tile before."""
    n = 2561
    X, Q = rows_of(n, dim, 90 + dim), rows_of(9, dim, 91)
    xb = BH.row_bits(X)
    rng = np.random.default_rng(92)
    tile = np.arange(n) // 256
    masks = {"unmasked": None,
             "tiles 1, 4, 10": np.isin(tile, (1, 4, 10)) & ((rng.random(n) < 0.5) | (tile == 10)),
             "tiles 3, 5, 9": np.isin(tile, (3, 5, 9)) & (rng.random(n) < 0.5),
             "one row": np.arange(n) == 1300}
    assert masks["tiles 1, 4, 10"][n - 1] and n - 1 == 10 * 256
    ix = make_index(eng, X, env=dict(knobs or {}, HX_DEBUG_BIN_GRID="3"))
    try:
        for what, mask in masks.items():
            want = BH.search(xb, Q, 2048, mask)
            for B in (1, 9):
                for limit in (10, 300, 2048):
                    BH.assert_same_lists(run(ix, Q[:B], limit, mask), BH.cut(want, B, limit), f"{what}: B {B} limit {limit}")
    finally:
        ix.close()


def test_a_corpus_ordered_worst_first_goes_through_the_redo(eng):
    """Row i agrees with the query in i * 65 // n columns: every chunk beats the threshold of the rows before it, the small
    buffer overflows, and the query is scanned again in fixed chunks -- the same list."""
    n, dim = 4000, 64
    q = np.ones((1, dim), np.float32)
    X = -np.ones((n, dim), np.float32)
    for i in range(n):
        X[i, :i * 65 // n] = 1.0
    Q = np.concatenate([q, -q, rows_of(1, dim, 50)])
    ix = make_index(eng, X, env=KNOBS)
    try:
        for limit in (10, 100):
            BH.assert_same_lists(run(ix, Q, limit), BH.search(BH.row_bits(X), Q, limit), f"limit {limit}")
    finally:
        ix.close()


# ---- ties ---------------------------------------------------------------------------------------------------------------------
def test_identical_rows_come_back_in_id_order(eng):
    X = np.tile(rows_of(1, 64, 60), (5000, 1))
    Q = rows_of(2, 64, 61)
    ix = make_index(eng, X, env=KNOBS)
    try:
        keys, cnt = run(ix, Q, 100)
        assert cnt.tolist() == [100, 100]
        ids = 0xFFFFFFFF - (keys.view(np.uint64) & np.uint64(0xFFFFFFFF))
        assert ids[0].tolist() == list(range(100)) and ids[1].tolist() == list(range(100))
        BH.assert_same_lists((keys, cnt), BH.search(BH.row_bits(X), Q, 100), "5000 identical rows")
    finally:
        ix.close()


@pytest.mark.parametrize("knobs", [None, KNOBS], ids=["default", "small-chunks"])
def test_a_corpus_of_four_sign_patterns(eng, knobs):
    rng = np.random.default_rng(62)
    pats = rows_of(4, 100, 63)
    X = pats[rng.integers(0, 4, size=9000)] * (0.5 + rng.random((9000, 1)).astype(np.float32))
    Q = np.concatenate([pats[:2], rows_of(7, 100, 64)])
    ix = make_index(eng, X, env=knobs)
    try:
        for limit in (7, 300, 2048):
            BH.assert_same_lists(run(ix, Q, limit), BH.search(BH.row_bits(X), Q, limit), f"limit {limit}")
    finally:
        ix.close()


# ---- masks, refusals, ids -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(eng):
    X, Q = rows_of(3001, 100, 70), rows_of(9, 100, 71)
    ix = make_index(eng, X)
    yield ix, X, Q
    ix.close()


def test_masks(eng, small):
    ix, X, Q = small
    n, xb = len(X), BH.row_bits(X)
    none, every = np.zeros(n, bool), np.ones(n, bool)
    third = np.arange(n) % 3 == 0
    last = np.zeros(n, bool)
    last[n - 1] = True
    BH.assert_same_lists(run(ix, Q, 10, none), (np.zeros((9, 10), np.uint64), np.zeros(9, np.int32)), "no row kept")
    plain = run(ix, Q, 50)
    BH.assert_same_lists(run(ix, Q, 50, every), (plain[0].view(np.uint64), plain[1]), "every row kept")
    BH.assert_same_lists(plain, BH.search(xb, Q, 50), "unmasked")
    for limit in (10, 2048):
        BH.assert_same_lists(run(ix, Q, limit, third), BH.search(xb, Q, limit, third), f"every third row, limit {limit}")
    got = run(ix, Q, 4, last)
    BH.assert_same_lists(got, BH.search(xb, Q, 4, last), "one kept row")
    assert got[1].tolist() == [1] * 9
    with pytest.raises(eng.HxError, match="mask_rows"):
        ix.search_bin(dev(Q), 10, mask=np.ones(n - 1, bool))


def test_refusals(eng, small):
    ix, X, Q = small
    plain = make_index(eng, X[:10], enable=False)
    try:
        with pytest.raises(eng.HxError, match="binary"):
            plain.search_bin(dev(Q), 10)
        with pytest.raises(eng.HxError, match="binary"):
            plain.binary_row(0)
    finally:
        plain.close()
    for bad in (np.nan, np.inf, -np.inf):
        Qb = Q.copy()
        Qb[4, 99] = bad
        with pytest.raises(eng.HxError, match="finite"):
            ix.search_bin(dev(Qb), 10)
    for limit in (0, 2049):
        with pytest.raises(eng.HxError, match="limit"):
            ix.search_bin(dev(Q), limit)
    BH.assert_same_lists(run(ix, Q, 10), BH.search(BH.row_bits(X), Q, 10), "the index still answers")


def test_an_id_base_gives_global_ids(eng):
    X, Q = rows_of(500, 64, 80), rows_of(4, 64, 81)
    ix = make_index(eng, X, id_base=1_000_000)
    try:
        got = run(ix, Q, 25)
        BH.assert_same_lists(got, BH.search(BH.row_bits(X), Q, 25, id_base=1_000_000), "id_base")
        ids = 0xFFFFFFFF - (got[0].view(np.uint64) & np.uint64(0xFFFFFFFF))
        assert ids.min() >= 1_000_000
    finally:
        ix.close()
