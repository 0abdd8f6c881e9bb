"""CPU: hx_dense_route (which kernels serve the tail of the dense stage: the fused k_dense_finish with 2 / 4 / 8 keys per
lane or the three launches, and the k_compact_top form behind every scan launch) against a restatement of the host
arithmetic, over every limit the ABI takes, the batch sizes on both sides of the fusing threshold, both candidate kinds
and both levels.

Restated here from rag_application_amd/csrc/engine.hip (geometry(), cand8_lprime()) and select.hip (dense_finish_e(),
compact_form()); search_dense, launch_dense_finish and launch_compact decide by the very functions hx_dense_route
calls, so a GPU test that asks engine.dense_route for a cell's route (tests/test_gpu_dense_limits.py) knows what ran."""
import pytest

CAND_CAP, MAX_LIMIT = 8192, 2048
BATCHES = (1, 32, 33, 64, 65, 1024)
KINDS = ("f16", "i8")


@pytest.fixture(scope="module")
def eng():
    from rag_application_amd import build
    build.build()
    from rag_application_amd import engine
    return engine


# ---- restatements of the host arithmetic ---------------------------------------------------------------------------------
def next_pow2(v):
    return 1 << max(0, (int(v) - 1).bit_length())


def cand8_lprime(L):                  # engine.hip cand8_lprime (defaults: mul2 = 9, add = 288)
    return min(max(9 * L // 2, L + 288), max(L, CAND_CAP // 4))


def geometry(L, cand, level):
    """engine.hip geometry(L, approx, safe = level > 0, cand8 = int8 candidates at level 0): (L', C)"""
    cand8 = cand == "i8" and level == 0                 # the retry level scans the fp16 copy whatever the first pass did
    lp = cand8_lprime(L) if cand8 else L + max(32, L // 2)
    if level > 0:
        lp = min(max(2 * lp, lp + 256), CAND_CAP // 4)
    c = next_pow2(max(8 * lp, 1024))
    if cand8:
        c = max(c, 4096)
    return lp, (CAND_CAP if level > 0 else min(c, CAND_CAP))


def finish_e(B, lp, L):               # select.hip dense_finish_e
    if B > 64 or lp > 512:
        return 0
    return 2 if L <= 128 else (4 if L <= 256 else 8)


def compact_form(C, keep):            # select.hip compact_form(list_len = C, keep, no dedupe)
    P = next_pow2(max(C, 256))
    if keep <= 256 and P <= 2048:
        return P // 256, 4
    if 256 < keep <= 512 and P <= 8192:
        return max(1, P // 512), 8
    return 0, 0


@pytest.fixture(scope="module")
def table(eng):
    return {(B, L, cand, level): eng.dense_route(B, L, cand, level)
            for B in BATCHES for L in range(1, MAX_LIMIT + 1) for cand in KINDS for level in (0, 1)}


# ---- the sweep -----------------------------------------------------------------------------------------------------------
def test_sizes_are_the_restated_geometry(table):
    bad = []
    for (B, L, cand, level), (lp, C, *_rest) in table.items():
        if (lp, C) != geometry(L, cand, level) or not (L <= lp and 2 * lp <= C):
            bad.append(((B, L, cand, level), (lp, C), geometry(L, cand, level)))
    assert not bad, f"{len(bad)} cells, e.g. {bad[:5]}"


def test_fused_exactly_for_small_batches_and_short_lists(table):
    bad = []
    for (B, L, cand, level), (lp, C, fe, _nw, _e) in table.items():
        fused = B <= 64 and lp <= 512
        ok = (fe != 0) == fused and fe == finish_e(B, lp, L)
        if fused:      # the top L end in one wave's registers, and no wider instantiation than that needs
            ok = ok and fe in (2, 4, 8) and L <= 64 * fe and fe == min(e for e in (2, 4, 8) if L <= 64 * e)
        if not ok:
            bad.append(((B, L, cand, level), (lp, fe)))
    assert not bad, f"{len(bad)} cells, e.g. {bad[:5]}"


def test_compaction_form_holds_the_list_and_what_it_keeps(table):
    bad, seen = [], set()
    for (B, L, cand, level), (lp, C, _fe, nw, e) in table.items():
        P = min(C, next_pow2(C))
        ok = (nw, e) == compact_form(C, lp)
        if (nw, e) != (0, 0):
            ok = ok and e in (4, 8) and nw in (1, 2, 4, 8, 16) and 64 * e >= lp and 64 * e * nw >= P
        else:          # no register form fits: none of those launch_compact has holds keep = L' of C keys
            ok = ok and not any(64 * e_ >= lp and 64 * e_ * nw_ >= P
                                for e_, nws in ((4, (1, 2, 4, 8)), (8, (1, 2, 4, 8, 16))) for nw_ in nws)
        seen.add((nw, e))
        if not ok:
            bad.append(((B, L, cand, level), (lp, C, nw, e)))
    assert not bad, f"{len(bad)} cells, e.g. {bad[:5]}"
    # the forms a scan's compaction takes (derived from the geometry: C >= 8 L' or 4096 / 8192): fp16 buffers of 1024 and
    # 2048 keys with 4 per lane, 4096 keys (fp16 L' > 256, int8 candidates) and the retry level's 8192 with 8 per lane,
    # the LDS sort from L' = 513
    assert seen == {(4, 4), (8, 4), (8, 8), (16, 8), (0, 0)}, seen


# (candidates, level) -> last fused limit, first unfused limit
BOUNDARIES = {("f16", 0): (341, 342), ("i8", 0): (113, 114), ("f16", 1): (171, 172), ("i8", 1): (171, 172)}


@pytest.mark.parametrize("cand,level", sorted(BOUNDARIES))
def test_boundaries_are_where_the_table_says(table, cand, level):
    last, first = BOUNDARIES[(cand, level)]
    assert first == last + 1
    for B in (1, 32, 33, 64):
        fused = [L for L in range(1, MAX_LIMIT + 1) if table[(B, L, cand, level)][2] != 0]
        assert fused == list(range(1, last + 1)), (B, cand, level, fused[-1])
        assert table[(B, last, cand, level)][0] <= 512 < table[(B, first, cand, level)][0]
    for B in (65, 1024):
        assert not any(table[(B, L, cand, level)][2] for L in range(1, MAX_LIMIT + 1)), (B, cand, level)


def test_every_instantiation_is_reached_on_every_route(table):
    """E = 2 up to L = 128, E = 4 up to 256, E = 8 above -- where the route fuses that far: the int8 route ends at 113
    (E = 2 only), the retry level at 171 (E = 2 and 4)."""
    want = {("f16", 0): {2: (1, 128), 4: (129, 256), 8: (257, 341)}, ("i8", 0): {2: (1, 113)},
            ("f16", 1): {2: (1, 128), 4: (129, 171)}, ("i8", 1): {2: (1, 128), 4: (129, 171)}}
    for (cand, level), spans in want.items():
        got = {}
        for L in range(1, MAX_LIMIT + 1):
            fe = table[(64, L, cand, level)][2]
            if fe:
                lo, hi = got.get(fe, (L, L))
                got[fe] = (min(lo, L), max(hi, L))
        assert got == spans, (cand, level, got)


def test_the_retry_level_ignores_the_candidate_kind(table):
    for B in BATCHES:
        for L in range(1, MAX_LIMIT + 1):
            assert table[(B, L, "i8", 1)] == table[(B, L, "f16", 1)], (B, L)


def test_route_rejects_its_own_bad_arguments(eng):
    import ctypes as C
    from rag_application_amd import _lib
    for B, L, level in ((0, 10, 0), (-1, 10, 0), (1, 0, 0), (1, MAX_LIMIT + 1, 0), (1, -5, 0), (1, 10, 2), (1, 10, -1)):
        with pytest.raises(eng.HxError):
            eng.dense_route(B, L, "i8", level)
    with pytest.raises(ValueError):
        eng.dense_route(1, 10, "f32")
    v = [C.c_int32() for _ in range(5)]
    lib = _lib.lib()
    for kind in (2, -1):                                            # the C entry itself: a candidate kind that is neither
        assert lib.hx_dense_route(1, 10, kind, 0, *[C.byref(x) for x in v]) != 0
        assert lib.hx_last_error()
    for hole in range(5):                                           # a NULL result pointer
        args = [C.byref(x) for x in v]
        args[hole] = None
        assert lib.hx_dense_route(1, 10, 1, 0, *args) != 0
        assert lib.hx_last_error()
