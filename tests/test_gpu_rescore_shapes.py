"""GPU: hx_rescore as an entry of its own, at the shapes a caller-defined query tree can give it:
every stride boundary of k_rescore_list + k_compact<256> / k_compact<1024> with dedupe up to 8192, limits up to 2048 and
above the stride, every prefix, counts 0 / 1 / stride - 1 / stride / above the stride / NULL, candidate lists with
repeated ids, zero keys anywhere, ids outside the collection and arbitrary incoming score bits -- against
OracleIndex.rescore over the valid ids of the counted slots, keys, zero tail and counts bit for bit.  Then an index whose
ids come in two blocks, hx_merge's dedupe path above limit 513, and the refusals.  The small index is 3000 rows of dim 192
with matryoshka sizes (64, 128) -- the engine takes multiples of 64 only, so this is its smallest index with two
prefixes shorter than the row -- the wide one 300 rows of dim 768."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import query_tree_helpers as T

pytestmark = pytest.mark.gpu

STRIDES = (1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8191, 8192)
B = 6
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from rag_application_amd import engine
    return engine


def build(eng, n, dim, ms, tables, **kw):
    rows = T.synth_rows(n, dim, tables)
    ix = eng.HxIndex(dim, ms, **kw)
    return ix, rows


@pytest.fixture(scope="module")
def small(eng, synth_tables):
    ix, rows = build(eng, 3000, 192, (64, 128), synth_tables)
    ix.add(*rows)
    ix.finalize()
    yield ix, T.oracle_index(rows, 192, (64, 128)), O.synth_dense(O.SEED_QUERY, 40, B, 192)
    ix.close()


@pytest.fixture(scope="module")
def wide(eng, synth_tables):
    ix, rows = build(eng, 300, 768, (64, 128, 256), synth_tables)
    ix.add(*rows)
    ix.finalize()
    yield ix, T.oracle_index(rows, 768, (64, 128, 256)), O.synth_dense(O.SEED_QUERY, 40, B, 768)
    ix.close()


def limits_of(stride):
    return sorted({1, 10, 257, 513, min(stride, 2048), 2048})


def counts_of(stride):
    """0, 1, stride - 1, stride, stride + 7 (read as the stride) and half the stride for the list of zeros"""
    return np.array([0, 1, stride - 1, stride, stride + 7, (stride + 1) // 2], dtype=np.int32)


def candidate_lists(rng, stride, id_range, beyond):
    """[B, stride] uint64 keys and the ids in them (-1 = a zero key).  Rows 0, 1, 3, 4: ids drawn with replacement from
    [0, id_range) (many repeats), 15 % zero keys anywhere, some ids from `beyond` (outside the collection); row 1 starts
    with a zero key; row 2 is one id repeated; row 5 is all zeros.  The score word of every key is an arbitrary bit
    pattern -- NaN, +Inf and 0 among them -- which hx_rescore must ignore."""
    ids = rng.integers(0, id_range, size=(B, stride)).astype(np.int64)
    out = rng.random((B, stride)) < 0.08
    ids[out] = rng.choice(beyond, size=int(out.sum()))
    ids[rng.random((B, stride)) < 0.15] = -1
    ids[1, 0] = -1
    ids[2, :] = int(rng.integers(0, id_range))
    ids[5, :] = -1
    hi = rng.integers(0, 1 << 32, size=(B, stride), dtype=np.uint64)
    # the key words of the scores NaN, +Inf, -NaN and -Inf (order_key's transform of their bits), all ones and 0
    special = np.array([0xFFC00000, 0xFF800000, 0x003FFFFF, 0x007FFFFF, 0xFFFFFFFF, 0], dtype=np.uint64)
    pick = rng.random((B, stride)) < 0.2
    hi[pick] = rng.choice(special, size=int(pick.sum()))
    keys = (hi << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.where(ids < 0, 0, ids).astype(np.uint64))
    keys[ids < 0] = 0
    assert (keys[ids >= 0] != 0).all()
    return keys, ids


def expected(ora, q, ids, prefix, to_local=None, to_global=None):
    """the oracle's full ranked list (as keys) of the valid ids among `ids` (-1 = empty slot)"""
    ids = ids[ids >= 0]
    ids = ids[ids < ora.n] if to_local is None else to_local(ids)
    if not len(ids):
        return np.zeros(0, dtype=np.uint64)
    sc, rows = ora.rescore(q, ids, 2048, prefix)
    return O.order_key(sc, rows if to_global is None else to_global(rows))


def sweep(eng, ix, ora, Q, stride, id_range, beyond, limits, prefixes, seed, to_local=None, to_global=None):
    import torch
    rng = np.random.default_rng(seed)
    keys, ids = candidate_lists(rng, stride, id_range, beyond)
    cnt = counts_of(stride)
    d_q = torch.from_numpy(Q).cuda()
    d_keys = torch.from_numpy(keys.view(np.int64)).cuda()
    d_cnt = torch.from_numpy(cnt).cuda()
    for prefix in prefixes:
        for counts in (cnt, None):
            # the oracle once per (list, prefix) at the largest limit: a shorter limit keeps a prefix of that list
            want = [expected(ora, Q[b], ids[b, :stride if counts is None else min(int(counts[b]), stride)], prefix,
                             to_local, to_global) for b in range(B)]
            for L in limits:
                gk, gc = ix.rescore(d_q, d_keys, None if counts is None else d_cnt, L, prefix)
                gk, gc = gk.cpu().numpy().view(np.uint64), gc.cpu().numpy()
                assert gk.shape == (B, L)
                for b in range(B):
                    w = want[b][:min(L, stride)]
                    what = f"stride {stride} limit {L} prefix {prefix} counts {'NULL' if counts is None else int(counts[b])} b {b}"
                    assert int(gc[b]) == len(w), f"{what}: count {int(gc[b])}, want {len(w)}"
                    assert np.array_equal(gk[b, :len(w)], w), what
                    assert not gk[b, len(w):].any(), f"{what}: slots behind the count are not 0"
    return ids


@pytest.mark.parametrize("stride", STRIDES)
def test_rescore_at_every_stride_limit_prefix_and_count(eng, small, stride):
    ix, ora, Q = small
    beyond = np.array([ora.n, ora.n + 1, ora.n + 977, 1 << 20, (1 << 31) + 5, (1 << 32) - 2], dtype=np.int64)
    ids = sweep(eng, ix, ora, Q, stride, min(ora.n, max(2, stride // 3 + 1)), beyond, limits_of(stride), (0, 64, 128),
                7000 + stride)
    if stride == 8192:                                       # the sweep reaches past 2048 distinct valid ids
        assert len(np.unique(ids[3][(ids[3] >= 0) & (ids[3] < ora.n)])) > 2048


@pytest.mark.parametrize("stride", STRIDES)
def test_rescore_on_rows_of_768_where_every_limit_exceeds_the_collection(eng, wide, stride):
    ix, ora, Q = wide
    beyond = np.array([ora.n, ora.n + 3, 1 << 24], dtype=np.int64)
    sweep(eng, ix, ora, Q, stride, ora.n, beyond, limits_of(stride), (0, 64, 128, 256), 9000 + stride)


def to_local(g):
    first, second = (g >= 1000) & (g < 2500), (g >= 4000) & (g < 5500)
    return np.concatenate([g[first] - 1000, g[second] - 4000 + 1500])


def to_global(r):
    return np.where(r < 1500, r + 1000, r - 1500 + 4000)


@pytest.fixture(scope="module")
def blocks(eng, synth_tables):
    """id_base 1000, 1500 rows, then set_next_id(4000) and 1500 more: ids 1000..2499 and 4000..5499"""
    ix, rows = build(eng, 3000, 192, (64, 128), synth_tables, id_base=1000)
    X, ip, si, sv = rows
    cut = int(ip[1500])
    ix.add(X[:1500], ip[:1501], si[:cut], sv[:cut])
    ix.set_next_id(4000)
    ix.add(X[1500:], ip[1500:] - cut, si[cut:], sv[cut:])
    ix.finalize()
    yield ix, T.oracle_index(rows, 192, (64, 128)), O.synth_dense(O.SEED_QUERY, 80, B, 192)
    ix.close()


def test_the_two_id_blocks_are_where_the_tests_believe_them(blocks):
    import torch
    ix, ora, Q = blocks
    k, c = ix.search_dense(torch.from_numpy(Q).cuda(), 2048, 0)
    got = T.key_ids(k.cpu().numpy().view(np.uint64))
    want = np.stack([to_global(ora.search_dense(q, 2048, 0)[1]) for q in Q])
    assert np.array_equal(got, want) and (want < 2500).any() and (want >= 4000).any()


@pytest.mark.parametrize("stride", [1, 257, 2049, 8192])
def test_rescore_over_two_id_blocks_skips_the_gap_and_answers_in_global_ids(eng, blocks, stride):
    """Candidates below the first id (1000), in the gap (2500..3999) and at or above 5500 are skipped; the kept keys
    carry global ids."""
    ix, ora, Q = blocks
    beyond = np.array([5500, 5501, 7000, 1 << 31], dtype=np.int64)
    ids = sweep(eng, ix, ora, Q, stride, 6000, beyond, sorted({1, 10, min(stride, 2048), 2048}), (0, 64), 11000 + stride,
                to_local, to_global)
    if stride > 256:
        flat = ids[ids >= 0]
        assert (flat < 1000).any() and ((flat >= 2500) & (flat < 4000)).any() and (flat >= 5500).any()


@pytest.mark.parametrize("stride", [2048, 4096, 5000, 8192])
def test_merge_with_dedupe_above_limit_513(eng, stride):
    """the part of k_compact's dedupe path tests/test_gpu_parity.py::test_compaction_all_sizes leaves out: limits 514,
    1024, 2047 and 2048.  Rows 0-2 hold every key twice, row 3 few distinct keys many times (fewer than the limit), the
    others keys drawn with replacement; zeros anywhere."""
    import torch
    rng = np.random.default_rng(13000 + stride)
    Bm = 9
    pool = rng.integers(1, 2 ** 63 - 1, size=(Bm, stride), dtype=np.int64)
    pool[:3, stride // 2:] = pool[:3, :stride - stride // 2]
    few = rng.integers(1, 2 ** 63 - 1, size=600, dtype=np.int64)
    pool[3] = rng.choice(few, size=stride)
    for b in range(4, Bm):
        pool[b] = rng.choice(pool[b, :stride // 3], size=stride)
    pool[rng.random((Bm, stride)) < 0.15] = 0
    pool[4, 0] = 0
    cnt = rng.integers(0, stride + 1, size=Bm).astype(np.int32)
    cnt[0], cnt[1], cnt[2], cnt[3], cnt[4] = 0, stride, 1, stride - 1, stride + 7
    d_pool = torch.from_numpy(pool).cuda()
    for limit in (514, 1024, 2047, 2048):
        for counts in (None, cnt):
            keys, kc = eng.merge(d_pool, None if counts is None else torch.from_numpy(counts).cuda(), limit, dedupe=True)
            keys, kc = keys.cpu().numpy().view(np.uint64), kc.cpu().numpy()
            for b in range(Bm):
                n = stride if counts is None else min(int(counts[b]), stride)
                u = pool[b, :n].view(np.uint64)
                u = np.unique(u[u != 0])[::-1][:limit]
                assert kc[b] == len(u), (stride, limit, b)
                assert np.array_equal(keys[b, :len(u)], u), (stride, limit, b)
                assert not keys[b, len(u):].any()
    assert len(np.unique(pool[3])) < 514 + 100                # row 3 really holds fewer distinct keys than the limits


def test_what_rescore_refuses_touches_no_output(eng, small):
    import torch
    from rag_application_amd import _lib
    ix, _, Q = small
    d_q = torch.from_numpy(Q).cuda()
    cand = torch.from_numpy(O.order_key(np.zeros((B, 8200), np.float32), np.arange(B * 8200).reshape(B, 8200) % 3000)
                            .view(np.int64)).cuda()
    keys = torch.full((B, 2100), SENTINEL, dtype=torch.int64, device="cuda")
    cnt = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(nq, stride, limit):
        return _lib.lib().hx_rescore(ix._h, d_q.data_ptr(), nq, 0, cand.data_ptr(), stride, None, limit, keys.data_ptr(),
                                     cnt.data_ptr(), stream)

    for nq, stride, limit in ((B, 0, 10), (B, 8193, 10), (B, 64, 0), (B, 64, 2049), (0, 64, 10)):
        with pytest.raises(eng.HxError):
            _lib.check(call(nq, stride, limit))
        torch.cuda.synchronize()
        assert (keys == SENTINEL).all() and (cnt == -7).all(), (nq, stride, limit)
        with pytest.raises(eng.HxError):                     # the same through the Python face
            if nq:
                ix.rescore(d_q, cand[:, :stride] if stride else cand[:, :0], None, limit, 0)
            else:
                ix.rescore(d_q[:0], cand[:0, :64], None, limit, 0)
    _lib.check(call(B, 8192, 2048))                          # the largest shape is served
    torch.cuda.synchronize()
    assert (cnt.cpu().numpy() == 2048).all()
