"""GPU: the headline corpus -- 10M x 768 rows + 1.0e9 postings, matryoshka 64 / 128 / 256 -- on every batch route and
stage, against the chunked host reference over ALL rows (oracle/full_size.py, itself checked against the numpy oracle by
tests/test_full_size_reference.py): ids, fp32 score bits, counts and trailing -1 ids.

The selection machinery (the scan's chunk plan, the threshold geometry, the staggered kernel's append logs, the int8
candidate margin) is tuned at this size and only takes its full-size shape here.  For queries [0, B) and every sampled
query id below B (SAMPLE):

    B = 1, 8, 32          k_scan with its query tile resident in LDS, the few-queries geometry
    B = 33, 100, 128      scan8, the 256 x 128 "HQ" form
    B = 129, 256          scan8, the 256 x 256 tile
    B = 1024              the bench's batch
    B = 4100              hybrid calls in two slices of 2050 (SAMPLE holds both sides of the cut)

  every B: dense L=100 (int8 candidates), dense prefix 64 L=100, int8 L=40, sparse L=100, tree P_MCP, tree
           p_fallback(10M), H1 (100 (+) 100 -> 10)
  B = 8 and 1024 also: dense and sparse L in (1, 10, 257, 1000, 2048), dense L=100 with fp16 candidates, prefix 128
           and 256 L=100

Calls with every limit <= 100 must have been served by the fast paths (no dense or sparse exact fallback); the rest
print their retry / uncertified / fallback counts (FULL-SIZE lines, pytest -s).  The later prefixes have no fp16
copy (the tree only re-scores them), so the exact path serves their stand-alone searches.

Then the candidates-first sharded H1 (distributed.H1Pipeline with rank 0's collectives emulated on this GPU) at the
shard sizes of the 8-GPU (8 x 1.25M rows) and 2-GPU (2 x 5M) layouts: all 1024 lists of a B = 1024 batch equal the
single index's, key for key.  At 5M rows per shard the nomination's select pass runs on the second stream.

Never two full corpora at once: the single index is closed before the first shard layout is built."""
import time

import numpy as np
import pytest

from rag_application_amd import synth
from tests.test_gpu_parity import P_MCP, assert_list_equal, p_fallback, unpack_np
from tests.test_gpu_shard_exchange import _cf_exchange, run_pipeline

pytestmark = pytest.mark.gpu

ROWS, DIM, MSIZES = 10_000_000, 768, (64, 128, 256)
# route and tile edges, and the slice edges of B = 4100 (slices [0, 2050), [2050, 4100))
SAMPLE = (0, 1, 7, 31, 32, 33, 63, 64, 99, 127, 128, 129, 255, 256, 511, 1023, 2049, 2050, 4095, 4099)
BATCHES = (1, 8, 32, 33, 100, 128, 129, 256, 1024, 4100)
WIDE_B, WIDE_L = (8, 1024), (1, 10, 257, 1000, 2048)
# the host pass's list lengths: the longest limit any cell asks of each stage (p_fallback(10M): 500 / 400 / 300 / 200 /
# 300 / 100; the 128 and 256 prefixes of the tree are re-scores, their stage lists are checked at L = 100)
LIMITS = dict(dense=2048, m64=500, m128=100, m256=100, i8=300, sparse=2048)
H1 = dict(P_MCP, dense_limit=100, sparse_limit=100, final_limit=10)
FAST = ("dense_fallback_queries", "sparse_fallback_queries")
SLOW = ("retry_queries", "cand8_uncertified_queries", "i8_fallback_queries", "cand8_switched_off", "tree_batches_redone")


def report(line):
    print(f"FULL-SIZE {line}", flush=True)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def eng():
    from rag_application_amd import engine
    return engine


@pytest.fixture(scope="module")
def tabs():
    return synth.tables()


def sparse_batch(tabs, b0, b1):
    return synth.sparse_queries(synth.SEED_SPQUERY, b0, b1 - b0, tabs)


@pytest.fixture(scope="module")
def full(eng, torch_mod, tabs):
    """The single 10M-row index (closed early by `single_h1`)."""
    ix = eng.HxIndex(DIM, MSIZES)
    t0 = time.perf_counter()
    try:
        ix.reserve(ROWS)
        ix.synth_fill(ROWS, synth.SEED_CORPUS, synth.SEED_SPDOC, tabs)
        ix.finalize()
        torch_mod.cuda.synchronize()
    except BaseException:
        ix.close()
        raise
    st = ix.stats()
    report(f"index: {st['n_rows']} rows, {st['nnz']} postings, {st['n_segments']} segments, "
           f"built in {time.perf_counter() - t0:.1f} s")
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def ref(tabs):
    """One host pass over all 10M rows for the sampled queries."""
    from oracle import c_oracle as CO
    from oracle import full_size as FS
    n = max(SAMPLE) + 1
    Q = CO.synth_dense(synth.SEED_QUERY, 0, n, DIM)[list(SAMPLE)]
    qip, qix, qv = sparse_batch(tabs, 0, n)
    lens = np.array([qip[b + 1] - qip[b] for b in SAMPLE])
    sp = (np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
          np.concatenate([qix[qip[b]:qip[b + 1]] for b in SAMPLE]), np.concatenate([qv[qip[b]:qip[b + 1]] for b in SAMPLE]))
    r = FS.FullSizeReference(FS.SynthSource(ROWS, DIM, tabs), Q, sp, LIMITS)
    report(f"host pass: {len(SAMPLE)} queries x {ROWS} rows in {r.chunks} chunks, {r.seconds:.1f} s "
           f"({CO.num_threads()} threads)")
    return r


@pytest.mark.timeout(900)
@pytest.mark.parametrize("B", BATCHES)
def test_every_stage_and_route_at_full_size(full, ref, eng, torch_mod, tabs, B):
    ix = full
    assert ix.dense_candidates() == "i8", "the int8 candidate pass is off: its route would go unchecked"
    Q = eng.synth_queries_dense(DIM, 0, B, synth.SEED_QUERY)
    sp = [torch_mod.from_numpy(a).cuda() for a in sparse_batch(tabs, 0, B)]
    rows = [(k, b) for k, b in enumerate(SAMPLE) if b < B]

    def cell(what, call, want, fast):
        """One call over the whole batch, its sampled lists against the reference; the fast paths must have served a
        `fast` cell (no query left them), the others report how many queries needed a retry or more."""
        before = ix.stats()
        keys, cnt = call()
        torch_mod.cuda.synchronize()
        after = ix.stats()
        d = {k: after[k] - before[k] for k in FAST + SLOW}
        s, i, c = unpack_np(eng, keys, cnt)
        for k, b in rows:
            es, ei = want(k)
            assert_list_equal(s[b], i[b], c[b], es, ei, f"B={B} {what} query {b} (stats {d})")
        if fast:
            assert all(d[k] == 0 for k in FAST), f"B={B} {what}: queries left the fast paths: {d}"
        else:
            report(f"B={B} {what}: {d}")

    c8 = ix.stats()["cand8_queries"]
    cell("dense L=100", lambda: ix.search_dense(Q, 100), lambda k: ref.dense(k, 100), True)
    assert ix.stats()["cand8_queries"] - c8 == B, "the int8 candidate pass did not nominate every query"
    cell("dense prefix 64 L=100", lambda: ix.search_dense(Q, 100, 64), lambda k: ref.dense(k, 100, 64), True)
    cell("int8 L=40", lambda: ix.search_i8(Q, 40), lambda k: ref.i8(k, 40), True)
    cell("sparse L=100", lambda: ix.search_sparse(*sp, 100), lambda k: ref.sparse(k, 100), True)
    cell("tree P_MCP", lambda: ix.hybrid_query(Q, *sp, eng.make_params(P_MCP)), lambda k: ref.tree(k, P_MCP), True)
    pf = p_fallback(ROWS)
    cell("tree p_fallback", lambda: ix.hybrid_query(Q, *sp, eng.make_params(pf)), lambda k: ref.tree(k, pf), False)
    cell("H1", lambda: ix.hybrid_query(Q, *sp, eng.make_params(H1, mode=eng.HX_MODE_H1)),
         lambda k: ref.h1(k, 100, 100, 10), True)
    if B not in WIDE_B:
        return
    for L in WIDE_L:
        cell(f"dense L={L}", lambda: ix.search_dense(Q, L), lambda k: ref.dense(k, L), L <= 100)
        cell(f"sparse L={L}", lambda: ix.search_sparse(*sp, L), lambda k: ref.sparse(k, L), L <= 100)
    for d in (128, 256):   # (no fp16 copy of the later prefixes -- the tree only re-scores them: the exact path serves)
        cell(f"dense prefix {d} L=100", lambda: ix.search_dense(Q, 100, d), lambda k: ref.dense(k, 100, d), False)
    # (at B = 1024 the L >= 1000 cells leave every query uncertified, enough for the index's guard to switch the int8
    # pass off: set back to "i8" below, the state the next batch's cells assert)
    ix.set_dense_candidates("f16")
    try:
        cell("dense L=100 fp16 candidates", lambda: ix.search_dense(Q, 100), lambda k: ref.dense(k, 100), True)
    finally:
        ix.set_dense_candidates("i8")
    assert ix.dense_candidates() == "i8"


# ---- candidates-first sharded H1 at the shard sizes of the 8- and 2-GPU layouts ------------------------------------------
SHARD_B = 1024
SHARD_BATCHES = [(0, 256), (256, 512), (512, 768), (768, 1024)]


@pytest.fixture(scope="module")
def single_h1(full, eng, torch_mod, tabs):
    """The single index's B = 1024 H1 lists (100 (+) 100 -> 10) of all 1024 queries, kept on the host; then the single
    index is closed, so that no shard layout is ever resident beside it."""
    Q = eng.synth_queries_dense(DIM, 0, SHARD_B, synth.SEED_QUERY)
    sp = [torch_mod.from_numpy(a).cuda() for a in sparse_batch(tabs, 0, SHARD_B)]
    k, c = full.hybrid_query(Q, *sp, eng.make_params(H1, mode=eng.HX_MODE_H1))
    out = (k.cpu(), c.cpu())
    full.close()
    return out


class ShardLayout:
    """What run_pipeline asks of a layout: the shards, a batch of queries on the device, the lists it must return."""

    def __init__(self, torch_mod, shards, Q, sp, want):
        self.t, self.shards, self.Q, self.sp, self.want = torch_mod, shards, Q, sp, want

    def batch(self, b0, b1):
        qip, qix, qv = self.sp
        lo, hi = int(qip[b0]), int(qip[b1])
        t = self.t
        return (self.Q[b0:b1].contiguous(), t.from_numpy(qip[b0:b1 + 1] - lo).cuda(), t.from_numpy(qix[lo:hi]).cuda(),
                t.from_numpy(qv[lo:hi]).cuda())

    def expected(self, b0, b1, dl, sl):
        assert (dl, sl) == (H1["dense_limit"], H1["sparse_limit"])
        return self.want[0][b0:b1].cuda(), self.want[1][b0:b1].cuda()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("world", [8, 2])
def test_candidates_first_shards_at_full_size(single_h1, eng, torch_mod, tabs, world):
    per = ROWS // world
    dl, sl, limit = H1["dense_limit"], H1["sparse_limit"], H1["final_limit"]
    shards = []
    try:
        t0 = time.perf_counter()
        for r in range(world):
            s = eng.HxIndex(DIM, (), id_base=r * per)     # global ids: the same corpus, row for row
            shards.append(s)
            s.reserve(per)
            s.synth_fill(per, synth.SEED_CORPUS, synth.SEED_SPDOC, tabs)
            s.finalize()
        wmax = max(s.sparse_wmax()[0] for s in shards)
        for s in shards:
            s.set_sparse_wmax(wmax)
        torch_mod.cuda.synchronize()
        t_build = time.perf_counter() - t0
        w = ShardLayout(torch_mod, shards, eng.synth_queries_dense(DIM, 0, SHARD_B, synth.SEED_QUERY),
                        sparse_batch(tabs, 0, SHARD_B), single_h1)
        # the exchange by hand, one batch of 1024: no list it reports final differs from the single index
        plan = eng.h1_plan(dl, sl, world)
        q = w.batch(0, SHARD_B)
        k, c, nf, fl = _cf_exchange(eng, torch_mod, shards, q[0], q[1:], dl, sl, limit, *plan, flags=True)
        wk, wc = w.expected(0, SHARD_B, dl, sl)
        differ = int(((k != wk).any(dim=1) | (c != wc)).sum())
        words = sorted(set(int(x) for x in fl if x))
        msg = f"world {world} ({per} rows per shard), plan {plan}: {nf} of {SHARD_B} queries flagged (flag words {words})"
        assert differ <= nf, f"{msg}, {differ} lists differ"
        # H1Pipeline over rank 0, flagged batches redone per shard: every list equals the single index's, key for key
        pipe = run_pipeline(eng, torch_mod, w, dl, sl, SHARD_BATCHES)
        assert pipe.cf, msg
        report(f"{msg}; {differ} lists differ before the redo; H1Pipeline redid {pipe.redone} of "
               f"{len(SHARD_BATCHES)} batches; shards built in {t_build:.1f} s")
    finally:
        for s in shards:
            s.close()
