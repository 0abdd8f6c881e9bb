"""GPU: the candidates-first row-sharded H1 exchange (hx_h1_plan / hx_h1_nominate_async / hx_h1_rescore_async /
hx_h1_finish, driven by distributed.H1Pipeline) over world sizes 1, 2, 3, 5 and 8 and the limit cells where the plan
used to go wrong, against ONE index over the same rows and, on a sample, against the oracle: ids and fp32 score bits.

Every shard lives in this process on one GPU, built side by side.  The collectives of rank 0 are emulated from the
other shards' real calls: the all-gather is the concatenation of every shard's nominations, the integer-sum all-reduce
is the sum of every shard's exact keys (as scripts/shard_cf.py does)."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

N, DIM, LIMIT = 24000, 256, 10
QN = 1024
# (dense_limit, sparse_limit): the issue's table and the boundaries of the plan's two bad ranges
CELLS = [(1, 1), (10, 10), (100, 100), (288, 64), (289, 64), (500, 100), (1000, 300), (100, 256), (100, 257),
         (100, 330), (100, 400), (100, 300), (2048, 10), (2048, 2048)]
# shard sizes per world: 3 and 5 unequal, 5 with an empty shard and (index 3) a shard without sparse vectors
LAYOUTS = {1: [N], 2: [N // 2] * 2, 3: [8400, 8000, 7600], 5: [7000, 6000, 0, 5500, 5500], 8: [N // 8] * 8}
NO_SPARSE = {5: 3}
NEAR_EQUAL = (1, 2, 3, 8)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def eng():
    from rag_application_amd import engine
    return engine


def unpack_np(eng, keys, cnt):
    s, i = eng.unpack(keys)
    return s.cpu().numpy(), i.cpu().numpy(), cnt.cpu().numpy()


def assert_list_equal(got_s, got_i, got_c, exp_s, exp_i, what=""):
    n = len(exp_i)
    assert got_c == n, f"{what}: count {got_c} != {n}"
    np.testing.assert_array_equal(got_i[:n], exp_i, err_msg=f"{what}: ids")
    np.testing.assert_array_equal(got_s[:n].view(np.uint32), np.asarray(exp_s, np.float32).view(np.uint32),
                                  err_msg=f"{what}: score bits")
    assert (got_i[n:] == -1).all(), f"{what}: tail ids"


def _cf_exchange(eng, torch_mod, shards, Qd, tq, dl, sl, limit, k1, k2, lp, k3, lout, flags=False):
    """The candidates-first H1 exchange by hand on one GPU: nominate on every shard, the all-gather = cat of the public
    parts, rescore on every shard, the integer-sum all-reduce = sum, finish.  Returns (keys, counts, failed queries),
    and with `flags` the per-query flag words of the rescore step as well (shardx.hip k_h1x_cuts: 1 dense overflow /
    int8 pass off, 2 dense cut, 4 sparse flag, 8 sparse cut, 16 sparse list, 32 scale)."""
    W, B = len(shards), Qd.shape[0]
    noms = [s.h1_nominate_async(Qd, *tq, dl, sl, k1, k2, lout) for s in shards]
    pub = B * (k1 + k2 + 2)
    g = torch_mod.cat([x[:pub] for x in noms])
    res = [s.h1_rescore_async(Qd, *tq, noms[r], g, W, r, dl, sl, k1, k2, lp, k3) for r, s in enumerate(shards)]
    red = torch_mod.stack(res).sum(dim=0)
    k, c, nf = eng.h1_finish(red, W, B, lp, k3, dl, sl, limit)
    if not flags:
        return k, c, int(nf.item())
    meta = red[B * (lp + W * k3 + W):].view(B, 4)
    return k, c, int(nf.item()), (meta[:, 2] // W).cpu().numpy()


def plan_or_none(eng, dl, sl, world):
    try:
        return tuple(eng.h1_plan(dl, sl, world))
    except eng.HxError:
        return None


# ---- the collection ------------------------------------------------------------------------------------------------------
def make_world(tables, sizes, no_sparse=None, n_total=None):
    """Rows, sparse vectors and queries for one shard layout: a near neighbour of queries 0-5 copied into every shard
    (dense ties across shards, ordered by id), document 7 repeated in every other shard with sparse vectors (equal
    sparse scores), query 0 asking for one of its terms; the rows of shard `no_sparse` carry no sparse vector."""
    n = sum(sizes) if n_total is None else n_total
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = O.synth_dense(O.SEED_CORPUS, 0, n, DIM)
    ip, si, sv = O.synth_sparse_docs(O.SEED_SPDOC, 0, n, tables)
    Q = O.synth_dense(O.SEED_QUERY, 0, QN, DIM)
    for r, sz in enumerate(sizes):
        for b in range(min(6, max(sz - 100, 0))):
            X[starts[r] + 100 + b] = Q[b] + 0.01 * X[b]
    for r in range(1, len(sizes)):
        if sizes[r] < 8 or r == no_sparse:
            continue
        a0, a1 = ip[7], ip[8]
        d = starts[r] + 7
        m = min(a1 - a0, ip[d + 1] - ip[d])
        si[ip[d]:ip[d] + m] = si[a0:a0 + m]
        sv[ip[d]:ip[d] + m] = sv[a0:a0 + m]
        if ip[d + 1] - ip[d] > m:             # (keep the row's ids unique: push the rest out of the vocabulary's way)
            si[ip[d] + m:ip[d + 1]] = 2 ** 30 + np.arange(ip[d + 1] - ip[d] - m)
    if no_sparse is not None:                 # that shard's rows: empty sparse vectors
        r0, r1 = starts[no_sparse], starts[no_sparse + 1]
        lens = np.diff(ip)
        lens[r0:r1] = 0
        keep = np.ones(len(si), bool)
        keep[ip[r0]:ip[r1]] = False
        si, sv = si[keep], sv[keep]
        ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    qip, qsi, qsv = O.synth_sparse_queries(O.SEED_SPQUERY, 0, QN, tables)
    qsi[qip[0]:qip[0] + 1] = si[ip[7]]        # query 0 asks for a term of the repeated document
    o = np.argsort(qsi[qip[0]:qip[1]], kind="stable")
    qsi[qip[0]:qip[1]] = qsi[qip[0]:qip[1]][o]
    qsv[qip[0]:qip[1]] = qsv[qip[0]:qip[1]][o]
    keep = np.ones(len(qsi), bool)            # (strictly ascending ids within query 0)
    keep[qip[0] + 1:qip[1]] = np.diff(qsi[qip[0]:qip[1]]) > 0
    cnt = np.add.reduceat(keep.astype(np.int64), qip[:-1])
    qsi, qsv = qsi[keep], qsv[keep]
    qip = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return dict(X=X, ip=ip, si=si, sv=sv, Q=Q, qip=qip, qsi=qsi, qsv=qsv, starts=starts, n=n)


class World:
    """The shards of one layout, ONE index over the same rows, and the oracle (built when first asked)."""

    def __init__(self, eng, torch_mod, data, sizes, no_sparse=None):
        self.eng, self.t, self.d = eng, torch_mod, data
        X, ip, si, sv, st = data["X"], data["ip"], data["si"], data["sv"], data["starts"]
        self.shards = []
        for r, sz in enumerate(sizes):
            r0, r1 = int(st[r]), int(st[r + 1])
            ix = eng.HxIndex(DIM, (), id_base=r0)
            if sz > 0 and r == no_sparse:
                ix.add(X[r0:r1])
            elif sz > 0:
                ix.add(X[r0:r1], ip[r0:r1 + 1] - ip[r0], si[ip[r0]:ip[r1]].astype(np.int32), sv[ip[r0]:ip[r1]])
            self.shards.append(ix)
        wmax = max(s.sparse_wmax()[0] for s in self.shards)
        for s in self.shards:
            s.set_sparse_wmax(wmax)
        self.one = eng.HxIndex(DIM, ())
        self.one.add(X, ip, si.astype(np.int32), sv)
        self._ora = None
        self._want = {}

    def batch(self, b0, b1):
        """(Qd, q_indptr, q_idx, q_val) of queries [b0, b1) on the device"""
        t, d = self.t, self.d
        qip = d["qip"]
        lo, hi = int(qip[b0]), int(qip[b1])
        return (t.from_numpy(np.ascontiguousarray(d["Q"][b0:b1])).cuda(), t.from_numpy(qip[b0:b1 + 1] - lo).cuda(),
                t.from_numpy(d["qsi"][lo:hi].astype(np.int32)).cuda(), t.from_numpy(d["qsv"][lo:hi]).cuda())

    def one_index(self, q, dl, sl):
        hp = self.eng.make_params(dict(matryoshka_64_limit=1, matryoshka_128_limit=1, matryoshka_256_limit=1,
                                       dense_limit=dl, quantized_limit=1, sparse_limit=sl, final_limit=LIMIT, hnsw_ef=1),
                                  mode=self.eng.HX_MODE_H1)
        return self.one.hybrid_query(*q, hp)

    def expected(self, b0, b1, dl, sl):
        """(keys, counts) the pipeline must return for queries [b0, b1): the one index's"""
        return self.one_index(self.batch(b0, b1), dl, sl)

    def oracle(self, b, dl, sl):
        if self._ora is None:
            d = self.d
            self._ora = O.OracleIndex(DIM, ())
            self._ora.add(d["X"], d["ip"], d["si"], d["sv"])
            self._ora.finalize()
        key = (b, dl, sl)
        if key not in self._want:
            d = self.d
            qip = d["qip"]
            self._want[key] = O.hybrid_h1(self._ora, d["Q"][b], d["qsi"][qip[b]:qip[b + 1]], d["qsv"][qip[b]:qip[b + 1]],
                                          dl, sl, LIMIT)
        return self._want[key]

    def close(self):
        for s in self.shards:
            s.close()
        self.one.close()


class _Rank0Local:
    """Shard 0 as rank 0 sees it; remembers its last call so that the emulated collectives can make the other
    shards' part of the same step."""

    def __init__(self, ix):
        self.ix = ix
        self.last = None
        self.last_rescore = None

    def __getattr__(self, name):
        return getattr(self.ix, name)

    def h1_nominate_async(self, *a):
        self.last = ("h1_nominate_async", a)
        return self.ix.h1_nominate_async(*a)

    def h1_local_async(self, *a):
        self.last = ("h1_local_async", a)
        return self.ix.h1_local_async(*a)

    def h1_local(self, *a):
        self.last = ("h1_local", a)
        return self.ix.h1_local(*a)

    def h1_rescore_async(self, *a):
        self.last_rescore = a
        return self.ix.h1_rescore_async(*a)


def rank0(shards):
    """A distributed.ShardedIndex of len(shards) ranks seen from rank 0, every collective filled from the other shards'
    real calls on this GPU."""
    import torch
    from rag_application_amd.distributed import ShardedIndex

    class Rank0(ShardedIndex):
        def __init__(self):
            super().__init__(_Rank0Local(shards[0]))
            self.world = len(shards)
            self.others_nom = []

        def gather_raw(self, keys):
            name, a = self.local.last
            others = [getattr(s, name)(*a) for s in shards[1:]]
            if name == "h1_nominate_async":      # [1, public words] per rank
                self.others_nom = others
                pub = keys.numel()
                return torch.cat([keys.reshape(1, -1)] + [o[:pub].view(1, -1) for o in others])
            return torch.cat([keys] + others, dim=0)

        def reduce_sum(self, t):
            a = self.local.last_rescore
            q, nom, g, world, _rank, rest = a[:4], a[4], a[5], a[6], a[7], a[8:]
            for r, s in enumerate(shards[1:], start=1):
                t.add_(s.h1_rescore_async(*q, self.others_nom[r - 1], g, world, r, *rest))
            return t

        def all_min(self, v):
            return min([int(v)] + [1 if s.dense_candidates() == "i8" else 0 for s in shards[1:]])

        def sync_sparse_scale(self):
            w = max(s.sparse_wmax()[0] for s in shards)
            for s in shards:
                s.set_sparse_wmax(w)

    return Rank0()


def run_pipeline(eng, torch_mod, w, dl, sl, batches, force=False, before_submit=None):
    """H1Pipeline over rank 0 of `w`'s shards: every batch's lists must equal `w.expected` (the one index's).  Returns
    the pipeline."""
    from rag_application_amd.distributed import H1Pipeline
    pipe = H1Pipeline(rank0(w.shards), dl, sl, LIMIT, force_side_stream=force)
    outs = []
    for i, (b0, b1) in enumerate(batches):
        if before_submit:
            before_submit(i, pipe)
        outs.append(pipe.submit(*w.batch(b0, b1)))
    pipe.wait()
    torch_mod.cuda.synchronize()
    for (b0, b1), (k, c) in zip(batches, outs):
        k1, c1 = w.expected(b0, b1, dl, sl)
        assert torch_mod.equal(c, c1) and torch_mod.equal(k, k1), f"pipeline ({dl}, {sl}) batch {b0}:{b1}"
    return pipe


SINGLE = (0, 1, 3, 5, 9, 17, 26, 40, 51, 64, 77, 88, 99, 110, 121, 129)   # the queries run one at a time (B = 1)


def check_cell(eng, torch_mod, w, world, dl, sl, must_serve, batch_sizes):
    plan = plan_or_none(eng, dl, sl, world)
    if plan is None:
        return None
    k1, k2, lp, k3, lout = plan
    for B in batch_sizes:
        q = w.batch(0, B)
        k, c, nf, fl = _cf_exchange(eng, torch_mod, w.shards, q[0], q[1:], dl, sl, LIMIT, k1, k2, lp, k3, lout, flags=True)
        k1_, c1_ = w.one_index(q, dl, sl)
        differ = int(((k != k1_).any(dim=1) | (c != c1_)).sum())
        assert differ <= nf, f"world {world} ({dl}, {sl}) B={B}: {differ} lists differ, {nf} flagged"
        if must_serve:
            assert nf == 0, (f"world {world} ({dl}, {sl}) B={B}: {nf} queries flagged, flag words "
                             f"{sorted(set(int(x) for x in fl if x))}")
    # one query at a time: no list reported final may be wrong
    for j, b in enumerate(SINGLE):
        q = w.batch(b, b + 1)
        k, c, nf = _cf_exchange(eng, torch_mod, w.shards, q[0], q[1:], dl, sl, LIMIT, k1, k2, lp, k3, lout)
        if must_serve:
            assert nf == 0, f"world {world} ({dl}, {sl}) query {b} flagged"
        if nf:
            continue
        s_, i_, c_ = unpack_np(eng, k, c)
        s1, i1, c1 = unpack_np(eng, *w.one_index(q, dl, sl))
        assert_list_equal(s_[0], i_[0], c_[0], s1[0, :c1[0]], i1[0, :c1[0]], f"world {world} ({dl}, {sl}) b={b} vs one")
        if j % 2 == 0:
            es, ei = w.oracle(b, dl, sl)
            assert_list_equal(s_[0], i_[0], c_[0], es, ei, f"world {world} ({dl}, {sl}) b={b} vs oracle")
    return plan


@pytest.mark.timeout(900)
@pytest.mark.parametrize("world", sorted(LAYOUTS))
def test_exchange_over_limits(eng, torch_mod, synth_tables, world):
    """Every limit cell at this world: the plan's shares go through nominate / rescore / finish, no list reported
    final differs from ONE index (nor, on a sample, from the oracle), and H1Pipeline serves every batch -- candidates
    first where the plan takes the limits, per shard where it does not, and it refuses at construction only limits
    neither exchange serves."""
    from rag_application_amd.distributed import H1Pipeline
    sizes = LAYOUTS[world]
    w = World(eng, torch_mod, make_world(synth_tables, sizes, NO_SPARSE.get(world)), sizes, NO_SPARSE.get(world))
    try:
        for dl, sl in CELLS:
            must = world in NEAR_EQUAL and dl <= 500
            if world * max(dl, sl) > 8192:
                with pytest.raises(ValueError, match="dense_limit"):
                    H1Pipeline(rank0(w.shards), dl, sl, LIMIT, force_side_stream=(world == 1))
                continue
            bs = (1, 33, 130) + ((1024,) if (world, dl, sl) == (8, 100, 100) else ())
            plan = check_cell(eng, torch_mod, w, world, dl, sl, must, bs)
            pipe = run_pipeline(eng, torch_mod, w, dl, sl, [(130, 163), (163, 196), (196, 229), (229, 262)],
                                force=(world == 1))
            assert pipe.cf == (plan is not None) or pipe.redone > 0, (world, dl, sl, plan)
            if plan is not None and must:
                assert pipe.cf and pipe.redone == 0, f"world {world} ({dl}, {sl}): redone {pipe.redone}"
        if world == 2:                        # where the nomination's select pass runs does not change a bit
            q = w.batch(0, 130)
            plan = eng.h1_plan(100, 100, 2)
            ref = _cf_exchange(eng, torch_mod, w.shards, q[0], q[1:], 100, 100, LIMIT, *plan)
            for fork in ("0", "1"):
                import os
                old = os.environ.get("HX_DEBUG_NOM_FORK")
                os.environ["HX_DEBUG_NOM_FORK"] = fork
                try:
                    got = _cf_exchange(eng, torch_mod, w.shards, q[0], q[1:], 100, 100, LIMIT, *plan)
                finally:
                    if old is None:
                        del os.environ["HX_DEBUG_NOM_FORK"]
                    else:
                        os.environ["HX_DEBUG_NOM_FORK"] = old
                assert got[2] == ref[2] == 0 and torch_mod.equal(got[0], ref[0]) and torch_mod.equal(got[1], ref[1]), fork
    finally:
        w.close()


def test_fewer_rows_than_dense_limit(eng, torch_mod, synth_tables):
    """300 rows over two shards, dense_limit 500: every shard's list holds all its rows."""
    sizes = [150, 150]
    w = World(eng, torch_mod, make_world(synth_tables, sizes), sizes)
    try:
        for dl, sl in ((500, 100), (100, 100)):
            plan = check_cell(eng, torch_mod, w, 2, dl, sl, False, (1, 33, 130))
            assert plan is not None
            run_pipeline(eng, torch_mod, w, dl, sl, [(130, 163), (163, 196), (196, 229)])
    finally:
        w.close()


def test_skewed_shards_are_flagged_and_widened(eng, torch_mod, synth_tables):
    """80 / 20 rows at world 2, dense_limit 500: the big shard holds ~1640 of the global L' = 2048 candidates, more than
    its share k1 = 1280, so its list is cut above the global cut on every query -- every query is flagged.  The pipeline
    redoes those batches per shard and widens k1 to L', after which the exchange serves the batches itself."""
    sizes = [N * 4 // 5, N // 5]
    w = World(eng, torch_mod, make_world(synth_tables, sizes), sizes)
    try:
        dl, sl = 500, 100
        k1, k2, lp, k3, lout = eng.h1_plan(dl, sl, 2)
        assert k1 < lp
        q = w.batch(0, 130)
        _, _, nf, fl = _cf_exchange(eng, torch_mod, w.shards, q[0], q[1:], dl, sl, LIMIT, k1, k2, lp, k3, lout, flags=True)
        assert nf == 130 and all(int(x) & 2 for x in fl), sorted(set(int(x) for x in fl))
        wide = (lp + 31) // 32 * 32
        _, _, nf_wide = _cf_exchange(eng, torch_mod, w.shards, q[0], q[1:], dl, sl, LIMIT, wide, k2, lp, k3, lout)
        assert nf_wide == 0
        ks = []
        batches = [(130 + 33 * i, 163 + 33 * i) for i in range(7)]
        pipe = run_pipeline(eng, torch_mod, w, dl, sl, batches, before_submit=lambda i, p: ks.append(p.k1))
        assert pipe.cf and pipe.k1 == wide and ks[0] == k1
        # the batches that went out with the plan's k1 were redone (depth + 1 of them), those with the widened k1 were not
        n_narrow = sum(1 for k in ks if k == k1)
        assert pipe.redone == n_narrow, (pipe.redone, ks)
        assert n_narrow < len(batches)
    finally:
        w.close()


@pytest.mark.parametrize("when", ["before the pipeline", "after the pipeline"])
def test_shard_without_int8_candidates(eng, torch_mod, synth_tables, when):
    """One shard switched to the fp16 candidate copy: submit() never raises, every batch equals the one index, and
    the pipeline ends up on the per-shard exchange within a bounded number of batches."""
    sizes = [N // 2] * 2
    w = World(eng, torch_mod, make_world(synth_tables, sizes), sizes)
    try:
        dl, sl = 100, 100
        batches = [(130 + 33 * i, 163 + 33 * i) for i in range(14)]
        if when == "before the pipeline":
            w.shards[1].set_dense_candidates("f16")
            pipe = run_pipeline(eng, torch_mod, w, dl, sl, batches[:4])
            assert not pipe.cf and pipe.redone == 0
        else:
            cf_at = []

            def switch(i, p):
                if i == 0:
                    assert p.cf
                    w.shards[0].set_dense_candidates("f16")     # rank 0 itself: its nominate must not raise
                cf_at.append(p.cf)

            pipe = run_pipeline(eng, torch_mod, w, dl, sl, batches, before_submit=switch)
            assert not pipe.cf, cf_at
            assert pipe.redone >= 1 and cf_at.index(False) <= 12, cf_at
            # the nomination of a shard without the int8 pass is flagged, never final
            plan = eng.h1_plan(dl, sl, 2)
            q = w.batch(0, 33)
            _, _, nf, fl = _cf_exchange(eng, torch_mod, w.shards, q[0], q[1:], dl, sl, LIMIT, *plan, flags=True)
            assert nf == 33 and all(int(x) & 1 for x in fl)
    finally:
        w.close()
