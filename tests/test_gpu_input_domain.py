"""GPU: inputs the ABI accepts that the rest of the suite does not reach -- the RRF settings of hx_params, dense rows and
queries holding a NaN or an infinity (refused), degenerate and extreme dense values, and sparse weights and term ids at
the ends of their ranges.  Every list is compared with the numpy oracle (ids and fp32 score bits), and every case
asserts through stats() which route served it, so that no case passes through the exact fallback alone."""
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
RRF_KS = (0.25, 1.0, 2.0, 60.0)
RANK_BASES = (0, 1, 7)
P_TREE = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, dense_limit=40,
              quantized_limit=40, sparse_limit=50, final_limit=30, hnsw_ef=128)
ROUTES = ("retry_queries", "dense_fallback_queries", "cand8_uncertified_queries", "cand8_queries",
          "sparse_fallback_queries", "i8_fallback_queries")


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


def routes(ix):
    s = ix.stats()
    return {k: s[k] for k in ROUTES}


def moved(ix, before):
    after = routes(ix)
    return {k: after[k] - before[k] for k in ROUTES}


def fast(d, what):
    """no query of the call was retried or served by an exact fallback"""
    slow = {k: v for k, v in d.items() if k != "cand8_queries" and v}
    assert not slow, f"{what}: left the fast paths {slow}"


class World:
    pass


# ---- 1. RRF settings ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rrf_world(eng, torch_mod, synth_tables):
    w = World()
    w.n, w.dim, w.B = 8000, 256, 16
    w.X = O.synth_dense(O.SEED_CORPUS, 0, w.n, w.dim)
    w.ip, w.si, w.sv = O.synth_sparse_docs(O.SEED_SPDOC, 0, w.n, synth_tables)
    w.ora = O.OracleIndex(w.dim, (64, 128, 256))
    w.ora.add(w.X, w.ip, w.si, w.sv)
    w.ora.finalize()
    w.ix = eng.HxIndex(w.dim, (64, 128, 256))
    w.ix.add(w.X, w.ip, w.si.astype(np.int32), w.sv)
    w.Q = O.synth_dense(O.SEED_QUERY, 0, w.B, w.dim)
    w.qip, w.qsi, w.qsv = O.synth_sparse_queries(O.SEED_SPQUERY, 0, w.B, synth_tables)
    w.qsi = w.qsi.astype(np.int32)
    w.Qd = torch_mod.from_numpy(w.Q).cuda()
    w.tq = (torch_mod.from_numpy(w.qip).cuda(), torch_mod.from_numpy(w.qsi).cuda(), torch_mod.from_numpy(w.qsv).cuda())
    w.qs = [(w.qsi[w.qip[b]:w.qip[b + 1]], w.qsv[w.qip[b]:w.qip[b + 1]]) for b in range(w.B)]
    # a mask keeping half the rows, and the oracle of an index holding only those rows
    w.mask = np.random.default_rng(5).random(w.n) < 0.5
    w.kept = np.nonzero(w.mask)[0]
    sub = [(w.si[w.ip[r]:w.ip[r + 1]], w.sv[w.ip[r]:w.ip[r + 1]]) for r in w.kept]
    mip = np.concatenate([[0], np.cumsum([len(a) for a, _ in sub])]).astype(np.int64)
    w.oram = O.OracleIndex(w.dim, (64, 128, 256))
    w.oram.add(w.X[w.kept], mip, np.concatenate([a for a, _ in sub]), np.concatenate([v for _, v in sub]))
    w.oram.finalize()
    # dense / sparse top-1100 of every query (a shorter limit's list is their prefix: one total order)
    w.dl = [w.ora.search_dense(w.Q[b], 1100)[1] for b in range(w.B)]
    w.sl = [w.ora.search_sparse(*w.qs[b], 1100)[1] for b in range(w.B)]
    w.dlm = [w.kept[w.oram.search_dense(w.Q[b], 1100)[1]] for b in range(w.B)]
    w.slm = [w.kept[w.oram.search_sparse(*w.qs[b], 1100)[1]] for b in range(w.B)]
    yield w
    w.ix.close()


# (dense_limit, sparse_limit, final_limit): k_rrf_top up to 256 keys, k_rrf from 257 (LDS), k_rrf beyond 1024 per list
H1_CELLS = [(100, 100, 1), (100, 100, 10), (100, 100, 256), (128, 128, 10), (128, 129, 10), (1100, 1100, 10)]


@pytest.mark.parametrize("k", RRF_KS)
@pytest.mark.parametrize("base", RANK_BASES)
def test_rrf_settings_h1(rrf_world, eng, torch_mod, k, base):
    """H1 through the host, the device and the 50 % masked entry at every rrf_k x rank base, with final limits 1 / 10 /
    256 and list pairs on each side of the k_rrf_top boundary (256 / 257 keys) and above 1024 keys per list."""
    w = rrf_world
    for dl, sl, fl in H1_CELLS:
        hp = eng.make_params(dict(P_TREE, dense_limit=dl, sparse_limit=sl, final_limit=fl), mode=eng.HX_MODE_H1,
                             rrf_k=k, rrf_rank_base=base)
        exp = [O.rrf([w.dl[b][:dl], w.sl[b][:sl]], limit=fl, k=k, rank_base=base) for b in range(w.B)]
        expm = [O.rrf([w.dlm[b][:dl], w.slm[b][:sl]], limit=fl, k=k, rank_base=base) for b in range(w.B)]
        what = f"h1 k={k} base={base} {dl}/{sl}/{fl}"
        r0 = routes(w.ix)
        s, i, c = w.ix.hybrid_query_host(w.Q, w.qip, w.qsi, w.qsv, hp)
        d = moved(w.ix, r0)
        for b in range(w.B):
            assert_list_equal(s[b], i[b], c[b], *exp[b], f"{what} host b={b}")
        assert d["cand8_queries"] >= w.B, (what, d)           # the int8 pass nominated every query
        if dl <= 128:
            fast(d, what)
        r0 = routes(w.ix)
        s, i, c = unpack_np(eng, *w.ix.hybrid_query(w.Qd, *w.tq, hp))
        assert moved(w.ix, r0) == d, (what, "device entry took another route")
        for b in range(w.B):
            assert_list_equal(s[b], i[b], c[b], *exp[b], f"{what} dev b={b}")
        r0 = routes(w.ix)
        s, i, c = w.ix.hybrid_query_host(w.Q, w.qip, w.qsi, w.qsv, hp, mask=w.mask)
        dm = moved(w.ix, r0)
        for b in range(w.B):
            assert_list_equal(s[b], i[b], c[b], *expm[b], f"{what} masked b={b}")
        if dl <= 128:
            fast(dm, what + " masked")


TREE_CELLS = [(k, b, 10, P_TREE) for k in RRF_KS for b in RANK_BASES] + [
    (60.0, 7, 1, P_TREE), (60.0, 7, 100, P_TREE), (0.25, 1, 100, dict(P_TREE, dense_limit=300, quantized_limit=300,
                                                                        sparse_limit=300)),
    (60.0, 1, 2048, dict(P_TREE, matryoshka_64_limit=2048, matryoshka_128_limit=2048, matryoshka_256_limit=2048,
                          dense_limit=2048, quantized_limit=2048, sparse_limit=2048, final_limit=100))]


@pytest.mark.parametrize("cell", range(len(TREE_CELLS)))
def test_rrf_settings_tree(rrf_world, eng, torch_mod, cell):
    """The reference tree at every rrf_k x rank base, rrf_limit 1 / 10 / 100 and 2048 (root union 4096 keys, the RRF of
    two 2048-key lists on the k_rrf path that reads global memory), through the host and the device entry."""
    w = rrf_world
    k, base, rl, P = TREE_CELLS[cell]
    B = 8
    hp = eng.make_params(P, rrf_k=k, rrf_rank_base=base, rrf_limit=rl)
    what = f"tree k={k} base={base} rrf_limit={rl} dense_limit={P['dense_limit']}"
    r0 = routes(w.ix)
    s, i, c = w.ix.hybrid_query_host(w.Q[:B], w.qip[:B + 1], w.qsi, w.qsv, hp)
    d = moved(w.ix, r0)
    r0 = routes(w.ix)
    sd, id_, cd = unpack_np(eng, *w.ix.hybrid_query(w.Qd[:B], w.tq[0][:B + 1], w.tq[1], w.tq[2], hp))
    assert moved(w.ix, r0) == d, (what, "device entry took another route")
    assert d["cand8_queries"] == 0, what                         # the tree's whole-collection dense scan is the prefix
    if P["dense_limit"] <= 300:
        fast(d, what)
    for b in range(B):
        es, ei = O.hybrid_tree(w.ora, w.Q[b], *w.qs[b], P, rrf_k=k, rank_base=base, rrf_limit=rl)
        assert_list_equal(s[b], i[b], c[b], es, ei, f"{what} host b={b}")
        assert_list_equal(sd[b], id_[b], cd[b], es, ei, f"{what} dev b={b}")


def _cf(eng, torch_mod, shards, Qd, tq, dl, sl, limit, k, base):
    """candidates-first H1 by hand on one GPU (as tests/test_gpu_shard_exchange.py _cf_exchange), with RRF settings"""
    W, B = len(shards), Qd.shape[0]
    k1, k2, lp, k3, lout = eng.h1_plan(dl, sl, W)
    noms = [s.h1_nominate_async(Qd, *tq, dl, sl, k1, k2, lout) for s in shards]
    pub = B * (k1 + k2 + 2)
    g = torch_mod.cat([x[:pub] for x in noms])
    res = [s.h1_rescore_async(Qd, *tq, noms[r], g, W, r, dl, sl, k1, k2, lp, k3) for r, s in enumerate(shards)]
    red = torch_mod.stack(res).sum(dim=0)
    keys, cnt, nf = eng.h1_finish(red, W, B, lp, k3, dl, sl, limit, k=k, rank_base=base)
    return keys, cnt, int(nf.item())


def test_rrf_settings_sharded(rrf_world, eng, torch_mod):
    """hx_h1_fuse at world 2 and the candidates-first hx_h1_finish at worlds 2 and 4 take the RRF settings as the single
    index does: the oracle's lists, and candidates-first serves every query (no batch to redo)."""
    w = rrf_world
    worlds = {}
    for W in (2, 4):
        cut = [w.n * r // W for r in range(W + 1)]
        sh = []
        for r in range(W):
            a, b = cut[r], cut[r + 1]
            ix = eng.HxIndex(w.dim, (64, 128, 256), id_base=a)
            ix.add(w.X[a:b], w.ip[a:b + 1] - w.ip[a], w.si[w.ip[a]:w.ip[b]].astype(np.int32), w.sv[w.ip[a]:w.ip[b]])
            sh.append(ix)
        wmax = max(s.sparse_wmax()[0] for s in sh)
        for s in sh:
            s.set_sparse_wmax(wmax)
        worlds[W] = sh
    try:
        for k, base in ((0.25, 0), (1.0, 1), (2.0, 7), (60.0, 0), (60.0, 7)):
            for dl, sl, fl in ((100, 100, 10), (128, 129, 10), (100, 100, 200)):
                exp = [O.rrf([w.dl[b][:dl], w.sl[b][:sl]], limit=fl, k=k, rank_base=base) for b in range(w.B)]
                what = f"k={k} base={base} {dl}/{sl}/{fl}"
                allk = torch_mod.cat([s.h1_local(w.Qd, *w.tq, dl, sl) for s in worlds[2]], dim=0)
                s_, i_, c_ = unpack_np(eng, *eng.h1_fuse(allk, 2, dl, sl, limit=fl, k=k, rank_base=base))
                for b in range(w.B):
                    assert_list_equal(s_[b], i_[b], c_[b], *exp[b], f"h1_fuse {what} b={b}")
                for W in (2, 4):
                    keys, cnt, nf = _cf(eng, torch_mod, worlds[W], w.Qd, w.tq, dl, sl, fl, k, base)
                    assert nf == 0, f"candidates-first W={W} {what}: {nf} queries to redo"
                    s_, i_, c_ = unpack_np(eng, keys, cnt)
                    for b in range(w.B):
                        assert_list_equal(s_[b], i_[b], c_[b], *exp[b], f"cf W={W} {what} b={b}")
        # a batch holding a NaN query goes out flagged (every query of it is redone, and refused by hx_h1_local)
        Qn = w.Q.copy()
        Qn[5, 100] = np.nan
        for W in (2, 4):
            _, _, nf = _cf(eng, torch_mod, worlds[W], torch_mod.from_numpy(Qn).cuda(), w.tq, 100, 100, 10, 2.0, 0)
            assert nf == w.B, f"candidates-first W={W}: a batch with a NaN query flagged {nf} of {w.B} queries"
    finally:
        for sh in worlds.values():
            for s in sh:
                s.close()


@pytest.mark.parametrize("k,base", [(0.0, 0), (-1.0, 0), (float("nan"), 0), (float("inf"), 0), (-0.0, 0), (1e-39, 0),
                                    (2.0, -1), (2.0, 2 ** 30 + 1)])
def test_bad_rrf_settings_refused(rrf_world, eng, torch_mod, k, base):
    """rrf_k non-finite, <= 0 or so small that 2 / rrf_k overflows, and a rank base outside [0, 2^30] give infinite or
    NaN keys (or an int32 overflow): every entry refuses them."""
    w = rrf_world
    for mode in (eng.HX_MODE_TREE, eng.HX_MODE_H1):
        hp = eng.make_params(P_TREE, mode=mode, rrf_k=k, rrf_rank_base=base)
        with pytest.raises(eng.HxError, match="rrf"):
            w.ix.hybrid_query_host(w.Q, w.qip, w.qsi, w.qsv, hp)
        with pytest.raises(eng.HxError, match="rrf"):
            w.ix.hybrid_query(w.Qd, *w.tq, hp)
        with pytest.raises(eng.HxError, match="rrf"):
            w.ix.hybrid_query_host(w.Q, w.qip, w.qsi, w.qsv, hp, mask=w.mask)
    keys = w.ix.h1_local(w.Qd, *w.tq, 10, 10)
    a, b = keys[:, :10].contiguous(), keys[:, 10:].contiguous()
    cnt = torch_mod.full((w.B,), 10, dtype=torch_mod.int32, device=keys.device)
    with pytest.raises(eng.HxError, match="rrf"):
        eng.rrf(a, cnt, b, cnt, limit=10, k=k, rank_base=base)
    with pytest.raises(eng.HxError, match="rrf"):
        eng.h1_fuse(keys, 1, 10, 10, limit=10, k=k, rank_base=base)
    k1, k2, lp, k3, lout = eng.h1_plan(10, 10, 2)
    red = torch_mod.zeros((w.B * (lp + 2 * k3 + 2 + 4),), dtype=torch_mod.int64, device=keys.device)
    with pytest.raises(eng.HxError, match="rrf"):
        eng.h1_finish(red, 2, w.B, lp, k3, 10, 10, 10, k=k, rank_base=base)
    # nothing was left behind: the default settings give the oracle's lists
    hp = eng.make_params(dict(P_TREE, dense_limit=100, sparse_limit=100, final_limit=10), mode=eng.HX_MODE_H1)
    s, i, c = w.ix.hybrid_query_host(w.Q, w.qip, w.qsi, w.qsv, hp)
    for b in range(w.B):
        assert_list_equal(s[b], i[b], c[b], *O.rrf([w.dl[b][:100], w.sl[b][:100]], limit=10), f"after refusal b={b}")


# ---- 2. non-finite dense input ------------------------------------------------------------------------------------------
BADS = [float("nan"), float("inf"), float("-inf")]


@pytest.mark.parametrize("bad", BADS)
def test_non_finite_rows_refused(eng, torch_mod, synth_tables, bad):
    """A batch holding one row with a NaN / +Inf / -Inf element is refused whole by the host and the device entry:
    count, nnz and the int8 copy's error bound stay as they were, and later queries return the oracle's lists."""
    n, dim = 3000, 256
    X = O.synth_dense(O.SEED_CORPUS, 0, n, dim)
    ip, si, sv = O.synth_sparse_docs(O.SEED_SPDOC, 0, n + 40, synth_tables)
    ora = O.OracleIndex(dim, (64, 128, 256))
    ora.add(X, ip[:n + 1], si[:ip[n]], sv[:ip[n]])
    ora.finalize()
    ix = eng.HxIndex(dim, (64, 128, 256))
    ix.add(X, ip[:n + 1], si[:ip[n]].astype(np.int32), sv[:ip[n]])
    st0 = ix.stats()
    Xb = O.synth_dense(O.SEED_CORPUS, n, 40, dim)
    Xb[17] *= F32(0.02)
    Xb[17, 0] = 1.0                                            # a row the int8 grid resolves badly: it would raise E_X
    Xb[29, 200] = bad
    bip = ip[n:n + 41] - ip[n]
    bsi, bsv = si[ip[n]:ip[n + 40]].astype(np.int32), sv[ip[n]:ip[n + 40]]
    for entry in ("host", "device"):
        with pytest.raises(eng.HxError, match="finite"):
            if entry == "host":
                ix.add(Xb, bip, bsi, bsv)
            else:
                ix.add_device(torch_mod.from_numpy(Xb).cuda(), bip, bsi, bsv)
        st = ix.stats()
        assert st["n_rows"] == n and st["nnz"] == st0["nnz"], entry
        assert st["cand8_row_error_max"] == st0["cand8_row_error_max"], entry
    Q = O.synth_dense(O.SEED_QUERY, 0, 8, dim)
    qip, qsi, qsv = O.synth_sparse_queries(O.SEED_SPQUERY, 0, 8, synth_tables)
    r0 = routes(ix)
    s, i, c = unpack_np(eng, *ix.search_dense(torch_mod.from_numpy(Q).cuda(), 20))
    fast(moved(ix, r0), "dense after a refused batch")
    for b in range(8):
        assert_list_equal(s[b], i[b], c[b], *ora.search_dense(Q[b], 20), f"dense b={b}")
    hp = eng.make_params(dict(P_TREE, dense_limit=50, sparse_limit=50, final_limit=10), mode=eng.HX_MODE_H1)
    s, i, c = ix.hybrid_query_host(Q, qip, qsi.astype(np.int32), qsv, hp)
    for b in range(8):
        es, ei = O.hybrid_h1(ora, Q[b], qsi[qip[b]:qip[b + 1]], qsv[qip[b]:qip[b + 1]], 50, 50, 10)
        assert_list_equal(s[b], i[b], c[b], es, ei, f"h1 b={b}")
    Xb[29, 200] = 0.5                                          # the same batch, finite: stored
    ix.add_device(torch_mod.from_numpy(Xb).cuda(), bip, bsi, bsv)
    assert ix.count() == n + 40
    # row 17 does raise the bound: the refused batches above had something to roll back
    assert ix.stats()["cand8_row_error_max"] > 2 * st0["cand8_row_error_max"], (st0["cand8_row_error_max"], ix.stats())
    ix.close()


@pytest.mark.parametrize("bad", BADS)
def test_non_finite_queries_refused(rrf_world, eng, torch_mod, bad):
    """A query with a NaN / +Inf / -Inf element (past the 64-prefix, so the prefix stage must look at the whole row) is
    an error through every dense entry; the asynchronous entries flag the batch.  Each refusal leaves nothing behind:
    the next good call returns the oracle's lists."""
    w = rrf_world
    B = 4
    Q = w.Q[:B].copy()
    Q[2, 200] = bad
    Qd = torch_mod.from_numpy(Q).cuda()
    tq = (w.tq[0][:B + 1], w.tq[1], w.tq[2])
    hp1 = eng.make_params(dict(P_TREE, dense_limit=100, sparse_limit=100, final_limit=10), mode=eng.HX_MODE_H1)
    hpt = eng.make_params(P_TREE)
    good = [O.rrf([w.dl[b][:100], w.sl[b][:100]], limit=10) for b in range(B)]

    def check_good():
        s, i, c = w.ix.hybrid_query_host(w.Q[:B], w.qip[:B + 1], w.qsi, w.qsv, hp1)
        for b in range(B):
            assert_list_equal(s[b], i[b], c[b], *good[b], f"good call after a refusal b={b}")

    calls = {
        "search_dense": lambda: w.ix.search_dense(Qd, 10),
        "search_dense m64": lambda: w.ix.search_dense(Qd, 10, 64),
        "search_dense m128 (exact)": lambda: w.ix.search_dense(Qd, 10, 128),
        "search_i8": lambda: w.ix.search_i8(Qd, 10),
        "tree host": lambda: w.ix.hybrid_query_host(Q, w.qip[:B + 1], w.qsi, w.qsv, hpt),
        "tree dev": lambda: w.ix.hybrid_query(Qd, *tq, hpt),
        "h1 host": lambda: w.ix.hybrid_query_host(Q, w.qip[:B + 1], w.qsi, w.qsv, hp1),
        "h1 dev": lambda: w.ix.hybrid_query(Qd, *tq, hp1),
        "tree masked": lambda: w.ix.hybrid_query_host(Q, w.qip[:B + 1], w.qsi, w.qsv, hpt, mask=w.mask),
        "h1 masked": lambda: w.ix.hybrid_query_host(Q, w.qip[:B + 1], w.qsi, w.qsv, hp1, mask=w.mask),
        "h1_local": lambda: w.ix.h1_local(Qd, *tq, 100, 100),
    }
    for name, call in calls.items():
        with pytest.raises(eng.HxError, match="finite"):
            call()
        check_good()
    for name, call in (("search_dense", lambda f: w.ix.search_dense(Qd, 10, 0, flag=f)),
                       ("search_dense m64", lambda f: w.ix.search_dense(Qd, 10, 64, flag=f)),
                       ("search_i8", lambda f: w.ix.search_i8(Qd, 10, flag=f))):
        flag = torch_mod.zeros((1,), dtype=torch_mod.int32, device=Qd.device)
        call(flag)
        assert int(flag.item()) != 0, f"{name} async: the batch is not flagged"
    assert int(w.ix.h1_local_async(Qd, *tq, 100, 100)[B, 0]) != 0, "h1_local_async: the batch is not flagged"
    check_good()


# ---- 3. degenerate dense values -----------------------------------------------------------------------------------------
def _near_unit(qn, target):
    """qn scaled so that spec_dot(x, x) - 1 lands at `target` (fp32); returns (x, len2 - 1)"""
    best = None
    for d in np.linspace(target / 2 * 0.8, target / 2 * 1.2, 401):
        x = (qn * F32(1.0 + d)).astype(F32)
        e = float(O.spec_dot(x[None, :], x)[0] - F32(1.0))
        if best is None or abs(e - target) < abs(best[1] - target):
            best = (x, e)
    return best


@pytest.fixture(scope="module")
def degen_world(eng, torch_mod, synth_tables):
    w = World()
    w.n, w.dim = 6000, 256
    X = O.synth_dense(O.SEED_CORPUS, 0, w.n, w.dim)
    X = (X * np.random.default_rng(3).uniform(0.2, 3.0, w.n).astype(F32)[:, None]).astype(F32)
    w.zero_rows = [0, 1000, w.n - 1]
    X[w.zero_rows] = 0.0
    X[10:15] = (O.synth_dense(21, 0, 5, w.dim) * F32(1e-39)).astype(F32)      # subnormal elements: kept unnormalised
    X[20:23] = (O.synth_dense(22, 0, 3, w.dim) * F32(3e19)).astype(F32)       # finite, squared length Inf: zero rows
    assert np.isinf(O.spec_dot(X[20:23], X[20:23])).all()
    # near-unit copies of the (normalised) queries 4..7: spec_dot(x, x) - 1 at about -1.1e-6, -0.9e-6 (-6 inside the
    # keep-if-unit threshold |len^2 - 1| <= 1e-6), +0.9e-6 and +1.1e-6
    Qs = O.synth_dense(O.SEED_QUERY, 0, 8, w.dim)
    w.near = {}
    for t in range(4):
        qn = O.cosine_preprocess(Qs[4 + t])
        for j, target in enumerate((-1.1e-6, -0.9e-6, 0.9e-6, 1.1e-6)):
            x, e = _near_unit(qn, target)
            r = 30 + 4 * t + j
            X[r] = x
            w.near[r] = e
    inside = [r for r, e in w.near.items() if abs(F32(e)) <= F32(1e-6)]
    outside = [r for r, e in w.near.items() if F32(1e-6) < abs(F32(e)) < F32(2e-6)]
    assert len(inside) >= 6 and len(outside) >= 6, w.near
    # 600 exact copies of one row: a tie group larger than L' = 450 at L = 100
    w.tie = O.synth_dense(23, 0, 1, w.dim)[0]
    X[2000:2600] = w.tie
    w.X = X
    w.ip, w.si, w.sv = O.synth_sparse_docs(O.SEED_SPDOC, 0, w.n, synth_tables)
    w.ora = O.OracleIndex(w.dim, (64, 128, 256))
    w.ora.add(X, w.ip, w.si, w.sv)
    w.ora.finalize()
    w.ix = eng.HxIndex(w.dim, (64, 128, 256))
    w.ix.add(X, w.ip, w.si.astype(np.int32), w.sv)
    # queries: zero, subnormal, finite with an infinite squared length, the tie row, queries 4..7 (near-unit rows), then
    # ordinary ones
    NQ = 300
    Q = O.synth_dense(O.SEED_QUERY, 0, NQ, w.dim)
    Q[0] = 0.0
    Q[1] = (O.synth_dense(24, 0, 1, w.dim)[0] * F32(1e-40)).astype(F32)
    Q[2] = (O.synth_dense(25, 0, 1, w.dim)[0] * F32(3e19)).astype(F32)
    Q[3] = w.tie
    w.Q = Q
    w.zeroish = (0, 2)                                         # queries that normalise to zero
    w.degenerate = (0, 1, 2, 3)                                # ... and the subnormal and the tie query
    w.qip, w.qsi, w.qsv = O.synth_sparse_queries(O.SEED_SPQUERY, 0, NQ, synth_tables)
    w.qsi = w.qsi.astype(np.int32)
    w.cache = {}
    yield w
    w.ix.close()


def _expect(w, what, b):
    key = (what, b)
    if key not in w.cache:
        q = w.Q[b]
        qs = (w.qsi[w.qip[b]:w.qip[b + 1]], w.qsv[w.qip[b]:w.qip[b + 1]])
        if what == "dense":
            w.cache[key] = w.ora.search_dense(q, 100)
        elif what == "m64":
            w.cache[key] = w.ora.search_dense(q, 100, 64)
        elif what == "i8":
            w.cache[key] = w.ora.search_i8(q, 50)
        elif what == "tree":
            w.cache[key] = O.hybrid_tree(w.ora, q, *qs, P_TREE)
        else:
            w.cache[key] = O.hybrid_h1(w.ora, q, *qs, 100, 100, 10)
    return w.cache[key]


def _tied(w, what, b):
    """query b's top 200 of the stage holds rows of the 600-row tie group: its candidate list may be cut inside the
    group (the certificate cannot hold, the query is retried and may need the exact path)"""
    key = (what + "200", b)
    if key not in w.cache:
        q = w.Q[b]
        ids = (w.ora.search_i8(q, 200) if what == "i8" else w.ora.search_dense(q, 200, 64 if what == "m64" else 0))[1]
        w.cache[key] = bool(((ids >= 2000) & (ids < 2600)).any())
    return w.cache[key]


def _batches(B):
    if B == 1:
        return [[b] for b in range(8)]
    return [list(range(B))]


@pytest.mark.parametrize("B", [1, 33, 129, 300])
@pytest.mark.parametrize("cand", ["i8", "f16"])
def test_degenerate_dense_values(degen_world, eng, torch_mod, B, cand):
    """Zero rows (row 0 and the last row among them), rows of subnormal size (kept unnormalised), rows whose squared
    length overflows (stored as zero rows), near-unit copies of queries on each side of the keep-if-unit threshold,
    600 exact copies of one row (ties beyond the candidate buffers, broken by id), against a zero query, a query of
    subnormal size and one whose squared length overflows -- through the full-vector stage on int8 and fp16 candidates,
    the 64-prefix, the quantized stage, the tree and H1, at the batch sizes of every scan routing."""
    w = degen_world
    w.ix.set_dense_candidates(cand)
    hpt = eng.make_params(P_TREE)
    hp1 = eng.make_params(dict(P_TREE, dense_limit=100, sparse_limit=100, final_limit=10), mode=eng.HX_MODE_H1)
    try:
        for sel in _batches(B):
            Q = w.Q[sel]
            Qd = torch_mod.from_numpy(np.ascontiguousarray(Q)).cuda()
            qip = np.concatenate([[0], np.cumsum([w.qip[b + 1] - w.qip[b] for b in sel])]).astype(np.int64)
            qsi = np.concatenate([w.qsi[w.qip[b]:w.qip[b + 1]] for b in sel])
            qsv = np.concatenate([w.qsv[w.qip[b]:w.qip[b + 1]] for b in sel])
            nz = sum(1 for b in sel if b in w.zeroish)
            # only these may leave the fast paths: the degenerate queries, and those the tie group reaches
            slow = {st: sum(1 for b in sel if b in w.degenerate or _tied(w, st, b)) for st in ("dense", "m64", "i8")}
            for what, call in (("dense", lambda: w.ix.search_dense(Qd, 100)),
                               ("m64", lambda: w.ix.search_dense(Qd, 100, 64)),
                               ("i8", lambda: w.ix.search_i8(Qd, 50))):
                r0 = routes(w.ix)
                s, i, c = unpack_np(eng, *call())
                d = moved(w.ix, r0)
                for j, b in enumerate(sel):
                    assert_list_equal(s[j], i[j], c[j], *_expect(w, what, b), f"{what} {cand} B={B} q={b}")
                where = (what, cand, B, d)
                ndeg = slow[what]
                assert d["sparse_fallback_queries"] == 0, where
                if what == "i8":
                    # (its retries -- a candidate buffer of the 300-query scan that overflowed, re-run at the safe
                    # geometry -- are not bounded here; the exact path is)
                    assert d["cand8_queries"] == 0 and d["dense_fallback_queries"] == 0, where
                    assert d["i8_fallback_queries"] <= ndeg, where
                    continue
                # a query that normalises to zero scores every row 0: no certificate holds, the exact path serves it
                assert d["retry_queries"] <= ndeg, where
                assert nz <= d["dense_fallback_queries"] <= ndeg and d["i8_fallback_queries"] == 0, where
                assert d["cand8_queries"] == (len(sel) if what == "dense" and cand == "i8" else 0), where
                assert d["cand8_uncertified_queries"] <= ndeg, where
            for what, hp in (("tree", hpt), ("h1", hp1)):
                r0 = routes(w.ix)
                s, i, c = w.ix.hybrid_query_host(Q, qip, qsi, qsv, hp)
                d = moved(w.ix, r0)
                for j, b in enumerate(sel):
                    assert_list_equal(s[j], i[j], c[j], *_expect(w, what, b), f"{what} {cand} B={B} q={b}")
                where = (what, cand, B, d)
                ndeg = slow["dense"] if what == "h1" else max(slow["m64"], slow["i8"])
                assert d["sparse_fallback_queries"] == 0 and d["cand8_uncertified_queries"] <= ndeg, where
                if what == "tree":          # one prefix scan and one int8 scan
                    assert d["cand8_queries"] == 0, where      # (its int8 scan's retries: as the quantized stage above)
                    assert nz <= d["dense_fallback_queries"] <= ndeg and d["i8_fallback_queries"] <= ndeg, where
                else:
                    assert d["cand8_queries"] == (len(sel) if cand == "i8" else 0), where
                    assert d["retry_queries"] <= ndeg and nz <= d["dense_fallback_queries"] <= ndeg, where
                    assert d["i8_fallback_queries"] == 0, where
    finally:
        w.ix.set_dense_candidates("i8")


def test_degenerate_rows_derived_as_the_contract_says(degen_world, eng, torch_mod):
    """The stored rows of the planted cases equal the oracle's bit for bit: the near-unit rows inside the threshold kept
    as they are, those just outside it normalised, subnormal rows kept, overflowing rows zero."""
    w = degen_world
    for r in list(w.near) + w.zero_rows + list(range(10, 15)) + list(range(20, 23)) + [2000, 2599]:
        np.testing.assert_array_equal(w.ix.debug_row(0, r).view(np.uint32), w.ora.dense[r].view(np.uint32), err_msg=str(r))
    for r, e in w.near.items():
        kept = np.array_equal(w.ora.dense[r].view(np.uint32), w.X[r].view(np.uint32))
        assert kept == (abs(F32(e)) <= F32(1e-6)), (r, e)
    assert not w.ora.dense[20:23].any() and not w.ora.dense[w.zero_rows].any()


# ---- 4. sparse extremes -----------------------------------------------------------------------------------------------
BIG = F32(1e18)
HOT, TINY, T0, T30, TM2, TM1 = 77, 91, 0, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 1
EXT = [2 ** 30 + 1 + j for j in range(64)]


def _sparse_docs(n, seed, big):
    """~20 terms per document from a pool in [1000, 2^29), weights in [0.5, 1.5], plus the planted extremes: weights
    1e-45 and 1e-38 (products underflow to +0), term ids 0, 2^30, 2^31-2, 2^31-1 -- and with `big` one posting at 1e18
    among weights near 1 and four documents of up to 64 terms at 1e18"""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(1000, 2 ** 29, 3000))
    rows = []
    for d in range(n):
        t = np.unique(rng.choice(pool, 20))
        v = rng.uniform(0.5, 1.5, t.size).astype(F32)
        extra = {}
        if d % 7 == 0:
            extra[HOT] = F32(rng.uniform(0.5, 1.5))
        if big and d == 5:
            extra[HOT] = BIG
        if d in (10, 11):
            extra[TINY] = F32(1e-45)
        if d in (12, 13):
            extra[TINY] = F32(1e-38)
        if big and d in (20, 21, 22, 23):
            for e in EXT[: 64 - (d - 20)]:
                extra[e] = BIG                                 # 64 x 1e18 x 1e18: sums near 6e37, finite
        if d in (30, n - 1):
            extra.update({T0: F32(1.0), TM1: F32(2.0)})
        if d in (31, n - 2):
            extra.update({T30: F32(1.5), TM2: F32(0.75)})
        t = np.concatenate([t, np.asarray(list(extra), np.int64)])
        v = np.concatenate([v, np.asarray(list(extra.values()), F32)])
        o = np.argsort(t)
        rows.append((t[o], v[o]))
    ip = np.concatenate([[0], np.cumsum([r[0].size for r in rows])]).astype(np.int64)
    return ip, np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])


# Query batches by the route they must take (k_sparse_prep): the integer scale of a query is (65535 - T - 8) /
# (sum of its weights x the index's largest weight); above 1e30 the query goes to the document-at-a-time path by
# design.  "select" batches must be served by the integer select pass (no query on the exact path).
SPARSE_BATCHES = {
    "small": {
        # ordinary terms, the term-id extremes, and a 1e-45 query weight beside a weight of 1 (its products with
        # weights near 1 and with 1e-45 / 1e-38 underflow): the select pass
        "select": [([HOT, 5000], [1.0, 1.0]), ([T0, T30, TM2, TM1], [1.0, 1.0, 1.0, 1.0]), ([T0], [1.0]),
                   ([TM1], [0.5]), ([HOT, TINY], [1e-45, 1.0])],
        # weights 1e-45 / 1e-38 alone: the scale would pass 1e30 -- both on the exact path
        "tiny": [([TINY], [1e-45]), ([TINY], [1e-38])],
    },
    "big": {
        # 64 terms at 1e18 against documents at 1e18 (sums near 6e37), and a 1e18 query weight: the select pass
        "select": [(EXT, [1e18] * 64), ([T0], [1e18]), ([T0, T30, TM2, TM1], [1.0, 1.0, 1.0, 1.0])],
        # the 1e18 posting of HOT puts every other posting of the term on the +1 integer floor
        "hot": [([HOT, 5000], [1.0, 1.0])],
    },
}
# queries of each batch served by the document-at-a-time path (sparse_fallback_queries), per limit
# (the 1e18 posting: the select pass keeps the whole set of documents on the +1 floor and serves the query itself)
SPARSE_ROUTES = {("small", "select"): 0, ("small", "tiny"): 2, ("big", "select"): 0, ("big", "hot"): 0}


def _csr(qs):
    ip = np.concatenate([[0], np.cumsum([len(t) for t, _ in qs])]).astype(np.int64)
    idx = np.concatenate([np.asarray(t, np.int64) for t, _ in qs])
    val = np.concatenate([np.asarray(v, F32) for _, v in qs])
    for b in range(len(qs)):
        o = np.argsort(idx[ip[b]:ip[b + 1]])
        idx[ip[b]:ip[b + 1]] = idx[ip[b]:ip[b + 1]][o]
        val[ip[b]:ip[b + 1]] = val[ip[b]:ip[b + 1]][o]
    return ip, idx, val


def _check_sparse(eng, torch_mod, ix, ora, kind, what, observed, limits=(10, 100)):
    for name, qs in SPARSE_BATCHES[kind].items():
        qip, qsi, qsv = _csr(qs)
        B = qip.size - 1
        tq = (torch_mod.from_numpy(qip).cuda(), torch_mod.from_numpy(qsi.astype(np.int32)).cuda(),
              torch_mod.from_numpy(qsv).cuda())
        for L in limits:
            r0 = routes(ix)
            s, i, c = unpack_np(eng, *ix.search_sparse(*tq, L))
            d = moved(ix, r0)
            for b in range(B):
                es, ei = ora.search_sparse(qsi[qip[b]:qip[b + 1]], qsv[qip[b]:qip[b + 1]], L)
                assert_list_equal(s[b], i[b], c[b], es, ei, f"{what} {name} L={L} q={b}")
            observed[(what, name, L)] = d["sparse_fallback_queries"]
            assert d["retry_queries"] == 0 and d["dense_fallback_queries"] == 0, (what, d)


@pytest.mark.parametrize("seg", ["32768", "65536", "spread"])
@pytest.mark.parametrize("kind", ["small", "big"])
def test_sparse_extremes(eng, torch_mod, monkeypatch, seg, kind):
    """Weights from 1e-45 to 1e18 and term ids 0, 2^30, 2^31-2, 2^31-1 in documents and queries, through a base build,
    a tail build and after truncate, at both segment sizes and once with the bank-spread posting order -- each query
    batch on the route SPARSE_ROUTES pins."""
    if seg == "spread":
        monkeypatch.setenv("HX_SP_SPREAD", "1")
    else:
        monkeypatch.setenv("HX_DEBUG_SEG_DOCS", seg)
    monkeypatch.setenv("HX_DEBUG_TAIL_MIN", "100000")          # the second batch goes to a tail index
    n0, n1, dim = 5000, 1500, 64
    ip, si, sv = _sparse_docs(n0 + n1, 11, kind == "big")
    X = O.synth_dense(O.SEED_CORPUS, 0, n0 + n1, dim)
    ix = eng.HxIndex(dim, ())
    observed = {}
    try:
        ix.add(X[:n0], ip[:n0 + 1], si[:ip[n0]].astype(np.int32), sv[:ip[n0]])
        ora0 = O.OracleIndex(dim, ())
        ora0.add(X[:n0], ip[:n0 + 1], si[:ip[n0]], sv[:ip[n0]])
        ora0.finalize()
        _check_sparse(eng, torch_mod, ix, ora0, kind, "base", observed)
        ix.add(X[n0:], ip[n0:] - ip[n0], si[ip[n0]:].astype(np.int32), sv[ip[n0]:])
        assert ix.stats()["n_segments"] > 0
        ora1 = O.OracleIndex(dim, ())
        ora1.add(X, ip, si, sv)
        ora1.finalize()
        _check_sparse(eng, torch_mod, ix, ora1, kind, "tail", observed)
        m = n0 - 3
        ix.truncate(m)
        ora2 = O.OracleIndex(dim, ())
        ora2.add(X[:m], ip[:m + 1], si[:ip[m]], sv[:ip[m]])
        ora2.finalize()
        _check_sparse(eng, torch_mod, ix, ora2, kind, "truncated", observed)
    finally:
        ix.close()
    want = {k: SPARSE_ROUTES[(kind, k[1])] for k in observed}
    assert observed == want, f"{kind} {seg}: queries on the exact path {observed}, pinned {want}"


def test_sparse_weight_bound_is_the_same_everywhere(eng, torch_mod):
    """The largest fp32 <= 1e18 is accepted and the next one refused, by the host entry, the device entry and the
    sharded front end's check alike; a refused batch stores nothing."""
    from rag_application_amd.sharded import check_sparse_rows
    top = F32(1e18)
    nxt = np.nextafter(top, F32(np.inf), dtype=F32)
    X = O.synth_dense(1, 0, 2, 64)
    ip = np.asarray([0, 1, 2], np.int64)
    idx = np.asarray([3, 2 ** 31 - 1], np.int32)
    ix = eng.HxIndex(64, ())
    for sign in (F32(1), F32(-1)):
        ok = np.asarray([sign * top, F32(1)], F32)
        bad = np.asarray([sign * nxt, F32(1)], F32)
        check_sparse_rows(ip, idx, ok)
        with pytest.raises(ValueError, match="1e18"):
            check_sparse_rows(ip, idx, bad)
        for entry in ("host", "device"):
            n0, z0 = ix.count(), ix.stats()["nnz"]
            add = ix.add if entry == "host" else (lambda x, *a: ix.add_device(torch_mod.from_numpy(x).cuda(), *a))
            with pytest.raises(eng.HxError, match="1e18"):
                add(X, ip, idx, bad)
            assert ix.count() == n0 and ix.stats()["nnz"] == z0
            add(X, ip, idx, ok)
            assert ix.count() == n0 + 2 and ix.stats()["nnz"] == z0 + 2
    ix.close()
