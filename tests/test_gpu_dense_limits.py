"""GPU: the dense stage's tail at every limit boundary, small batches -- k_dense_finish with 2, 4 and 8 keys per lane
(select.hip; L <= 128 / 256 / 512, B <= 64, L' <= 512), the three launches on the other side of each boundary, and the
k_compact_top forms behind the scan launches that the limits drive (tests/test_dense_route_host.py: where the
boundaries are and why).

Every list is compared bit for bit, ids AND fp32 score bits, with the C restatement (CO.search_dense on
CO.cosine_preprocess'ed rows).  Every cell first asks engine.dense_route which kernels serve it and asserts that this is
the route the cell is about; the dense stage decides by the functions behind that report.  The route counters are read
around every search, as in tests/test_gpu_row_widths.py: a wrong finish must not hide behind a retry or the exact path.

Corpus A: 20,000 x 128, X = synth_dense(31) * 2.5, Q = synth_dense(32) * 0.3, one prefix size (64); more than two scan
launches at every geometry (C <= 8192).  On it the exact scores at ranks L and L' are at least 0.0075 apart in every
fp16 cell (six times HX_EPS_F16) and 0.045 in every int8 cell (ordinary rows' int8 error: 0.0046), so which queries
certify does not hang on a rounding.
Corpus B (the retry level): 20,000 x 768, same seeds, one row replaced by (1, c, ..., c), c = 0.49 / 127 -- see
test_retry_level_at_its_limit_boundaries."""
import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import oracle as O
from tests.test_gpu_parity import P_MCP, unpack_np
from tests.test_gpu_row_widths import ROUTES, assert_list_equal, check_lists, corpus, dense_cell, measured

pytestmark = pytest.mark.gpu

F32 = np.float32
N, DIM, PREFIX = 20000, 128, 64
NQ = 65                      # queries of corpus A: the batches are its first B
LMAX = 342                   # the longest limit of the module: a shorter limit's list is the prefix (one total order)
BATCHES = (1, 32, 33, 64, 65)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def eng():
    from rag_application_amd import engine
    return engine


def route_name(eng, B, L, cand, level=0):
    fe = eng.dense_route(B, L, cand, level)[2]
    return f"E={fe}" if fe else "unfused"


def want_route(L, B, cand, level=0):
    """what the cell's NAME says: the table of the host test, written out"""
    last = 171 if level else (113 if cand == "i8" else 341)
    if B > 64 or L > last:
        return "unfused"
    return "E=2" if L <= 128 else ("E=4" if L <= 256 else "E=8")


def state_route(eng, B, L, cand, level=0):
    got = route_name(eng, B, L, cand, level)
    assert got == want_route(L, B, cand, level), f"B={B} L={L} {cand} level {level}: on route {got}"
    return got


class WorldA:
    """corpus A, its references and the default index (dense rows only; profile on)"""

    def __init__(self, eng, torch_mod):
        self.X, self.Q = corpus(N, DIM, NQ)
        self.Xn, self.Qn = CO.cosine_preprocess(self.X), CO.cosine_preprocess(self.Q)
        self.ref = CO.search_dense(self.Xn, self.Qn, LMAX)
        self.ref64 = CO.search_dense(CO.cosine_preprocess(self.X, PREFIX), CO.cosine_preprocess(self.Q, PREFIX), LMAX)
        self.Qd = torch_mod.from_numpy(self.Q).cuda()
        self.ix = self.index(eng)

    def index(self, eng):
        ix = eng.HxIndex(DIM, (PREFIX,))
        ix.add(self.X)
        ix.profile(True)
        return ix


@pytest.fixture(scope="module")
def world(eng, torch_mod):
    w = WorldA(eng, torch_mod)
    yield w
    w.ix.close()


# ---- a. the sweep ------------------------------------------------------------------------------------------------------------
SWEEP = ([("f16", L) for L in (1, 64, 65, 128, 129, 255, 256, 257, 340, 341, 342)] + [("i8", L) for L in (1, 50, 113, 114)] +
         [("prefix", L) for L in (128, 129, 256, 257, 341, 342)])


def run_cell(eng, w, ix, kind, L, B):
    """one cell of the sweep on `ix`: the route it is on, then dense_cell (lists against the oracle, route counters)"""
    cand = "i8" if kind == "i8" else "f16"
    rt = state_route(eng, B, L, cand)
    if kind == "prefix":
        return dense_cell(eng, ix, w.Qd, B, L, "f16", w.ref64, f"limits {rt}", prefix=PREFIX)
    return dense_cell(eng, ix, w.Qd, B, L, cand, w.ref, f"limits {rt}")


@pytest.mark.parametrize("kind,L", SWEEP)
def test_limit_sweep(world, eng, torch_mod, kind, L):
    """Both sides of every boundary of the finish (L = 128 | 129: E 2 | 4; 256 | 257: E 4 | 8; 341 | 342 with fp16 and
    113 | 114 with int8 candidates: fused | three launches) at B = 1, 32, 33, 64 and 65 (never fused), through the
    full-vector stage on fp16 and int8 candidates and the first prefix stage.  fp16 cells: no retry, no exact fallback,
    every counter delta zero; int8 cells: at most B // 4 + 1 queries uncertified, each retried once, none served exactly
    (dense_cell).  The limits also drive the scan's compaction through k_compact_top<4, 4> (L' <= 128), <8, 4> (L' <=
    256), <8, 8> (L' <= 512) and the LDS sort, each with its threshold rank and underflow flag."""
    for B in BATCHES:
        run_cell(eng, world, world.ix, kind, L, B)


# ---- b. fused against unfused against forced grids -----------------------------------------------------------------------------
FUSED_CELLS = [(kind, L, B) for kind, L in SWEEP for B in (1, 64) if want_route(L, B, "i8" if kind == "i8" else "f16") != "unfused"]


def raw_call(w, ix, kind, L, B):
    if kind != "prefix":
        ix.set_dense_candidates("i8" if kind == "i8" else "f16")
    k, c = ix.search_dense(w.Qd[:B], L, PREFIX if kind == "prefix" else 0)
    return k.cpu(), c.cpu()


@pytest.fixture(scope="module")
def default_outputs(world, eng):
    """keys and counts of every fused cell on the default index, each checked against the oracle"""
    out = {}
    for kind, L, B in FUSED_CELLS:
        run_cell(eng, world, world.ix, kind, L, B)
        out[(kind, L, B)] = raw_call(world, world.ix, kind, L, B)
    return out


@pytest.mark.parametrize("env", [("HX_DEBUG_NO_FINISH_FUSE", "1"), ("HX_DEBUG_FINISH_NB", "1"), ("HX_DEBUG_FINISH_NB", "3"),
                                 ("HX_DEBUG_FINISH_NB", "128"), ("HX_DEBUG_FINISH_NB", "200")],
                         ids=lambda e: f"{e[0][9:]}={e[1]}")
def test_fused_equals_unfused_and_every_forced_grid(world, default_outputs, eng, torch_mod, monkeypatch, env):
    """A second index over the same rows with the three launches forced, then with 1 block per query (one block does
    everything), 3 (the stride loop with a remainder), 128 and 200 (more blocks than candidates of most cells: blocks
    without work still count toward "last"): keys and counts torch.equal to the default index's on every fused cell of
    the sweep at B = 1 and 64 -- and so, through default_outputs, to the oracle's.  The switches are read by hx_create."""
    monkeypatch.setenv(*env)
    ix = world.index(eng)
    monkeypatch.delenv(env[0])
    try:
        for cell in FUSED_CELLS:
            k, c = raw_call(world, ix, *cell)
            dk, dc = default_outputs[cell]
            assert torch_mod.equal(c, dc), (env, cell, "counts")
            assert torch_mod.equal(k, dk), (env, cell, "keys")
    finally:
        ix.close()


# ---- c. the per-query counters across calls --------------------------------------------------------------------------------------
def test_counters_survive_a_sequence_of_calls(world, eng, torch_mod):
    """The kernel leaves its per-query counters at zero and the host clears them only when the batch grows: growing and
    shrinking batches, another instantiation, the int8 route (its own L' and grid) and back, on ONE index, every call
    against the oracle.  Then one call eight times over: bit-identical outputs (the determinism of a call that
    succeeds, nothing else)."""
    w = world
    ix = w.index(eng)
    try:
        for cand, L, B in [("f16", 129, 8), ("f16", 129, 64), ("f16", 129, 1), ("f16", 129, 64), ("f16", 129, 33), ("f16", 341, 64),
                           ("f16", 341, 8), ("i8", 10, 64), ("f16", 129, 64), ("f16", 129, 8)]:
            run_cell(eng, w, ix, cand, L, B)
        state_route(eng, 64, 257, "f16")
        first = raw_call(w, ix, "f16", 257, 64)
        check_lists(eng, (first[0].cuda(), first[1].cuda()), w.ref, 64, 257, "repeat 0")
        for r in range(1, 8):
            k, c = raw_call(w, ix, "f16", 257, 64)
            assert torch_mod.equal(k, first[0]) and torch_mod.equal(c, first[1]), f"repeat {r} differs"
    finally:
        ix.close()


# ---- d. short lists ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 300, 400, 511, 512])
def test_short_lists_through_the_widest_finish(world, eng, torch_mod, n):
    """Indexes over the first n rows, L = 341 (L' = 511, E = 8), fp16 candidates, B = 1 and 40: a single row; n < L (the
    count is n, the tail empty); L <= n < L' (the candidate list is not full: no certificate); n = L' and L' + 1.  The
    lists are the oracle's; the route counters are printed, and the exact path -- which would serve the same lists --
    is not what is under test, so only the lists are asserted."""
    w, L = world, 341
    ref = CO.search_dense(w.Xn[:n], w.Qn[:40], L)
    ix = eng.HxIndex(DIM, ())
    ix.add(w.X[:n])
    ix.profile(True)
    ix.set_dense_candidates("f16")
    try:
        for B in (1, 40):
            assert state_route(eng, B, L, "f16") == "E=8"
            out, d, launches = measured(ix, lambda: ix.search_dense(w.Qd[:B], L))
            print(f"[limits] n={n} B={B} L={L}: {d} launches {launches}")
            s, i, c = unpack_np(eng, *out)
            for b in range(B):
                m = int(ref[2][b])
                assert m == min(n, L)
                assert_list_equal(s[b], i[b], c[b], ref[0][b, :m], ref[1][b, :m], f"n={n} B={B} b={b}")
    finally:
        ix.close()


# ---- the certificate's own rank: a list that must NOT certify -------------------------------------------------------------------
def designed_corpus(L, n=N, ties=700, seed=11):
    """Rows s_j * q + sqrt(1 - s_j^2) * u_j (u_j unit, orthogonal to the unit query q) with chosen scores s_j: ranks 1 to
    L - 1 descend from 0.95 in steps of 2.5e-3 (twice HX_EPS_F16), then `ties` copies of ONE row 2.5e-3 below the last of
    them, the rest in [-0.6, 0]; row order shuffled.  The tie group starts at rank L and reaches beyond L' = L + L / 2."""
    rng = np.random.default_rng(seed + L)
    q = rng.standard_normal(DIM)
    q /= np.linalg.norm(q)
    s = np.concatenate([0.95 - 2.5e-3 * np.arange(L - 1), np.full(ties, 0.95 - 2.5e-3 * (L - 1)),
                        rng.uniform(-0.6, 0.0, n - (L - 1) - ties)])
    u = rng.standard_normal((n, DIM))
    u[L - 1:L - 1 + ties] = u[L - 1]
    u -= np.outer(u @ q, q)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    X = (s[:, None] * q + np.sqrt(1.0 - s * s)[:, None] * u).astype(F32)
    return X[rng.permutation(n)], q.astype(F32)


@pytest.mark.parametrize("L", [128, 129, 257, 341])
def test_a_list_cut_inside_a_tie_group_is_never_certified(eng, torch_mod, L):
    """The other side of the certificate m + eps < e_L: the sweep shows that it holds where it must (a finish that read
    a LOWER key than the L-th would flag queries there), this cell that it fails where it must.  The exact L-th key is
    the first of 700 equal rows and the candidate list is cut inside that group, so m is the same score and no eps > 0
    lets it pass; every key above rank L is at least 2.5e-3 better, so a finish that took its e_L from any other lane
    or register of the sorted run (the pick is kr & (E - 1), kr / E) would certify.  Every query of the call must be
    retried, with 2, 4 and 8 keys per lane, at B = 1 and 64; the lists are still the oracle's, ties broken by id."""
    X, q = designed_corpus(L)
    lp = eng.dense_route(1, L, "f16")[0]
    Xn, qn = CO.cosine_preprocess(X), CO.cosine_preprocess(q[None, :] * F32(0.3))
    es, ei, ec = CO.search_dense(Xn, qn, lp + 1)
    assert ec[0] == lp + 1 and es[0, L - 2] - es[0, L - 1] > 2e-3 and es[0, L - 1] == es[0, lp], "the design does not hold"
    Qd = torch_mod.from_numpy(np.tile(q * F32(0.3), (64, 1))).cuda()
    ix = eng.HxIndex(DIM, ())
    ix.add(X)
    ix.profile(True)
    ix.set_dense_candidates("f16")
    try:
        for B in (1, 64):
            rt = state_route(eng, B, L, "f16")
            out, d, launches = measured(ix, lambda: ix.search_dense(Qd[:B], L))
            print(f"[limits] tie group at rank {L} ({rt}) B={B}: {d} launches {launches}")
            s, i, c = unpack_np(eng, *out)
            for b in range(B):
                assert_list_equal(s[b], i[b], c[b], es[0, :L], ei[0, :L], f"ties L={L} B={B} b={b}")
            assert d["retry_queries"] == B, (L, B, d)
    finally:
        ix.close()


# ---- e. the retry level ----------------------------------------------------------------------------------------------------------
def test_retry_level_at_its_limit_boundaries(eng, torch_mod):
    """Corpus B: one row (1, c, ..., c), c = 0.49 / 127, whose small components all round to zero on the int8 grid: its
    stored error, 0.106, is the index's largest row error E_X, and the int8 certificate's radius contains E_X * |q|
    (prep.hip, k_prep_queries_s8) -- more than the exact gap between ranks L and L' of any query (at most 0.075 at L = 1,
    less above).  So every query of an int8 call is uncertified and re-run at level 1 on the fp16 copy, where L' is
    doubled: L = 1, 128 (E = 2), 129, 171 (E = 4) and 172 (L' = 516: three launches).  The smallest gap at the doubled
    L' is 0.0139, so the certificate holds there.  160 queries in all: the guard's window of 4096 never closes."""
    n, dim, B, bad_row = 20000, 768, 32, 12345
    X, Q = corpus(n, dim, B)
    X[bad_row] = F32(0.49 / 127)
    X[bad_row, 0] = 1.0
    ref = CO.search_dense(CO.cosine_preprocess(X), CO.cosine_preprocess(Q), 172)
    Qd = torch_mod.from_numpy(Q).cuda()
    ix = eng.HxIndex(dim, ())
    ix.add(X)
    del X
    ix.profile(True)
    ix.set_dense_candidates("i8")
    try:
        for L, level1 in ((1, "E=2"), (128, "E=2"), (129, "E=4"), (171, "E=4"), (172, "unfused")):
            assert state_route(eng, B, L, "f16", 1) == level1
            out, d, launches = measured(ix, lambda: ix.search_dense(Qd, L))
            print(f"[limits] retry level L={L} ({level1}): retried {d['retry_queries']} of {B}; {d} launches {launches}")
            check_lists(eng, out, ref, B, L, f"retry level L={L}")
            assert d["retry_queries"] == d["cand8_uncertified_queries"] >= 1, (L, d)
            assert d["dense_fallback_queries"] == 0, (L, d)
            assert ix.stats()["cand8_switched_off"] == 0, L
    finally:
        ix.close()


# ---- f. the same kernel inside the hybrid entries ----------------------------------------------------------------------------------
class Hybrid:
    pass


@pytest.fixture(scope="module")
def hybrid(world, eng, torch_mod, synth_tables):
    h, w = Hybrid(), world
    h.B = 24
    h.ip, h.si, h.sv = CO.synth_sparse_docs(O.SEED_SPDOC, 0, N, synth_tables)
    h.qip, h.qsi, h.qsv = O.synth_sparse_queries(O.SEED_SPQUERY, 0, h.B, synth_tables)
    h.qsi = h.qsi.astype(np.int32)
    h.qs = [(h.qsi[h.qip[b]:h.qip[b + 1]].astype(np.int64), h.qsv[h.qip[b]:h.qip[b + 1]]) for b in range(h.B)]
    h.Q = w.Q[:h.B]
    h.Qd = w.Qd[:h.B]
    h.tq = tuple(torch_mod.from_numpy(a).cuda() for a in (h.qip, h.qsi, h.qsv))
    h.ora = O.OracleIndex(DIM, (PREFIX,))
    h.ora.add(w.X, h.ip, h.si.astype(np.int64), h.sv)
    h.ora.finalize()
    h.mask = np.random.default_rng(5).random(N) < 0.5
    h.kept = np.flatnonzero(h.mask)
    lens = (h.ip[1:] - h.ip[:-1])[h.kept]
    mip = np.zeros(len(h.kept) + 1, np.int64)
    np.cumsum(lens, out=mip[1:])
    take = np.concatenate([np.arange(h.ip[r], h.ip[r + 1]) for r in h.kept])
    h.oram = O.OracleIndex(DIM, (PREFIX,))
    h.oram.add(w.X[h.kept], mip, h.si[take].astype(np.int64), h.sv[take])
    h.oram.finalize()
    h.ix = eng.HxIndex(DIM, (PREFIX,))
    h.ix.add(w.X, h.ip, h.si.astype(np.int32), h.sv)
    h.ix.set_dense_candidates("f16")
    yield h
    h.ix.close()


def moved(ix, call):
    s0 = ix.stats()
    out = call()
    s1 = ix.stats()
    return out, {k: s1[k] - s0[k] for k in ROUTES}


@pytest.mark.parametrize("dl", [129, 257])
def test_h1_dense_stage_on_the_wider_finishes(hybrid, eng, torch_mod, dl):
    """H1 with fp16 candidates and dense_limit 129 (E = 4) and 257 (E = 8) at B = 24, through the host entry and the
    device entry; with dense_limit 257 also under a 50 % row mask, against the oracle of the kept rows."""
    h, sl, fl = hybrid, 50, 30
    assert state_route(eng, h.B, dl, "f16") == ("E=4" if dl == 129 else "E=8")
    hp = eng.make_params(dict(P_MCP, dense_limit=dl, sparse_limit=sl, final_limit=fl), mode=eng.HX_MODE_H1)
    exp = [O.hybrid_h1(h.ora, h.Q[b], *h.qs[b], dl, sl, fl) for b in range(h.B)]
    (s, i, c), d = moved(h.ix, lambda: h.ix.hybrid_query_host(h.Q, h.qip, h.qsi, h.qsv, hp))
    print(f"[limits] h1 dense_limit={dl} host: {d}")
    for b in range(h.B):
        assert_list_equal(s[b], i[b], c[b], *exp[b], f"h1 {dl} host b={b}")
    assert not any(d.values()), (dl, d)
    out, d = moved(h.ix, lambda: h.ix.hybrid_query(h.Qd, *h.tq, hp))
    s, i, c = unpack_np(eng, *out)
    for b in range(h.B):
        assert_list_equal(s[b], i[b], c[b], *exp[b], f"h1 {dl} dev b={b}")
    assert not any(d.values()), (dl, d)
    if dl == 257:
        (s, i, c), d = moved(h.ix, lambda: h.ix.hybrid_query_host(h.Q, h.qip, h.qsi, h.qsv, hp, mask=h.mask))
        print(f"[limits] h1 dense_limit={dl} masked: {d}")
        for b in range(h.B):
            es, ei = O.hybrid_h1(h.oram, h.Q[b], *h.qs[b], dl, sl, fl)
            assert_list_equal(s[b], i[b], c[b], es, h.kept[ei], f"h1 {dl} masked b={b}")
        assert not any(d.values()), (dl, d)


@pytest.mark.parametrize("m64", [129, 341, 342])
def test_tree_prefix_stage_on_the_wider_finishes(hybrid, eng, torch_mod, m64):
    """The reference tree with matryoshka_64_limit 129 (E = 4), 341 (E = 8: the reference's fallback parameters on a
    collection of 3,410 points) and 342 (three launches), the other limits as P_MCP, at B = 1 and 24."""
    h = hybrid
    P = dict(P_MCP, matryoshka_64_limit=m64)
    hp = eng.make_params(P)
    exp = [O.hybrid_tree(h.ora, h.Q[b], *h.qs[b], P) for b in range(h.B)]
    for B in (1, 24):
        assert state_route(eng, B, m64, "f16") == {129: "E=4", 341: "E=8", 342: "unfused"}[m64]
        (s, i, c), d = moved(h.ix, lambda: h.ix.hybrid_query_host(h.Q[:B], h.qip[:B + 1], h.qsi[:h.qip[B]], h.qsv[:h.qip[B]], hp))
        print(f"[limits] tree matryoshka_64_limit={m64} B={B}: {d}")
        for b in range(B):
            assert_list_equal(s[b], i[b], c[b], *exp[b], f"tree {m64} B={B} b={b}")
        assert d["dense_fallback_queries"] == 0 and d["retry_queries"] == 0, (m64, B, d)
