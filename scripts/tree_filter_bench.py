"""Diagnostic: node filters of the query trees on a 10M x 768 synthetic corpus (hx_synth_fill).
  1. each masked leaf (hx_search_*_masked) against its unmasked form at B = 1 and B = 1024, keep = 100 / 50 / 10 / 1 %,
     limit 100: dense, matryoshka_64 (the prefix with a scanned copy), quantized, sparse.  The later prefixes have no
     scanned copy: their leaf is the exact pass over every row, masked or not, and is measured at B = 1 only;
  2. hx_list_keep at 1024 x 200 and 1024 x 8192 (mask, thresholds, both; limit = the stride and limit 10);
  3. the reference's tree with filter_stages="all" through the handler's query_points path against the fixed pipeline's
     hybrid_search path with filter_stages="all" on the same filter, alternated, with the view's share (hx_prof slot 5:
     the list of kept rows and the gathers) of either.  The collection is a stand-in whose ids and payloads are computed
     on demand and whose row mask is put into the cache: what is timed is the steady state of a cached filter.
ms per call from HIP events (median [min-max] of 20 after 3 warm-up calls), as scripts/prefilter_bench.py.  Not part of
bench.py.  argv: rows (default 10M).  Output: one table on stdout (kept as profiles/tree_filter_*.txt)."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rag_application_amd import _lib, engine as eng, filters as FL, handler as HD, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
REPS, WARM = 20, 3
P = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, dense_limit=100,
         quantized_limit=40, sparse_limit=100, final_limit=10, hnsw_ef=128)
FRACTIONS = (1.0, 0.5, 0.1, 0.01)


def view_total_ms(ix):
    p = _lib.HxProf()
    _lib.check(_lib.lib().hx_profile_read(ix._h, C.byref(p)))
    return p.ms[5]


def timed(fn, reps=REPS):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def fmt(t):
    return f"{t[0]:9.3f} [{t[1]:.3f}-{t[2]:.3f}]"


class Rows:
    """ids / payloads of N rows, made when asked for: page = the row's residue mod 100 (the filters below keep ranges)"""

    def __init__(self, n, make):
        self.n, self.make = n, make

    def __len__(self):
        return self.n

    def __getitem__(self, r):
        return self.make(r)


def leaves(ix, tabs, masks):
    print(f"\n1. masked leaves, limit 100, ms per call; unmasked = the entry without a mask")
    for B in (1, 1024):
        Q = eng.synth_queries_dense(768, 0, B, synth.SEED_QUERY)
        tq = [torch.from_numpy(a).cuda() for a in synth.sparse_queries(synth.SEED_SPQUERY, 0, B, tabs)]
        kinds = [("dense", lambda **kw: ix.search_dense(Q, 100, 0, **kw)),
                 ("matryoshka_64", lambda **kw: ix.search_dense(Q, 100, 64, **kw)),
                 ("quantized", lambda **kw: ix.search_i8(Q, 100, **kw)),
                 ("sparse", lambda **kw: ix.search_sparse(*tq, 100, **kw))]
        if B == 1:
            kinds.insert(2, ("matryoshka_128 (exact pass)", lambda **kw: ix.search_dense(Q, 100, 128, **kw)))
        for name, fn in kinds:
            print(f"  {name} B={B}\n    {'unmasked':12s} {fmt(timed(fn))}")
            for frac, words, kept in masks:
                print(f"    keep {frac * 100:5.1f}% {fmt(timed(lambda: fn(mask=words)))}   kept {kept}")


def list_keep(ix, masks):
    print(f"\n2. hx_list_keep, B = 1024, random ids, 50 % mask, thresholds at the median score")
    rng = np.random.default_rng(1)
    words = masks[1][1]
    for stride in (200, 8192):
        ids = rng.integers(0, N, size=(1024, stride))
        sc = -np.sort(-rng.random((1024, stride)).astype(np.float32), axis=1)
        u = sc.view(np.uint32).astype(np.uint64) | np.uint64(0x80000000)
        keys = torch.from_numpy(((u << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - ids.astype(np.uint64))).view(np.int64)).cuda()
        thr = torch.full((1024,), 0.5, dtype=torch.float32, device="cuda")
        for limit in (stride, 10):
            for name, kw in (("mask", dict(mask=words)), ("thresholds", dict(thresholds=thr)),
                             ("both", dict(mask=words, thresholds=thr))):
                t = timed(lambda: ix.list_keep(keys, None, limit, **kw))
                print(f"    1024 x {stride:4d} -> limit {limit:4d}  {name:10s} {fmt(t)}")


def reference_tree(q, sp, p=P):
    c = {"query": q, "using": "matryoshka_64", "limit": p["matryoshka_64_limit"]}
    c = {"prefetch": [c], "query": q, "using": "matryoshka_128", "limit": p["matryoshka_128_limit"]}
    c = {"prefetch": [c], "query": q, "using": "matryoshka_256", "limit": p["matryoshka_256_limit"]}
    c = {"prefetch": [c], "query": q, "using": "dense", "limit": p["dense_limit"]}
    quant = {"prefetch": [{"query": q, "using": "quantized", "limit": p["quantized_limit"]}], "query": q, "using": "dense",
             "limit": p["dense_limit"]}
    fusion = {"prefetch": [quant, {"query": sp, "using": "sparse", "limit": p["sparse_limit"]}], "query": {"fusion": "rrf"}}
    return {"prefetch": [c, fusion], "query": q, "using": "dense", "limit": p["final_limit"]}


def trees(ix, tabs):
    print(f"\n3. the reference's tree, filter_stages='all': query_points' path (every masked leaf builds its own view) against "
          f"hybrid_search's (one view), alternated; view = hx_prof slot 5 per call")
    h = HD.QdrantHandler()
    col = HD._Collection(768, (64, 128, 256), 0, index=ix)
    col.ids = Rows(N, lambda r: f"p{r}")
    col.payloads = Rows(N, lambda r: {"page_number": r % 100})
    h._collections["u"] = col
    r = np.arange(N) % 100
    for B in (1024, 1):
        Q = eng.synth_queries_dense(768, 0, B, synth.SEED_QUERY).cpu().numpy()
        qip, qsi, qsv = synth.sparse_queries(synth.SEED_SPQUERY, 0, B, tabs)
        sps = [{"indices": qsi[qip[b]:qip[b + 1]], "values": qsv[qip[b]:qip[b + 1]]} for b in range(B)]
        for lt in (100, 50, 10):                             # 100: no filter at all, the two paths as they are without one
            flt = {"must": [{"key": "page_number", "range": {"lt": lt}}]} if lt < 100 else None
            if flt:
                col._masks[FL.filter_key(flt)] = (N, eng.pack_rows(r < lt))
            reqs = [dict(reference_tree(Q[b], sps[b]), **(dict(filters=flt, filter_stages="all") if flt else {}))
                    for b in range(B)]
            tree = lambda: h._query_points_sync("u", reqs)
            fixed = lambda: h._search_sync("u", Q, sps, P, flt, "tree", "all")
            a, b_ = tree(), fixed()
            same = [[(p.id, p.score) for p in x] for x in a] == [[(p.id, p.score) for p in x] for x in b_]
            for _ in range(WARM):
                tree(), fixed()
            tt, tf = [], []
            for _ in range(REPS):                            # alternated: one of each per round
                for fn, ts in ((tree, tt), (fixed, tf)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1))
            view = []
            for fn in (tree, fixed):
                ix.profile(True)
                view_total_ms(ix)
                for _ in range(5):
                    fn()
                view.append(view_total_ms(ix) / 5)
                ix.profile(False)
            mt, mf = float(np.median(tt)), float(np.median(tf))
            print(f"  B={B:4d} keep {lt:3d}%  tree {mt:9.3f} [{min(tt):.3f}-{max(tt):.3f}] view {view[0]:8.3f}   "
                  f"fixed {mf:9.3f} [{min(tf):.3f}-{max(tf):.3f}] view {view[1]:8.3f}   tree / fixed {mt / mf:.2f}   "
                  f"same answers {same}")


def main():
    tabs = synth.tables()
    ix = eng.HxIndex(768, (64, 128, 256))
    ix.reserve(N)
    ix.synth_fill(N, synth.SEED_CORPUS, synth.SEED_SPDOC, tabs)
    ix.finalize()
    rng = np.random.default_rng(0)
    masks = []
    for f in FRACTIONS:
        keep = np.ones(N, bool) if f == 1.0 else rng.random(N) < f
        masks.append((f, torch.from_numpy(eng.pack_rows(keep).view(np.int32)).cuda(), int(keep.sum())))
    print(f"node filters of the query trees, {N} rows x 768, ms per call (HIP events, median [min-max] of {REPS})")
    leaves(ix, tabs, masks)
    sys.stdout.flush()
    list_keep(ix, masks)
    sys.stdout.flush()
    trees(ix, tabs)
    ix.close()


if __name__ == "__main__":
    main()
