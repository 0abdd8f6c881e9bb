"""Side measurement: upsert by an existing id (hx_replace_rows) on a 10M x 768 synthetic index
(hx_synth_fill).  For a random 0.01 %, 1 % and 10 % of the rows, replaced by new dense and sparse vectors:
  - the steady 1024-query H1 step of the fresh index, before anything is replaced;
  - the wall time of hx_replace_rows (a host clock around the call: it starts and ends with a device synchronisation;
    the raw rows and the sparse batch come from host memory, as the handler passes them);
  - the first search afterwards (it rebuilds the inverted index) and the steady step;
  - the only other route to the same vectors, in the same run on a second index: hx_retain_rows of those rows plus
    hx_add_rows of the new ones (they land at the end of the collection), its first search and its steady step, the two
    indexes' steps alternating.
Expected, not claimed: the in-place route is the shorter one, and the steady step afterwards lies within the run-to-run
spread of the steady step on the fresh index.  Not part of bench.py.
argv: rows (default 10M).  Output: one table on stdout (kept as profiles/replace_10m.txt)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import c_oracle as CO  # noqa: E402
from rag_application_amd import engine as eng, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
D, MS, B = 768, (64, 128, 256), 1024
CH = 250_000
REPS, WARM = 15, 3
FRACTIONS = (0.0001, 0.01, 0.1)
P = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, dense_limit=100,
         quantized_limit=40, sparse_limit=100, final_limit=10, hnsw_ef=128)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def step_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def steady(*fns):
    """the steady steps of one or two indexes, alternating: (median, min, max) of REPS each"""
    for _ in range(WARM):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(REPS):
        for t, f in zip(ts, fns):
            t.append(step_ms(f))
    return [(float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in ts]


def fmt(s):
    return f"{s[0]:10.3f} [{s[1]:.3f}-{s[2]:.3f}]"


def new_vectors(m, tabs):
    """m new rows on the host: dense rows N .. N + m of the synthetic corpus (rows the index does not hold), their sparse
    vectors likewise"""
    dense = np.empty((m, D), np.float32)
    for r0 in range(0, m, CH):
        k = min(CH, m - r0)
        dense[r0:r0 + k] = eng.synth_queries_dense(D, N + r0, k, synth.SEED_CORPUS).cpu().numpy()
    ip, si, sv = CO.synth_sparse_docs(synth.SEED_SPDOC, N, m, tabs)
    return dense, np.ascontiguousarray(ip, np.int64), np.ascontiguousarray(si, np.int32), np.ascontiguousarray(sv, np.float32)


def fresh(tabs):
    ix = eng.HxIndex(D, MS)
    ix.reserve(N + N // 8)
    ix.synth_fill(N, synth.SEED_CORPUS, synth.SEED_SPDOC, tabs)
    ix.finalize()
    return ix


def main():
    tabs = synth.tables()
    hp = eng.make_params(P, mode=eng.HX_MODE_H1)
    Q = eng.synth_queries_dense(D, 0, B, synth.SEED_QUERY)
    tq = [torch.from_numpy(a).cuda() for a in synth.sparse_queries(synth.SEED_SPQUERY, 0, B, tabs)]
    print(f"upsert by an existing id, {N} rows x {D}")
    print(f"steps: H1, B = {B}, ms from HIP events, median [min-max] of {REPS} after {WARM} warm-up steps (two indexes: "
          f"alternating); walls: host clock around a call that ends in a device synchronise")
    rng = np.random.default_rng(0)
    for frac in FRACTIONS:
        m = max(int(N * frac), 1)
        rows = rng.permutation(N)[:m].astype(np.int64)
        dense, ip, si, sv = new_vectors(m, tabs)
        ix = fresh(tabs)
        ix.hybrid_query(Q, *tq, hp)
        (s_fresh,) = steady(lambda: ix.hybrid_query(Q, *tq, hp))
        nnz0 = ix.stats()["nnz"]
        t_rep, _ = wall(lambda: ix.replace(rows, dense, ip, si, sv))
        t_first, _ = wall(lambda: ix.hybrid_query(Q, *tq, hp))
        # the other route on a second index: delete those rows, add the new vectors at the end
        jx = fresh(tabs)
        jx.hybrid_query(Q, *tq, hp)
        keep = np.ones(N, bool)
        keep[rows] = False
        words = eng.pack_rows(keep)
        t_del, _ = wall(lambda: jx.retain(words))
        t_add, _ = wall(lambda: jx.add(dense, ip, si, sv))
        t_first2, _ = wall(lambda: jx.hybrid_query(Q, *tq, hp))
        s_rep, s_da = steady(lambda: ix.hybrid_query(Q, *tq, hp), lambda: jx.hybrid_query(Q, *tq, hp))
        assert ix.count() == jx.count() == N and ix.stats()["nnz"] == jx.stats()["nnz"], "the two routes differ in size"
        print(f"\n{frac * 100:g} % of the rows: {m} rows replaced, first replaced row {int(rows.min())}, "
              f"nnz {nnz0} -> {ix.stats()['nnz']}")
        print(f"  steady step, fresh index        {fmt(s_fresh)}")
        print(f"  hx_replace_rows                 {t_rep:10.1f} ms")
        print(f"  first search afterwards         {t_first:10.1f} ms   (rebuilds the inverted index)")
        print(f"  steady step after the replace   {fmt(s_rep)}")
        print(f"  hx_retain_rows + hx_add_rows    {t_del + t_add:10.1f} ms   ({t_del:.1f} + {t_add:.1f})   "
              f"replace / (delete + add) = {t_rep / (t_del + t_add):.3f}")
        print(f"  first search afterwards         {t_first2:10.1f} ms")
        print(f"  steady step after delete + add  {fmt(s_da)}")
        sys.stdout.flush()
        ix.close()
        jx.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
