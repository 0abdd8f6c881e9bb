"""Side measurement: per-point deletes (hx_retain_rows) on a 10M x 768 synthetic index
(hx_synth_fill).  For 0.1 %, 10 % and 50 % random deletes and one contiguous 10 % block:
  - the wall time of hx_retain_rows (a host clock around the call: it returns behind a device synchronisation), the bytes
    it moved -- every stored copy of every row behind the first deleted one read once and written once, the moved
    postings read and written twice (spare buffer and back) -- and those bytes per second against the 8 TB/s HBM peak;
  - the first search afterwards (it rebuilds the inverted index) and the steady 1024-query H1 step;
  - the only other route to the same state: a NEW index built from the kept raw rows with add_device + finalize (raw
    rows on the device, their sparse vectors on the host as the ingest path takes them, 1M source rows per call), its
    wall time and its steady step, measured in the same run, the two indexes' steps alternating.
The lists of the two indexes are compared (they must be equal).  Not part of bench.py.
argv: rows (default 10M).  Output: one table on stdout (kept as profiles/delete_*.txt)."""
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
CH = 1_000_000
REPS, WARM = 15, 3
HBM_PEAK = 8.0e12
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


def alternate(f1, f2):
    """the steady steps of two indexes, alternating: median [min-max] of REPS each"""
    for _ in range(WARM):
        f1()
        f2()
    torch.cuda.synchronize()
    t1, t2 = [], []
    for _ in range(REPS):
        t1.append(step_ms(f1))
        t2.append(step_ms(f2))
    return [(float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in (t1, t2)]


def cases(n):
    rng = np.random.default_rng(0)
    out = [(f"{f * 100:g}% random", rng.random(n) >= f) for f in (0.001, 0.1, 0.5)]
    keep = np.ones(n, bool)
    keep[n // 2: n // 2 + n // 10] = False
    out.append(("10% contiguous block", keep))
    return out


def row_bytes():
    """bytes of every stored copy of one row (engine.hip: dim 768 is its own padding)"""
    return D * 4 + D * 2 + D + 4 + D + 4 + sum(m * 4 for m in MS) + MS[0] * 2


def main():
    tabs = synth.tables()
    hp = eng.make_params(P, mode=eng.HX_MODE_H1)
    Q = eng.synth_queries_dense(D, 0, B, synth.SEED_QUERY)
    tq = [torch.from_numpy(a).cuda() for a in synth.sparse_queries(synth.SEED_SPQUERY, 0, B, tabs)]
    t0 = time.perf_counter()
    docs = [CO.synth_sparse_docs(synth.SEED_SPDOC, r0, min(CH, N - r0), tabs) for r0 in range(0, N, CH)]
    print(f"per-point deletes, {N} rows x {D}; host CSR of the corpus generated in {time.perf_counter() - t0:.1f} s "
          f"(not part of any timing below)")
    print(f"steps: H1, B = {B}, ms from HIP events, median [min-max] of {REPS} after {WARM} warm-up steps, the deleted "
          f"and the rebuilt index alternating; walls: host clock around a call that ends in a device synchronise")
    for name, keep in cases(N):
        ix = eng.HxIndex(D, MS)
        ix.reserve(N)
        ix.synth_fill(N, synth.SEED_CORPUS, synth.SEED_SPDOC, tabs)
        ix.finalize()
        ix.hybrid_query(Q, *tq, hp)
        nnz0 = ix.stats()["nnz"]
        words = eng.pack_rows(keep)
        t_del, removed = wall(lambda: ix.retain(words))
        first = int(np.argmin(keep))
        nnz1 = ix.stats()["nnz"]
        lens = np.concatenate([np.diff(d[0]) for d in docs])
        nnz_front = int(lens[:first].sum())
        moved = (N - removed - first) * row_bytes() * 2 + (nnz1 - nnz_front) * 8 * 4
        t_first, _ = wall(lambda: ix.hybrid_query(Q, *tq, hp))
        # the same state from the kept raw rows
        parts = []
        for k, r0 in enumerate(range(0, N, CH)):
            kc = keep[r0:r0 + CH]
            ip, si, sv = docs[k]
            ln = np.diff(ip)
            take = np.repeat(kc, ln)
            nip = np.zeros(int(kc.sum()) + 1, np.int64)
            np.cumsum(ln[kc], out=nip[1:])
            raw = eng.synth_queries_dense(D, r0, len(kc), synth.SEED_CORPUS)
            parts.append((raw[torch.from_numpy(np.flatnonzero(kc)).cuda()].contiguous(), nip,
                          np.ascontiguousarray(si[take], np.int32), np.ascontiguousarray(sv[take], np.float32)))
            del raw

        def rebuild():
            nx = eng.HxIndex(D, MS)
            nx.reserve(N - removed)
            for k in range(len(parts)):
                raw, ip, si, sv = parts[k]
                if raw.shape[0]:
                    nx.add_device(raw, ip, si, sv)
                parts[k] = None                      # (the raw rows are dropped as they are consumed)
            nx.finalize()
            return nx
        t_new, nx = wall(rebuild)
        del parts
        k0, c0 = ix.hybrid_query(Q, *tq, hp)
        k1, c1 = nx.hybrid_query(Q, *tq, hp)
        equal = bool(torch.equal(k0, k1) and torch.equal(c0, c1))
        (sd, sn) = alternate(lambda: ix.hybrid_query(Q, *tq, hp), lambda: nx.hybrid_query(Q, *tq, hp))
        print(f"\n{name}: {removed} rows removed, {ix.count()} kept, first deleted row {first}, nnz {nnz0} -> {nnz1}")
        print(f"  hx_retain_rows            {t_del:10.1f} ms   moved {moved / 1e9:7.2f} GB = {moved / (t_del * 1e-3) / 1e12:5.2f} TB/s "
              f"= {moved / (t_del * 1e-3) / HBM_PEAK * 100:4.1f} % of the HBM peak")
        print(f"  first search afterwards   {t_first:10.1f} ms   (rebuilds the inverted index)")
        print(f"  rebuild from raw rows     {t_new:10.1f} ms   (add_device x {(N + CH - 1) // CH} + finalize)   "
              f"delete / rebuild = {t_del / t_new:.3f}, delete + first search / rebuild = {(t_del + t_first) / t_new:.3f}")
        print(f"  steady step after delete  {sd[0]:10.3f} [{sd[1]:.3f}-{sd[2]:.3f}]")
        print(f"  steady step, rebuilt      {sn[0]:10.3f} [{sn[1]:.3f}-{sn[2]:.3f}]   lists equal: {equal}")
        sys.stdout.flush()
        ix.close()
        nx.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
