"""Diagnostic: MMR search (hx_mmr / hx_hybrid_query_mmr_host) on a 10M x 768 synthetic corpus
(hx_synth_fill).  B = 1024 queries, 10 picks at diversity 0.5, over the reference tree (dense_limit 40: a pool of 50) and
H1 (dense_limit = sparse_limit = 50 and 100: pools of 100 and 200).  Per pool, ms per call, median [min-max] of 20 after
3 warm-up calls:
  k_mmr_select alone     HIP events around hx_mmr over the pool of the batch, already on the device, for each workgroup
                         size (HX_DEBUG_MMR_NT is read once per process: the script first starts itself once per size
                         with --kernel-only), with the bytes/s of the cost model (limit - 1) * n * row_bytes per query;
  k_rescore_list         HIP events around hx_rescore of the same pool: n row reads per query, the stream the model is
                         held against;
  MMR host call          hx_hybrid_query_mmr_host, wall clock (the call returns when its results are on the host);
  plain host call        hx_hybrid_query_host at final_limit = the pool, wall clock: what a caller who runs MMR in Python
                         has to ask for, before pulling pool x dim floats to the host.
The two host calls are timed in alternation, so a drift of the box hits both.  --plain-only times the plain host call
alone and needs no MMR entry: run from a checkout of the parent commit it gives the parent's figure on the same box.
Not part of bench.py.  argv: [rows (default 10M)] [--plain-only] [--kernel-only] [--label TEXT].  Output: one table on
stdout (kept as profiles/mmr_*.txt)."""
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rag_application_amd import engine as eng, synth  # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
PLAIN_ONLY = "--plain-only" in sys.argv
KERNEL_ONLY = "--kernel-only" in sys.argv
LABEL = sys.argv[sys.argv.index("--label") + 1] if "--label" in sys.argv else ""
if LABEL in ARGS:
    ARGS.remove(LABEL)
N = int(ARGS[0]) if ARGS else 10_000_000
B, LIMIT, DIVERSITY = 1024, 10, 0.5
REPS, WARM = 20, 3
BASE = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, quantized_limit=40,
            final_limit=10, hnsw_ef=128)
CASES = (("tree", dict(BASE, dense_limit=40, sparse_limit=50)), ("h1", dict(BASE, dense_limit=50, sparse_limit=50)),
         ("h1", dict(BASE, dense_limit=100, sparse_limit=100)))


def spread(ts):
    return f"{np.median(ts):9.3f} [{np.min(ts):.3f}-{np.max(ts):.3f}]"


def events(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def wall_alternating(fns):
    """every fn timed REPS times, one call of each per round"""
    for _ in range(WARM):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(REPS):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    forced = {}                                             # the forced workgroup sizes, each in a process of its own, one
    if not (PLAIN_ONLY or KERNEL_ONLY):                     # at a time and before this process holds an index
        for force in ("256", "1024"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), str(N), "--kernel-only"], check=True,
                                 capture_output=True, text=True, env=dict(os.environ, HX_DEBUG_MMR_NT=force)).stdout
            for ln in out.splitlines():
                if "|" in ln:
                    forced.setdefault(ln.split("|", 1)[0], []).append(ln.split("|", 1)[1])
    tabs = synth.tables()
    ix = eng.HxIndex(768, (64, 128, 256))
    ix.reserve(N)
    ix.synth_fill(N, synth.SEED_CORPUS, synth.SEED_SPDOC, tabs)
    ix.finalize()
    nt = os.environ.get("HX_DEBUG_MMR_NT", "default")
    if not KERNEL_ONLY:
        print(f"MMR search, {N} rows x 768, B = {B}, {LIMIT} picks, diversity {DIVERSITY}; ms per call, median [min-max] of "
              f"{REPS} after {WARM} warm-up calls; {torch.cuda.get_device_name(0)}; {LABEL}")
    Qd = eng.synth_queries_dense(768, 0, B, synth.SEED_QUERY)
    Q = Qd.cpu().numpy()
    qip, qsi, qsv = synth.sparse_queries(synth.SEED_SPQUERY, 0, B, tabs)
    tq = [torch.from_numpy(a).cuda() for a in (qip, qsi, qsv)]
    for mode, p in CASES:
        pool = p["dense_limit"] + (10 if mode == "tree" else p["sparse_limit"])
        hp = eng.make_params(dict(p, final_limit=pool), mode=eng.HX_MODE_TREE if mode == "tree" else eng.HX_MODE_H1)
        plain = lambda: ix.hybrid_query_host(Q, qip, qsi, qsv, hp)                                   # noqa: E731
        if not KERNEL_ONLY:
            print(f"\n{mode}, pool {pool}")
        if PLAIN_ONLY:
            print(f"  {'plain host call, final_limit = pool':44s} {spread(wall_alternating([plain])[0])}")
            continue
        keys, cnt = ix.hybrid_query(Qd, *tq, hp)
        if mode == "h1":                                    # relevance is the cosine: the pool as the MMR call sees it
            keys, cnt = ix.rescore(Qd, keys, cnt, pool)
        n_mean = float(cnt.float().mean())
        k_ms = events(lambda: ix.mmr(keys, cnt, LIMIT, DIVERSITY))
        gbs = B * (LIMIT - 1) * n_mean * 768 * 4 / (np.median(k_ms) * 1e-3) / 1e9
        line = (f"  {'k_mmr_select alone, ' + nt + ' threads (HIP events)':44s} {spread(k_ms)}   "
                f"{gbs:7.1f} GB/s of (limit - 1) * n * row_bytes, n = {n_mean:.1f}")
        if KERNEL_ONLY:
            print(f"{mode} {pool}|{line}")
            continue
        print(line)
        for ln in forced.get(f"{mode} {pool}", []):
            print(ln)
        r_ms = events(lambda: ix.rescore(Qd, keys, cnt, pool))
        rgbs = B * n_mean * 768 * 4 / (np.median(r_ms) * 1e-3) / 1e9
        print(f"  {'hx_rescore of the pool (HIP events)':44s} {spread(r_ms)}   {rgbs:7.1f} GB/s of n * row_bytes (prep, "
              f"k_rescore_list and the sort)")
        mmr = lambda: ix.hybrid_query_mmr_host(Q, qip, qsi, qsv, hp, LIMIT, DIVERSITY)               # noqa: E731
        t_plain, t_mmr = wall_alternating([plain, mmr])
        diff = float(np.median(t_mmr) - np.median(t_plain))
        print(f"  {'MMR host call':44s} {spread(t_mmr)}")
        print(f"  {'plain host call, final_limit = pool':44s} {spread(t_plain)}")
        print(f"  MMR - plain (medians) {diff:+.3f} ms")
        _, _, _, counts = ix.hybrid_query_mmr_host(Q, qip, qsi, qsv, hp, LIMIT, DIVERSITY)
        print(f"  picks per query: mean {counts.mean():.2f} of {LIMIT}")
    ix.close()


if __name__ == "__main__":
    main()
