"""Diagnostic: grouped hybrid search (hx_group / hx_hybrid_query_groups_host) on a 10M x 768
synthetic corpus (hx_synth_fill) whose rows carry 10^4 distinct `document_id` codes in runs, as a collection ingested
file by file does.  B = 1024 queries, the best 10 documents with at most 3 chunks each, the reference tree
(dense_limit 40: a pool of 50) and H1 (dense_limit = sparse_limit = 100: a pool of 200).  Per mode, ms per call, median
[min-max] of 20 after 3 warm-up calls:
  k_group_select alone   HIP events around hx_group over the pool of the batch, already on the device;
  grouped host call      hx_hybrid_query_groups_host, wall clock (the call returns when its results are on the host);
  plain host call        hx_hybrid_query_host at final_limit = the pool, wall clock: what a caller who groups in Python
                         has to ask for.
The two host calls are timed in alternation, so a drift of the box hits both.  --plain-only times the plain host call
alone and needs no grouped entry: run from a checkout of the parent commit it gives the parent's figure on the same box.
Not part of bench.py.  argv: [rows (default 10M)] [--plain-only] [--label TEXT].  Output: one table on stdout (kept as
profiles/groups_*.txt)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rag_application_amd import engine as eng, synth  # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
PLAIN_ONLY = "--plain-only" in sys.argv
LABEL = sys.argv[sys.argv.index("--label") + 1] if "--label" in sys.argv else ""
if LABEL in ARGS:
    ARGS.remove(LABEL)
N = int(ARGS[0]) if ARGS else 10_000_000
B, G, S, DOCS = 1024, 10, 3, 10_000
REPS, WARM = 20, 3
TREE = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, dense_limit=40,
            quantized_limit=40, sparse_limit=50, final_limit=30, hnsw_ef=128)
H1 = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, dense_limit=100,
          quantized_limit=40, sparse_limit=100, final_limit=10, hnsw_ef=128)


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
    tabs = synth.tables()
    ix = eng.HxIndex(768, (64, 128, 256))
    ix.reserve(N)
    ix.synth_fill(N, synth.SEED_CORPUS, synth.SEED_SPDOC, tabs)
    ix.finalize()
    col = None
    if not PLAIN_ONLY:
        col = ix.payload_create(eng.PAY_U32)
        ix.payload_append(col, (np.arange(N, dtype=np.int64) // max(N // DOCS, 1)).astype(np.uint32))
    print(f"grouped search, {N} rows x 768, {DOCS} documents in runs, B = {B}, {G} groups of {S}; ms per call, median "
          f"[min-max] of {REPS} after {WARM} warm-up calls; {torch.cuda.get_device_name(0)}; {LABEL}")
    Qd = eng.synth_queries_dense(768, 0, B, synth.SEED_QUERY)
    Q = Qd.cpu().numpy()
    qip, qsi, qsv = synth.sparse_queries(synth.SEED_SPQUERY, 0, B, tabs)
    tq = [torch.from_numpy(a).cuda() for a in (qip, qsi, qsv)]
    for mode, p in (("tree", TREE), ("h1", H1)):
        pool = p["dense_limit"] + (10 if mode == "tree" else p["sparse_limit"])
        hp = eng.make_params(dict(p, final_limit=pool), mode=eng.HX_MODE_TREE if mode == "tree" else eng.HX_MODE_H1)
        plain = lambda: ix.hybrid_query_host(Q, qip, qsi, qsv, hp)                                   # noqa: E731
        print(f"\n{mode}, pool {pool}")
        if PLAIN_ONLY:
            print(f"  {'plain host call, final_limit = pool':38s} {spread(wall_alternating([plain])[0])}")
            continue
        keys, cnt = ix.hybrid_query(Qd, *tq, hp)
        k_ms = events(lambda: ix.group(col, keys, cnt, G, S))
        grouped = lambda: ix.hybrid_query_groups_host(Q, qip, qsi, qsv, hp, col, G, S)               # noqa: E731
        t_plain, t_grouped = wall_alternating([plain, grouped])
        diff = float(np.median(t_grouped) - np.median(t_plain))
        print(f"  {'k_group_select alone (HIP events)':38s} {spread(k_ms)}")
        print(f"  {'grouped host call':38s} {spread(t_grouped)}")
        print(f"  {'plain host call, final_limit = pool':38s} {spread(t_plain)}")
        print(f"  grouped - plain (medians) {diff:+.3f} ms; the kernel is {np.median(k_ms):.3f} ms of the grouped call "
              f"({100 * np.median(k_ms) / np.median(t_grouped):.2f} %)")
        _, _, _, counts = ix.hybrid_query_groups_host(Q, qip, qsi, qsv, hp, col, G, S)
        print(f"  groups opened per query: mean {counts.mean():.2f} of {G}")
    ix.close()


if __name__ == "__main__":
    main()
