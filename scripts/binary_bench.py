"""Diagnostic: binary quantization (hx_binary_enable / hx_search_bin) on a 10M x 768 synthetic corpus
(hx_synth_fill, dense rows only).  ms per call, median [min-max] of REPS after WARM warm-up calls, HIP events around the
call (the span holds every launch of the stage: query bits, one scan + one compaction + one threshold kernel per chunk,
and the stage's one host round trip).
  kernel     hx_search_bin at limit 1000, B = 1 / 8 / 32 / 128 / 1024, with the fraction of HBM peak its rows (96 B each)
             stand for; beside it hx_search_dense (prefix 0) and hx_search_i8 at the same B and limit, same process;
  tree       B = 1 and 8: search_bin(1000) -> rescore(10), the tree of search_binary, against search_dense(10) alone,
             alternating;
  ties       the scan over 10M identical rows against the 10M distinct ones, B = 8;
  recall     recall@10 of the two-level tree against the exact dense list at oversampling 1 / 2 / 4 / 8, 64 queries;
  ingest     hx_binary_enable over the 10M rows; a 131072-row add_device batch with and without the copy.
--trace-b B1,B2: nothing but REPS + WARM hx_search_bin calls at limit 1000 for each listed B (B = 1 runs k_bin_scan<1>
alone, B = 8 k_bin_scan<8>), for a kernel trace of its own: the kernels' total time over the calls is the per-call share.
Not part of bench.py.  argv: [rows (default 10M)] [--label TEXT] [--trace-b LIST].  Output: one table on stdout (kept as
profiles/binary_10m.txt)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rag_application_amd import engine as eng, synth  # noqa: E402

LABEL = sys.argv[sys.argv.index("--label") + 1] if "--label" in sys.argv else ""
TRACE_B = sys.argv[sys.argv.index("--trace-b") + 1] if "--trace-b" in sys.argv else ""
ARGS = [a for a in sys.argv[1:] if not a.startswith("--") and a not in (LABEL, TRACE_B)]
N = int(ARGS[0]) if ARGS else 10_000_000
DIM, LIMIT, REPS, WARM = 768, 1000, 20, 3
HBM_PEAK = 8.0e12                # bytes / s (MI355X)
BATCH = 131072
ENABLE_REPS = 5


def spread(ts):
    return f"{np.median(ts):9.3f} [{np.min(ts):.3f}-{np.max(ts):.3f}]"


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def events(fn, reps=REPS):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    return [one(fn) for _ in range(reps)]


def alternating(f, g, reps=REPS):
    for _ in range(WARM):
        f()
        g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(reps):
        tf.append(one(f))
        tg.append(one(g))
    return tf, tg


def ids_of(keys, cnt):
    k = keys.cpu().numpy().view(np.uint64)
    c = cnt.cpu().numpy()
    return [set((0xFFFFFFFF - (k[b, :c[b]] & np.uint64(0xFFFFFFFF))).tolist()) for b in range(k.shape[0])]


def trace_only():
    ix = eng.HxIndex(DIM, ())
    ix.reserve(N)
    ix.synth_fill(N, synth.SEED_CORPUS)
    ix.binary_enable()
    for B in (int(b) for b in TRACE_B.split(",")):
        Q = eng.synth_queries_dense(DIM, 0, B, synth.SEED_QUERY)
        ts = events(lambda: ix.search_bin(Q, LIMIT))
        print(f"B = {B}: {WARM + REPS} hx_search_bin calls, limit {LIMIT}; under the tracer {spread(ts)} ms per call")
    ix.close()


def main():
    if TRACE_B:
        return trace_only()
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    print(f"binary quantization, {N} rows x {DIM}; ms per call, median [min-max] of {REPS} after {WARM} warm-up calls; "
          f"one {arch} device{'; ' + LABEL if LABEL else ''}")
    # hx_binary_enable runs once per index: ENABLE_REPS fresh indexes, one call each (the first includes the kernel's load)
    ts = []
    for _ in range(ENABLE_REPS):
        ix = eng.HxIndex(DIM, ())
        ix.reserve(N)
        ix.synth_fill(N, synth.SEED_CORPUS)
        torch.cuda.synchronize()
        ts.append(one(ix.binary_enable))
        if len(ts) < ENABLE_REPS:
            ix.close()
    read = N * DIM * 4.0
    print(f"ingest: hx_binary_enable over {N} rows ({read / 1e9:.1f} GB read), one call on each of {ENABLE_REPS} fresh "
          f"indexes: {spread(ts)} ms, {read / (np.median(ts) * 1e-3) / HBM_PEAK:.3f} of HBM peak at the median")
    bits_bytes = N * (DIM // 8)
    print(f"kernel: limit {LIMIT}; hx_search_bin (fraction of HBM peak on {bits_bytes / 1e9:.2f} GB of row bits) | "
          "hx_search_dense prefix 0 | hx_search_i8 | bin / i8")
    for B in (1, 8, 32, 128, 1024):
        Q = eng.synth_queries_dense(DIM, 0, B, synth.SEED_QUERY)
        tb = events(lambda: ix.search_bin(Q, LIMIT))
        td = events(lambda: ix.search_dense(Q, LIMIT))
        t8 = events(lambda: ix.search_i8(Q, LIMIT))
        frac = bits_bytes / (np.median(tb) * 1e-3) / HBM_PEAK
        print(f"  B = {B:4d}   {spread(tb)} ({frac:.3f}) | {spread(td)} | {spread(t8)} | {np.median(tb) / np.median(t8):.3f}")
    print("tree: search_bin(1000) -> rescore(10) against search_dense(10) alone, alternating")
    for B in (1, 8):
        Q = eng.synth_queries_dense(DIM, 0, B, synth.SEED_QUERY)

        def tree():
            k, c = ix.search_bin(Q, 1000)
            return ix.rescore(Q, k, c, 10)
        tt, td = alternating(tree, lambda: ix.search_dense(Q, 10))
        print(f"  B = {B:4d}   tree {spread(tt)} | dense {spread(td)} | tree / dense {np.median(tt) / np.median(td):.3f}")
    print("recall@10 of search_bin(10 * oversampling) -> rescore(10) against search_dense(10), 64 queries")
    Q = eng.synth_queries_dense(DIM, 0, 64, synth.SEED_QUERY)
    exact = ids_of(*ix.search_dense(Q, 10))
    for over in (1, 2, 4, 8, 100):
        k, c = ix.search_bin(Q, min(10 * over, 2048))
        got = ids_of(*ix.rescore(Q, k, c, 10))
        print(f"  oversampling {over:3d}: {np.mean([len(g & e) / 10 for g, e in zip(got, exact)]):.3f}")
    Q8 = eng.synth_queries_dense(DIM, 0, 8, synth.SEED_QUERY)
    distinct = events(lambda: ix.search_bin(Q8, LIMIT))
    ix.close()
    # ties: the same number of rows, all identical
    tied = eng.HxIndex(DIM, ())
    tied.reserve(N)
    tied.binary_enable()
    row = eng.synth_queries_dense(DIM, 7, 1, synth.SEED_QUERY)
    block = row.repeat(BATCH, 1).contiguous()
    for r0 in range(0, N, BATCH):
        tied.add_device(block[:min(BATCH, N - r0)])
    tt = events(lambda: tied.search_bin(Q8, LIMIT))
    print(f"ties, B = 8, limit {LIMIT}: {N} identical rows {spread(tt)} | distinct rows {spread(distinct)}")
    tied.close()
    # ingest: one batch with and without the copy
    raw = torch.randn((BATCH, DIM), device="cuda", dtype=torch.float32)
    res = {}
    for on in (False, True):
        small = eng.HxIndex(DIM, ())
        small.reserve(BATCH * (REPS + WARM + 1))
        if on:
            small.binary_enable()
        res[on] = events(lambda: small.add_device(raw))
        small.close()
    print(f"ingest: one add_device batch of {BATCH} rows: without the copy {spread(res[False])} | with it {spread(res[True])}")


if __name__ == "__main__":
    main()
