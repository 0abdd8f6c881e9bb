"""Diagnostic: the asymmetric binary stage (hx_search_bin_asym) on a 10M x 768 synthetic corpus
(hx_synth_fill, dense rows only).  ms per call, median [min-max] of REPS after WARM warm-up calls, HIP events around the
whole call (the span holds every launch of the stage: the query kernel, one scan + one compaction + one threshold kernel
per chunk, and the stage's one host round trip).  One part per run, so that each runs under a time limit of its own:
  --part kernel   hx_search_bin_asym at 4 and 8 query bits, limit 1000, B = 1 / 2 / 8 / 32; beside them hx_search_bin and
                  hx_search_i8 at the same B and limit (unchanged code: the parent's numbers), same process;
  --part condition  hx_search_bin_asym at 8 bits against hx_search_i8, B = 1, limit 1000, alternating in one process: the
                  stage is the better choice there when the difference of the medians exceeds the min-max spread of either;
  --part tree     B = 1 and 8: leaf(1000) -> rescore(10) for the three encodings, alternating with search_dense(10);
  --part recall   recall@10 of leaf(10 * oversampling) -> rescore(10) against the exact dense list at oversampling
                  1 / 2 / 4 / 8 / 100 for the three encodings, the same 64 queries;
  --trace-b B1,B2 nothing but REPS + WARM hx_search_bin_asym calls at 8 bits (--bits 4: at 4) and limit 1000 for each listed
                  B, for a kernel trace of its own: the kernels' total time over the calls is the per-call share.
Not part of bench.py.  argv: [rows (default 10M)] [--part NAME] [--trace-b LIST] [--bits 4|8] [--label TEXT].  Output: a
table on stdout (kept as profiles/binary_asym_10m.txt)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rag_application_amd import engine as eng, synth  # noqa: E402


def opt(name, default=""):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


LABEL, TRACE_B, PART, BITS = opt("--label"), opt("--trace-b"), opt("--part", "kernel"), int(opt("--bits", "8"))
_skip = set()
for _i, _a in enumerate(sys.argv):
    if _a.startswith("--"):
        _skip.update((_i, _i + 1))
ARGS = [a for i, a in enumerate(sys.argv) if i and i not in _skip]
N = int(ARGS[0]) if ARGS else 10_000_000
DIM, LIMIT, REPS, WARM = 768, 1000, 20, 3
HBM_PEAK = 8.0e12                # bytes / s (MI355X)
LEAVES = ("binary", "scalar4bits", "scalar8bits")


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


def corpus():
    ix = eng.HxIndex(DIM, ())
    ix.reserve(N)
    ix.synth_fill(N, synth.SEED_CORPUS)
    ix.binary_enable()
    return ix


def leaf(ix, enc, Q, limit):
    if enc == "binary":
        return ix.search_bin(Q, limit)
    return ix.search_bin_asym(Q, limit, 4 if enc == "scalar4bits" else 8)


def head(what):
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    print(f"asymmetric binary stage, {what}; {N} rows x {DIM}; ms per call, median [min-max] of {REPS} after {WARM} warm-up "
          f"calls; one {arch} device{'; ' + LABEL if LABEL else ''}", flush=True)


def part_kernel(ix):
    bits_bytes = N * (DIM // 8)
    head(f"limit {LIMIT}")
    print(f"  hx_search_bin_asym 8 bits (fraction of HBM peak on {bits_bytes / 1e9:.2f} GB of row bits) | 4 bits (fraction) | "
          "hx_search_bin | hx_search_i8 | asym8 / i8")
    for B in (1, 2, 8, 32):
        Q = eng.synth_queries_dense(DIM, 0, B, synth.SEED_QUERY)
        t8 = events(lambda: ix.search_bin_asym(Q, LIMIT, 8))
        t4 = events(lambda: ix.search_bin_asym(Q, LIMIT, 4))
        tb = events(lambda: ix.search_bin(Q, LIMIT))
        ti = events(lambda: ix.search_i8(Q, LIMIT))
        f8, f4 = (bits_bytes / (np.median(t) * 1e-3) / HBM_PEAK for t in (t8, t4))
        print(f"  B = {B:3d}   {spread(t8)} ({f8:.3f}) | {spread(t4)} ({f4:.3f}) | {spread(tb)} | {spread(ti)} | "
              f"{np.median(t8) / np.median(ti):.3f}", flush=True)


def part_condition(ix):
    head(f"the condition: 8 bits against hx_search_i8, B = 1, limit {LIMIT}, alternating")
    Q = eng.synth_queries_dense(DIM, 0, 1, synth.SEED_QUERY)
    ta, ti = alternating(lambda: ix.search_bin_asym(Q, LIMIT, 8), lambda: ix.search_i8(Q, LIMIT))
    diff = np.median(ti) - np.median(ta)
    sa, si = np.max(ta) - np.min(ta), np.max(ti) - np.min(ti)
    print(f"  hx_search_bin_asym 8 bits {spread(ta)} | hx_search_i8 {spread(ti)}")
    print(f"  i8 - asym8 = {diff:.3f} ms at the medians; min-max spread {sa:.3f} (asym8) and {si:.3f} (i8): the condition "
          f"{'HOLDS' if diff > max(sa, si) else 'DOES NOT HOLD'}")


def part_tree(ix):
    head("tree: leaf(1000) -> rescore(10) against search_dense(10) alone, alternating")
    for B in (1, 8):
        Q = eng.synth_queries_dense(DIM, 0, B, synth.SEED_QUERY)
        for enc in LEAVES:
            def tree():
                k, c = leaf(ix, enc, Q, 1000)
                return ix.rescore(Q, k, c, 10)
            tt, td = alternating(tree, lambda: ix.search_dense(Q, 10))
            print(f"  B = {B:3d}  {enc:12s} tree {spread(tt)} | dense {spread(td)} | tree / dense "
                  f"{np.median(tt) / np.median(td):.3f}", flush=True)


def part_recall(ix):
    head("recall@10 of leaf(10 * oversampling) -> rescore(10) against search_dense(10), 64 queries")
    Q = eng.synth_queries_dense(DIM, 0, 64, synth.SEED_QUERY)
    exact = ids_of(*ix.search_dense(Q, 10))
    print("  oversampling | " + " | ".join(f"{e:>11s}" for e in LEAVES))
    for over in (1, 2, 4, 8, 100):
        row = []
        for enc in LEAVES:
            k, c = leaf(ix, enc, Q, min(10 * over, 2048))
            got = ids_of(*ix.rescore(Q, k, c, 10))
            row.append(np.mean([len(g & e) / 10 for g, e in zip(got, exact)]))
        print(f"  {over:12d} | " + " | ".join(f"{r:11.3f}" for r in row), flush=True)


def trace_only(ix):
    for B in (int(b) for b in TRACE_B.split(",")):
        Q = eng.synth_queries_dense(DIM, 0, B, synth.SEED_QUERY)
        ts = events(lambda: ix.search_bin_asym(Q, LIMIT, BITS))
        print(f"B = {B}: {WARM + REPS} hx_search_bin_asym calls, {BITS} bits, limit {LIMIT}; under the tracer {spread(ts)} "
              "ms per call", flush=True)


def main():
    parts = {"kernel": part_kernel, "condition": part_condition, "tree": part_tree, "recall": part_recall}
    if not TRACE_B and PART not in parts:
        raise SystemExit(f"--part must be one of {tuple(parts)}, got {PART!r}")
    ix = corpus()
    try:
        trace_only(ix) if TRACE_B else parts[PART](ix)
    finally:
        ix.close()


if __name__ == "__main__":
    main()
