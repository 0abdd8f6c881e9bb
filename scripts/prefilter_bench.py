"""Diagnostic: the pre-filtered hybrid query (hx_hybrid_query_dev_masked) on a 10M x 768 synthetic
corpus (hx_synth_fill).  H1 at B = 1024 and B = 1, the reference tree at B = 1024; keep-fractions 100 % (through the
masked entry), 50, 10, 1 and 0.1 % as random masks and 10 % as contiguous 4096-row blocks.  ms per call from HIP events
(median of 20 after 3 warm-up calls), with the list of kept rows and the gathered copies of the scanned matrices
(hx_prof slot 5) split out; the unmasked call of the same batch for comparison.  Not part of bench.py.
argv: rows (default 10M).  Output: one table on stdout (kept as profiles/prefilter_*.txt)."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rag_application_amd import _lib, engine as eng, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
REPS, WARM = 20, 3
P = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, dense_limit=100,
         quantized_limit=40, sparse_limit=100, final_limit=10, hnsw_ef=128)


def view_ms(ix):
    p = _lib.HxProf()
    _lib.check(_lib.lib().hx_profile_read(ix._h, C.byref(p)))
    return p.ms[5] / max(p.launches[5], 1), p.launches[5]


def timed(fn):
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
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def masks(n):
    rng = np.random.default_rng(0)
    out = [("100% (masked entry)", np.ones(n, bool))]
    for f in (0.5, 0.1, 0.01, 0.001):
        out.append((f"{f * 100:g}% random", rng.random(n) < f))
    keep = np.zeros(n, bool)
    blocks = rng.choice(n // 4096, max(1, n // 4096 // 10), replace=False)
    for b in blocks:
        keep[b * 4096:(b + 1) * 4096] = True
    out.append(("10% clustered (4096-row blocks)", keep))
    return out


def main():
    tabs = synth.tables()
    ix = eng.HxIndex(768, (64, 128, 256))
    ix.reserve(N)
    ix.synth_fill(N, synth.SEED_CORPUS, synth.SEED_SPDOC, tabs)
    ix.finalize()
    ms = [(name, torch.from_numpy(eng.pack_rows(k).view(np.int32)).cuda(), int(k.sum())) for name, k in masks(N)]
    print(f"pre-filtered query, {N} rows x 768, ms per call (HIP events, median [min-max] of {REPS}); "
          f"view = the list of kept rows + the gathers of the scanned copies (hx_prof slot 5, mean per call)")
    for mode, B in (("h1", 1024), ("h1", 1), ("tree", 1024)):
        hp = eng.make_params(P, mode=eng.HX_MODE_H1 if mode == "h1" else eng.HX_MODE_TREE)
        Q = eng.synth_queries_dense(768, 0, B, synth.SEED_QUERY)
        tq = [torch.from_numpy(a).cuda() for a in synth.sparse_queries(synth.SEED_SPQUERY, 0, B, tabs)]
        med, lo, hi = timed(lambda: ix.hybrid_query(Q, *tq, hp))
        print(f"\n{mode} B={B}\n  {'unmasked':34s} {med:9.3f} [{lo:.3f}-{hi:.3f}]")
        for name, words, kept in ms:
            ix.profile(True)
            view_ms(ix)
            med, lo, hi = timed(lambda: ix.hybrid_query(Q, *tq, hp, mask=words))
            v, nv = view_ms(ix)
            ix.profile(False)
            print(f"  {name:34s} {med:9.3f} [{lo:.3f}-{hi:.3f}]   kept {kept:9d}   view {v:8.3f}" +
                  ("" if nv else "   (no view: short-circuit)"))
    ix.close()


if __name__ == "__main__":
    main()
