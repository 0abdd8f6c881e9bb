"""Diagnostic: discovery and context search (hx_discover) on a 10M x 768 synthetic corpus
(hx_synth_fill, dense rows only), beside hx_recommend(best_score) with as many examples in the same session.  ms per call,
median [min-max] of 20 after 3 warm-up calls, HIP events around the call: the span holds the scan's launches (one per chunk
and per group of requests whose examples share the LDS), the compactions and -- for discover -- the threshold kernels
between them.  Cases: discovery with a target and 1 / 3 / 15 pairs (3 / 7 / 31 examples), context search with 1 / 16 pairs
(2 / 32 examples); R = 1 and 16 requests; limit 10; stored examples.  The 1-pair context search is the tied case: about
half the rows score exactly +0; hx_discover_redone is printed behind it.
Not part of bench.py.  argv: [rows (default 10M)] [--label TEXT].  Output: one table on stdout (kept as
profiles/discover_*.txt)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rag_application_amd import engine as eng, synth  # noqa: E402

LABEL = sys.argv[sys.argv.index("--label") + 1] if "--label" in sys.argv else ""
ARGS = [a for a in sys.argv[1:] if not a.startswith("--") and a != LABEL]
N = int(ARGS[0]) if ARGS else 10_000_000
DIM, LIMIT, REPS, WARM = 768, 10, 20, 3
BEST_SCORE = 1


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


def main():
    ix = eng.HxIndex(DIM, ())
    ix.reserve(N)
    ix.synth_fill(N, synth.SEED_CORPUS)
    print(f"discovery and context search, {N} rows x {DIM}, limit {LIMIT}; ms per call, median [min-max] of {REPS} after "
          f"{WARM} warm-up calls; {torch.cuda.get_device_name(0)}; {LABEL}")
    print("each line: hx_discover | hx_recommend(best_score) with as many examples, same session | discover / recommend")
    rng = np.random.default_rng(29)
    for R in (1, 16):
        for name, with_target, pairs in (("discovery, target + 1 pair ", True, 1), ("discovery, target + 3 pairs", True, 3),
                                         ("discovery, target + 15 pairs", True, 15), ("context, 1 pair (tied)     ", False, 1),
                                         ("context, 16 pairs          ", False, 16)):
            E = int(with_target) + 2 * pairs
            rows = [[int(r) for r in rng.choice(N, E, replace=False)] for _ in range(R)]
            dreq = [(ex[0] if with_target else None,
                     [(ex[with_target + 2 * k], ex[with_target + 2 * k + 1]) for k in range(pairs)]) for ex in rows]
            rreq = [[(r, 1 if k % 3 else -1) for k, r in enumerate(ex)] for ex in rows]
            keys, cnt = ix.discover(dreq, LIMIT)
            before = ix.discover_redone()
            d = events(lambda: ix.discover(dreq, LIMIT, keys=keys, counts=cnt))
            redone = ix.discover_redone() - before
            r = events(lambda: ix.recommend(rreq, BEST_SCORE, LIMIT, keys=keys, counts=cnt))
            zeros = ""
            if not with_target:
                sc = ix.discover_host(dreq[:1], 1024)[0][0]
                zeros = f"; {int((sc == 0).sum())} of the best 1024 scores of request 0 are 0"
            print(f"  R = {R:2d}, {name} ({E:2d} examples)   {spread(d)} | {spread(r)} | {np.median(d) / np.median(r):.3f}"
                  f"   requests redone in {WARM + REPS} discover calls: {redone}{zeros}")
    ix.close()


if __name__ == "__main__":
    main()
