"""Diagnostic: distance matrix search (hx_search_matrix) on synthetic 768-wide corpora
(hx_synth_fill, dense rows only).  ms per call, median [min-max] of 20 after 3 warm-up calls, HIP events around the call:
  1  independence of the collection   hx_search_matrix at S = 64 / 1024 / 4096, limit 3 / 64, over a small index (100k
                                      rows) and over the large one (10M rows): the same sample sizes, the same calls;
  2  per kernel                       the same calls on an index created under HX_DEBUG_MATRIX_SCAN_ONLY=1 (the call stops
                                      behind k_matrix_scan): the scan alone, the selection = the difference; the scan's
                                      rates by the cost model S * S * dim multiply-adds (one product and one sum each) and
                                      S * S * dim_pad * 4 * (1 / TI + 1 / TJ) bytes of rows read by the workgroups;
  3  the route that exists today      hx_recommend BEST_SCORE with one stored positive per request under the packed mask
                                      of the sample, 16 requests per call, S / 16 calls, on the large index: the same
                                      lists (checked here for the first requests), every call a scan of the collection.
Not part of bench.py.  argv: [rows of the large index (default 10M)] [--label TEXT].  Output: one table on stdout (kept as
profiles/matrix_*.txt)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rag_application_amd import engine as eng, synth  # noqa: E402
from rag_application_amd.filters import pack_rows  # noqa: E402

LABEL = sys.argv[sys.argv.index("--label") + 1] if "--label" in sys.argv else ""
ARGS = [a for a in sys.argv[1:] if not a.startswith("--") and a != LABEL]
N_BIG = int(ARGS[0]) if ARGS else 10_000_000
N_SMALL = min(100_000, N_BIG)
DIM, REPS, WARM = 768, 20, 3
SIZES, LIMITS = (64, 1024, 4096), (3, 64)
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


def index(n, scan_only=False):
    if scan_only:
        os.environ["HX_DEBUG_MATRIX_SCAN_ONLY"] = "1"
    try:
        ix = eng.HxIndex(DIM, ())
    finally:
        os.environ.pop("HX_DEBUG_MATRIX_SCAN_ONLY", None)
    ix.reserve(n)
    ix.synth_fill(n, synth.SEED_CORPUS)
    return ix


def sample(n, S):
    return np.random.default_rng(S).permutation(min(n, N_SMALL))[:S].astype(np.int64)   # the same rows in both indexes


def matrix_calls(ix, n):
    out = {}
    for S in SIZES:
        rows = sample(n, S)
        for L in LIMITS:
            keys, cnt = ix.search_matrix(rows, L)
            out[(S, L)] = events(lambda: ix.search_matrix(rows, L, keys=keys, counts=cnt))
    return out


def tiles(S, dim_pad):
    """TJ, TI of matrix.hip's launcher (rows of at most 1024 floats)"""
    tj = min(max(12288 // dim_pad, 8), 64)
    ti = 16
    if ((S + ti - 1) // ti) * ((S + tj - 1) // tj) >= 8192:
        ti *= 4
    return tj, ti


def main():
    print(f"distance matrix search, width {DIM}; ms per call, median [min-max] of {REPS} after {WARM} warm-up calls, HIP "
          f"events around hx_search_matrix; {torch.cuda.get_device_name(0)}; {LABEL}")
    small = index(N_SMALL)
    t_small = matrix_calls(small, N_SMALL)
    only = index(N_SMALL, scan_only=True)
    t_scan = matrix_calls(only, N_SMALL)
    only.close()
    small.close()
    big = index(N_BIG)
    t_big = matrix_calls(big, N_BIG)
    print(f"\n1. independence of the collection: {N_SMALL} rows | {N_BIG} rows")
    for key in t_small:
        S, L = key
        print(f"  S = {S:4d}, limit {L:2d}   {spread(t_small[key])}   |   {spread(t_big[key])}")
    print(f"\n2. per kernel ({N_SMALL} rows): the whole call | k_matrix_scan alone (HX_DEBUG_MATRIX_SCAN_ONLY) | the difference "
          "(k_matrix_select); the scan's multiply-adds and row bytes by the cost model")
    for key in t_small:
        S, L = key
        whole, scan = np.median(t_small[key]), np.median(t_scan[key])
        tj, ti = tiles(S, DIM)
        fma = S * S * DIM
        byts = S * S * DIM * 4 * (1 / ti + 1 / tj)
        print(f"  S = {S:4d}, limit {L:2d}   {spread(t_small[key])}   |   {spread(t_scan[key])}   |   {whole - scan:8.3f}      "
              f"{fma / (scan * 1e-3) / 1e12:6.2f} T multiply-adds/s, {byts / (scan * 1e-3) / 1e9:7.1f} GB/s (TJ {tj}, TI {ti})")
    print(f"\n3. the same lists by hx_recommend BEST_SCORE under the sample's mask, 16 requests per call ({N_BIG} rows), "
          "limit 3: the matrix call | S / 16 recommend calls | ratio")
    for S in (64, 1024):
        rows = sample(N_BIG, S)
        keep = np.zeros(N_BIG, bool)
        keep[rows] = True
        words = torch.from_numpy(pack_rows(keep).view(np.int32)).cuda()
        reqs = [[[(int(r), 1)] for r in rows[g:g + 16]] for g in range(0, S, 16)]
        keys, cnt = big.recommend(reqs[0], BEST_SCORE, 3, mask=words)
        mk, mc = big.search_matrix(rows, 3)
        assert (mk[:16].cpu() == keys.cpu()).all() and (mc[:16].cpu() == cnt.cpu()).all(), "the two routes disagree"

        def route():
            for rq in reqs:
                big.recommend(rq, BEST_SCORE, 3, mask=words, keys=keys, counts=cnt)
        t_reco = events(route)
        t_mat = t_big[(S, 3)]
        print(f"  S = {S:4d}   {spread(t_mat)}   |   {spread(t_reco)}   |   {np.median(t_reco) / np.median(t_mat):9.1f} x")
    print("  (the dense stage with the stored rows as queries under that mask: not measured)")
    big.close()


if __name__ == "__main__":
    main()
