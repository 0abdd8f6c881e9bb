"""Diagnostic: the payload index (hx_payload_mask) on the 10M x 768 synthetic corpus (hx_synth_fill)
with three columns: a keyword of 10^4 distinct codes, a number, a bool.  For a 1-predicate filter, a 3-predicate filter
(`match any` + `range` + `must_not match value`, about 1 % kept) and an IN over 10^5 codes it prints
  - the device time of the evaluation (HIP events around the enqueue-only call: the program's copy and the kernel),
    its algorithmic bytes (every referenced plane read once + n / 8 written) and their fraction of 8 TB/s;
  - the call with n_kept read back (what a caller that needs the count pays);
  - the device -> host copy of the mask;
  - the first use of the filter through _Collection.row_mask (compile + evaluate + copy), against the Python loop
    (filters.row_mask) measured at 1M rows of the same table and stated per row;
and the one bar: the 3-predicate mask with n_kept must not take longer than the B = 1 masked H1 call it feeds (same
mask, same process).  Median [min-max] of 20 after 3 warm-up calls.  Not part of bench.py.
argv: rows (default 10M) [kernel].  Output: one table on stdout (kept as profiles/payload_index_*.txt).
With `kernel` as the second argument only the three programs run, 20 times each, over a 64-d index of the same row count
(the kernel does not read the vectors): the run to put under `rocprofv3 --kernel-trace --stats`, which gives
k_payload_mask's own duration without the program's copy."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rag_application_amd import engine as eng, filters as F, payload_index as PI, synth  # noqa: E402
from rag_application_amd.handler import _Collection  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
KERNEL_ONLY = len(sys.argv) > 2 and sys.argv[2] == "kernel"
N_PY = min(N, 1_000_000)
REPS, WARM = 20, 3
HBM_PEAK = 8e12
P = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, dense_limit=100,
         quantized_limit=40, sparse_limit=100, final_limit=10, hnsw_ef=128)


def timed(fn):
    """(HIP-event ms, wall ms) per call: median, min, max"""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    f = lambda v: (float(np.median(v)), float(np.min(v)), float(np.max(v)))
    return f(ev), f(wall)


def fmt(t):
    return f"{t[0]:8.3f} [{t[1]:.3f}-{t[2]:.3f}]"


def main():
    if KERNEL_ONLY:
        ix = eng.HxIndex(64, (64,))
        ix.synth_fill(N, synth.SEED_CORPUS)
    else:
        tabs = synth.tables()
        ix = eng.HxIndex(768, (64, 128, 256))
        ix.reserve(N)
        ix.synth_fill(N, synth.SEED_CORPUS, synth.SEED_SPDOC, tabs)
        ix.finalize()
    rng = np.random.default_rng(0)
    kw = rng.integers(0, 10_000, N).astype(np.uint32)
    num = rng.integers(0, 100, N).astype(np.float64)
    flag = (rng.random(N) < 0.1).astype(np.uint32)
    # the collection's payload index, built column by column (10M payload dicts are not needed for the device path)
    col = _Collection.__new__(_Collection)
    col.dim, col.msizes, col.index, col.sparse_enabled = 768, (64, 128, 256), ix, True
    col.ids, col.payloads, col._masks = range(N), None, {}
    pi = col.pindex = PI.PayloadIndex()
    for key, schema, cells in (("document_id", "keyword", kw), ("page_number", "number", num.view(np.uint64)),
                               ("is_chat", "bool", flag)):
        k = pi.keys[key] = PI._Key(schema)
        k.col = ix.payload_create(k.kind)
        ix.payload_append(k.col, cells)
    pi.keys["document_id"].codes = {f"doc{c}": c for c in range(10_000)}
    f1 = {"must": [{"key": "page_number", "range": {"lt": 1}}]}
    f3 = {"must": [{"key": "document_id", "match": {"any": [f"doc{c}" for c in range(0, 10_000, 50)]}},
                   {"key": "page_number", "range": {"gte": 0, "lt": 50}}],
          "must_not": [{"key": "is_chat", "match": {"value": True}}]}
    big = np.sort(rng.choice(200_000, 100_000, replace=False)).astype(np.uint32)
    kcol = pi.keys["document_id"].col
    progs = [("1 predicate (range lt)", pi.compile(f1), f1, 8),
             ("3 predicates (any + range + must_not value)", pi.compile(f3), f3, 16),
             ("IN over 100000 codes", ([(PI.IN, kcol, 0)], [big]), None, 4)]
    if KERNEL_ONLY:
        for name, (ops, sets), _, _ in progs:       # launches 1-20, 21-40, 41-60 of k_payload_mask in the trace
            for _ in range(REPS):
                ix.payload_mask(ops, sets, want_count=False)
            torch.cuda.synchronize()
            print("ran", REPS, "x", name)
        ix.close()
        return
    print(f"payload index, {N} rows x 768, three columns; ms per call, median [min-max] of {REPS}")
    print("device = HIP events around the enqueue-only call (program copy + kernel); bytes = referenced planes once + n / 8")
    masks = {}
    for name, (ops, sets), flt, plane_bytes in progs:
        dev, _ = timed(lambda: ix.payload_mask(ops, sets, want_count=False))
        cnt_ev, cnt_wall = timed(lambda: ix.payload_mask(ops, sets, want_count=True))
        mask, kept = ix.payload_mask(ops, sets)
        masks[name] = mask
        _, d2h = timed(lambda: ix.mask_host(mask))
        nbytes = N * plane_bytes + N / 8
        print(f"\n{name}: kept {kept} ({100.0 * kept / N:.3f} %)")
        print(f"  device                      {fmt(dev)}   {nbytes / 1e6:7.1f} MB  {nbytes / (dev[0] * 1e-3) / 1e12:6.3f} TB/s "
              f"= {100 * nbytes / (dev[0] * 1e-3) / HBM_PEAK:5.1f} % of the 8 TB/s peak")
        print(f"  with n_kept (events)        {fmt(cnt_ev)}")
        print(f"  with n_kept (wall)          {fmt(cnt_wall)}")
        print(f"  mask device -> host (wall)  {fmt(d2h)}   {N / 8 / 1e6:.2f} MB")
        if flt is not None:
            first = []
            for _ in range(5):
                col._masks.clear()
                t0 = time.perf_counter()
                col.row_mask(flt)
                first.append((time.perf_counter() - t0) * 1e3)
            print(f"  first use, _Collection.row_mask (wall, median of 5)  {np.median(first):8.3f}")
    # the Python loop on the same table, at N_PY rows
    docs = [f"doc{c}" for c in kw[:N_PY]]
    pays = [{"document_id": d, "page_number": int(p), "is_chat": bool(c)} for d, p, c in zip(docs, num[:N_PY], flag[:N_PY])]
    ids = [str(r) for r in range(N_PY)]
    print(f"\nthe Python loop (filters.row_mask) at {N_PY} rows of the same table:")
    for name, flt in (("1 predicate", f1), ("3 predicates", f3)):
        t0 = time.perf_counter()
        want = F.row_mask(ids, pays, flt)
        dt = time.perf_counter() - t0
        got = ix.mask_host(masks[[n for n in masks if n.startswith(name)][0]])[:len(want)]
        tail = (1 << (N_PY % 32)) - 1 if N_PY % 32 else 0xFFFFFFFF
        same = np.array_equal(got[:-1], want[:-1]) and (int(got[-1]) & tail) == int(want[-1])
        print(f"  {name:14s} {dt:8.2f} s = {dt / N_PY * 1e6:6.2f} us per row -> {dt / N_PY * N:8.1f} s at {N} rows (extrapolated); "
              f"device mask equal on these rows: {same}")
    # the bar: the mask must not cost more than the query it feeds
    name3 = [n for n in masks if n.startswith("3 predicates")][0]
    ops, sets = progs[1][1]
    hp = eng.make_params(P, mode=eng.HX_MODE_H1)
    Q = eng.synth_queries_dense(768, 0, 1, synth.SEED_QUERY)
    tq = [torch.from_numpy(a).cuda() for a in synth.sparse_queries(synth.SEED_SPQUERY, 0, 1, tabs)]
    words = masks[name3]
    q_ev, q_wall = timed(lambda: ix.hybrid_query(Q, *tq, hp, mask=words))
    m_ev, m_wall = timed(lambda: ix.payload_mask(ops, sets, want_count=True))
    print(f"\nthe bar (3-predicate filter, same mask):")
    print(f"  hx_payload_mask with n_kept   events {fmt(m_ev)}   wall {fmt(m_wall)}")
    print(f"  masked H1 call, B = 1         events {fmt(q_ev)}   wall {fmt(q_wall)}")
    print(f"  ratio mask / query            events {m_ev[0] / q_ev[0]:.3f}   wall {m_wall[0] / q_wall[0]:.3f}   "
          f"({'met' if m_ev[0] <= q_ev[0] and m_wall[0] <= q_wall[0] else 'NOT met'}: the mask must not cost more)")
    ix.close()


if __name__ == "__main__":
    main()
