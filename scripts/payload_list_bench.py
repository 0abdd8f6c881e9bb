"""Diagnostic: list columns of the payload index (hx_payload_append_lists, the ANY ops of hx_payload_mask; DESIGN.md
section 17) on the 10M x 768 synthetic corpus (hx_synth_fill) with
  - `languages`: a keyword-list column of 10^4 codes, lengths 0-64 skewed to short (geometric, mean about 4);
  - `scores`: a number-list column, lengths geometric with mean about 2, integers 0-99;
  - the three scalar columns of scripts/payload_bench.py (document_id, page_number, is_chat).
For ANY_EQ, ANY_IN of 200 codes, ANY_RANGE, `except` of 200 codes and a 3-predicate mix (list `any` + list `range` +
`must_not` on the scalar bool) it prints the columns of section 15's table:
  - the device time of the evaluation (HIP events around the enqueue-only call: the program's copy and the kernel), its
    algorithmic bytes (per referenced list column: heads 4 n + offsets 8 n + 4 or 8 per element; per scalar plane 4 n;
    n / 8 written) and their fraction of 8 TB/s;
  - the call with n_kept read back; the device -> host copy of the mask;
  - the first use of the filter through _Collection.row_mask (compile + evaluate + copy), against the Python loop
    (filters.row_mask) measured at 200 000 rows of the same table and stated per row;
and the bar: the 3-predicate mask with n_kept must not take longer than the B = 1 masked H1 call it feeds (same mask,
same process).  Median [min-max] of 20 after 3 warm-up calls.  Not part of bench.py.
argv: rows (default 10M) [kernel].  Output: one table on stdout (kept as profiles/payload_lists_*.txt).
With `kernel` as the second argument only the programs run, 20 times each, over a 64-d index of the same row count: the
run to put under `rocprofv3 --kernel-trace --stats`, which gives k_payload_mask's own duration."""
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
N_PY = min(N, 200_000)
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
    lang_len = np.minimum(rng.geometric(0.2, N) - 1, 64).astype(np.uint32)
    lang_val = rng.integers(0, 10_000, int(lang_len.sum())).astype(np.uint32)
    score_len = np.minimum(rng.geometric(1 / 3, N) - 1, 64).astype(np.uint32)
    score_val = rng.integers(0, 100, int(score_len.sum())).astype(np.float64)
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
    for key, schema, heads, vals in (("languages", "keyword_list", lang_len, lang_val),
                                     ("scores", "number_list", score_len, score_val)):
        k = pi.keys[key] = PI._Key(schema)
        k.col = ix.payload_create(k.kind)
        ix.payload_append_lists(k.col, heads, vals)
    pi.keys["document_id"].codes = {f"doc{c}": c for c in range(10_000)}
    pi.keys["languages"].codes = {f"l{c}": c for c in range(10_000)}
    some = [f"l{c}" for c in range(0, 10_000, 50)]
    lang_b = 12 * N + 4 * len(lang_val)               # heads + offsets + elements
    score_b = 12 * N + 8 * len(score_val)
    flts = [("ANY_EQ (match value)", {"must": [{"key": "languages", "match": {"value": "l17"}}]}, lang_b),
            ("ANY_IN of 200 (match any)", {"must": [{"key": "languages", "match": {"any": some}}]}, lang_b),
            ("ANY_RANGE (range gte lt)", {"must": [{"key": "scores", "range": {"gte": 10, "lt": 12}}]}, score_b),
            ("except of 200", {"must": [{"key": "languages", "match": {"except": some}}]}, lang_b),
            ("3 predicates (list any + list range + must_not scalar value)",
             {"must": [{"key": "languages", "match": {"any": some}}, {"key": "scores", "range": {"gte": 0, "lt": 20}}],
              "must_not": [{"key": "is_chat", "match": {"value": True}}]}, lang_b + score_b + 4 * N)]
    progs = [(name, pi.compile(flt), flt, b) for name, flt, b in flts]
    assert all(p[1] is not None for p in progs), pi.declined
    if KERNEL_ONLY:
        for name, (ops, sets), _, _ in progs:       # launches 1-20, 21-40, ... of k_payload_mask in the trace
            for _ in range(REPS):
                ix.payload_mask(ops, sets, want_count=False)
            torch.cuda.synchronize()
            print("ran", REPS, "x", name)
        ix.close()
        return
    print(f"payload list columns, {N} rows x 768; languages: {len(lang_val)} elements (mean {len(lang_val) / N:.2f}, max "
          f"{int(lang_len.max())}), scores: {len(score_val)} elements (mean {len(score_val) / N:.2f}); ms per call, median [min-max] of {REPS}")
    print("device = HIP events around the enqueue-only call (program copy + kernel); bytes = heads + offsets + elements of the "
          "referenced list columns + scalar planes + n / 8")
    masks = {}
    for name, (ops, sets), flt, plane_bytes in progs:
        dev, _ = timed(lambda: ix.payload_mask(ops, sets, want_count=False))
        cnt_ev, cnt_wall = timed(lambda: ix.payload_mask(ops, sets, want_count=True))
        mask, kept = ix.payload_mask(ops, sets)
        masks[name] = mask
        _, d2h = timed(lambda: ix.mask_host(mask))
        nbytes = plane_bytes + N / 8
        print(f"\n{name}: kept {kept} ({100.0 * kept / N:.3f} %)")
        print(f"  device                      {fmt(dev)}   {nbytes / 1e6:7.1f} MB  {nbytes / (dev[0] * 1e-3) / 1e12:6.3f} TB/s "
              f"= {100 * nbytes / (dev[0] * 1e-3) / HBM_PEAK:5.1f} % of the 8 TB/s peak")
        print(f"  with n_kept (events)        {fmt(cnt_ev)}")
        print(f"  with n_kept (wall)          {fmt(cnt_wall)}")
        print(f"  mask device -> host (wall)  {fmt(d2h)}   {N / 8 / 1e6:.2f} MB")
        first = []
        for _ in range(5):
            col._masks.clear()
            t0 = time.perf_counter()
            col.row_mask(flt)
            first.append((time.perf_counter() - t0) * 1e3)
        print(f"  first use, _Collection.row_mask (wall, median of 5)  {np.median(first):8.3f}")
    # the Python loop on the same table, at N_PY rows
    lo = np.concatenate([[0], np.cumsum(lang_len[:N_PY].astype(np.int64))])
    so = np.concatenate([[0], np.cumsum(score_len[:N_PY].astype(np.int64))])
    pays = [{"languages": [f"l{c}" for c in lang_val[lo[r]:lo[r + 1]]], "scores": [int(v) for v in score_val[so[r]:so[r + 1]]],
             "is_chat": bool(flag[r])} for r in range(N_PY)]
    ids = [str(r) for r in range(N_PY)]
    print(f"\nthe Python loop (filters.row_mask) at {N_PY} rows of the same table:")
    for name, _, flt, _ in progs:
        t0 = time.perf_counter()
        want = F.row_mask(ids, pays, flt)
        dt = time.perf_counter() - t0
        got = ix.mask_host(masks[name])[:len(want)]
        tail = (1 << (N_PY % 32)) - 1 if N_PY % 32 else 0xFFFFFFFF
        same = np.array_equal(got[:-1], want[:-1]) and (int(got[-1]) & tail) == int(want[-1])
        print(f"  {name[:26]:26s} {dt:8.2f} s = {dt / N_PY * 1e6:6.2f} us per row -> {dt / N_PY * N:8.1f} s at {N} rows (extrapolated); "
              f"device mask equal on these rows: {same}")
    # the bar: the mask must not cost more than the query it feeds
    name3, (ops, sets) = progs[-1][0], progs[-1][1]
    hp = eng.make_params(P, mode=eng.HX_MODE_H1)
    Q = eng.synth_queries_dense(768, 0, 1, synth.SEED_QUERY)
    tq = [torch.from_numpy(a).cuda() for a in synth.sparse_queries(synth.SEED_SPQUERY, 0, 1, tabs)]
    words = masks[name3]
    q_ev, q_wall = timed(lambda: ix.hybrid_query(Q, *tq, hp, mask=words))
    m_ev, m_wall = timed(lambda: ix.payload_mask(ops, sets, want_count=True))
    print(f"\nthe bar (3-predicate list filter, same mask):")
    print(f"  hx_payload_mask with n_kept   events {fmt(m_ev)}   wall {fmt(m_wall)}")
    print(f"  masked H1 call, B = 1         events {fmt(q_ev)}   wall {fmt(q_wall)}")
    print(f"  ratio mask / query            events {m_ev[0] / q_ev[0]:.3f}   wall {m_wall[0] / q_wall[0]:.3f}   "
          f"({'met' if m_ev[0] <= q_ev[0] and m_wall[0] <= q_wall[0] else 'NOT met'}: the mask must not cost more)")
    ix.close()


if __name__ == "__main__":
    main()
