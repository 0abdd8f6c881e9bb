"""Diagnostic: text columns of the payload index (hx_payload_append_text, HX_PAY_TEXT_ALL of hx_payload_mask; DESIGN.md
section 19) on the 10M x 768 synthetic corpus (hx_synth_fill) with
  - `content`: a text column whose byte lengths are log-normal (median about 300, mean about 400, cut to 0 .. 4000;
    about 4 GB in all); the bytes are lower-case letters and blanks drawn with a skew (6 blanks in 32), with the searched
    words written over them: "vector" into 30 % of the rows, "zebra" into 0.01 %, each of "hybrid" / "dense" / "sparse"
    into 40 % independently;
  - the three scalar columns of scripts/payload_bench.py (document_id, page_number, is_chat).
For one common word, one rare word, three words and a text filter beside a scalar range it prints
  - the rows kept and the algorithmic bytes (the column's words + heads 4 n + offsets 8 n, 4 n per scalar plane, n / 8
    per plane written and read) and their fraction of 8 TB/s at the measured time;
  - the enqueue-only call (HIP events: the program's copy, k_payload_text per TEXT_ALL and k_payload_mask);
  - the call with n_kept read back; the first use through _Collection.row_mask;
  - the Python loop (filters.row_mask) on a 200 000-row slice, per row, with the device mask compared on that slice.
Median [min-max] of 20 after 3 warm-up calls.  Not part of bench.py.
argv: rows (default 10M) [kernel | ab].  Output: one table on stdout (kept as profiles/payload_text_*.txt).
  kernel  only the programs run, 20 times each, over a 64-d index of the same row count: the run to put under
          `rocprofv3 --kernel-trace --stats`, which gives k_payload_text's and k_payload_mask's own durations.
  ab      the regression figures of the filters that existed before (the three scalar filters of scripts/payload_bench.py
          and the five list filters of scripts/payload_list_bench.py) over a 64-d index: one line of medians of 20 --
          one enqueue-only call, 50 enqueue-only calls between one event pair divided by 50, the call with n_kept.  Run
          it once per library (HX_LIB_PATH names another build, e.g. the parent commit's), alternating, one process each."""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rag_application_amd import _lib  # noqa: E402

MODE = sys.argv[2] if len(sys.argv) > 2 else ""
if MODE == "ab" and os.environ.get("HX_LIB_PATH"):      # an older build lacks the entries this commit adds: bind what it has
    torch.cuda.is_available()
    _probe = ctypes.CDLL(os.environ["HX_LIB_PATH"])
    for _name in [s for s in _lib._SIGS if not hasattr(_probe, s)]:
        del _lib._SIGS[_name]

from rag_application_amd import engine as eng, filters as F, payload_index as PI, synth  # noqa: E402
from rag_application_amd.handler import _Collection  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
N_PY = min(N, 200_000)
REPS, WARM = 20, 3
HBM_PEAK = 8e12
LETTERS = np.frombuffer(b"etaoinshrdlucmfwypvbgkjxzq      ", np.uint8)
CHUNK = 1_000_000


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


def text_chunk(rng, n):
    """(lengths, bytes) of n rows of the `content` column"""
    lens = np.clip(rng.lognormal(np.log(300.0), 0.75, n), 0, 4000).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    flat = LETTERS[rng.integers(0, 32, int(off[-1]), dtype=np.uint8)]
    for word, share in ((b"vector", 0.30), (b"zebra", 0.0001), (b"hybrid", 0.40), (b"dense", 0.40), (b"sparse", 0.40)):
        rows = np.flatnonzero((rng.random(n) < share) & (lens >= 64))
        at = off[rows] + (rng.random(len(rows)) * (lens[rows] - 16)).astype(np.int64)
        for i, ch in enumerate(word):
            flat[at + i] = ch
    return lens.astype(np.uint32), flat


def scalar_columns(ix, pi, rng):
    kw = rng.integers(0, 10_000, N).astype(np.uint32)
    num = rng.integers(0, 100, N).astype(np.float64)
    flag = (rng.random(N) < 0.1).astype(np.uint32)
    for key, schema, cells in (("document_id", "keyword", kw), ("page_number", "number", num.view(np.uint64)),
                               ("is_chat", "bool", flag)):
        k = pi.keys[key] = PI._Key(schema)
        k.col = ix.payload_create(k.kind)
        ix.payload_append(k.col, cells)
    pi.keys["document_id"].codes = {f"doc{c}": c for c in range(10_000)}
    return kw, num, flag


def collection(ix, dim, msizes):
    col = _Collection.__new__(_Collection)
    col.dim, col.msizes, col.index, col.sparse_enabled = dim, msizes, ix, True
    col.ids, col.payloads, col._masks = range(N), None, {}
    col.pindex = PI.PayloadIndex()
    return col


def ab():
    """the filters that existed before this commit, one line of medians"""
    ix = eng.HxIndex(64, (64,))
    ix.synth_fill(N, synth.SEED_CORPUS)
    col = collection(ix, 64, (64,))
    pi = col.pindex
    rng = np.random.default_rng(0)
    scalar_columns(ix, pi, rng)
    lang_len = np.minimum(rng.geometric(0.2, N) - 1, 64).astype(np.uint32)
    lang_val = rng.integers(0, 10_000, int(lang_len.sum())).astype(np.uint32)
    score_len = np.minimum(rng.geometric(1 / 3, N) - 1, 64).astype(np.uint32)
    score_val = rng.integers(0, 100, int(score_len.sum())).astype(np.float64)
    for key, schema, heads, vals in (("languages", "keyword_list", lang_len, lang_val), ("scores", "number_list", score_len, score_val)):
        k = pi.keys[key] = PI._Key(schema)
        k.col = ix.payload_create(k.kind)
        ix.payload_append_lists(k.col, heads, vals)
    pi.keys["languages"].codes = {f"l{c}": c for c in range(10_000)}
    some = [f"l{c}" for c in range(0, 10_000, 50)]
    big = np.sort(rng.choice(200_000, 100_000, replace=False)).astype(np.uint32)
    progs = [("f1", pi.compile({"must": [{"key": "page_number", "range": {"lt": 1}}]})),
             ("f3", pi.compile({"must": [{"key": "document_id", "match": {"any": [f"doc{c}" for c in range(0, 10_000, 50)]}},
                                         {"key": "page_number", "range": {"gte": 0, "lt": 50}}],
                                "must_not": [{"key": "is_chat", "match": {"value": True}}]})),
             ("in1e5", ([(PI.IN, pi.keys["document_id"].col, 0)], [big])),
             ("any_eq", pi.compile({"must": [{"key": "languages", "match": {"value": "l17"}}]})),
             ("any_in", pi.compile({"must": [{"key": "languages", "match": {"any": some}}]})),
             ("any_range", pi.compile({"must": [{"key": "scores", "range": {"gte": 10, "lt": 12}}]})),
             ("except", pi.compile({"must": [{"key": "languages", "match": {"except": some}}]})),
             ("list3", pi.compile({"must": [{"key": "languages", "match": {"any": some}}, {"key": "scores", "range": {"gte": 0, "lt": 20}}],
                                   "must_not": [{"key": "is_chat", "match": {"value": True}}]}))]
    out = []
    for name, (ops, sets) in progs:
        one, _ = timed(lambda: ix.payload_mask(ops, sets, want_count=False))
        x50, _ = timed(lambda: [ix.payload_mask(ops, sets, want_count=False) for _ in range(50)])
        kept, _ = timed(lambda: ix.payload_mask(ops, sets, want_count=True))
        out.append(f"{name} enqueue={one[0]:.4f} x50={x50[0] / 50:.4f} kept={kept[0]:.4f}")
    print(os.environ.get("HX_LIB_PATH") or "this tree's library", "|", " | ".join(out), flush=True)
    ix.close()


def main():
    if MODE == "ab":
        return ab()
    kernel_only = MODE == "kernel"
    if kernel_only:
        ix = eng.HxIndex(64, (64,))
        ix.synth_fill(N, synth.SEED_CORPUS)
        col = collection(ix, 64, (64,))
    else:
        tabs = synth.tables()
        ix = eng.HxIndex(768, (64, 128, 256))
        ix.reserve(N)
        ix.synth_fill(N, synth.SEED_CORPUS, synth.SEED_SPDOC, tabs)
        ix.finalize()
        col = collection(ix, 768, (64, 128, 256))
    pi = col.pindex
    rng = np.random.default_rng(0)
    kw, num, flag = scalar_columns(ix, pi, rng)
    k = pi.keys["content"] = PI._Key("text")
    k.col = ix.payload_create(k.kind)
    n_bytes = n_words = 0
    all_lens, head_rows = [], None
    for lo in range(0, N, CHUNK):
        lens, flat = text_chunk(rng, min(CHUNK, N - lo))
        ix.payload_append_text(k.col, lens, flat)
        n_bytes += len(flat)
        n_words += int(((lens.astype(np.int64) + 3) // 4).sum())
        all_lens.append(lens)
        if lo == 0:
            head_rows = (lens[:N_PY].copy(), flat[:int(lens[:N_PY].astype(np.int64).sum())].copy())
    lens = np.concatenate(all_lens)
    text_b = 4 * n_words + 12 * N                       # the words + heads + offsets
    plane = N / 8
    flts = [("one common word (vector)", {"must": [{"key": "content", "match": {"text": "vector"}}]}, text_b + 2 * plane),
            ("one rare word (zebra)", {"must": [{"key": "content", "match": {"text": "zebra"}}]}, text_b + 2 * plane),
            ("three words (hybrid dense sparse)", {"must": [{"key": "content", "match": {"text": "Hybrid dense SPARSE"}}]}, text_b + 2 * plane),
            ("text + scalar range", {"must": [{"key": "content", "match": {"text": "vector"}},
                                              {"key": "page_number", "range": {"gte": 0, "lt": 50}}]}, text_b + 2 * plane + 8 * N)]
    progs = [(name, pi.compile(flt), flt, b) for name, flt, b in flts]
    assert all(p[1] is not None for p in progs), pi.declined
    if kernel_only:
        for name, (ops, sets), _, _ in progs:       # launches 1-20, 21-40, ... of k_payload_text / k_payload_mask in the trace
            for _ in range(REPS):
                ix.payload_mask(ops, sets, want_count=False)
            torch.cuda.synchronize()
            print("ran", REPS, "x", name)
        ix.close()
        return
    q = np.percentile(lens, [50, 90, 99])
    print(f"payload text column, {N} rows x 768; content: {n_bytes} bytes ({n_bytes / 1e9:.2f} GB; mean {n_bytes / N:.0f}, median {q[0]:.0f}, "
          f"p90 {q[1]:.0f}, p99 {q[2]:.0f}, max {int(lens.max())}; log-normal(ln 300, 0.75) cut to 0 .. 4000), {4 * n_words} bytes stored; "
          f"ms per call, median [min-max] of {REPS}")
    print("device = HIP events around the enqueue-only call (program copy + k_payload_text per TEXT_ALL + k_payload_mask); "
          "bytes = words + heads + offsets of the text column + scalar planes + n / 8 per plane written and read")
    masks = {}
    for name, (ops, sets), flt, nbytes in progs:
        dev, _ = timed(lambda: ix.payload_mask(ops, sets, want_count=False))
        cnt_ev, cnt_wall = timed(lambda: ix.payload_mask(ops, sets, want_count=True))
        mask, kept = ix.payload_mask(ops, sets)
        masks[name] = mask
        print(f"\n{name}: kept {kept} ({100.0 * kept / N:.4f} %)")
        print(f"  device                      {fmt(dev)}   {nbytes / 1e6:7.1f} MB  {nbytes / (dev[0] * 1e-3) / 1e12:6.3f} TB/s "
              f"= {100 * nbytes / (dev[0] * 1e-3) / HBM_PEAK:5.1f} % of the 8 TB/s peak")
        print(f"  with n_kept (events)        {fmt(cnt_ev)}")
        print(f"  with n_kept (wall)          {fmt(cnt_wall)}")
        first = []
        for _ in range(5):
            col._masks.clear()
            t0 = time.perf_counter()
            col.row_mask(flt)
            first.append((time.perf_counter() - t0) * 1e3)
        print(f"  first use, _Collection.row_mask (wall, median of 5)  {np.median(first):8.3f}")
    # the Python loop on the same table, at N_PY rows
    hl, hb = head_rows
    o = np.concatenate([[0], np.cumsum(hl.astype(np.int64))])
    pays = [{"content": hb[o[r]:o[r + 1]].tobytes().decode("ascii"), "page_number": int(num[r])} for r in range(N_PY)]
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
    # the ratio to the query the mask feeds (no bar: the floor of a text scan is the column's bytes once)
    name4, (ops, sets) = progs[-1][0], progs[-1][1]
    P = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, dense_limit=100,
             quantized_limit=40, sparse_limit=100, final_limit=10, hnsw_ef=128)
    hp = eng.make_params(P, mode=eng.HX_MODE_H1)
    Q = eng.synth_queries_dense(768, 0, 1, synth.SEED_QUERY)
    tq = [torch.from_numpy(a).cuda() for a in synth.sparse_queries(synth.SEED_SPQUERY, 0, 1, tabs)]
    q_ev, q_wall = timed(lambda: ix.hybrid_query(Q, *tq, hp, mask=masks[name4]))
    m_ev, m_wall = timed(lambda: ix.payload_mask(ops, sets, want_count=True))
    print(f"\nthe mask against the query it feeds (text + scalar range, same mask; reported, no bar):")
    print(f"  hx_payload_mask with n_kept   events {fmt(m_ev)}   wall {fmt(m_wall)}")
    print(f"  masked H1 call, B = 1         events {fmt(q_ev)}   wall {fmt(q_wall)}")
    print(f"  ratio mask / query            events {m_ev[0] / q_ev[0]:.3f}   wall {m_wall[0] / q_wall[0]:.3f}")
    ix.close()


if __name__ == "__main__":
    main()
