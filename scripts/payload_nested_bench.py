"""Diagnostic: nested blocks of the payload index (HX_PAY_NESTED of hx_payload_mask, k_payload_nested; DESIGN.md section
26) over a synthetic table of object arrays: N rows (default 10M) x 64-d (hx_synth_fill), an array `rels` of a geometric
number of objects per row (mean about 4, at most 64) with four indexed fields -- four element-aligned sibling columns:
  - `rels[].kind`  keyword, 16 codes;        - `rels[].src`  keyword, 10^4 codes;
  - `rels[].conf`  number, 0.0 .. 1.0 in steps of 0.1;   - `rels[].hops`  number, integers 0-9.
For a 2-condition and a 4-condition nested filter and -- the same-session yardstick -- an ANY_EQ over one of the same
columns it prints
  - the device time of the evaluation (HIP events around the enqueue-only call: the program's copy and the kernels), its
    algorithmic bytes (the anchor's offsets 8 n, 4 or 8 per element and referenced element plane, n / 8 for the mask; an
    ANY op also reads its head plane, 4 n, and its own offsets) and the resulting TB/s;
  - the call with n_kept read back;
and the Python loop (filters.row_mask) at 200 000 rows of the same table, extrapolated, with "device mask equal on these
rows".  Median [min-max] of 20 after 3 warm-up calls.  Not part of bench.py.
argv: rows (default 10M) [plain].  Output: one table on stdout (kept as profiles/payload_nested_*.txt).
With `plain` as the second argument the script times only programs older than the nested block -- the three scalar
filters of profiles/payload_index_10m.txt and three list filters of profiles/payload_lists_10m.txt -- and prints one
line: the run to alternate between two builds of the library to show that k_payload_mask did not move."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rag_application_amd import engine as eng, filters as F, payload_index as PI, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
PLAIN = len(sys.argv) > 2 and sys.argv[2] == "plain"
N_PY = min(N, 200_000)
REPS, WARM = 20, 3
HBM_PEAK = 8e12
KINDS = [f"K{i}" for i in range(16)]


def timed(fn, inner=1):
    """HIP-event ms per call (`inner` calls between one event pair): median, min, max"""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ev.append(a.elapsed_time(b) / inner)
    return float(np.median(ev)), float(np.min(ev)), float(np.max(ev))


def fmt(t):
    return f"{t[0]:8.3f} [{t[1]:.3f}-{t[2]:.3f}]"


def plain(ix, rng):
    """programs of the ops that existed before the nested block, one line of medians"""
    kw = rng.integers(0, 10_000, N).astype(np.uint32)
    num = rng.integers(0, 100, N).astype(np.float64)
    flag = (rng.random(N) < 0.1).astype(np.uint32)
    lang_len = np.minimum(rng.geometric(0.2, N) - 1, 64).astype(np.uint32)
    lang_val = rng.integers(0, 10_000, int(lang_len.sum())).astype(np.uint32)
    score_len = np.minimum(rng.geometric(1 / 3, N) - 1, 64).astype(np.uint32)
    score_val = rng.integers(0, 100, int(score_len.sum())).astype(np.float64)
    c_kw, c_num, c_flag = ix.payload_create(PI.PAY_U32), ix.payload_create(PI.PAY_F64), ix.payload_create(PI.PAY_U32)
    ix.payload_append(c_kw, kw)
    ix.payload_append(c_num, num.view(np.uint64))
    ix.payload_append(c_flag, flag)
    c_lang, c_score = ix.payload_create(PI.PAY_LIST_U32), ix.payload_create(PI.PAY_LIST_F64)
    ix.payload_append_lists(c_lang, lang_len, lang_val)
    ix.payload_append_lists(c_score, score_len, score_val)
    big = np.unique(rng.integers(0, 200_000, 100_000).astype(np.uint32))
    some = np.arange(0, 10_000, 50, dtype=np.uint32)
    progs = [("f1", [(PI.EQ, c_kw, 17)], []),
             ("f3", [(PI.EQ, c_kw, 17), (PI.GE, c_num, PI.f64_bits(10.0)), (PI.AND, 0, 0), (PI.EQ, c_flag, 1), (PI.NOT, 0, 0),
                     (PI.AND, 0, 0)], []),
             ("in1e5", [(PI.IN, c_kw, 0)], [big]),
             ("any_eq", [(PI.ANY_EQ, c_lang, 17)], []),
             ("any_in200", [(PI.ANY_IN, c_lang, 0)], [some]),
             ("any_range", [(PI.ANY_RANGE, c_score, 0)], [np.array([10.0, 11.0])])]
    out = []
    for name, ops, sets in progs:
        one = timed(lambda: ix.payload_mask(ops, sets, want_count=False))
        many = timed(lambda: ix.payload_mask(ops, sets, want_count=False), inner=50)
        out.append(f"{name} enqueue={one[0]:.4f} x50={many[0]:.4f}")
    print(" | ".join(out))


def main():
    ix = eng.HxIndex(64, (64,))
    ix.synth_fill(N, synth.SEED_CORPUS)
    rng = np.random.default_rng(0)
    if PLAIN:
        plain(ix, rng)
        ix.close()
        return
    lens = np.minimum(rng.geometric(0.2, N) - 1, 64).astype(np.uint32)
    total = int(lens.sum())
    kind = rng.integers(0, 16, total).astype(np.uint32)
    src = rng.integers(0, 10_000, total).astype(np.uint32)
    conf = rng.integers(0, 11, total).astype(np.float64) / 10
    hops = rng.integers(0, 10, total).astype(np.float64)
    pi = PI.PayloadIndex()              # built column by column: 10M payload dicts are not needed for the device path
    for key, schema, vals in (("rels[].kind", "keyword", kind), ("rels[].src", "keyword", src), ("rels[].conf", "number", conf),
                              ("rels[].hops", "number", hops)):
        k = pi.keys[key] = PI._Key(schema, key)
        k.col = ix.payload_create(k.kind)
        ix.payload_append_lists(k.col, lens, vals)
    pi.keys["rels[].kind"].codes = {s: c for c, s in enumerate(KINDS)}
    pi.keys["rels[].src"].codes = {f"s{c}": c for c in range(10_000)}
    cols = [k.col for k in pi.keys.values()]
    assert all(ix.payload_same_offsets(cols[0], c) for c in cols[1:])
    two = {"must": [{"nested": {"key": "rels", "filter": {"must": [{"key": "kind", "match": {"value": "K3"}},
                                                                     {"key": "conf", "range": {"gte": 0.8}}]}}}]}
    four = {"must": [{"nested": {"key": "rels", "filter": {"must": [{"key": "kind", "match": {"any": ["K3", "K5", "K7"]}},
                                                                      {"key": "conf", "range": {"gte": 0.5}},
                                                                      {"key": "hops", "range": {"lt": 4}}],
                                                             "must_not": [{"key": "src", "match": {"any": [f"s{c}" for c in range(0, 10_000, 50)]}}]}}}]}
    loose = {"must": [{"key": "rels[].kind", "match": {"value": "K3"}}, {"key": "rels[].conf", "range": {"gte": 0.8}}]}
    any_eq = {"must": [{"key": "rels[].kind", "match": {"value": "K3"}}]}
    off_b = 8 * N
    flts = [("nested, 2 conditions (kind == K3 and conf >= 0.8)", two, off_b + (4 + 8) * total + N / 8),
            ("nested, 4 conditions (kind in 3, conf >= 0.5, hops < 4, src not in 200)", four, off_b + (4 + 8 + 8 + 4) * total + N / 8),
            ("the same 2 conditions as projections (two ANY ops: any two objects)", loose, 2 * (4 * N + off_b) + (4 + 8) * total + N / 8),
            ("yardstick: ANY_EQ over rels[].kind", any_eq, 4 * N + off_b + 4 * total + N / 8)]
    progs = [(name, pi.compile(flt), flt, b) for name, flt, b in flts]
    assert all(p[1] is not None for p in progs), pi.declined
    print(f"nested blocks, {N} rows x 64; rels: {total} objects (mean {total / N:.2f}, max {int(lens.max())}), 4 sibling columns; "
          f"ms per call, median [min-max] of {REPS}")
    print("device = HIP events around the enqueue-only call (program copy + k_payload_nested + k_payload_mask); bytes = offsets + the "
          "referenced element planes + n / 8 (+ heads for an ANY op)")
    masks = {}
    for name, (ops, sets), flt, nbytes in progs:
        dev = timed(lambda: ix.payload_mask(ops, sets, want_count=False))
        cnt = timed(lambda: ix.payload_mask(ops, sets, want_count=True))
        mask, kept = ix.payload_mask(ops, sets)
        masks[name] = mask
        print(f"\n{name}: kept {kept} ({100.0 * kept / N:.3f} %)")
        print(f"  device                      {fmt(dev)}   {nbytes / 1e6:7.1f} MB  {nbytes / (dev[0] * 1e-3) / 1e12:6.3f} TB/s "
              f"= {100 * nbytes / (dev[0] * 1e-3) / HBM_PEAK:5.1f} % of the 8 TB/s peak")
        print(f"  with n_kept (events)        {fmt(cnt)}")
    off = np.concatenate([[0], np.cumsum(lens[:N_PY].astype(np.int64))])
    pays = [{"rels": [{"kind": KINDS[kind[e]], "src": f"s{src[e]}", "conf": float(conf[e]), "hops": int(hops[e])}
                      for e in range(off[r], off[r + 1])]} for r in range(N_PY)]
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
    ix.close()


if __name__ == "__main__":
    main()
