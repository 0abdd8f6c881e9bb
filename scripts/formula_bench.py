"""Diagnostic: score-boosting search (hx_formula / hx_hybrid_query_formula_host) on a 10M x 768
synthetic corpus (hx_synth_fill) with a datetime column, a number column and a keyword per row.  H1 pools of 100
(dense_limit = sparse_limit = 50) and 2048 (1024 + 1024), B = 1 / 64 / 1024 queries, limit 10, two formulas:
  recency          sum[$score, mult[0.2, exp_decay(datetime_key timestamp, target = a datetime, scale = 1 day)]]
  two conditions   mult[$score, sum[1, mult[0.5, file_type == pdf], mult[-0.5, page_number >= 100]]]
Per case, ms per call, median [min-max] of 20 after 3 warm-up calls:
  k_formula alone    HIP events around hx_formula over the pool of the batch, already on the device;
  boosted host call  hx_hybrid_query_formula_host, wall clock (the condition planes are uploaded inside the call);
  plain host call    hx_hybrid_query_host at final_limit = the pool, wall clock, timed in alternation with the boosted
                     call: what a caller who boosts in Python has to ask for first;
  Python path        boosting.evaluate + boosting.rank over the payloads of that pool, for B <= 64 (3 calls; it is linear
                     in B x pool), on top of the plain host call.
Not part of bench.py.  argv: [rows (default 10M)] [--label TEXT].  Output: one table on stdout (kept as
profiles/formula_*.txt)."""
import datetime as dt
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rag_application_amd import boosting, engine as eng, filters, synth  # noqa: E402
from rag_application_amd.payload_index import PayloadIndex, _Key  # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
LABEL = sys.argv[sys.argv.index("--label") + 1] if "--label" in sys.argv else ""
if LABEL in ARGS:
    ARGS.remove(LABEL)
N = int(ARGS[0]) if ARGS else 10_000_000
LIMIT, REPS, WARM = 10, 20, 3
BASE = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, quantized_limit=40, final_limit=10,
            hnsw_ef=128)
T0 = dt.datetime(2024, 3, 1, tzinfo=dt.timezone.utc)
T0_US = 1_709_251_200_000_000
TYPES = ("pdf", "docx", "txt", "md")
FORMULAS = {
    "recency": {"sum": ["$score", {"mult": [0.2, {"exp_decay": {"x": {"datetime_key": "timestamp"},
                                                                  "target": {"datetime": T0}, "scale": 86400}}]}]},
    "two conditions": {"mult": ["$score", {"sum": [1, {"mult": [0.5, {"key": "file_type", "match": {"value": "pdf"}}]},
                                                  {"mult": [-0.5, {"key": "page_number", "range": {"gte": 100}}]}]}]},
}
DEFAULTS = {"timestamp": T0}


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


def wall_alternating(fns, reps=REPS, warm=WARM):
    for _ in range(warm):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
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
    rng = np.random.default_rng(27)
    ts_us = T0_US - rng.integers(0, 90 * 86400 * 10 ** 6, N)
    page = rng.integers(0, 400, N)
    ftype = rng.integers(0, len(TYPES), N)
    c_ts = ix.payload_create(2)
    ix.payload_append(c_ts, ts_us.astype(np.float64))
    pi = PayloadIndex()
    for key, schema, col in (("timestamp", "datetime", c_ts), ("file_type", "keyword", 1000), ("page_number", "number", 1001)):
        pi.keys[key] = _Key(schema, key)
        pi.keys[key].col = col
    pi.keys["file_type"].codes = {t: i for i, t in enumerate(TYPES)}
    plane_of = {filters.filter_key({"must": [FORMULAS["two conditions"]["mult"][1]["sum"][1]["mult"][1]]}): ftype == 0,
                filters.filter_key({"must": [FORMULAS["two conditions"]["mult"][1]["sum"][2]["mult"][1]]}): page >= 100}

    def payload(r):
        t = dt.datetime.fromtimestamp(int(ts_us[r]) / 1e6, dt.timezone.utc)
        return {"timestamp": t.isoformat(), "file_type": TYPES[ftype[r]], "page_number": int(page[r])}

    print(f"score boosting, {N} rows x 768, H1, limit {LIMIT}; ms per call, median [min-max] of {REPS} after {WARM} warm-up "
          f"calls; {torch.cuda.get_device_name(0)}; {LABEL}")
    for dl in (50, 1024):
        pool = 2 * dl
        hp = eng.make_params(dict(BASE, dense_limit=dl, sparse_limit=dl, final_limit=pool), mode=eng.HX_MODE_H1)
        for B in (1, 64, 1024):
            Qd = eng.synth_queries_dense(768, 0, B, synth.SEED_QUERY)
            Q = Qd.cpu().numpy()
            qip, qsi, qsv = synth.sparse_queries(synth.SEED_SPQUERY, 0, B, tabs)
            tq = [torch.from_numpy(a).cuda() for a in (qip, qsi, qsv)]
            keys, cnt = ix.hybrid_query(Qd, *tq, hp)
            plain = lambda: ix.hybrid_query_host(Q, qip, qsi, qsv, hp)                                   # noqa: E731
            for name, formula in FORMULAS.items():
                ops, conds = boosting.compile(formula, DEFAULTS, pi)
                planes = [filters.pack_rows(plane_of[filters.filter_key(c)]) for c in conds]
                print(f"\npool {pool}, B = {B}, {name} ({len(ops)} ops, {len(planes)} planes), mean pool "
                      f"{float(cnt.float().mean()):.1f}")
                dev_planes = [torch.from_numpy(p.view(np.int32)).cuda() for p in planes]
                import ctypes as C
                from rag_application_amd import _lib
                parr = (C.c_void_p * max(len(dev_planes), 1))(*[t.data_ptr() for t in dev_planes])
                arr = ix._formula_ops(ops)
                out = (torch.empty((B, LIMIT), dtype=torch.int64, device="cuda"),
                       torch.empty((B, LIMIT), dtype=torch.int32, device="cuda"),
                       torch.empty((B,), dtype=torch.int32, device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda"))

                def stage():
                    _lib.check(_lib.lib().hx_formula(ix._h, arr, len(ops), parr if dev_planes else None, len(dev_planes), N,
                                                     keys.data_ptr(), pool, cnt.data_ptr(), B, LIMIT, float("nan"), None, 0,
                                                     out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                     out[3].data_ptr(), torch.cuda.current_stream().cuda_stream))
                print(f"  {'k_formula alone (HIP events)':40s} {spread(events(stage))}")
                boosted = lambda: ix.hybrid_query_formula_host(Q, qip, qsi, qsv, hp, ops, LIMIT, planes=planes)   # noqa: E731
                t_plain, t_boost = wall_alternating([plain, boosted])
                print(f"  {'boosted host call':40s} {spread(t_boost)}")
                print(f"  {'plain host call, final_limit = pool':40s} {spread(t_plain)}")
                print(f"  boosted - plain (medians) {float(np.median(t_boost) - np.median(t_plain)):+.3f} ms")
                if B <= 64:
                    scores, rows, counts = plain()

                    def python_path():
                        for sc, rw, n in zip(scores.tolist(), rows.tolist(), counts.tolist()):
                            vals = [boosting.value_f32(boosting.evaluate(formula, DEFAULTS, s, payload(r), r))
                                    for s, r in zip(sc[:n], rw[:n])]
                            boosting.rank(vals, LIMIT)
                    print(f"  {'Python path over the pool (3 calls)':40s} {spread(wall_alternating([python_path], 3, 1)[0])}")
    ix.close()


if __name__ == "__main__":
    main()
