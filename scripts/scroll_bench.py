"""Diagnostic: scroll (hx_scroll_rows / hx_payload_order and their _host forms) over 10M rows with
  - `timestamp`: microseconds around 1.7e15 ascending in row order, asked newest first (desc) -- the everyday call, and the
    adversarial one for a running threshold: every row beats the rows before it;
  - `page`: about 200 values in runs (a collection ingested file by file), asked ascending -- thousands of equal cells;
  - `uniform`: uniform random doubles, asked ascending.
The index is 64-dimensional: the kernels read the planes and the mask, never a vector.  Each column unmasked and under a
random half mask, at limit 10 and 2048, ms per call, median [min-max] of 20 after 3 warm-up calls:
  order   HIP events around the enqueue-only hx_payload_order (17 launches), beside its byte floor -- three passes over the
          high-word plane, three over both planes, one count pass over both, each with n / 8 of mask when masked -- over
          the 8 TB/s HBM peak (the emit pass reads only the slices that hold a tie it takes: not counted);
  rows    HIP events around hx_scroll_rows from row 0 (floor: n / 8 of mask);
  host    the _host forms, wall clock: mask in, page out;
  topk    torch.topk (limit 10) / torch.sort (limit 2048: topk's k is capped below it on some builds) over a float64 tensor
          of the same column on the same device -- unmasked, and no row tie-break: what a caller without this engine has;
and the Python model (scrolling.ordered_rows) over the payload dicts of the first 200 000 rows, stated per row and
extrapolated: the only path the parent commit offers.  Every device page is checked against numpy's sort of the column.
Not part of bench.py.  argv: [rows (default 10M)] [kernel COLUMN].  Output: one table on stdout (kept as
profiles/scroll_*.txt).  With `kernel` and a column number (0, 1, 2) only hx_payload_order runs on that column, unmasked,
20 times at each limit: the run to put under `rocprofv3 --kernel-trace --stats`, which gives the kernels' own durations
(no launch gaps)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rag_application_amd import engine as eng, filters as F, scrolling as SC, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
KERNEL_COLUMN = int(sys.argv[3]) if len(sys.argv) > 3 and sys.argv[2] == "kernel" else None
N_PY = min(N, 200_000)
REPS, WARM = 20, 3
HBM_PEAK = 8e12


def timed(fn, wall=False):
    """ms per call (HIP events, or the wall clock around a call that ends synchronised): median, min, max"""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        if wall:
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def fmt(t):
    return f"{t[0]:7.3f} [{t[1]:.3f}-{t[2]:.3f}]"


def want_rows(vals, keep, desc, limit):
    """numpy's answer: value in the direction, then the row ascending"""
    idx = np.arange(vals.shape[0]) if keep is None else np.flatnonzero(keep)
    v = -vals[idx] if desc else vals[idx]
    if v.shape[0] > limit:                             # only the rows up to the limit-th value need the sort
        near = v <= np.partition(v, limit - 1)[limit - 1]
        idx, v = idx[near], v[near]
    return idx[np.lexsort((idx, v))[:limit]]


def main():
    ix = eng.HxIndex(64, (64,))
    ix.synth_fill(N, synth.SEED_CORPUS)
    rng = np.random.default_rng(0)
    r = np.arange(N, dtype=np.int64)
    run = max(N // 200 // 40, 1)                       # each of the 200 values comes back about 40 times
    columns = (("timestamp (ascending rows, asked desc)", 1.7e15 + r * 1000.0 + rng.integers(0, 1000, N), True),
               ("page (200 values in runs, asked asc)", (r // run % 200).astype(np.float64), False),
               ("uniform random (asked asc)", rng.random(N) * 2e6 - 1e6, False))
    half = rng.random(N) < 0.5
    words = F.pack_rows(half)
    mask_dev = torch.from_numpy(words.view(np.int32)).cuda()
    if KERNEL_COLUMN is not None:
        name, vals, desc = columns[KERNEL_COLUMN]
        c = ix.payload_create(eng.PAY_F64)
        ix.payload_append(c, np.ascontiguousarray(vals, np.float64))
        for limit in (10, 2048):                       # launches 1-20 of every kernel: limit 10, 21-40: limit 2048
            for _ in range(REPS):
                ix.payload_order(c, limit, desc=desc)
            torch.cuda.synchronize()
        print("ran 2 x", REPS, "x", name)
        ix.close()
        return
    print(f"scroll, {N} rows x 64; the half mask keeps {int(half.sum())} rows; ms per call, median [min-max] of {REPS} after "
          f"{WARM} warm-up calls; {torch.cuda.get_device_name(0)}")
    print("order = HIP events around hx_payload_order; floor = its bytes over the 8 TB/s peak; host = hx_payload_order_host, "
          "wall clock; topk = torch.topk / torch.sort of the float64 column, unmasked")
    medians = {}
    for name, vals, desc in columns:
        vals = np.ascontiguousarray(vals, np.float64)
        c = ix.payload_create(eng.PAY_F64)
        ix.payload_append(c, vals)
        t_dev = torch.from_numpy(vals).cuda()
        print(f"\n{name}")
        for limit in (10, 2048):
            if limit == 10:
                t_torch = timed(lambda: torch.topk(t_dev, limit, largest=desc))
            else:
                t_torch = timed(lambda: torch.sort(t_dev, descending=desc))
            for what, m_dev, m_host, keep in (("unmasked", None, None, None), ("half mask", mask_dev, words, half)):
                b = 3 * 4 * N + 4 * 8 * N + (7 * N / 8 if keep is not None else 0)
                t_order = timed(lambda: ix.payload_order(c, limit, desc=desc, mask=m_dev))
                t_host = timed(lambda: ix.payload_order_host(c, limit, desc=desc, mask=m_host), wall=True)
                rows, bits = ix.payload_order_host(c, limit, desc=desc, mask=m_host)
                same = np.array_equal(rows, want_rows(vals, keep, desc, limit)) and np.array_equal(bits.view(np.float64), vals[rows])
                floor_ms = b / HBM_PEAK * 1e3
                medians[(name, limit, what)] = t_order[0]
                print(f"  limit {limit:4d} {what:9s} order {fmt(t_order)}   {b / 1e6:6.1f} MB = {b / (t_order[0] * 1e-3) / 1e12:.3f} TB/s, "
                      f"floor {floor_ms:.4f} ms = {100 * floor_ms / t_order[0]:4.1f} % of the time   host {fmt(t_host)}   "
                      f"{'topk' if limit == 10 else 'sort'} {fmt(t_torch)}   equal to numpy's sort: {same}")
        ix.payload_drop(c)
        del t_dev
    print("\nspread of the three columns (largest median over smallest, same limit and mask):")
    for limit in (10, 2048):
        for what in ("unmasked", "half mask"):
            ms = [medians[(name, limit, what)] for name, _, _ in columns]
            print(f"  limit {limit:4d} {what:9s} {max(ms) / min(ms):.3f}  ({', '.join(f'{m:.3f}' for m in ms)} ms)")
    print("\nhx_scroll_rows from row 0:")
    for limit in (10, 2048):
        for what, m_dev, m_host, keep in (("unmasked", None, None, None), ("half mask", mask_dev, words, half)):
            t_rows = timed(lambda: ix.scroll_rows(limit, 0, mask=m_dev))
            t_host = timed(lambda: ix.scroll_rows_host(limit, 0, mask=m_host), wall=True)
            got = ix.scroll_rows_host(limit, N // 3, mask=m_host)
            want = (np.arange(N // 3, N) if keep is None else N // 3 + np.flatnonzero(keep[N // 3:]))[:limit]
            print(f"  limit {limit:4d} {what:9s} rows {fmt(t_rows)}   host {fmt(t_host)}   equal to numpy's: {np.array_equal(got, want)}")
    # the Python model over the payload dicts of the first N_PY rows
    print(f"\nthe Python model (scrolling.ordered_rows) at {N_PY} rows of the same table:")
    for name, vals, desc in columns:
        pays = [{"k": float(v)} for v in np.asarray(vals[:N_PY], np.float64)]
        for what, keep in (("unmasked", None), ("half mask", half[:N_PY])):
            t0 = time.perf_counter()
            SC.ordered_rows(pays, "k", desc, keep=keep, limit=10)
            dt = time.perf_counter() - t0
            print(f"  {name[:22]:22s} {what:9s} {dt:7.3f} s = {dt / N_PY * 1e6:5.2f} us per row -> {dt / N_PY * N:7.1f} s at {N} rows (extrapolated)")
    ix.close()


if __name__ == "__main__":
    main()
