"""An independent numpy restatement of the contract of hx_scroll_rows / hx_payload_order, written from include/hx.h and
kept apart from rag_application_amd/scrolling.py: a full sort of (s, row) over the eligible rows."""
import numpy as np

MISSING, NULL = 0x7FF80000FFFFFFFF, 0x7FF80000FFFFFFFE
SIGN = np.uint64(1 << 63)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def bits_of(values) -> np.ndarray:
    return np.ascontiguousarray(values, np.float64).view(np.uint64).copy()


def order_s(bits, desc: bool) -> np.ndarray:
    """s of hx.h for cells given as bit patterns: b = bits of x + 0.0, u = b ^ (sign ? ~0 : 1 << 63), s = u or ~u."""
    b = np.array(bits, np.uint64, ndmin=1, copy=True)
    b[b == SIGN] = 0                                       # -0.0 + 0.0 = 0.0; nothing else changes under + 0.0 as bits
    u = np.where((b >> np.uint64(63)) != 0, b ^ ALL, b ^ SIGN)
    return (u ^ ALL) if desc else u


def s_of_value(x: float, desc: bool) -> int:
    return int(order_s(bits_of([x]), desc)[0])


def ref_scroll_rows(n, keep, start_row, limit):
    """(rows [limit] uint32, 0 past the hits; count)"""
    k = np.ones(n, bool) if keep is None else np.asarray(keep, bool)
    rows = np.flatnonzero(k & (np.arange(n) >= start_row))[:limit]
    out = np.zeros(limit, np.uint32)
    out[:rows.shape[0]] = rows
    return out, int(rows.shape[0])


def ref_payload_order(cells, keep, desc, start_from, after, limit):
    """cells: uint64 bit patterns; keep: None or bools; start_from: None or a float; after: None or (value, row).
    (rows [limit] uint32, bits [limit] uint64, count), zeros past the hits."""
    cells = np.asarray(cells, np.uint64)
    n = cells.shape[0]
    rows = np.arange(n, dtype=np.int64)
    ok = np.ones(n, bool) if keep is None else np.asarray(keep, bool).copy()
    ok &= (cells != np.uint64(MISSING)) & (cells != np.uint64(NULL))
    s = order_s(cells, desc) if n else np.zeros(0, np.uint64)
    if start_from is not None:
        ok &= s >= np.uint64(s_of_value(start_from, desc))
    if after is not None:
        sa = np.uint64(s_of_value(after[0], desc))
        ok &= (s > sa) | ((s == sa) & (rows > int(after[1])))
    idx = np.flatnonzero(ok)
    idx = idx[np.lexsort((idx, s[idx]))][:limit]
    out_rows, out_bits = np.zeros(limit, np.uint32), np.zeros(limit, np.uint64)
    out_rows[:idx.shape[0]] = idx
    out_bits[:idx.shape[0]] = cells[idx]
    return out_rows, out_bits, int(idx.shape[0])
