"""Host model of the sparse IDF modifier (include/hx.h states the arithmetic).

numpy only.  It is the statement the device kernels (csrc/spstats.hip) are held to bit for bit, and the path a
CPU (gloo) shard group takes.  Every line of hx_ln / idf is one IEEE double operation: numpy's float64 arithmetic
neither fuses nor reorders them."""
from __future__ import annotations

import numpy as np

LN2 = 0.6931471805599453
SQRT_HALF = 0.7071067811865476
LN_COEF = tuple(1.0 / (2 * i + 1) for i in range(12))      # c_i = (double)(1.0 / (2 i + 1))


def hx_ln(x):
    """The project's natural logarithm of positive normal doubles (a scalar or an array; float64 out)."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)                                      # m in [0.5, 1)
    low = m < SQRT_HALF
    m = np.where(low, m * 2.0, m)
    e = np.where(low, e - 1, e)
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = np.full_like(z, LN_COEF[11])
    for i in range(10, -1, -1):
        p = p * z
        p = p + LN_COEF[i]
    t = 2.0 * s
    t = t * p
    return e.astype(np.float64) * LN2 + t


def idf(n_docs, df):
    """float32 idf of terms with document frequency df in a collection of n_docs sparse rows."""
    n = max(int(n_docs), 0)
    d = np.clip(np.asarray(df, dtype=np.int64), 0, n)
    x = 1.0 + ((n - d).astype(np.float64) + 0.5) / (d.astype(np.float64) + 0.5)
    return hx_ln(x).astype(np.float32)


def idf_weights(val, df, n_docs):
    """val * idf(n_docs, df): one fp32 multiply per position."""
    return np.asarray(val, dtype=np.float32) * idf(n_docs, df)


def term_stats_of(indptr, idx, terms):
    """(df [len(terms)] int64, N) of a document-major CSR: df = rows holding the term (term ids are unique within a
    row; a negative or absent id: 0), N = rows that are not empty."""
    indptr = np.asarray(indptr, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)[int(indptr[0]):int(indptr[-1])] if indptr.size else np.zeros(0, np.int64)
    n_docs = int((np.diff(indptr) > 0).sum()) if indptr.size else 0
    terms = np.asarray(terms, dtype=np.int64).reshape(-1)
    if idx.size == 0:
        return np.zeros(terms.shape[0], np.int64), n_docs
    uniq, counts = np.unique(idx, return_counts=True)
    pos = np.minimum(np.searchsorted(uniq, terms), uniq.shape[0] - 1)
    df = np.where((uniq[pos] == terms) & (terms >= 0), counts[pos], 0).astype(np.int64)
    return df, n_docs

