"""The host model of the MMR search (include/hx.h states the arithmetic): numpy float32, the
similarity by oracle.spec_dot (the reshape of section 2).  The oracle of tests/test_mmr_host.py and
tests/test_gpu_mmr.py; nothing the product imports."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

F32 = np.float32


def mmr_select(rel, rows, limit, diversity, eligible=None):
    """rel [n] = the relevance of every pool position, rows [n, dim] = its normalised fp32 row, eligible [n] bool or
    None (= every position).  Returns (positions, values): the picks in pick order and the value each was picked at.
    Step 0 values position i at a * rel_i, step t > 0 at (a * rel_i) - (d * m_i), d = float32(diversity), a = 1 - d,
    m_i = the largest spec_dot(row_i, row_s) over the picks s so far; + 0.0 makes -0 and +0 one value; the largest value
    wins, the smaller position on a tie; picking ends after `limit` picks or when no eligible position is left."""
    rel = np.ascontiguousarray(rel, dtype=F32)
    n = rel.shape[0]
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=F32)
    rows = np.ascontiguousarray(rows, dtype=F32).reshape(n, -1)
    free = np.ones(n, dtype=bool) if eligible is None else np.array(eligible, dtype=bool)
    d = F32(diversity)
    a = F32(1.0) - d
    arel = (a * rel).astype(F32)
    m = np.full(n, -np.inf, dtype=F32)
    positions, values = [], []
    for t in range(int(limit)):
        cand = np.flatnonzero(free)
        if cand.size == 0:
            break
        with np.errstate(invalid="ignore"):                 # (picked and ineligible positions: never looked at)
            v = arel if t == 0 else (arel - (d * m).astype(F32)).astype(F32)
        v = (v + F32(0.0)).astype(F32)
        s = int(cand[np.argmax(v[cand])])                   # argmax: the first of equal values
        positions.append(s)
        values.append(v[s])
        free[s] = False
        sim = O.spec_dot(rows, rows[s])
        m = np.where(sim > m, sim, m).astype(F32)
    return np.asarray(positions, dtype=np.int64), np.asarray(values, dtype=F32)
