"""Distance matrix search on the host side: the sampling rule and the two response shapes.

Qdrant's `search_matrix_pairs` / `search_matrix_offsets`, as this project states them (parity unpinned): a SAMPLE of the
points a filter keeps, and for every sample point its nearest neighbours among the OTHER sample points (include/hx.h
"distance matrix search" states the arithmetic and the order).  The engine call takes the sample as local rows; which
rows those are is decided here, on the host, from the packed row mask:

  the rows the mask keeps, ascending (no mask: every row);
  at most `sample` of them: all of them;
  more: np.sort(np.random.default_rng(seed).choice(len(kept), size=sample, replace=False)) applied to them --
  seed = None draws fresh entropy, a given seed makes the call repeatable.

Both responses are views of one engine result: per sample point, in sample order, its neighbours best first.  Symmetric
pairs are not merged: (a, b) appears in a's list and (b, a) in b's whenever each is among the other's best."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, List, Optional, Sequence

import numpy as np

MAX_SAMPLE = 4096     # hx.h: HX_MATRIX_MAX_SAMPLE
MAX_LIMIT = 1024      # hx.h: HX_MATRIX_MAX_LIMIT


@dataclass
class MatrixPair:
    """One neighbour of the pairs form (shape-compatible with qdrant_client's SearchMatrixPair)"""
    a: Any
    b: Any
    score: float


@dataclass
class MatrixOffsets:
    """The offsets form (qdrant_client's SearchMatrixOffsetsResponse): entry k says ids[offsets_col[k]] is a neighbour of
    ids[offsets_row[k]] with scores[k]; `ids` = the sample's point ids in sample order."""
    offsets_row: List[int]
    offsets_col: List[int]
    scores: List[float]
    ids: List[Any]


def kept_rows(mask_words: Optional[np.ndarray], n_rows: int) -> np.ndarray:
    """the rows a packed mask keeps (bit r & 31 of word r >> 5 = row r), ascending; None keeps every row"""
    n_rows = int(n_rows)
    if mask_words is None:
        return np.arange(n_rows, dtype=np.int64)
    words = np.ascontiguousarray(mask_words, dtype=np.uint32)
    if words.shape[0] != (n_rows + 31) // 32:
        raise ValueError(f"mask: {words.shape[0]} words for {n_rows} rows (want {(n_rows + 31) // 32})")
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n_rows]
    return np.flatnonzero(bits).astype(np.int64)


def choose_rows(mask_words: Optional[np.ndarray], n_rows: int, sample: int, seed=None) -> np.ndarray:
    """The sample of a call: int64 local rows, ascending and distinct (the rule of the module docstring)."""
    sample = int(sample)
    if sample < 0:
        raise ValueError(f"sample must not be negative, got {sample}")
    kept = kept_rows(mask_words, n_rows)
    if len(kept) <= sample:
        return kept
    pick = np.sort(np.random.default_rng(seed).choice(len(kept), size=sample, replace=False))
    return kept[pick]


def neighbour_positions(rows: Sequence[int], nbr_rows: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """The engine's result names neighbours by row; the responses name them by their position in the sample.
    rows [S] the sample; nbr_rows [S, L] with counts [S] filled slots per line -> int64 [S, L], -1 in the empty slots."""
    pos_of = {int(r): i for i, r in enumerate(rows)}
    nbr_rows = np.asarray(nbr_rows)
    out = np.full(nbr_rows.shape, -1, dtype=np.int64)
    for i, n in enumerate(np.asarray(counts).tolist()):
        for k in range(n):
            out[i, k] = pos_of[int(nbr_rows[i, k])]
    return out


def pairs(ids: Sequence[Any], scores: np.ndarray, nbr: np.ndarray, counts: np.ndarray) -> List[MatrixPair]:
    """ids [S] the sample's point ids; scores / nbr [S, L] (nbr = positions in the sample); counts [S]"""
    sc, nb = np.asarray(scores).tolist(), np.asarray(nbr).tolist()
    return [MatrixPair(a=ids[i], b=ids[nb[i][k]], score=sc[i][k])
            for i, n in enumerate(np.asarray(counts).tolist()) for k in range(n)]


def offsets(ids: Sequence[Any], scores: np.ndarray, nbr: np.ndarray, counts: np.ndarray) -> MatrixOffsets:
    sc, nb = np.asarray(scores).tolist(), np.asarray(nbr).tolist()
    out = MatrixOffsets(offsets_row=[], offsets_col=[], scores=[], ids=list(ids))
    for i, n in enumerate(np.asarray(counts).tolist()):
        for k in range(n):
            out.offsets_row.append(i)
            out.offsets_col.append(nb[i][k])
            out.scores.append(sc[i][k])
    return out
