"""Caller-defined query trees: the general form of the reference's call,
client.query_points(prefetch=[...], query=..., using=..., limit=...), parsed into a *shape* (the tree without its
vectors) and run for B queries of one shape at once over the engine's stage entries.

A request is a dict, or an object with attributes of the same names (qdrant_client's Prefetch / QueryRequest fit):
  nearest node  query = a dense vector, or a sparse one ({"indices", "values"} or .indices / .values); using = "dense",
                "matryoshka_<d>", "quantized", "sparse" or "binary".  Without prefetch: a whole-collection search.  With
                prefetch: the union of the children's lists re-scored by the named vector ("dense" and "matryoshka_<d>"
                only).  "binary"  takes a dense vector and ranks by the sign bits of a collection
                created with binary_quantization=True: the leaf under a dense re-scoring node is Qdrant's
                BinaryQuantization with oversampling and rescore (handler.search_binary builds exactly that).
                "binary_scalar4bits" / "binary_scalar8bits"  are the same leaf with Qdrant's
                query_encoding: the rows stay at one bit, the query keeps 4 or 8 bits per dimension.
  fusion node   query = {"fusion": "rrf" | "dbsf"} with optional "weights", "rrf_k", "rank_base"; 1 to 8 prefetches.
A missing limit is 10, at the root too.  Everything else raises ValueError with the reason: nothing is answered with
something else.

Node filters (parse_nodes): every node may carry "filter" (or "filters") and "score_threshold".  Such
a node is wrapped in the shape as ("keep", filter key | None, has threshold, limit, (node,)) -- the key is
filters.filter_key's canonical JSON, the threshold's VALUE travels with the vectors -- and run() serves it with the masked
stage entries and stages.keep (hx_list_keep).  A tree without any of them has the shape parse gives it."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import filters as _filters
from . import fusion as _fusion

PREFETCH_DEFAULT_LIMIT = 10
MAX_DEPTH = 8
MAX_LIMIT = 2048                 # the largest list a stage keeps (hx.h)
RESCORE_MAX = 8192               # the widest candidate list hx_rescore takes
USINGS = ("dense", "quantized", "sparse", "binary", "binary_scalar4bits", "binary_scalar8bits")
# the leaves over the 1-bit copy: using -> the query's bits per dimension (None: the sign alone, hx_search_bin)
BINARY_USINGS = {"binary": None, "binary_scalar4bits": 4, "binary_scalar8bits": 8}
# Qdrant's BinaryQuantization.query_encoding -> the leaf
QUERY_ENCODINGS = {"binary": "binary", "scalar4bits": "binary_scalar4bits", "scalar8bits": "binary_scalar8bits"}
NODE_KEYS = ("prefetch", "query", "using", "limit", "filter", "score_threshold", "params", "lookup_from")
# what Qdrant's query interface also offers and a tree here does not
FOREIGN_QUERIES = ("order_by", "recommend", "discover", "context", "formula", "mmr", "sample")
_MISSING = object()


def _get(node, name, default=None):
    if isinstance(node, dict):
        return node.get(name, default)
    return getattr(node, name, default)


def _is_sparse(q) -> bool:
    if isinstance(q, dict):
        return "indices" in q and "values" in q
    return hasattr(q, "indices") and hasattr(q, "values")


def _fusion_of(q):
    """(method name, the query object) when q is a fusion query, else None"""
    f = _get(q, "fusion", _MISSING) if (isinstance(q, dict) or hasattr(q, "fusion")) else _MISSING
    if f is _MISSING or f is None:
        return None
    return str(getattr(f, "value", f)).lower()


def _limit(node, where: str) -> int:
    limit = _get(node, "limit")
    if limit is None:
        return PREFETCH_DEFAULT_LIMIT
    if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or not 1 <= int(limit) <= MAX_LIMIT:
        raise ValueError(f"{where}: limit must be an integer in [1, {MAX_LIMIT}], got {limit!r}")
    return int(limit)


def _dense(q, using: str, prefix: int, dim: int, where: str) -> np.ndarray:
    try:
        v = np.asarray(q, dtype=np.float32).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{where}: the query of a nearest node is a vector of numbers or a sparse vector") from None
    if not np.isfinite(v).all():
        raise ValueError(f"{where}: query vector values must be finite")
    if prefix and v.shape[0] == prefix:                      # the prefix stage reads the first d values only
        v = np.concatenate([v, np.zeros(dim - prefix, dtype=np.float32)])
    if v.shape[0] != dim:
        want = f"{prefix} or {dim}" if prefix else f"{dim}"
        raise ValueError(f"{where}: a query of {v.shape[0]} values under using={using!r}, want {want}")
    return v


def _sparse(q, where: str):
    idx, val = (q["indices"], q["values"]) if isinstance(q, dict) else (q.indices, q.values)
    try:
        idx = np.asarray(list(idx), dtype=np.int64).reshape(-1)
        val = np.asarray(list(val), dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{where}: a sparse query holds integer indices and numeric values") from None
    if idx.shape[0] != val.shape[0]:
        raise ValueError(f"{where}: a sparse query needs as many values as indices")
    if idx.size and (idx.min() < -2 ** 31 or idx.max() >= 2 ** 31):
        raise ValueError(f"{where}: sparse index out of range")
    if not np.isfinite(val).all():
        raise ValueError(f"{where}: sparse query values must be finite")
    return idx.astype(np.int32), val.astype(np.float32)


def parse(node, dim: int, msizes: Sequence[int], _depth: int = 1, _root: bool = True, _vecs: Optional[list] = None,
          _notes: Optional["_Notes"] = None):
    """A request -> (shape, vectors).  shape: ("nearest", using, prefix, limit, children) or ("fusion", method, weights,
    rrf_k, rank_base, limit, children), hashable; vectors: the nearest nodes' queries in pre-order, a float32 [dim] array
    or an (indices int32, values float32) pair each.  The root's filter and score_threshold are the caller's business
    (handler.query_points); below the root both are refused.  (_notes: parse_nodes' mode, where every node takes both.)"""
    where = "query_points" if _root else f"prefetch (depth {_depth})"
    vecs = [] if _vecs is None else _vecs
    if _depth > MAX_DEPTH:
        raise ValueError(f"a query tree is at most {MAX_DEPTH} levels deep")
    if node is None or isinstance(node, (str, bytes, int, float, list, tuple, np.ndarray)):
        raise ValueError(f"{where}: a node is a dict or an object with prefetch / query / using / limit")
    if isinstance(node, dict):
        allowed = NODE_KEYS + (("filters", "with_payload", "with_vector") if _root else
                               ("filters",) if _notes is not None else ())
        unknown = [k for k in node if k not in allowed]
        if unknown:
            raise ValueError(f"{where}: unknown field(s) {unknown}")
    if not _root and _notes is None:
        if _get(node, "filter") is not None or _get(node, "filters") is not None:
            raise ValueError(f"{where}: a filter inside a prefetch is not supported (the stage entries take no mask); "
                             "filter at the root")
        if _get(node, "score_threshold") is not None:
            raise ValueError(f"{where}: score_threshold belongs to the root")
    if _get(node, "lookup_from") is not None:
        raise ValueError(f"{where}: lookup_from is not supported")
    q = _get(node, "query")
    if q is None:
        raise ValueError(f"{where}: a node needs a query (a vector or a fusion)")
    if isinstance(q, (dict,)) and "nearest" in q:            # NearestQuery(nearest=vector)
        if q.get("mmr") is not None:
            raise ValueError(f"{where}: an MMR query cannot be part of a tree (hybrid_search_mmr reranks a pool)")
        q = q["nearest"]
    elif not isinstance(q, dict) and hasattr(q, "nearest"):
        if getattr(q, "mmr", None) is not None:
            raise ValueError(f"{where}: an MMR query cannot be part of a tree (hybrid_search_mmr reranks a pool)")
        q = q.nearest
    for name in FOREIGN_QUERIES:
        if (isinstance(q, dict) and name in q) or (not isinstance(q, (dict, list, tuple, np.ndarray)) and hasattr(q, name)):
            raise ValueError(f"{where}: a {name} query cannot be part of a tree")
    if isinstance(q, (str, bytes, int, np.integer)) and not isinstance(q, bool):
        raise ValueError(f"{where}: a query by point id cannot be part of a tree")
    pre = _get(node, "prefetch")
    if pre is None:
        pre = []
    elif isinstance(pre, dict) or not isinstance(pre, (list, tuple)):
        pre = [pre]
    limit = _limit(node, where)
    wrap = (lambda shape: shape) if _notes is None else _notes.take(node, where, _root, limit)
    method = _fusion_of(q)
    if method is not None:
        if isinstance(q, dict):
            unknown = [k for k in q if k not in ("fusion", "weights", "rrf_k", "rank_base")]
            if unknown:
                raise ValueError(f"{where}: unknown field(s) {unknown} in a fusion query")
        if method not in _fusion.METHODS:
            raise ValueError(f"{where}: fusion must be one of {tuple(_fusion.METHODS)}, got {method!r}")
        if not 1 <= len(pre) <= _fusion.MAX_LISTS:
            raise ValueError(f"{where}: a fusion takes 1 to {_fusion.MAX_LISTS} prefetches, got {len(pre)}")
        rrf_k = _get(q, "rrf_k")
        rank_base = _get(q, "rank_base")
        rrf_k = _fusion.RRF_K if rrf_k is None else rrf_k
        rank_base = _fusion.RRF_RANK_BASE if rank_base is None else rank_base
        if isinstance(rrf_k, bool) or not isinstance(rrf_k, (int, float, np.integer, np.floating)):
            raise ValueError(f"{where}: rrf_k must be a number")
        if isinstance(rank_base, bool) or not isinstance(rank_base, (int, np.integer)):
            raise ValueError(f"{where}: rank_base must be an integer")
        children = tuple(parse(c, dim, msizes, _depth + 1, False, vecs, _notes)[0] for c in pre)
        try:
            code, w = _fusion.check(method, [c[-2] for c in children], _get(q, "weights"), limit, rrf_k, rank_base)
        except ValueError as e:
            raise ValueError(f"{where}: {e}") from None
        weights = None if _get(q, "weights") is None else tuple(float(x) for x in w)
        if code != _fusion.RRF:                              # DBSF ignores both: one shape whatever they are
            rrf_k, rank_base = _fusion.RRF_K, _fusion.RRF_RANK_BASE
        return wrap(("fusion", code, weights, float(np.float32(rrf_k)), int(rank_base), limit, children)), vecs
    # a nearest node
    using = _get(node, "using")
    using = "dense" if using is None else using
    prefix = 0
    if isinstance(using, str) and using.startswith("matryoshka_"):
        try:
            prefix = int(using[len("matryoshka_"):])
        except ValueError:
            prefix = -1
        if prefix not in tuple(msizes):
            raise ValueError(f"{where}: using={using!r}, but the collection's matryoshka sizes are {tuple(msizes)}")
    elif using not in USINGS:
        raise ValueError(f"{where}: using must be 'dense', 'matryoshka_<d>', 'quantized', 'sparse' or 'binary', got {using!r}")
    if _is_sparse(q):
        if using != "sparse":
            raise ValueError(f"{where}: a sparse query needs using='sparse', got {using!r}")
        vec = _sparse(q, where)
    else:
        if isinstance(q, dict) or not isinstance(q, (list, tuple, np.ndarray)) and not hasattr(q, "__iter__"):
            raise ValueError(f"{where}: unknown query {type(q).__name__}: a vector, a sparse vector or a fusion")
        if using == "sparse":
            raise ValueError(f"{where}: using='sparse' needs a sparse query ({{'indices', 'values'}})")
        vec = _dense(q, using, prefix, dim, where)
    if pre and (using in ("quantized", "sparse") or using in BINARY_USINGS):
        raise ValueError(f"{where}: using={using!r} cannot re-score a prefetch (only 'dense' and 'matryoshka_<d>' can)")
    vecs.append(vec)
    children = tuple(parse(c, dim, msizes, _depth + 1, False, vecs, _notes)[0] for c in pre)
    if sum(c[-2] for c in children) > RESCORE_MAX:
        raise ValueError(f"{where}: the prefetches hold {sum(c[-2] for c in children)} candidates together, the "
                         f"re-scoring stage takes at most {RESCORE_MAX}")
    return wrap(("nearest", using, prefix, limit, children)), vecs


class _Notes:
    """What parse_nodes collects while parse walks a request: the thresholds of the nodes that have one, in pre-order, and
    the filters by their canonical key."""

    def __init__(self, check_filter, prefetch_filters: bool):
        self.check_filter, self.prefetch_filters = check_filter, prefetch_filters
        self.thresholds: List[np.float32] = []
        self.filters: Dict[str, Any] = {}

    def take(self, node, where: str, root: bool, limit: int):
        """Validates the node's filter and score_threshold (called before the node's children are parsed, so the
        thresholds are in pre-order) and returns the wrapper of its shape."""
        flt = _get(node, "filters")
        if flt is None:
            flt = _get(node, "filter")
        thr = _get(node, "score_threshold")
        if flt:
            if not root and not self.prefetch_filters:
                raise ValueError(f"{where}: filter_stages='all' pushes the root's filters into every leaf; a filter inside "
                                 "a prefetch needs filter_stages='node'")
            if not isinstance(flt, dict):
                raise ValueError(f"{where}: a filter is a dict of must / should / must_not clauses")
            if self.check_filter is not None:
                try:
                    self.check_filter(flt)
                except ValueError as e:
                    raise ValueError(f"{where}: {e}") from None
        if thr is not None and (isinstance(thr, bool) or not isinstance(thr, (int, float, np.integer, np.floating))
                                or thr != thr):
            raise ValueError(f"{where}: score_threshold must be a number, got {thr!r}")
        key = None
        if flt:
            key = _filters.filter_key(flt)
            self.filters[key] = flt
        if thr is not None:
            self.thresholds.append(np.float32(thr))
        if key is None and thr is None:
            return lambda shape: shape
        return lambda shape: ("keep", key, thr is not None, limit, (shape,))


def parse_nodes(node, dim: int, msizes: Sequence[int], check_filter=None, prefetch_filters: bool = True):
    """parse() in node-filter mode: a request -> (shape, vectors, thresholds, filters).  Every node, the root included (its
    "filters" / "score_threshold" are the request's), may carry a filter and a threshold; a node that does is wrapped as
    ("keep", filter key | None, has threshold, limit, (node,)).  thresholds: the float32 values of the nodes that have
    one, in pre-order; filters: {filter key: the filter}.  check_filter(flt) validates a filter's clauses (ValueError;
    by default the clause check of filters.matches, the handler's); prefetch_filters=False refuses a filter below the
    root (handler: filter_stages="all")."""
    if check_filter is None:
        check_filter = lambda flt: _filters.matches({}, flt)
    notes = _Notes(check_filter, prefetch_filters)
    shape, vecs = parse(node, dim, msizes, _notes=notes)
    return shape, vecs, notes.thresholds, notes.filters


def push_to_leaves(shape):
    """filter_stages="all": the root's filter moves into every leaf (every list above the leaves then holds kept rows
    only); the root keeps its threshold.  A shape whose root carries no filter comes back as it is."""
    if shape[0] != "keep" or shape[1] is None:
        return shape
    _, key, has_thr, limit, (inner,) = shape

    def push(s):
        if s[0] == "keep":
            node = push(s[-1][0])
            if node[0] == "keep":                            # a leaf, wrapped below: the threshold joins its wrapper
                return ("keep", node[1], s[2], s[3], node[-1])
            return s[:-1] + ((node,),)
        if not s[-1]:
            return ("keep", key, False, s[-2], (s,))
        return s[:-1] + (tuple(push(c) for c in s[-1]),)

    pushed = push(inner)
    if not has_thr:
        return pushed
    if pushed[0] == "keep":                                  # the root is a leaf
        return ("keep", pushed[1], True, limit, pushed[-1])
    return ("keep", None, True, limit, (pushed,))


def uses_binary(shape) -> bool:
    """whether some leaf of the shape ranks by the 1-bit copy, which the collection must then keep: using="binary" or
    one of its query encodings"""
    if shape[0] == "nearest" and shape[1] in BINARY_USINGS:
        return True
    return any(uses_binary(c) for c in shape[-1])


def binary_request(vector, limit=10, oversampling=4.0, rescore=True, filters=None, query_encoding="binary"):
    """The request of handler.search_binary -- Qdrant's QuantizationSearchParams(oversampling, rescore) -- for one query
    vector: a using="binary" leaf of min(ceil(limit * oversampling), 2048) hits under a dense re-scoring node of `limit`,
    or with rescore=False the leaf alone at `limit`.  `filters` becomes the root's.  query_encoding -- Qdrant's
    BinaryQuantization.query_encoding: "binary" (the default: the request is what it was), "scalar4bits" or "scalar8bits"
    -- names the leaf: using="binary_scalar4bits" / "binary_scalar8bits".  ValueError for a limit outside [1, 2048], for an
    oversampling that is no finite number >= 1 and for an unknown query_encoding."""
    if not isinstance(query_encoding, str) or query_encoding not in QUERY_ENCODINGS:
        raise ValueError(f"search_binary: query_encoding must be one of {tuple(QUERY_ENCODINGS)}, got {query_encoding!r}")
    if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or not 1 <= int(limit) <= MAX_LIMIT:
        raise ValueError(f"search_binary: limit must be an integer in [1, {MAX_LIMIT}], got {limit!r}")
    if isinstance(oversampling, bool) or not isinstance(oversampling, (int, float, np.integer, np.floating)):
        raise ValueError(f"search_binary: oversampling must be a number, got {oversampling!r}")
    if not np.isfinite(oversampling) or oversampling < 1:
        raise ValueError(f"search_binary: oversampling must be finite and at least 1, got {oversampling!r}")
    limit = int(limit)
    leaf = {"using": QUERY_ENCODINGS[query_encoding], "query": vector}
    if rescore:
        wide = min(int(np.ceil(limit * float(oversampling))), MAX_LIMIT)
        req = {"using": "dense", "query": vector, "limit": limit, "prefetch": [dict(leaf, limit=max(wide, limit))]}
    else:
        req = dict(leaf, limit=limit)
    if filters:
        req["filters"] = filters
    return req


def shape_limit(shape) -> int:
    return shape[-2]


def input_width(shape) -> int:
    """The candidates a node with prefetches sees: the sum of its children's limits (0 for a leaf)."""
    return sum(shape_limit(c) for c in shape[-1])


def group_by_shape(shapes: Sequence[Any]) -> Dict[Any, List[int]]:
    """shape -> the positions of the requests that have it, in request order (dicts keep insertion order)."""
    groups: Dict[Any, List[int]] = {}
    for i, s in enumerate(shapes):
        groups.setdefault(s, []).append(i)
    return groups


def batch_vectors(vector_lists: Sequence[Sequence[Any]]) -> List[Any]:
    """The vectors of B requests of one shape -> per nearest node (pre-order) a float32 [B, dim] array or a list of B
    (indices, values) pairs."""
    out = []
    for slot in zip(*vector_lists):
        out.append(list(slot) if isinstance(slot[0], tuple) else np.stack(slot).astype(np.float32, copy=False))
    return out


def batch_thresholds(threshold_lists: Sequence[Sequence[Any]]) -> List[np.ndarray]:
    """The thresholds of B requests of one shape (parse_nodes) -> per node that has one (pre-order) a float32 [B] array."""
    return [np.asarray(slot, dtype=np.float32) for slot in zip(*threshold_lists)]


def run(shape, vectors: Sequence[Any], stages, root_limit: Optional[int] = None, thresholds: Sequence[Any] = ()):
    """Run one shape for the B queries whose vectors are `vectors` (batch_vectors).  `stages` offers the stage entries:
    dense(Q, limit, prefix), i8(Q, limit), sparse(pairs, limit), bin(Q, limit) (only a shape with a using="binary" leaf
    calls it), bin_asym(Q, limit, query_bits) (only one with a "binary_scalar4bits" / "binary_scalar8bits" leaf),
    rescore(Q, [(keys, counts)], limit, prefix) and
    fuse([(keys, counts)], method, weights, limit, rrf_k, rank_base), each returning (keys [B, limit], counts [B]) in
    whatever array type it keeps lists in -- they stay where the stages put them between nodes.  root_limit overrides
    the root's limit (a filtered root runs at the width of its input).

    A ("keep", filter key, has threshold, limit, (node,)) wrapper (parse_nodes; thresholds = batch_thresholds) asks more
    of `stages`: the leaf stages called with mask=<filter key> (the best `limit` among the rows the filter keeps), and
    keep(lists_or_list, mask, thresholds, limit) -- one (keys, counts) list, or several taken side by side, walked in rank
    order and cut to the first `limit` slots whose row the mask keeps and whose score is not below the query's threshold.
      leaf           the masked stage; a threshold: keep behind it;
      re-scoring     a filter: keep(mask) over the children's lists at the union's full width, BEFORE the re-score, so no
                     hit is lost to the widest list a stage keeps; a threshold: keep behind the re-score;
      fusion         a filter: the fusion at min(the children's limits together, 2048), then ONE keep (mask and threshold)
                     down to `limit` -- filtering the inputs would change the ranks the fusion reads; a threshold alone:
                     keep behind the fusion at `limit` (its scores descend, so the cut commutes).
    A node without a wrapper calls the stages exactly as before."""
    cursor, tcursor = [0], [0]
    begin = getattr(stages, "begin_run", None)
    if begin is not None:
        begin()

    def leaf(using, prefix, q, limit, **mask):
        if using == "sparse":
            return stages.sparse(q, limit, **mask)
        if using == "quantized":
            return stages.i8(q, limit, **mask)
        if using == "binary":
            return stages.bin(q, limit, **mask)
        if using in BINARY_USINGS:
            return stages.bin_asym(q, limit, BINARY_USINGS[using], **mask)
        return stages.dense(q, limit, prefix, **mask)

    def walk(s, limit=None, key=None, thr=None):
        limit = shape_limit(s) if limit is None else limit
        if s[0] == "keep":
            _, key, has_thr, _, (inner,) = s
            if has_thr:
                thr = thresholds[tcursor[0]]
                tcursor[0] += 1
            return walk(inner, limit, key, thr)
        if s[0] == "fusion":
            _, method, weights, rrf_k, rank_base, _, children = s
            lists = [walk(c) for c in children]
            if key is not None:
                wide = min(sum(shape_limit(c) for c in children), MAX_LIMIT)
                return stages.keep(stages.fuse(lists, method, weights, wide, rrf_k, rank_base), key, thr, limit)
            out = stages.fuse(lists, method, weights, limit, rrf_k, rank_base)
            return out if thr is None else stages.keep(out, None, thr, limit)
        _, using, prefix, _, children = s
        q = vectors[cursor[0]]
        cursor[0] += 1
        if children:
            lists = [walk(c) for c in children]
            if key is not None:
                lists = [stages.keep(lists, key, None, sum(shape_limit(c) for c in children))]
            out = stages.rescore(q, lists, limit, prefix)
        else:
            out = leaf(using, prefix, q, limit) if key is None else leaf(using, prefix, q, limit, mask=key)
        return out if thr is None else stages.keep(out, None, thr, limit)

    return walk(shape, root_limit)


class DeviceStages:
    """The stage entries of one engine index (engine.HxIndex), lists as int64 device tensors."""

    def __init__(self, index, engine, sparse_modifier=None, masks=None):
        import torch
        self.ix, self.eng, self.torch = index, engine, torch
        self.sparse_modifier = sparse_modifier          # the collection's (handler.create_collection): None | "idf"
        self.dev = index._tdev
        self.masks = masks                              # filter key -> the packed row mask (uint32 words, host)
        self._dev_masks: Dict[str, Any] = {}            # ... on the device: every distinct mask is uploaded once per run

    def begin_run(self):
        self._dev_masks = {}

    def _kw(self, key):
        """the keyword a masked stage call adds (an unmasked one is called exactly as before)"""
        return {} if key is None else {"mask": self._mask(key)}

    def _mask(self, key):
        if key is None:
            return None
        words = self._dev_masks.get(key)
        if words is None:
            if self.masks is None:
                raise ValueError("a node filter needs DeviceStages(masks=...): filter key -> packed row mask")
            host = np.ascontiguousarray(self.masks(key), dtype=np.uint32)
            words = self._dev_masks[key] = self.torch.from_numpy(host.view(np.int32)).to(self.dev)
        return words

    def _q(self, Q):
        return self.torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).to(self.dev)

    def dense(self, Q, limit, prefix, mask=None):
        return self.ix.search_dense(self._q(Q), limit, prefix, **self._kw(mask))

    def i8(self, Q, limit, mask=None):
        return self.ix.search_i8(self._q(Q), limit, **self._kw(mask))

    def bin(self, Q, limit, mask=None):
        return self.ix.search_bin(self._q(Q), limit, **self._kw(mask))

    def bin_asym(self, Q, limit, query_bits, mask=None):
        return self.ix.search_bin_asym(self._q(Q), limit, query_bits, **self._kw(mask))

    def keep(self, lists, mask, thresholds, limit):
        # several lists: side by side, every slot walked (a stage's slots past its count are 0, and hx_list_keep skips a 0)
        if isinstance(lists, tuple):
            keys, counts = lists
        elif len(lists) == 1:
            keys, counts = lists[0]
        else:
            keys, counts = self.torch.cat([k for k, _ in lists], dim=1), None
        return self.ix.list_keep(keys, counts, limit, mask=self._mask(mask), thresholds=thresholds)

    def sparse(self, pairs, limit, mask=None):
        t = self.torch
        indptr = np.zeros(len(pairs) + 1, dtype=np.int64)
        np.cumsum([len(i) for i, _ in pairs], out=indptr[1:])
        idx = np.concatenate([i for i, _ in pairs]).astype(np.int32) if indptr[-1] else np.zeros(0, np.int32)
        val = np.concatenate([v for _, v in pairs]).astype(np.float32) if indptr[-1] else np.zeros(0, np.float32)
        d_idx, d_val = t.from_numpy(idx).to(self.dev), t.from_numpy(val).to(self.dev)
        if self.sparse_modifier == "idf":               # Modifier.IDF: scaled on the device, no host round trip -- by the
            d_val = self.ix.sparse_idf(d_idx, d_val)    # statistics of the WHOLE collection, whatever the mask keeps
        return self.ix.search_sparse(t.from_numpy(indptr).to(self.dev), d_idx, d_val, limit, **self._kw(mask))

    def rescore(self, Q, lists, limit, prefix):
        # a stage's slots past its count are 0, and hx_rescore skips a 0: the union is the lists side by side
        if len(lists) == 1:
            return self.ix.rescore(self._q(Q), lists[0][0], lists[0][1], limit, prefix)
        return self.ix.rescore(self._q(Q), self.torch.cat([k for k, _ in lists], dim=1), None, limit, prefix)

    def fuse(self, lists, method, weights, limit, rrf_k, rank_base):
        return self.eng.fuse([k for k, _ in lists], [c for _, c in lists], method, weights, limit, rrf_k, rank_base)

    @staticmethod
    def to_host(keys, counts) -> Tuple[np.ndarray, np.ndarray]:
        return keys.cpu().numpy().view(np.uint64), counts.cpu().numpy()
