"""Random lifecycle sequences against a host model of the index (DESIGN.md sections 1a, 14, 18): the model, the
generator and the driver.  Shared by tests/test_lifecycle_model_host.py (the driver on a CPU fake, the coverage table,
the brute-force restatement) and tests/test_gpu_lifecycle_sequences.py (the driver on HxIndex).  No GPU code is
imported here.

The MODEL holds what an index carries from one call to the next as far as a caller can observe it: the stored rows as
corpus row numbers into a pool (`Pool`, a `Corpus` of tests/test_gpu_prefilter.py with its own width) -- one number for
the dense vector, one for the sparse vector (-1 = none), because the dense-only replace separates them --, how many
leading rows have a sparse row (sp_rows), every payload column (`ModelPay`: the host models of the payload helpers plus
truncate, replace and the reset of a load) and the inverted index as finalize()'s rule gives it (base / tail documents,
stale or not), from which stats()["n_segments"] follows.

A search finalizes the inverted index, so WHETHER a step is followed by the searching part of `check` belongs to the
sequence: every op carries a `search` flag.  Without it no op would ever meet a stale or never-built inverted index.
Everything else of `check` runs after every op -- the 1-bit copy of the rows (`Model.bin_on`, the touch form
binary_enable) and the Hamming scan stage among it: they do not touch the inverted index.  The term statistics
(hx_sparse_idf_host finalizes) are read in the searching part."""
from __future__ import annotations

import os

import numpy as np

from oracle import oracle as O
from rag_application_amd import filters as F
from rag_application_amd import payload_index as PI
from tests import binary_helpers as BH
from tests import sparse_idf_helpers as SH
from tests.payload_helpers import U32_NULL, random_filter
from tests.payload_list_helpers import PAY_LIST_F64, PAY_LIST_U32, ListCol, list_filter
from tests.payload_text_helpers import PAY_TEXT, FakeTextIndex, TextCol, interp_text, text_filter, text_table
from tests.test_gpu_delete import same
from tests.test_gpu_prefilter import Corpus, P

MS = (64,)
MODES = ("tree", "h1")
N_QUERIES = 8
SEG_DOCS, TAIL_MIN = 32768, 1 << 18                 # kernels.hpp SEG_DOCS_SMALL; finalize()'s floor of the tail rule
# one key of each of the five column kinds (the tables of tests/payload_text_helpers.py hold them all)
PAY_KEYS = {"kw": "keyword", "num": "number", "langs": "keyword_list", "nums": "number_list", "body": "text"}
PAY_POOL = 1500
ADD_SIZES = (1, 3, 64, 257, 1500)
RETAIN_FORMS = ("keep50", "keep90", "keep99", "row0", "last", "middle", "all", "none")
TRUNCATE_FORMS = ("n", "n-1", "tail", "below_base", "zero")
TOUCH_FORMS = ("finalize", "rebuild_sparse", "search", "masked_search", "set_dense_candidates", "binary_enable")
REFUSED_FORMS = ("mask_length", "duplicate_row", "append_past_count", "nan_add", "repeated_term")
MUTATING = ("add", "retain", "replace_sparse", "replace_dense", "truncate")
INV_STATES = ("never", "stale", "base", "base+tail")

_common = dict(dim=128, start=(0, 3000), max_rows=6000, pool=16000, env={}, cand="i8", oracle="all", gentle=False,
               dense_adds=False, weight={}, binary=False)
PROFILES = {
    "small": dict(_common, n_ops=30, seeds=(9, 13, 33, 35, 42, 82, 88, 95)),
    "padded": dict(_common, dim=100, n_ops=20, seeds=(6, 25)),
    "chunked": dict(_common, n_ops=20, seeds=(18, 20), env={"HX_DEBUG_COMPACT_CHUNK": "64"}),
    "segments": dict(_common, n_ops=10, seeds=(57,), start=(34000, 34001), max_rows=40000, pool=52000, oracle="ends",
                     gentle=True, env={"HX_DEBUG_SEG_DOCS": "32768", "HX_DEBUG_TAIL_MIN": "2000"}),
    "trailing_dense": dict(_common, n_ops=15, seeds=(284,), dense_adds=True, gentle=True,
                           weight=dict(pay=0.25, refused=0.5)),
    "fp16_only": dict(_common, n_ops=15, seeds=(1,), cand="f16", env={"HX_DENSE_CAND": "f16"}),
    # the 1-bit copy: enabled at a random step, dropped by every load; save / load come more often
    "binary": dict(_common, n_ops=20, seeds=(1, 2), binary=True, weight=dict(save_load=2.5, touch=1.5)),
    "binary_padded": dict(_common, dim=100, n_ops=20, seeds=(1, 2), binary=True, weight=dict(save_load=2.5, touch=1.5)),
    # ... and the Hamming scan in several chunks with compactions and the overflow redo at a few hundred rows
    "binary_chunks": dict(_common, n_ops=20, seeds=(1, 2), binary=True, weight=dict(save_load=2.5, touch=1.5),
                          env={"HX_DEBUG_BIN_CHUNK0": "96", "HX_DEBUG_BIN_CAP": "64", "HX_DEBUG_COMPACT_CHUNK": "64"}),
}
# the generator's stream of a profile is seeded by this number, not by the profile's place in PROFILES: a new profile
# leaves the committed sequences of the others as they are (tests/test_lifecycle_model_host.py pins their op logs)
PROFILE_IDS = dict(chunked=0, fp16_only=1, padded=2, segments=3, small=4, trailing_dense=5, binary=6, binary_padded=7,
                   binary_chunks=8)
CASES = [(seed, name) for name, p in PROFILES.items() for seed in p["seeds"]]


# ---- the pool -----------------------------------------------------------------------------------------------------------
class Pool(Corpus):
    """a Corpus of `dim`-wide rows; csr() and oracle() take sparse row numbers with -1 = no sparse vector"""

    def __init__(self, n, tables, dim):
        # A scan prunes by per-tile maxima (256 rows) of two per-row factors, cached until the row count changes: the
        # scale of the int8 candidate copy, taken from the NORMALISED row (its peak-to-norm ratio), and 1 / |q8 row| of
        # the "quantized" stage.  Both must differ from TILE to tile, or stale maxima equal fresh ones: every second
        # block of 256 pool rows is spiky (one element 12 times larger: peak / norm about 0.8 against 0.25), and the
        # length goes with the block too.  Adds take consecutive pool rows, so stored tiles inherit the blocks.
        X = O.synth_dense(O.SEED_CORPUS, 0, n, dim)
        r = np.arange(n)
        self.spiky = (r // 256) % 2 == 1
        X[r[self.spiky], r[self.spiky] % dim] = np.float32(4.0) * np.abs(X[self.spiky]).max(axis=1)
        X *= (np.float32(4.0) ** ((r // 256 * 3 % 5) - 2))[:, None].astype(np.float32)
        super().__init__(n, tables, X=X)
        self.dim = dim
        self.lens = np.diff(self.ip).astype(np.int64)

    def csr(self, srow):
        """the CSR of the listed sparse rows in their order, -1 = an empty document"""
        srow = np.asarray(srow, np.int64)
        lens = np.where(srow >= 0, self.lens[np.maximum(srow, 0)], 0)
        ip = np.zeros(len(srow) + 1, np.int64)
        np.cumsum(lens, out=ip[1:])
        start = np.repeat(self.ip[np.maximum(srow, 0)], lens)
        take = start + (np.arange(ip[-1]) - np.repeat(ip[:-1], lens))
        return ip, self.si[take].astype(np.int32), self.sv[take].astype(np.float32)

    def oracle(self, xrow, srow=None):
        ora = O.OracleIndex(self.dim, MS)
        ip, si, sv = self.csr(xrow if srow is None else srow)
        ora.add(self.X[xrow], ip, si.astype(np.int64), sv)
        ora.finalize()
        return ora


_pools, _pays = {}, {}


def pool_of(profile, tables):
    p = PROFILES[profile]
    key = (p["dim"], p["pool"])
    if key not in _pools:
        _pools[key] = Pool(p["pool"], tables, p["dim"])
    return _pools[key]


def pool_lens(profile, tables):
    """the document lengths of the pool alone: all the generator needs"""
    n = PROFILES[profile]["pool"]
    if ("lens", n) not in _pools:
        _pools[("lens", n)] = np.diff(O.synth_sparse_docs(O.SEED_SPDOC, 0, n, tables)[0]).astype(np.int64)
    return _pools[("lens", n)]


def payloads():
    """(payload pool, a PayloadIndex whose keyword dictionaries already hold every word of the pool: the codes of a
    cell do not depend on the order of the ops)"""
    if not _pays:
        _, pays = text_table(PAY_POOL, seed=7)
        pidx = PI.PayloadIndex()
        for key, schema in PAY_KEYS.items():
            pidx.keys[key] = PI._Key(schema)
            assert pidx.encode(key, pays) is not None, key
        _pays["v"] = (pays, pidx)
    return _pays["v"]


def queries(dim, tables):
    Q = O.synth_dense(O.SEED_QUERY, 0, N_QUERIES, dim)
    qip, qsi, qsv = O.synth_sparse_queries(O.SEED_SPQUERY, 0, N_QUERIES, tables)
    return Q, qip, qsi.astype(np.int32), qsv.astype(np.float32)


# ---- payload columns ---------------------------------------------------------------------------------------------------
def _list_col(kind, cells):
    c = ListCol(kind)
    c.heads = np.array([h if h >= U32_NULL else 0 for h, _ in cells], np.uint32)
    c.off = np.concatenate([[0], np.cumsum([len(v) for _, v in cells])]).astype(np.int64)
    c.vals = (np.concatenate([v for _, v in cells]) if cells else c.vals).astype(c.vals.dtype)
    return c


def _split(heads, values):
    """the rows' element (byte) runs of an append / replace call"""
    out, at = [], 0
    for h in heads:
        k = 0 if int(h) >= U32_NULL else int(h)
        out.append((int(h), values[at:at + k]))
        at += k
    assert at == len(values)
    return out


class ModelPay(FakeTextIndex):
    """the payload columns of the model: FakeTextIndex plus what the host models lack -- truncate, scalar and list
    replace, the readers of the debug entries (a lagging column dropped by retain is FakeTextIndex.retain's; a loaded
    index has no columns: the model makes a new ModelPay)"""

    def kind_of(self, col):
        c = self.cols[col]
        if isinstance(c, TextCol):
            return PAY_TEXT
        if isinstance(c, ListCol):
            return c.kind
        return PI.PAY_U32 if c.dtype == np.uint32 else PI.PAY_F64

    def truncate(self, n_rows):
        for c, v in self.cols.items():
            if len(v) > n_rows:
                self.cols[c] = v.take(np.arange(len(v)) < n_rows) if isinstance(v, (ListCol, TextCol)) else v[:n_rows]
        self.n = n_rows

    def _rows_ok(self, col, rows):
        rows = np.asarray(rows, np.int64)
        if len(np.unique(rows)) != len(rows):
            raise ValueError("rows must be unique")
        if len(rows) and (rows.min() < 0 or rows.max() >= len(self.cols[col])):
            raise RuntimeError("a row lies outside [0, filled)")
        return rows

    def payload_replace(self, col, rows, cells):
        rows = self._rows_ok(col, rows)
        v = self.cols[col].copy()
        v[rows] = np.asarray(cells).view(v.dtype)
        self.cols[col] = v

    def payload_replace_lists(self, col, rows, heads, values):
        rows, c = self._rows_ok(col, rows), self.cols[col]
        cells = [c.row(r) for r in range(len(c))]
        for r, cell in zip(rows, _split(heads, np.asarray(values))):
            cells[int(r)] = cell
        self.cols[col] = _list_col(c.kind, cells)

    def payload_replace_text(self, col, rows, heads, data):
        super().payload_replace_text(col, self._rows_ok(col, rows), heads, bytes(data))

    def payload_cell(self, col, row, kind):
        return int(self.cols[col][row])

    def payload_list(self, col, row, kind):
        return self.cols[col].row(row)

    def payload_debug_text(self, col, row):
        return self.cols[col].row(row)


# ---- the model ---------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, profile, lens):
        self.profile, self.p, self.lens = profile, PROFILES[profile], lens
        env = self.p["env"]
        self.seg = int(env.get("HX_DEBUG_SEG_DOCS", SEG_DOCS))
        self.tail_min = int(env["HX_DEBUG_TAIL_MIN"]) if "HX_DEBUG_TAIL_MIN" in env else None
        self.x = np.zeros(0, np.int64)           # corpus row of the dense vector, per stored row
        self.s = np.zeros(0, np.int64)           # corpus row of the sparse vector, -1 = none
        self.sp_rows = 0
        self.base = self.tail = 0                # documents of the inverted index's base and tail
        self.stale, self.ever = False, False
        self.cand = self.p["cand"]
        self.bin_on = False                      # the 1-bit copy of the rows (hx_binary_enable); a load drops it
        self.pay = ModelPay(0)
        self.keys = {}                           # payload key -> column id
        self.touched = np.zeros(0, np.int64)     # the rows the last op touched (or their new neighbours)
        self.next_row = 0                        # the next unused corpus row
        self.emptied = self.regrown = False

    @property
    def n(self):
        return len(self.x)

    def doc_lens(self):
        return np.where(self.s >= 0, self.lens[np.maximum(self.s, 0)], 0)

    def nnz(self):
        return int(self.doc_lens()[:self.sp_rows].sum())

    def n_segments(self):
        return -(-self.base // self.seg) + -(-self.tail // self.seg)

    def inv_state(self):
        if not self.base and not self.tail:      # never built, or dropped since and not built again: the engine
            return "never"                       # holds no inverted index either way
        return "stale" if self.stale else "base+tail" if self.tail else "base"

    def full(self, key):
        return key in self.keys and self.n > 0 and len(self.pay.cols[self.keys[key]]) == self.n

    def finalize(self):
        """engine.hip finalize(): a base is rebuilt when none exists or fresh > max(built / 4, 2^18) (the forced
        value when HX_DEBUG_TAIL_MIN is set), otherwise the documents behind the base become the tail"""
        if not self.stale:
            return
        if self.nnz() > 0:
            self.sp_rows = max(self.sp_rows, self.n)
            built, fresh = self.base, self.sp_rows - self.base
            tail_max = self.tail_min if self.tail_min is not None else max(built // 4, TAIL_MIN)
            if built == 0 or fresh > tail_max:
                self.base, self.tail = self.sp_rows, 0
            elif fresh > 0:
                self.tail = fresh if self.doc_lens()[built:self.sp_rows].sum() > 0 else 0
        else:
            self.base = self.tail = 0
        self.stale, self.ever = False, True

    # -- ops -------------------------------------------------------------------------------------------------------------
    def apply(self, op):
        k = op["kind"]
        if k != "refused":
            self.touched = np.zeros(0, np.int64)
        getattr(self, "_" + k)(op)
        self.pay.n = self.n
        if self.n == 0 and k in ("retain", "truncate"):
            self.emptied = True
        if self.emptied and k == "add" and self.n > 0:
            self.regrown = True

    def _add(self, op):
        rows = op["rows"]
        self.next_row = max(self.next_row, int(rows.max()) + 1) if len(rows) else self.next_row
        self.touched = np.array([self.n - 1, self.n, self.n + len(rows) - 1])
        self.x = np.concatenate([self.x, rows])
        self.s = np.concatenate([self.s, rows if op["sparse"] else np.full(len(rows), -1)])
        if op["sparse"] and len(rows):
            self.sp_rows, self.stale = self.n, True

    def _retain(self, op):
        keep = op["keep"]
        if keep.all():
            return
        self.pay.n = self.n
        self.pay.retain(F.pack_rows(keep))
        self.keys = {k: c for k, c in self.keys.items() if c in self.pay.cols}
        gone = np.flatnonzero(~keep)
        self.touched = np.unique(np.cumsum(keep)[gone[[0, -1, len(gone) // 2]]])
        if self.sp_rows > 0:
            self.sp_rows = int(keep[:self.sp_rows].sum())
        self.x, self.s = self.x[keep], self.s[keep]
        self.base = self.tail = 0
        self.stale = True

    def _replace(self, op):
        rows, new = op["rows"], op["new"]
        if not len(rows):
            return
        self.next_row = max(self.next_row, int(new.max()) + 1)
        self.touched = rows[:6]
        self.x[rows] = new
        if op["sparse"]:
            self.s[rows] = new
            if rows.max() >= self.sp_rows:
                self.sp_rows = self.n
            self.base = self.tail = 0
            self.stale = True

    def _truncate(self, op):
        k = op["n"]
        self.pay.truncate(k)
        self.touched = np.array([k - 1, k])
        if k == self.n and self.sp_rows <= k:
            return
        self.x, self.s = self.x[:k], self.s[:k]
        self.sp_rows = min(self.sp_rows, k)
        self.tail = 0
        if self.base > self.sp_rows:
            self.base = 0
        self.stale = True

    def _save_load(self, op):
        self.pay, self.keys = ModelPay(self.n), {}
        self.base = self.tail = 0
        self.stale, self.ever = self.sp_rows > 0, False
        self.cand = self.p["cand"]
        self.bin_on = False

    def _touch(self, op):
        f = op["form"]
        if f == "rebuild_sparse":
            self.base = self.tail = 0
            self.stale = True
        if f == "set_dense_candidates":
            self.cand = op["to"]
        elif f == "binary_enable":                # (idempotent; the inverted index is not touched)
            self.bin_on = True
        else:
            self.finalize()

    def _refused(self, op):
        pass

    def _pay_create(self, op):
        self.keys[op["key"]] = self.pay.payload_create(PI._Key(PAY_KEYS[op["key"]]).kind)

    def _pay_drop(self, op):
        self.pay.payload_drop(self.keys.pop(op["key"]))

    def _pay_append(self, op):
        pays, pidx = payloads()
        for key, src in op["cols"]:
            pay_call(self.pay, "append", self.keys[key], key, None, [pays[i] for i in src], pidx)

    def _pay_replace(self, op):
        pays, pidx = payloads()
        self.touched = op["rows"][:6]
        pay_call(self.pay, "replace", self.keys[op["key"]], op["key"], op["rows"], [pays[i] for i in op["src"]], pidx)


def pay_call(index, what, col, key, rows, pays, pidx):
    """append / replace the cells of `pays` through the entry of the key's kind"""
    cells = pidx.encode(key, pays)
    k = pidx.keys[key]
    name = "payload_" + what + ("_text" if k.is_text else "_lists" if k.is_list else "")
    args = cells if isinstance(cells, tuple) else (cells,)
    getattr(index, name)(col, *(args if rows is None else (rows, *args)))


# ---- the generator -------------------------------------------------------------------------------------------------------
def brief(op):
    k = op["kind"]
    d = {"add": lambda: f"{len(op['rows'])}{'' if op['sparse'] else ' dense-only'}",
         "retain": lambda: f"{op['form']} -{int((~op['keep']).sum())}",
         "replace": lambda: f"{len(op['rows'])} {'sparse' if op['sparse'] else 'dense-only'}",
         "truncate": lambda: f"{op['form']} -> {op['n']}", "touch": lambda: op["form"], "refused": lambda: op["form"],
         "pay_create": lambda: op["key"], "pay_drop": lambda: op["key"],
         "pay_append": lambda: ",".join(f"{key}+{len(src)}" for key, src in op["cols"]),
         "pay_replace": lambda: f"{op['key']} {len(op['rows'])}", "save_load": lambda: ""}[k]()
    return f"{k}({d}){'*' if op['search'] else ''}"


WEIGHTS = dict(add=0.14, retain=0.13, replace=0.15, truncate=0.10, save_load=0.05, touch=0.08, pay=0.30, refused=0.05)


def _draw(rng, m, p):
    """one op for the model's state, or None when the drawn kind has no valid form now"""
    n, gentle = m.n, p["gentle"]
    w = np.array([WEIGHTS[k] * p["weight"].get(k, 1.0) for k in WEIGHTS])
    kind = str(rng.choice(list(WEIGHTS), p=w / w.sum()))
    if kind == "add":
        k = int(rng.choice(ADD_SIZES[3:] if n < 300 and rng.random() < 0.7 else ADD_SIZES))   # (not for long at a few rows)
        if n + k > p["max_rows"] or m.next_row + k > p["pool"]:
            return None
        sparse = not (p["dense_adds"] and rng.random() < 0.5)
        return dict(kind="add", rows=np.arange(m.next_row, m.next_row + k), sparse=sparse)
    if kind == "retain" and n > 0:
        form = str(rng.choice(RETAIN_FORMS[2:7])) if gentle or rng.random() < 0.7 else str(rng.choice(RETAIN_FORMS))
        keep = np.ones(n, bool)
        if form.startswith("keep"):
            keep = rng.random(n) < float(form[4:]) / 100.0
        elif form == "row0":
            keep[0] = False
        elif form == "last":
            keep[n - 1] = False
        elif form == "middle":
            keep[n // 3: n // 3 + max(n // (100 if gentle else 10), 1)] = False
        elif form == "none":
            keep[:] = False
        return dict(kind="retain", form=form, keep=keep)
    if kind == "replace" and n > 0:
        k = 0 if rng.random() < 0.12 else int(rng.integers(1, min(300, n) + 1))
        if m.next_row + k > p["pool"]:
            return None
        return dict(kind="replace", rows=rng.permutation(n)[:k].astype(np.int64), new=np.arange(m.next_row, m.next_row + k),
                    sparse=bool(rng.random() < 0.5))
    if kind == "truncate" and n > 0:
        form = str(rng.choice(TRUNCATE_FORMS[:4])) if gentle or rng.random() < 0.75 else str(rng.choice(TRUNCATE_FORMS))
        if form == "tail":
            if not 0 < m.base < n - 1:
                return None
            cut = int(rng.integers(m.base + 1, n))
        elif form == "below_base":
            if m.base < 2:
                return None
            cut = int(rng.integers(max(m.base - 500, 1) if gentle else 1, m.base))
        else:
            cut = {"n": n, "n-1": n - 1, "zero": 0}[form]
        return dict(kind="truncate", form=form, n=cut)
    if kind == "save_load":
        return dict(kind="save_load")
    if kind == "touch":
        forms = [f for f in TOUCH_FORMS if (f != "set_dense_candidates" or p["cand"] == "i8") and
                 (f != "binary_enable" or p["binary"])]          # (weight 0 where the profile has no binary copy)
        form = str(rng.choice(forms))
        op = dict(kind="touch", form=form)
        if form == "set_dense_candidates":
            op["to"] = "f16" if m.cand == "i8" else "i8"
        if form == "masked_search":
            if n == 0:
                return None
            op["keep"] = rng.random(n) < 0.5
        return op
    if kind == "refused":
        form = str(rng.choice(REFUSED_FORMS))
        if form in ("mask_length", "duplicate_row") and n == 0 or form == "append_past_count" and not m.keys:
            return None
        op = dict(kind="refused", form=form)
        if form == "append_past_count":
            op["key"] = sorted(m.keys)[int(rng.integers(len(m.keys)))]
        if form == "repeated_term":
            op["row"] = int(np.flatnonzero(m.lens >= 2)[0])
        return op
    if kind == "pay":
        missing = [k for k in PAY_KEYS if k not in m.keys]
        lag = [k for k in m.keys if len(m.pay.cols[m.keys[k]]) < n]
        has = [k for k in m.keys if len(m.pay.cols[m.keys[k]]) > 0]
        u = rng.random()
        if lag and u < 0.7:
            if rng.random() < 0.8:
                return _fill(rng, m)
            k = lag[int(rng.integers(len(lag)))]       # ... or one column, deliberately short of count()
            room = n - len(m.pay.cols[m.keys[k]])
            return dict(kind="pay_append", cols=[(k, rng.integers(0, PAY_POOL, int(rng.integers(0, room))))])
        if missing and (u < 0.85 or not m.keys):
            return dict(kind="pay_create", key=missing[int(rng.integers(len(missing)))])
        if has and u < 0.95:
            k = has[int(rng.integers(len(has)))]
            filled = len(m.pay.cols[m.keys[k]])
            rows = rng.permutation(filled)[:int(rng.integers(1, min(300, filled) + 1))].astype(np.int64)
            return dict(kind="pay_replace", key=k, rows=rows, src=rng.integers(0, PAY_POOL, len(rows)))
        if m.keys:
            return dict(kind="pay_drop", key=sorted(m.keys)[int(rng.integers(len(m.keys)))])
    return None


def _fill(rng, m):
    """every lagging column up to count()"""
    lag = [k for k in m.keys if len(m.pay.cols[m.keys[k]]) < m.n]
    return dict(kind="pay_append", cols=[(k, rng.integers(0, PAY_POOL, m.n - len(m.pay.cols[m.keys[k]]))) for k in lag])


def sequence(seed, n_ops, profile, tables=None, lens=None, with_states=False):
    """the first n_ops ops of the (seed, profile) sequence -- a prefix of every longer one.  with_states: also what the
    coverage table needs about the model in front of every op"""
    p = PROFILES[profile]
    lens = pool_lens(profile, tables) if lens is None else lens
    rng = np.random.default_rng([seed, PROFILE_IDS[profile]])
    m = Model(profile, lens)
    ops, states = [], []
    lo, hi = p["start"]
    first = [dict(kind="add", rows=np.arange(0, int(rng.integers(lo, hi))), sparse=True)]
    if p["dense_adds"]:
        first.append(dict(kind="add", rows=np.arange(len(first[0]["rows"]), len(first[0]["rows"]) + 700), sparse=False))
    if p["binary"] and rng.random() < 0.5:        # enable, then rows; otherwise rows, then enable at a random step
        first.insert(0, dict(kind="touch", form="binary_enable"))
    while len(ops) < n_ops:
        op = first.pop(0) if first else None
        last = ops[-1] if ops else None
        if op is None and last and last["kind"] in ("retain", "truncate") and not last["search"] and rng.random() < 0.4:
            # as many rows back as went: what the engine keys on the row count (the per-tile maxima of a scan) then
            # meets the count of the last search with other rows behind it
            k = states[-1]["n"] - m.n
            if 0 < k <= 1500 and m.next_row + k <= p["pool"]:
                op = dict(kind="add", rows=np.arange(m.next_row, m.next_row + k), sparse=True, form="refill")
        if op is None and ops and ops[-1]["kind"] in ("add", "pay_create") and rng.random() < 0.7:
            op = _fill(rng, m)                    # (columns that follow the rows: otherwise the next retain drops them)
            op = op if op["cols"] else None
        if op is None and p["binary"] and not m.bin_on and rng.random() < 0.3:
            op = dict(kind="touch", form="binary_enable")       # (the first time, or again behind a load)
        while op is None:
            op = _draw(rng, m, p)
        op["search"] = bool(rng.random() < 0.5) or (p["dense_adds"] and not ops) or op.get("form") == "refill"
        #                                            (the refill is searched at once; a dense-only tail survives a
        #                                             search only behind an inverted index that is not stale)
        states.append(dict(inv=m.inv_state(), full=[k for k in PAY_KEYS if m.full(k)], n=m.n, bin_on=m.bin_on,
                           lagging=[k for k in m.keys if len(m.pay.cols[m.keys[k]]) < m.n]))
        m.apply(op)
        if op["search"]:
            m.finalize()                          # (the searching part of `check` behind this op)
        ops.append(op)
    return (ops, states) if with_states else ops


# ---- the driver ----------------------------------------------------------------------------------------------------------
def _add_dense(index, X):
    """rows without a sparse row: hx_add_dense, which HxIndex.add never calls (it passes an empty CSR)"""
    if hasattr(index, "add_dense"):
        return index.add_dense(X)
    from rag_application_amd import _lib
    X = np.ascontiguousarray(X, np.float32)
    _lib.check(_lib.lib().hx_add_dense(index._h, X.ctypes.data, len(X)))


REFUSAL_WORDS = {"mask_length": "mask_rows", "duplicate_row": "unique", "append_past_count": "past", "nan_add": "finite",
                 "repeated_term": "unique within a vector"}


def _refused(index, model, op, pool):
    """the call must raise the refusal of its form -- a ValueError of the binding or the engine's error (HxError is a
    RuntimeError), its message holding REFUSAL_WORDS[form]; any other exception is the driver's own mistake"""
    f, n = op["form"], model.n
    rows = np.arange(model.p["pool"] - 4, model.p["pool"])
    ip, si, sv = pool.csr(rows)
    X = pool.X[rows].copy()
    dup = np.array([n - 1, 0, n - 1], np.int64)
    if f == "mask_length":
        call = lambda: index.retain(np.ones(n + 1, bool))
    elif f == "duplicate_row":
        call = lambda: index.replace(dup, X[:3], *pool.csr(rows[:3]))
    elif f == "append_past_count":
        key, (pays, pidx) = op["key"], payloads()
        room = n - index.payload_rows(model.keys[key])
        cells = [pays[i % PAY_POOL] for i in range(room + 1)]
        call = lambda: pay_call(index, "append", model.keys[key], key, None, cells, pidx)
    elif f == "nan_add":
        X[3, 17] = np.nan                          # the LAST row of the batch
        call = lambda: index.add(X, ip, si, sv)
    else:
        ip, si, sv = pool.csr([op["row"], op["row"] + 1])
        si = si.copy()
        si[1] = si[0]
        call = lambda: index.add(pool.X[[op["row"], op["row"] + 1]], ip, si, sv)
    try:
        call()
    except (ValueError, RuntimeError) as e:
        assert REFUSAL_WORDS[f] in str(e), f"{f}: refused with another message: {e}"
    else:
        raise AssertionError(f"{f}: the call was not refused")
    if f == "duplicate_row" and hasattr(index, "_h"):      # ... and the engine's own check, behind the binding's
        from rag_application_amd import _lib
        Xd = np.ascontiguousarray(X[:3], np.float32)
        ipd, sid, svd = (np.ascontiguousarray(a) for a in pool.csr(rows[:3]))
        rc = _lib.lib().hx_replace_rows(index._h, dup.ctypes.data, 3, Xd.ctypes.data, ipd.ctypes.data, sid.ctypes.data,
                                        svd.ctypes.data)
        assert rc != 0 and b"unique" in _lib.lib().hx_last_error(), "hx_replace_rows took a repeated row"


def apply(index, model, op):
    """the op on the index (anything with HxIndex's method names), then on the model; returns the index to go on with
    (save_load: the loaded one).  model.pool / model.tmp: the Pool and a directory for save files."""
    pool, k = model.pool, op["kind"]
    if k == "add":
        rows = op["rows"]
        if op["sparse"]:
            index.add(pool.X[rows], *pool.csr(rows))
        elif len(rows):
            _add_dense(index, pool.X[rows])
    elif k == "retain":
        assert index.retain(op["keep"]) == int((~op["keep"]).sum())
    elif k == "replace":
        rows, new = op["rows"], op["new"]
        index.replace(rows, pool.X[new].reshape(len(new), pool.dim), *(pool.csr(new) if op["sparse"] else ()))
    elif k == "truncate":
        index.truncate(op["n"])
    elif k == "save_load":
        path = os.path.join(str(model.tmp), "index.hx")
        index.save(path)
        back = type(index).load(path)
        index.close()
        index = back
    elif k == "touch":
        f = op["form"]
        if f in ("finalize", "rebuild_sparse"):
            getattr(index, f)()
        elif f == "set_dense_candidates":
            index.set_dense_candidates(op["to"])
        elif f == "binary_enable":
            index.binary_enable()
        else:
            index.hybrid_query_host(*model.qs, model.hp["h1"], mask=op.get("keep"))
    elif k == "refused":
        _refused(index, model, op, pool)
    elif k == "pay_create":
        assert index.payload_create(PI._Key(PAY_KEYS[op["key"]]).kind) == model.pay.next
    elif k == "pay_drop":
        index.payload_drop(model.keys[op["key"]])
    elif k == "pay_append":
        pays, pidx = payloads()
        for key, src in op["cols"]:
            pay_call(index, "append", model.keys[key], key, None, [pays[i] for i in src], pidx)
    elif k == "pay_replace":
        pays, pidx = payloads()
        pay_call(index, "replace", model.keys[op["key"]], op["key"], op["rows"], [pays[i] for i in op["src"]], pidx)
    model.apply(op)
    return index


def fresh_index(index, model):
    """a new index of the model's rows, added in one batch (the rows behind sp_rows through hx_add_dense)"""
    pool, sp = model.pool, model.sp_rows
    sub = type(index)(pool.dim, MS)
    if model.bin_on and model.n % 2:              # the copy follows the adds, or is derived from the rows behind them
        sub.binary_enable()
    if sp:
        sub.add(pool.X[model.x[:sp]], *pool.csr(model.s[:sp]))
    if model.n > sp:
        _add_dense(sub, pool.X[model.x[sp:]])
    if model.n and sub.dense_candidates() != index.dense_candidates():
        sub.set_dense_candidates(index.dense_candidates())
    if model.bin_on:
        sub.binary_enable()
    return sub


def copies(index, rows, cand8):
    """the bytes of every stored copy hx_debug_row reaches (tests/test_gpu_delete.stored_rows for this index's prefix
    sizes; an index with fp16 candidates only keeps no copies 5 and 6)"""
    which = [0] + list(range(1, len(MS) + 1)) + [4] + ([5, 6] if cand8 else [])
    return [[index.debug_row(w, int(r)).tobytes() for w in which] for r in rows]


def sample_rows(model, rng, limit=None):
    n = model.n if limit is None else limit
    if n <= 0:
        return np.zeros(0, np.int64)
    t = np.asarray(model.touched, np.int64)
    rows = np.unique(np.concatenate([[0, n - 1], t - 1, t, t + 1, rng.integers(0, n, 16)]))
    return rows[(rows >= 0) & (rows < n)]


def draw_filter(model, rng):
    """one random filter over the full columns that compiles: (filter, ops, sets), or None when no column is full"""
    _, pidx = payloads()
    full = [k for k in PAY_KEYS if model.full(k)]
    if not full:
        return None
    for key in PAY_KEYS:
        pidx.keys[key].col = model.keys[key] if key in full else None
    gen = text_filter if "body" in full else list_filter if {"langs", "nums"} & set(full) else random_filter
    n = model.n
    id_rows = lambda: {f"id{r}": r for r in range(n)}
    for _ in range(200):
        flt = gen(rng, int(rng.integers(0, 3)), n)
        prog = pidx.compile(flt, id_rows) if flt else None
        if prog is not None and any(PI.IS_MISSING <= op <= PI.GE or op >= PI.ANY_EQ for op, _, _ in prog[0]):
            return flt, prog[0], prog[1]
    flt = {"must_not": [{"is_null": {"key": full[0]}}]}
    return (flt, *pidx.compile(flt, id_rows))


def own_queries(model):
    """the 8 queries, the last three to five replaced by stored rows' own vectors (dense row, the first 32 terms of the
    sparse row): row 0, the first row behind the inverted index's base, the last row and the first and last spiky row
    (Pool) -- the lists then depend on single rows at the seams of the stored arrays and of the inverted index, and on
    the rows a scan with stale per-tile maxima loses"""
    pool, n = model.pool, model.n
    Q, qip, qsi, qsv = model.qs
    if n == 0:
        return model.qs
    Q, terms = Q.copy(), [(qsi[qip[b]:qip[b + 1]], qsv[qip[b]:qip[b + 1]]) for b in range(N_QUERIES)]
    rows = [0, min(model.base, n - 1), n - 1]
    spiky = np.flatnonzero(pool.spiky[model.x])     # rows with a large scale in the int8 candidate copy: the ones a
    if len(spiky):                                  # scan with too low a per-tile maximum drops first
        rows += [int(spiky[0]), int(spiky[-1])]
    for b, r in zip(range(N_QUERIES - 1, -1, -1), rows[::-1]):
        Q[b] = pool.X[model.x[r]]
        ip, si, sv = pool.csr(model.s[r:r + 1])
        if ip[1]:
            terms[b] = (si[:32], sv[:32])
    ip = np.concatenate([[0], np.cumsum([len(t) for t, _ in terms])]).astype(np.int64)
    return (Q, ip, np.concatenate([t for t, _ in terms]).astype(np.int32),
            np.concatenate([w for _, w in terms]).astype(np.float32))


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _bin_lists(index, Q, limit, mask=None):
    """search_bin with host queries: HxIndex takes them on its device, a CPU index as they are"""
    if hasattr(index, "_tdev"):
        import torch
        Q = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).to(index._tdev)
    keys, cnt = index.search_bin(Q, limit, mask=mask)
    return _host(keys).view(np.uint64), _host(cnt)


def _refuses(call, word, what):
    try:
        call()
    except (ValueError, RuntimeError) as e:
        assert word in str(e), f"{what}: refused with another message: {e}"
    else:
        raise AssertionError(f"{what}: the call was not refused")


def check_binary(index, sub, model, rows, keep, full):
    """the 1-bit copy and the Hamming scan stage (integer: every comparison exact) against the fresh index and
    tests/binary_helpers.py; the stage does not touch the inverted index, so this runs after every op.  rows: the sampled
    rows; keep: the drawn payload filter's rows or None; full: also at the limit min(n, 2048)"""
    pool, n = model.pool, model.n
    assert index.binary_enabled() == model.bin_on, ("binary_enabled", index.binary_enabled(), model.bin_on)
    Q = own_queries(model)[0]
    if not model.bin_on:
        _refuses(lambda: _bin_lists(index, Q, 10), "binary", "search_bin without the binary copy")
        _refuses(lambda: index.binary_row(0), "binary", "binary_row without the binary copy")
        return
    if n == 0:
        keys, cnt = _bin_lists(index, Q, 10)
        assert not keys.any() and not cnt.any(), "search_bin over an empty index"
        return
    want = BH.words(BH.row_bits(pool.X[model.x[rows]]))
    for r, w in zip(rows, want):
        got = np.asarray(index.binary_row(int(r)))
        assert got.tobytes() == w.tobytes(), ("binary_row vs the model", int(r))
        assert got.tobytes() == np.asarray(sub.binary_row(int(r))).tobytes(), ("binary_row vs the fresh index", int(r))
    xb = BH.row_bits(pool.X[model.x])
    for limit in (10, min(n, 2048)) if full else (10,):
        for mask, name in ((None, "unmasked"), (keep, "under the payload filter's mask")):
            if mask is None and name != "unmasked":
                continue
            model_lists = BH.search(xb, Q, limit, mask)
            for B in (N_QUERIES, 1):              # the QG = 8 and the QG = 1 kernel
                what = f"search_bin, B {B} limit {limit}, {name}"
                got = _bin_lists(index, Q[:B], limit, mask)
                BH.assert_same_lists(got, _bin_lists(sub, Q[:B], limit, mask), what + ", vs the fresh index")
                BH.assert_same_lists(got, BH.cut(model_lists, B, limit), what + ", vs the model")


FIXED_TERMS = (0, 1, 2, 2 ** 31 - 1, -1, -7, -2 ** 31)


def probe_terms(si, rng, n):
    """n term ids as tests/test_gpu_sparse_idf.probe_terms draws them: live ones, their absent neighbours, ids nobody
    holds, negative ones -- with repeats (the pool's ids lie far apart: t - 1 and t + 1 are almost always absent)"""
    live = np.unique(np.asarray(si, np.int64))
    ends = [int(live.min()), int(live.max())] if len(live) else []
    cand = np.concatenate([live, live - 1, live + 1, FIXED_TERMS, ends])
    cand = cand[(cand >= -2 ** 31) & (cand < 2 ** 31)]
    return rng.choice(cand, n, replace=True).astype(np.int32)


def counted_stats(ip, si, terms):
    """(df list, N) as sparse_idf_helpers.stats gives them, counted with numpy: ids are unique within a row (ingest
    refuses others), so a term's df is how often it occurs at all, and N the rows that are not empty"""
    held, cnt = np.unique(np.asarray(si, np.int64), return_counts=True)
    terms = np.asarray(terms, np.int64)
    at = np.minimum(np.searchsorted(held, terms), max(len(held) - 1, 0))
    hit = (held[at] == terms) if len(held) else np.zeros(len(terms), bool)
    df = np.where(hit, cnt[at] if len(held) else 0, 0)
    return [int(d) for d in df], int((np.diff(np.asarray(ip, np.int64)) > 0).sum())


def check_term_stats(index, sub, model, rng, full):
    """df, N and the scaled weights (hx_sparse_idf_host: bit-exact by contract) of probe terms against the fresh index
    and against the model's sparse rows: counted with numpy and weighed by sparse_idf_helpers.weights at EVERY searched
    step of every profile, and on `full` steps also by the row-by-row sparse_idf_helpers.stats (seconds over the 34 000
    rows of `segments`, so there at the ends only; the two counts must agree).  The entry finalizes the inverted
    index: the caller has told the model.  df is read off the base's AND the tail's posting directories and N off the
    rows that have a sparse row: a stale directory or trailing dense-only rows show here."""
    ip, si, _ = model.pool.csr(model.s[:model.sp_rows])
    terms = probe_terms(si, rng, 48)
    vals = (rng.random(len(terms)) * 3 + 0.01).astype(np.float32)
    w, df, nd = index.sparse_idf_host(terms, vals, want_stats=True)
    fw, fdf, fnd = sub.sparse_idf_host(terms, vals, want_stats=True)
    at = (model.inv_state(), "sp_rows", model.sp_rows, "n", model.n)
    assert nd == fnd, ("N vs the fresh index", nd, fnd) + at
    assert np.asarray(df).tolist() == np.asarray(fdf).tolist(), ("df vs the fresh index",) + at
    assert SH.same_bits(w, fw), ("weights vs the fresh index",) + at
    assert SH.same_bits(index.sparse_idf_host(terms, vals), w), "sparse_idf_host without the optional outputs"
    want_df, want_n = counted_stats(ip, si, terms)
    if full:
        assert (want_df, want_n) == SH.stats(ip, si, terms), "the two host counts of the model's rows differ"
    assert nd == want_n, ("N vs the model", nd, want_n) + at
    assert np.asarray(df).tolist() == want_df, ("df vs the model",) + at
    assert SH.same_bits(w, SH.weights(vals, want_df, want_n)), ("weights vs the model",) + at


def check(index, model, search=True, oracle=True, seed=0, full=None):
    """everything a caller can observe of `index` against the model; `search`: the searching part too (it finalizes the
    inverted index: the model was told so by the op's flag); `oracle`: the first query against the numpy oracle; `full`
    (default: as `oracle`): the step carries the reads whose host model walks every row"""
    pool, n = model.pool, model.n
    full = oracle if full is None else full
    rng = np.random.default_rng([seed, n, model.next_row])
    st = index.stats()
    assert index.count() == n, ("count", index.count(), n)
    assert st["nnz"] == model.nnz(), ("nnz", st["nnz"], model.nnz())
    assert index.dense_candidates() == model.cand, ("dense_candidates", index.dense_candidates(), model.cand)
    segs = lambda: (index.stats()["n_segments"], model.n_segments(), "base", model.base, "tail", model.tail)
    assert segs()[0] == segs()[1], ("n_segments", *segs())
    sub = fresh_index(index, model)
    try:
        assert st["cand8_row_error_max"] >= sub.stats()["cand8_row_error_max"], "cand8_row_error_max is no upper bound"
        rows = sample_rows(model, rng)
        cand8 = model.p["cand"] == "i8"
        assert copies(index, rows, cand8) == copies(sub, rows, cand8), "a stored copy differs from the fresh index's"
        # ---- payload columns ----
        for key, col in model.keys.items():
            filled = len(model.pay.cols[col])
            kind = model.pay.kind_of(col)
            assert index.payload_rows(col) == filled, (key, "payload_rows", index.payload_rows(col), filled)
            for r in sample_rows(model, rng, filled):
                r = int(r)
                if kind == PAY_TEXT:
                    got, want = index.payload_debug_text(col, r), model.pay.payload_debug_text(col, r)
                elif kind in (PAY_LIST_U32, PAY_LIST_F64):
                    (h, v), (eh, ev) = index.payload_list(col, r, kind), model.pay.payload_list(col, r, kind)
                    got, want = (h, np.asarray(v).tobytes()), (eh, np.asarray(ev).tobytes())
                else:
                    got, want = index.payload_cell(col, r, kind), model.pay.payload_cell(col, r, kind)
                assert got == want, (key, r, got, want)
        keep = None
        prog = draw_filter(model, rng)
        if prog is not None:
            flt, ops, sets = prog
            mask, kept = index.payload_mask(ops, sets)
            keep = interp_text(ops, list(sets), model.pay.cols, n)
            np.testing.assert_array_equal(index.mask_host(mask), F.pack_rows(keep), err_msg=str(flt)[:300])
            assert kept == int(keep.sum())
        check_binary(index, sub, model, rows, keep, full)
        if not search:
            return
        # ---- the lists ----
        model.finalize()                          # the first search does what finalize() does; checked behind the lists
        check_term_stats(index, sub, model, rng, full)
        ora = pool.oracle(model.x, model.s) if oracle and n else None
        qs = Q, qip, qsi, qsv = own_queries(model)
        for mode in MODES:
            hp = model.hp[mode]
            got = index.hybrid_query_host(*qs, hp)
            if n == 0:
                assert (got[2] == 0).all() and (got[1] == -1).all(), (mode, "empty index")
                continue
            same(got, sub.hybrid_query_host(*qs, hp), f"{mode} vs the fresh index")
            if keep is not None:
                same(index.hybrid_query_host(*qs, hp, mask=keep), sub.hybrid_query_host(*qs, hp, mask=keep),
                     f"{mode}, masked by the payload filter, vs the fresh index")
            if ora is not None:
                qa, qb = qsi[qip[0]:qip[1]].astype(np.int64), qsv[qip[0]:qip[1]]
                if mode == "tree":
                    os_, oi = O.hybrid_tree(ora, Q[0], qa, qb, P)
                else:
                    os_, oi = O.hybrid_h1(ora, Q[0], qa, qb, P["dense_limit"], P["sparse_limit"], P["final_limit"])
                s, i, c = got
                m = len(oi)
                assert c[0] == m, (mode, "count vs oracle", c[0], m)
                np.testing.assert_array_equal(i[0, :m], oi, err_msg=f"{mode}: ids vs oracle")
                np.testing.assert_array_equal(s[0, :m].view(np.uint32), np.asarray(os_, np.float32).view(np.uint32),
                                              err_msg=f"{mode}: score bits vs oracle")
        assert segs()[0] == segs()[1], ("n_segments behind the search", *segs())
    finally:
        sub.close()


def run(eng, index_type, seed, profile, tables, tmp, n_ops=None, oracle=True):
    """the whole (seed, profile) sequence on a new index of `index_type`, `check` after every op.  A failure names the
    seed, the step and the op log so far: sequence(seed, step + 1, profile) replays it."""
    p = PROFILES[profile]
    ops = sequence(seed, p["n_ops"] if n_ops is None else n_ops, profile, tables)
    pool = pool_of(profile, tables)
    model = Model(profile, pool.lens)
    model.pool, model.tmp, model.qs = pool, tmp, queries(p["dim"], tables)
    model.hp = {m: eng.make_params(P, mode=eng.HX_MODE_TREE if m == "tree" else eng.HX_MODE_H1) for m in MODES}
    index = index_type(p["dim"], MS)
    log = []
    try:
        for step, op in enumerate(ops):
            log.append(brief(op))
            try:
                index = apply(index, model, op)
                full = p["oracle"] == "all" or step in (0, len(ops) - 1)
                check(index, model, search=op["search"] or step == len(ops) - 1, oracle=oracle and full,
                      seed=seed * 1000 + step, full=full)         # (a sequence, and every replayed prefix, ends with the lists)
            except Exception as e:
                what = " | ".join(ln.strip() for ln in str(e).splitlines() if ln.strip())[:600]
                raise AssertionError(f"seed {seed} profile {profile} step {step}: {type(e).__name__}: {what}\n"
                                     f"ops so far: {' '.join(log)}") from e
    finally:
        index.close()
    return model
