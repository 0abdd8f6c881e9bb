"""CPU: the handler sequences of tests/handler_model.py without a GPU.

  * the driver (`apply`, `check`, `compare`, `run_case`) on `FakeHandler`, a QdrantHandler whose collections hold
    `HFakeIndex` -- the FakeIndex of tests/test_lifecycle_model_host.py plus what the handler calls: packed masks, token
    columns, files on disk.  The fake has payload columns and payload_mask, so filters on live keys compile and run as
    programs; it has no facet, scroll or grouped-query entries, so the handler's hasattr guards take the Python paths,
    and no MMR, rerank or recommend, which have no Python path: the driver's capability set leaves those out.  A broken
    model or driver is found here;
  * the coverage table of the committed (seed, profile) list, computed from the generator alone and asserted;
  * seven mutants of the handler's cached state, each of which the driver must catch, naming seed and step;
  * the brute-force restatement: after every op the model equals the state re-derived from the op log in plain Python."""
import hashlib
import os
import re

import numpy as np
import pytest

from rag_application_amd import handler as HD
from rag_application_amd import late_interaction as LI
from tests import handler_model as H
from tests import lifecycle_model as L
from tests.payload_helpers import unpack
from tests.test_lifecycle_model_host import FakeIndex

CAPS = frozenset({"counters"})


# ---- a CPU index with what the handler calls -----------------------------------------------------------------------------
class HFakeIndex(FakeIndex):
    profile = "small"                                         # (only the inverted-index rule of that Model is used)

    def __init__(self, dim, ms):
        # FakeIndex.__init__ restated: it reads the profile off FakeIndex itself, which another test module sets
        L.ModelPay.__init__(self, 0)
        self.dim, self.msizes = dim, ms
        self.X = np.zeros((0, dim), np.float32)
        self.sp = []
        self.inv = L.Model(type(self).profile, np.zeros(1, np.int64))
        self.cand = L.PROFILES[type(self).profile]["cand"]
        self.tok = {}                                         # token column -> one cell per row: (head, x8, scales)
        self.bits = self.terms = None                         # (FakeIndex: the 1-bit copy, the term table)

    def _bools(self, mask):
        mask = np.asarray(mask)
        return unpack(mask, len(self.X)) if mask.dtype == np.uint32 else mask.astype(bool)

    def retain(self, keep):
        keep = self._bools(keep)
        n = len(self.X)
        for c in list(self.tok):
            if len(self.tok[c]) != n:
                del self.tok[c]
            else:
                self.tok[c] = [v for v, k in zip(self.tok[c], keep) if k]
        return super().retain(keep)

    def truncate(self, k):
        for c in self.tok:
            del self.tok[c][k:]
        super().truncate(k)

    def replace(self, rows, dense, ip=None, si=None, sv=None):
        if not np.isfinite(dense).all():
            raise RuntimeError("dense rows must be finite")
        super().replace(rows, dense, ip, si, sv)

    def hybrid_query_host(self, Q, qip, qsi, qsv, hp, mask=None):
        return super().hybrid_query_host(Q, qip, qsi, qsv, hp, None if mask is None else self._bools(mask))

    def save(self, path):
        super().save(path)
        open(path, "wb").close()

    # -- token columns --
    def payload_create_tokens(self, dim_t):
        self.tok[self.next] = []
        self.next += 1
        return self.next - 1

    def payload_rows(self, col):
        return len(self.tok[col]) if col in self.tok else super().payload_rows(col)

    def payload_drop(self, col):
        if col in self.tok:
            del self.tok[col]
        else:
            super().payload_drop(col)

    @staticmethod
    def _cells(heads, x8, scales):
        out, at = [], 0
        for h in heads:
            k = 0 if int(h) >= LI.NULL else int(h)
            out.append((int(h), x8[at:at + k].copy(), scales[at:at + k].copy()))
            at += k
        assert at == len(x8) == len(scales)
        return out

    def payload_append_tokens(self, col, heads, x8, scales):
        if len(self.tok[col]) + len(heads) > len(self.X):
            raise RuntimeError("past the row count")
        self.tok[col] += self._cells(heads, x8, scales)

    def payload_replace_tokens(self, col, rows, heads, x8, scales):
        for r, cell in zip(rows, self._cells(heads, x8, scales)):
            self.tok[col][int(r)] = cell

    def payload_debug_tokens(self, col, row):
        return self.tok[col][row]


class FakeHandler(HD.QdrantHandler):
    """QdrantHandler over CPU indexes: the two places a collection's engine index is made, as sharded.ShardedHandler
    overrides them"""
    index_type = HFakeIndex

    def _open_collection(self, user_id, dim, msizes, sparse_enabled, force_recreate):
        base = self._base(user_id)
        if base and not force_recreate and os.path.exists(base + ".hx") and os.path.exists(base + ".json"):
            return HD._Collection.load(base, self.device, index_loader=lambda path, meta: self.index_type.load(path))
        col = HD._Collection(dim, msizes, self.device, index=self.index_type(dim, tuple(msizes)))
        col.sparse_enabled = sparse_enabled
        return col


def maker(cls):
    return lambda persist: cls(persist_dir=persist)


# ---- the driver on the fake ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,profile", H.CASES)
def test_driver_on_the_fake(synth_tables, tmp_path, seed, profile):
    m = H.run_case(maker(FakeHandler), seed, profile, synth_tables, tmp_path, caps=CAPS)
    assert all(h._collections == {} for h in m.opened), "a handler was left open"


def test_sequences_are_prefixes_of_longer_ones(synth_tables):
    pool = H.pool_of(128, synth_tables)
    a, b = H.sequence(3, 9, "small", pool), H.sequence(3, 24, "small", pool)
    assert [H.brief(x) for x in a] == [H.brief(x) for x in b[:9]]


# ---- the coverage table ----------------------------------------------------------------------------------------------------
def coverage(cases, tables):
    """what the sequences of `cases` cover, from the generator alone"""
    t = dict(kinds={}, store={}, upsert={}, refused={}, sel={}, target={}, index={}, token={}, refills=0, rollbacks=0,
             binary_loads_searched=0, binary_rollbacks=0, idf_deletes_searched=0, poisoned_reads=0, cures=0, indexed_removals=0, seam_deletes=0, wide_seam_deletes=0, old_poison_scrolls=0, empty_steps=0, regrown=0, full_saves=0, filled_token_index=0, appending_upserts=0)

    def count(table, what):
        t[table][what] = t[table].get(what, 0) + 1

    for seed, profile in cases:
        p = H.PROFILES[profile]
        pool = H.pool_of(p["dim"], tables)
        ops, states = H.sequence(seed, p["n_ops"], profile, pool, with_states=True)
        m = H.Model(profile, pool)
        stale = 0
        for step, (op, st) in enumerate(zip(ops, states)):
            k = op["kind"]
            count("kinds", k)
            if k == "store":
                count("store", (op["form"], len(op["specs"]) if op["form"] != "refill" and step > 2 else None))
                if op["form"] == "refill" and ops[step - 1]["kind"] == "delete" and len(op["specs"]) == st["removed"] > 0:
                    t["refills"] += 1                         # (check evaluates every filter of the set after every op)
            elif k == "upsert":
                count("upsert", op["form"])
                if all(target is None or target[0] == "name" for target, _ in op["items"]) and step > 0:
                    t["appending_upserts"] += 1               # (... so the masks of the set are cached before it)
            elif k == "upsert_refused":
                count("refused", op["form"])
                if op["form"] == "nan_rollback":
                    t["rollbacks"] += 1                       # (the form brings one named and one unnamed unknown id)
            elif k == "delete":
                # a filter "on an indexed key" counts where the key IS live in front of the op: only then the delete's
                # mask comes from the device (apply asserts that it does)
                if op["sel"] not in ("indexed", "ids+filter") or all(key in st["live"] for key in op["keys"]):
                    count("sel", op["sel"])
                    t["indexed_removals"] += op["sel"] == "indexed" and len(m.gone(op)) > 0
                count("target", op["target"])
                # the chunked profile: cells of a token column and of a list column move across 64-row seams -- the delete
                # takes a row that is not the last, of more than 64, under a token index and a live languages index
                gone = m.gone(op)
                if (p["env"].get("HX_DEBUG_COMPACT_CHUNK") == "64" and st["n"] > 64 and st["tdim"] and "languages" in st["live"]
                        and gone and gone[0] < st["n"] - len(gone)):
                    t["seam_deletes"] += 1
                    t["wide_seam_deletes"] += op["target"] in ("half", "run") and len(gone) > 1
            elif k == "index":
                count("index", (op["form"], H.SCHEMAS[op["key"]]) if op["form"] == "create" else op["form"])
                t["cures"] += op["form"] == "cure"
            elif k == "token_index":
                count("token", op["form"])
                t["filled_token_index"] += op["form"] == "create_filled"
            elif k == "save_load" and st["tdim"] and len(st["live"]) >= 2:
                t["full_saves"] += 1
            # the two later profiles: what their flag or statistics must survive, read at once or one op on
            soon = op["search"] or step == len(ops) - 1 or ops[step + 1]["search"]
            if p["collection"].get("binary_quantization"):
                t["binary_loads_searched"] += k == "save_load" and soon
                t["binary_rollbacks"] += k == "upsert_refused" and op["form"] == "nan_rollback"
            if p["collection"].get("sparse_modifier") and k == "delete":
                t["idf_deletes_searched"] += soon and 0 < len(m.gone(op)) < st["n"]
            m.apply(op)
            t["poisoned_reads"] += any(key in H.POISON for key in m.dead)     # (check reads every key after the op)
            # an ordered scroll by page_number (check runs four after every op) on a key poisoned two ops ago or more
            stale = stale + 1 if "page_number" in m.dead else 0
            t["old_poison_scrolls"] += stale >= 3 and m.n > 0
            t["empty_steps"] += m.n == 0 and step > 2
        t["regrown"] += bool(m.regrown)
    return t


def test_coverage_table(synth_tables):
    t = coverage(H.CASES, synth_tables)
    few = lambda table, wanted: [w for w in wanted if t[table].get(w, 0) < 2]
    assert not few("kinds", H.WEIGHTS), few("kinds", H.WEIGHTS)
    sizes = [(what, k) for what in ("docs", "chats") for k in H.STORE_SIZES]
    assert not few("store", sizes + [("refill", None)]), few("store", sizes + [("refill", None)])
    assert not few("upsert", H.UPSERT_FORMS), few("upsert", H.UPSERT_FORMS)
    assert not few("refused", H.REFUSED_FORMS), few("refused", H.REFUSED_FORMS)
    assert not few("sel", H.DELETE_SELECTORS), few("sel", H.DELETE_SELECTORS)
    assert not few("target", H.DELETE_TARGETS), few("target", H.DELETE_TARGETS)
    forms = [("create", s) for s in H.SCHEMAS.values()] + ["recreate", "drop", "poison", "cure"]
    assert not few("index", forms), few("index", forms)
    assert not few("token", H.TOKEN_FORMS), few("token", H.TOKEN_FORMS)
    assert t["indexed_removals"] >= 2, "too few deletes by a filter on a live key that remove rows"
    assert t["seam_deletes"] >= 2 and t["wide_seam_deletes"] >= 1, "the chunked cases move no token / list cells over a seam"
    assert t["refills"] >= 3, "too few stores that bring the count back to what it was before a delete"
    assert t["rollbacks"] >= 2
    assert t["poisoned_reads"] >= 2 and t["cures"] >= 1
    assert t["old_poison_scrolls"] >= 2, "no ordered scroll on a page_number poisoned two ops before"
    assert t["empty_steps"] <= 2 * len(H.CASES), "the sequences idle on empty collections"
    assert t["regrown"] >= 1, "no collection is emptied and grown again"
    assert t["full_saves"] >= 2, "no save_load with a token index and two live payload indexes"
    assert t["filled_token_index"] >= 1
    assert t["appending_upserts"] >= 2
    assert t["binary_loads_searched"] >= 2, "no searched step behind a save_load of the binary collection"
    assert t["binary_rollbacks"] >= 2, "no rolled-back upsert under the binary copy"
    assert t["idf_deletes_searched"] >= 2, "no searched step behind a delete of the IDF collection"


# the op logs of the ten cases committed before the binary and idf profiles, taken at the commit before them
LEGACY = ("small", "padded", "persist", "bare", "chunked")
LEGACY_DIGEST = "3ceb4e77cea16ae79a506006933e144844ae68640aa322529be0812d270c19cc"


def test_the_earlier_cases_keep_their_op_logs(synth_tables):
    h = hashlib.sha256()
    cases = [c for c in H.CASES if c[1] in LEGACY]
    assert list(H.PROFILES)[:len(LEGACY)] == list(LEGACY) and len(cases) == 10
    for seed, profile in cases:
        p = H.PROFILES[profile]
        ops = H.sequence(seed, p["n_ops"], profile, H.pool_of(p["dim"], synth_tables))
        h.update((f"{seed} {profile}: " + " ".join(H.brief(op) for op in ops) + "\n").encode())
    assert h.hexdigest() == LEGACY_DIGEST


# ---- mutants: each stands for one piece of cached state --------------------------------------------------------------------
def caught(make, synth_tables, tmp_path, cases=H.CASES):
    """the driver must fail on the mutant in one of the cases, with a message that names seed and step"""
    for seed, profile in cases:
        try:
            H.run_case(make, seed, profile, synth_tables, tmp_path / f"{profile}{seed}", caps=CAPS)
        except AssertionError as e:
            assert str(e).startswith(f"seed {seed} profile {profile} step ") and "ops so far: " in str(e), str(e)[:300]
            return str(e)
    raise AssertionError("the driver passed the mutant in every case")


def last_op(msg):
    """the last entry of a failure's op log (an entry may hold blanks: "delete(ids last)*")"""
    return re.findall(r"\w+\([^)]*\)\*?", msg.split("ops so far:")[1])[-1]


def test_mutant_delete_keeps_the_cached_masks(synth_tables, tmp_path):
    class Mutant(FakeHandler):
        def _delete_sync(self, user_id, filters, point_ids):
            col = self._collections[str(user_id)]
            before = dict(col._masks)
            n = super()._delete_sync(user_id, filters, point_ids)
            col._masks.update(before)
            return n
    caught(maker(Mutant), synth_tables, tmp_path)


def test_mutant_upsert_keeps_the_cached_masks(synth_tables, tmp_path):
    class Mutant(FakeHandler):
        def _upsert_sync(self, user_id, items, point_ids):
            col = self._collections[str(user_id)]
            before = dict(col._masks)
            n = super()._upsert_sync(user_id, items, point_ids)
            col._masks.update(before)
            return n
    caught(maker(Mutant), synth_tables, tmp_path)


def test_mutant_rollback_leaves_the_appended_ids(synth_tables, tmp_path):
    class Mutant(FakeHandler):
        def _upsert_sync(self, user_id, items, point_ids):
            col = self._collections[str(user_id)]
            n0 = len(col.payloads)
            try:
                return super()._upsert_sync(user_id, items, point_ids)
            except RuntimeError:
                if len(col.payloads) == n0 and len(col.ids) == n0:     # rolled back: the ids come back
                    col.ids.extend(f"ghost-{k}" for k in range(2))
                raise
    msg = caught(maker(Mutant), synth_tables, tmp_path)
    assert "upsert_refused(nan_rollback)" in msg.split("ops so far:")[1].split()[-1]


def test_mutant_replace_forgets_the_host_token_cells(synth_tables, tmp_path, monkeypatch):
    """the engine column is right, the host cells are stale: it surfaces when the column is next rebuilt from them"""
    def replace_token_cells(self, rows, cells):
        tk = getattr(self, "tokens", None)
        if tk is not None and tk["col"] is not None:
            self.index.payload_replace_tokens(tk["col"], np.asarray(rows, np.int64), *LI.pack_tokens(cells, tk["dim"])[:3])
    monkeypatch.setattr(HD._Collection, "replace_token_cells", replace_token_cells)
    msg = caught(maker(FakeHandler), synth_tables, tmp_path)
    assert "token cell" in msg


def test_mutant_retain_leaves_a_payload_column_uncompacted(synth_tables, tmp_path):
    class Lazy(HFakeIndex):
        def retain(self, keep):
            cols = {c: v for c, v in self.cols.items()}
            removed = super().retain(keep)
            if removed and cols:
                c = min(cols)
                if c in self.cols:
                    self.cols[c] = cols[c]
            return removed

    class Mutant(FakeHandler):
        index_type = Lazy
    caught(maker(Mutant), synth_tables, tmp_path)


def test_mutant_load_forgets_the_binary_copy(synth_tables, tmp_path, monkeypatch):
    """_Collection.load without its binary_enable(): while a load runs, the index ignores that call"""
    real = HD._Collection.load.__func__

    class Deaf(HFakeIndex):
        loading = False

        def binary_enable(self):
            if not Deaf.loading:
                super().binary_enable()

    def load(cls, base, device, index_loader=None):
        Deaf.loading = True
        try:
            return real(cls, base, device, index_loader)
        finally:
            Deaf.loading = False

    class Mutant(FakeHandler):
        index_type = Deaf
    monkeypatch.setattr(HD._Collection, "load", classmethod(load))
    msg = caught(maker(Mutant), synth_tables, tmp_path, [c for c in H.CASES if c[1] == "binary"])
    assert "the index keeps a binary copy" in msg and last_op(msg).startswith("save_load(")


def test_mutant_term_statistics_keep_the_count_from_before_a_delete(synth_tables, tmp_path):
    """a fake whose sparse_idf_host answers with the N of the rows before the last retain"""
    class Stale(HFakeIndex):
        old_n = None

        def retain(self, keep):
            self.finalize()
            self.old_n = self._term_table()[1]
            return super().retain(keep)

        def sparse_idf_host(self, idx, val, want_stats=False):
            out = super().sparse_idf_host(idx, val, want_stats=True)
            if self.old_n is not None:
                out = (out[0], out[1], self.old_n)
            return out if want_stats else out[0]

    class Mutant(FakeHandler):
        index_type = Stale
    cases = [c for c in H.CASES if c[1] == "idf"]
    msg = caught(maker(Mutant), synth_tables, tmp_path, cases)
    assert "term_stats n_docs" in msg and last_op(msg).startswith("delete(")


# ---- the brute-force restatement -------------------------------------------------------------------------------------------
def replay(ops, pool):
    """the state after `ops`, re-derived from the log from scratch: plain lists, one point at a time.  Ids are the
    model's made-up ones, in the order the model hands them out."""
    rows, defs, dead, tdim, synth = [], {}, set(), None, 0      # rows: [id, spec, kind, has tokens]

    def payload(row):
        return H.doc_payload(pool, row[1]) if row[2] == "doc" else H.chat_payload(pool, row[1])

    def fits(key, row):
        return H.conforms(H.SCHEMAS[key], payload(row).get(key, H._MISSING))

    def arrive(new):
        for key in defs:
            if key not in dead and not all(fits(key, r) for r in new):
                dead.add(key)

    def recreate(key):
        dead.discard(key)
        if not all(fits(key, r) for r in rows):
            dead.add(key)

    for op in ops:
        k = op["kind"]
        if k == "store" or (k == "index" and op["form"] == "poison"):
            new = []
            for spec in op["specs"]:
                synth += 1
                new.append([f"synth-{synth}", spec, "chat" if op.get("what") == "chats" else "doc", tdim is not None])
            rows += new
            arrive(new)
        elif k == "upsert":
            tail, swapped = [], []
            for target, spec in op["items"]:
                if target is not None and target[0] == "pos":
                    rows[target[1]] = [rows[target[1]][0], spec, "doc", tdim is not None]
                    swapped.append(rows[target[1]])
                elif target is not None:
                    tail.append([target[1], spec, "doc", tdim is not None])
                else:
                    synth += 1
                    tail.append([f"synth-{synth}", spec, "doc", tdim is not None])
            rows += tail
            arrive(tail + swapped)
        elif k == "delete":
            ids = [r[0] for r in rows]
            flt = op["flt"]

            def res(f):
                if isinstance(f, dict):
                    if "has_id_pos" in f:
                        return {"has_id": [ids[q] for q in f["has_id_pos"] if q < len(ids)] + list(f.get("also", []))}
                    return {a: res(b) for a, b in f.items()}
                return [res(x) for x in f] if isinstance(f, list) else f
            gone = set(op["pos"])
            if flt is not None:
                gone |= {q for q, r in enumerate(rows) if H.F.matches(payload(r), res(flt), r[0])}
            rows = [r for q, r in enumerate(rows) if q not in gone]
        elif k == "index":
            f, key = op["form"], op["key"]
            if f in ("create", "recreate"):
                defs[key] = H.SCHEMAS[key]
                recreate(key)
            elif f == "drop":
                del defs[key]
                dead.discard(key)
            elif f == "cure":
                rows = [r for r in rows if fits(key, r)]
                recreate(key)
        elif k == "token_index" and op["form"].startswith("create"):
            tdim = H.TDIM
        elif k == "save_load":
            for key in list(defs):
                recreate(key)
    return rows, defs, dead, tdim


@pytest.mark.parametrize("seed,profile", H.CASES)
def test_model_equals_the_state_rederived_from_the_log(synth_tables, seed, profile):
    p = H.PROFILES[profile]
    pool = H.pool_of(p["dim"], synth_tables)
    ops = H.sequence(seed, p["n_ops"], profile, pool)
    m = H.Model(profile, pool)
    for step, op in enumerate(ops):
        m.apply(op)
        rows, defs, dead, tdim = replay(ops[:step + 1], pool)
        what = (seed, profile, step, H.brief(op))
        assert [(q["id"], q["spec"], q["kind"]) for q in m.pts] == [(r[0], r[1], r[2]) for r in rows], what
        assert [q["tokf"] is not None for q in m.pts] == [r[3] and H.token_floats(pool, r[1]) is not None for r in rows], what
        assert (m.defs, m.dead, m.tdim) == (defs, dead, tdim), what
