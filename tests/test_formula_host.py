"""Score boosting on the host, no GPU: boosting.evaluate against an independent brute-force
evaluator (exact rational arithmetic rounded once per operation), hx_exp against math.exp, the compiler's programs and
declines, tests/formula_helpers.py (the numpy restatement of hx_formula) against evaluate followed by sorted(), and the
handler -- its refusals, its Python path and its device path -- over stub indexes answered by the helpers."""
from __future__ import annotations

import asyncio
import datetime as dt
import math
import random
from fractions import Fraction

import numpy as np
import pytest

from rag_application_amd import boosting as B
from rag_application_amd import filters as F
from rag_application_amd.handler import BoostedPoint, QdrantHandler, ScoredPoint, _Collection
from rag_application_amd.payload_index import PayloadIndex, _Key
from tests import formula_helpers as H

P = dict(matryoshka_64_limit=100, matryoshka_128_limit=80, matryoshka_256_limit=60, dense_limit=40, quantized_limit=40,
         sparse_limit=50, final_limit=30, hnsw_ef=128)
NAN, INF = float("nan"), float("inf")
EPOCH = dt.datetime(1970, 1, 1, tzinfo=dt.timezone.utc)


def same(a: float, b: float) -> bool:
    return (a != a and b != b) or H.bits(a) == H.bits(b)


# ---- the brute-force evaluator: every exact operation as a rational, rounded once -----------------------------------------
def _exact(fn, plain, *xs):
    """fn over the Fractions of finite doubles, rounded once; the plain float operation where an operand is not finite or
    the exact result is 0 (the sign of a zero is IEEE's own rule)."""
    if not all(math.isfinite(x) for x in xs):
        return plain(*xs)
    q = fn(*[Fraction(x) for x in xs])
    if q == 0:
        return plain(*xs)
    try:
        return float(q)                      # (int / int true division: correctly rounded)
    except OverflowError:
        return INF if q > 0 else -INF


def fadd(a, b):
    return _exact(lambda x, y: x + y, lambda x, y: x + y, a, b)


def fmul(a, b):
    return _exact(lambda x, y: x * y, lambda x, y: x * y, a, b)


def fdiv(a, b):
    return _exact(lambda x, y: x / y, lambda x, y: x / y, a, b)


def brute_exp(x):
    if x != x:
        return x
    if x > 709.0:
        return INF
    if x < -708.0:
        return 0.0
    k = round(Fraction(fmul(x, 1.4426950408889634)))                     # (half to even)
    r = fadd(fadd(x, -fmul(float(k), 6.93147180369123816490e-01)), -fmul(float(k), 1.90821492927058770002e-10))
    p = fdiv(1.0, float(math.factorial(13)))
    for i in range(12, -1, -1):
        p = fadd(fmul(p, r), fdiv(1.0, float(math.factorial(i))))
    return float(Fraction(p) * Fraction(2) ** k)


def brute_micros(v):
    if isinstance(v, str):
        try:
            v = dt.datetime.fromisoformat(v.replace("Z", "+00:00"))
        except ValueError:
            return None
    if not isinstance(v, dt.datetime):
        return None
    if v.tzinfo is None:
        v = v.replace(tzinfo=dt.timezone.utc)
    return (v - EPOCH) // dt.timedelta(microseconds=1)


def brute_cond(c, payload):
    if any(k in c for k in ("must", "should", "must_not")):
        must = all(brute_cond(x, payload) for x in c.get("must", []))
        mnot = any(brute_cond(x, payload) for x in c.get("must_not", []))
        should = c.get("should", [])
        return must and not mnot and (not should or any(brute_cond(x, payload) for x in should))
    v = payload.get(c["key"])
    vals = v if isinstance(v, (list, tuple)) else (v,)                  # (a list matches when one element does)
    if "match" in c:
        want = c["match"]["value"]
        return any(x is not None and type(x) is type(want) and x == want for x in vals)
    r = c["range"]
    return any(not isinstance(x, bool) and isinstance(x, (int, float))
               and all(op(x, r[k]) for k, op in (("gte", lambda a, b: a >= b), ("lt", lambda a, b: a < b)) if k in r)
               for x in vals)


def brute(e, defaults, score, payload):
    ev = lambda x: brute(x, defaults, score, payload)   # noqa: E731
    if isinstance(e, (int, float)):
        return float(e)
    if e == "$score":
        return float(score)
    if isinstance(e, str):
        v = payload.get(e)
        return float(v) if isinstance(v, (int, float)) and not isinstance(v, bool) and v == v else float(defaults[e])
    if any(k in e for k in ("must", "should", "must_not", "key")):
        return 1.0 if brute_cond(e, payload) else 0.0
    (name, a), = e.items()
    if name == "sum":
        acc = ev(a[0])
        for t in a[1:]:
            acc = fadd(acc, ev(t))
        return acc
    if name == "mult":
        acc = ev(a[0])
        for t in a[1:]:
            acc = fmul(acc, ev(t))
        return acc
    if name == "neg":
        return fmul(-1.0, ev(a))                         # (an exact product: the sign flips, a NaN stays one)
    if name == "abs":
        return math.copysign(ev(a), 1.0)
    if name == "div":
        x, y = ev(a["left"]), ev(a["right"])
        if y == 0.0:
            return float(a["by_zero_default"]) if "by_zero_default" in a else NAN
        return fdiv(x, y)
    if name == "sqrt":
        x = ev(a)
        if x != x or x < 0.0:
            return NAN
        if x == 0.0 or x == INF:
            return x
        q = Fraction(x)                                  # correctly rounded: the double nearest to the exact root
        y = math.sqrt(x)
        cands = [y, math.nextafter(y, 0.0), math.nextafter(y, INF)]
        lo = max(c for c in cands if Fraction(c) ** 2 <= q)
        hi = math.nextafter(lo, INF)
        mid = (Fraction(lo) + Fraction(hi)) / 2
        if mid ** 2 == q:                                # (cannot happen for a double: a root is never a midpoint)
            return lo
        return lo if mid ** 2 > q else hi
    if name == "exp":
        return brute_exp(ev(a))
    if name in ("ln", "log10"):
        x = ev(a)
        if x != x or x < 0.0:
            return NAN
        if x == 0.0:
            return -INF
        return x if x == INF else (math.log(x) if name == "ln" else math.log10(x))
    if name == "pow":
        try:
            return math.pow(ev(a["base"]), ev(a["exponent"]))
        except ValueError:
            return NAN
        except OverflowError:
            return INF
    if name == "datetime":
        return fdiv(float(brute_micros(a)), 1e6)
    if name == "datetime_key":
        us = brute_micros(payload.get(a))
        if us is None:
            d = defaults[a]
            us = brute_micros(d) if isinstance(d, (str, dt.datetime)) else None
            return fdiv(float(us), 1e6) if us is not None else fdiv(fmul(float(d), 1e6), 1e6)
        return fdiv(float(us), 1e6)
    scale, mid = float(a.get("scale", 1.0)), float(a.get("midpoint", 0.5))
    d = fadd(ev(a["x"]), fmul(-1.0, ev(a.get("target", 0.0))))
    if name == "lin_decay":
        t = fadd(1.0, -fmul(fdiv(fadd(1.0, -mid), scale), math.copysign(d, 1.0)))
        return 0.0 if t < 0.0 else t
    if name == "exp_decay":
        return brute_exp(fmul(fdiv(math.log(mid), scale), math.copysign(d, 1.0)))
    return brute_exp(fmul(fdiv(math.log(mid), fmul(scale, scale)), fmul(d, d)))


# ---- random payloads and formula trees ----------------------------------------------------------------------------------------
DEFAULTS = {"n": 1.5, "m": -2, "ts": "2024-03-01T00:00:00Z", "ts2": 1.7e9}
T0 = dt.datetime(2024, 3, 1, tzinfo=dt.timezone.utc)


def rand_payload(rng: random.Random, poison: bool = True):
    p = {}
    u = rng.random()
    if u < 0.10:
        pass
    elif u < 0.15:
        p["n"] = None
    else:
        p["n"] = rng.choice([rng.randint(-50, 50), rng.uniform(-30, 30), -0.0, 0, 2 ** 53, -(2 ** 53), 1e-3, 705.5, -709.25])
    if rng.random() < 0.8:
        p["m"] = rng.choice([rng.randint(-5, 5), rng.uniform(-800.0, 800.0), 0.0])
    u = rng.random()
    if u < 0.10:
        pass
    elif u < 0.15:
        p["ts"] = None
    else:
        t = T0 + dt.timedelta(seconds=rng.randint(-40 * 86400, 40 * 86400), microseconds=rng.randint(0, 999999))
        kind = rng.randrange(4)
        p["ts"] = (t if kind == 0 else t.replace(tzinfo=None) if kind == 1
                   else t.strftime("%Y-%m-%dT%H:%M:%S.%fZ") if kind == 2
                   else t.astimezone(dt.timezone(dt.timedelta(hours=5, minutes=30))).isoformat())
    if poison and rng.random() < 0.05:
        p["n"] = rng.choice(["12", True, [1, 2], NAN])                  # (no number: the default)
    if poison and rng.random() < 0.05:
        p["ts"] = rng.choice([17, "yesterday", [T0]])
    if rng.random() < 0.9:
        p["tag"] = rng.choice(["chat", "pdf", "doc"])
    return p


CONDS = [{"key": "tag", "match": {"value": "chat"}},
         {"must": [{"key": "tag", "match": {"value": "pdf"}}], "must_not": [{"key": "n", "range": {"gte": 0}}]},
         {"key": "n", "range": {"gte": -10, "lt": 10}}]


def rand_tree(rng: random.Random, depth: int, device_only: bool = False):
    if depth == 0 or rng.random() < 0.25:
        k = rng.randrange(8)
        if k == 0:
            return rng.choice([0, 1, -1, 0.5, 2.5, -0.0, 1e-3, 3, 100.0, -700.0])
        if k == 1:
            return "$score"
        if k == 2:
            return rng.choice(["n", "m"])
        if k == 3:
            return {"datetime_key": "ts"}
        if k == 4:
            return {"datetime": rng.choice(["2024-03-05T12:00:00Z", "2024-02-20T08:30:00+02:00", T0])}
        if k == 5:
            return rng.choice(CONDS)
        return rng.uniform(-3, 3)
    sub = lambda: rand_tree(rng, depth - 1, device_only)   # noqa: E731
    names = ["sum", "mult", "neg", "abs", "div", "sqrt", "exp", "lin_decay", "exp_decay", "gauss_decay"]
    if not device_only:
        names += ["pow", "ln", "log10"]
    name = rng.choice(names)
    if name in ("sum", "mult"):
        return {name: [sub() for _ in range(rng.randint(1, 3))]}
    if name in ("neg", "abs", "sqrt", "exp", "ln", "log10"):
        return {name: sub()}
    if name == "div":
        d = {"left": sub(), "right": sub()}
        if rng.random() < 0.5:
            d["by_zero_default"] = rng.choice([0, 1.0, -2.5])
        return {"div": d}
    if name == "pow":
        return {"pow": {"base": sub(), "exponent": rng.choice([2, 0.5, -1, sub()])}}
    d = {"x": sub()}
    if rng.random() < 0.7:
        d["target"] = sub()
    if rng.random() < 0.7:
        d["scale"] = rng.choice([1, 0.25, 86400.0, 7 * 86400, 3.5])
    if rng.random() < 0.7:
        d["midpoint"] = rng.choice([0.5, 0.1, 0.9, 0.01])
    return {name: d}


@pytest.mark.parametrize("seed", range(12))
def test_evaluate_equals_the_brute_force_evaluator(seed):
    rng = random.Random(5000 + seed)
    n = [0, 1, 7, 300][seed % 4] if seed < 4 else rng.randint(0, 300)
    payloads = [rand_payload(rng) for _ in range(n)]
    for _ in range(25):
        tree = rand_tree(rng, rng.randint(0, 4))
        B.check(tree, DEFAULTS)
        for r, p in enumerate(payloads):
            score = float(np.float32(rng.uniform(-1, 1)))
            got, want = B.evaluate(tree, DEFAULTS, score, p, f"p{r}"), brute(tree, DEFAULTS, score, p)
            assert same(got, want), (tree, p, score, got, want)


def test_evaluate_edge_values():
    ev = lambda e, s=0.25, p=None: B.evaluate(e, DEFAULTS, s, p or {})   # noqa: E731
    assert same(ev({"neg": 0}), -0.0) and same(ev({"abs": -0.0}), 0.0) and same(ev({"sqrt": -0.0}), -0.0)
    assert ev({"sqrt": -1}) != ev({"sqrt": -1})
    assert ev({"div": {"left": 1, "right": 0}}) != ev({"div": {"left": 1, "right": 0}})
    assert ev({"div": {"left": "$score", "right": -0.0, "by_zero_default": 7}}) == 7.0
    assert ev({"exp": 710}) == INF and ev({"exp": -708.5}) == 0.0 and ev({"exp": -708}) > 0.0
    assert ev("n", p={"n": 2 ** 53}) == float(2 ** 53) and ev("n", p={"n": None}) == 1.5 and ev("n", p={"n": "3"}) == 1.5
    assert ev({"datetime_key": "ts"}, p={"ts": "1970-01-01T00:00:01.5Z"}) == 1.5
    assert ev({"datetime_key": "ts2"}) == 1.7e9 * 1e6 / 1e6
    assert ev({"lin_decay": {"x": 5, "scale": 2}}) == 0.0 and ev({"lin_decay": {"x": 1, "scale": 2}}) == 0.75
    assert ev({"exp_decay": {"x": 3, "target": 1, "scale": 2}}) == B.hx_exp(math.log(0.5) / 2 * 2.0)
    assert float(B.value_f32(1e39)) == INF and H.bits(float(B.value_f32(-0.0))) == 0
    assert B.rank([np.float32(1), None, np.float32(NAN), np.float32(2), np.float32(1), np.float32(INF)], 10) == ([3, 0, 4], 2)
    assert B.rank([np.float32(1), np.float32(2), np.float32(3)], 10, 2.0) == ([2, 1], 0)


def test_formula_value_errors():
    bad = ["x",                                                       # a variable without a default
           {"sum": []}, {"mult": "n"}, {"frobnicate": 1}, {"sum": [1], "mult": [2]}, None, True, [1, 2], NAN,
           {"div": {"left": 1}}, {"div": {"left": 1, "right": 2, "by_zero_default": "0"}}, {"pow": {"base": 1}},
           {"lin_decay": {"x": 1, "scale": 0}}, {"exp_decay": {"x": 1, "scale": -1}}, {"gauss_decay": {"target": 1}},
           {"exp_decay": {"x": 1, "midpoint": 0}}, {"exp_decay": {"x": 1, "midpoint": 1}}, {"lin_decay": {"x": 1, "midpoint": 1.5}},
           {"gauss_decay": {"x": 1, "sigma": 2}}, {"datetime": "noon"}, {"datetime": 5}, {"datetime_key": "missing"},
           {"datetime_key": 5}, {"mustn't": []}, {"must": [], "mustnt": []}]
    for f in bad:
        with pytest.raises(ValueError):
            B.check(f, DEFAULTS)
        with pytest.raises(ValueError):
            B.compile(f, DEFAULTS, None)
    with pytest.raises(ValueError, match="defaults"):
        B.check("n", {"n": "1"})
    with pytest.raises(ValueError, match="defaults"):
        B.check({"datetime_key": "ts"}, {"ts": "soon"})
    with pytest.raises(ValueError):
        B.evaluate("x", {}, 0.0, {})


# ---- hx_exp ---------------------------------------------------------------------------------------------------------------------
def test_hx_exp_against_math_exp():
    """Measured on [-708, 709] over the points below: at most 1.0 eps from math.exp on either side of 0; the bound is
    that, as an integer number of eps."""
    rng = np.random.default_rng(20270)
    ln2 = math.log(2.0)
    xs = np.concatenate([rng.uniform(-708.0, 709.0, 1_000_000),
                         [-708.0, 709.0, 0.0, -0.0, 1.0, -1.0, 1e-300, -1e-300, 708.999, -707.999],
                         np.arange(-1021, 1024) * ln2, (np.arange(-1021, 1024) + 0.5) * ln2])
    xs = xs[(xs >= -708.0) & (xs <= 709.0)]
    ref = np.array([math.exp(x) for x in xs.tolist()])
    got = H.hx_exp(xs)
    err = np.abs(got - ref) / np.spacing(ref)
    print("hx_exp: largest error", err.max(), "eps at", xs[err.argmax()], "; below 0:", err[xs <= 0].max())
    assert err.max() <= 1.0
    assert np.isfinite(got).all() and (got >= 2.0 ** -1022).all()       # no subnormal, no overflow inside the range
    some = xs[:: max(1, len(xs) // 20000)]
    assert np.array_equal(np.array([B.hx_exp(x) for x in some.tolist()]), H.hx_exp(some))   # the scalar and the numpy form
    for x in rng.uniform(-708.0, 709.0, 300).tolist() + [-708.0, 709.0, 0.0]:
        assert B.hx_exp(x) == brute_exp(x)
    edge = np.array([709.0000001, 1e308, INF, -708.0000001, -1e308, -INF])
    assert np.array_equal(H.hx_exp(edge), [INF, INF, INF, 0.0, 0.0, 0.0])
    assert [B.hx_exp(x) for x in edge.tolist()] == [INF, INF, INF, 0.0, 0.0, 0.0]
    assert np.isnan(H.hx_exp(np.array([NAN])))[0] and B.hx_exp(NAN) != B.hx_exp(NAN)


# ---- the compiler ---------------------------------------------------------------------------------------------------------------
def index_over(payloads, live=("n", "m", "ts", "tag")):
    """A PayloadIndex whose keys hold column ids (no engine), and the cells it encodes for `payloads`."""
    pi = PayloadIndex()
    schemas = {"n": "number", "m": "number", "ts": "datetime", "tag": "keyword"}
    columns = {}
    for c, key in enumerate(live):
        pi.keys[key] = _Key(schemas[key], key)
        cells = pi.encode(key, payloads)
        assert cells is not None, key
        pi.keys[key].col = 10 + c
        columns[10 + c] = cells
    return pi, columns


def test_compiler_programs():
    pi, _ = index_over([])
    ops, conds = B.compile({"sum": ["$score", {"mult": [0.2, {"exp_decay": {"x": {"datetime_key": "ts"},
                                                                            "target": {"datetime": "2024-03-01T00:00:00Z"},
                                                                            "scale": 86400}}]}]}, DEFAULTS, pi)
    assert [o[0] for o in ops] == [B.F_SCORE, B.F_CONST, B.F_VAR, B.F_CONST, B.F_DIV, B.F_CONST, B.F_NEG, B.F_ADD,
                                   B.F_EXP_DECAY, B.F_MUL, B.F_ADD]
    assert conds == [] and B.stack_depth(ops) == 4
    assert ops[2][1] == pi.keys["ts"].col and ops[2][2] == H.bits(float(B._scrolling.datetime_micros(DEFAULTS["ts"])))
    assert H.from_bits(ops[3][2]) == 1e6 and H.from_bits(ops[8][2]) == math.log(0.5) / 86400.0
    ops, conds = B.compile({"mult": ["$score", {"sum": [1, {"mult": [-0.5, CONDS[0]]}, CONDS[1], CONDS[0]]}]}, DEFAULTS, pi)
    assert conds == [{"must": [CONDS[0]]}, CONDS[1]]                   # one plane per distinct condition
    assert [o[1] for o in ops if o[0] == B.F_COND] == [0, 1, 0]
    ops, _ = B.compile({"div": {"left": "n", "right": "m", "by_zero_default": 3}}, DEFAULTS, pi)
    assert ops == [(B.F_VAR, pi.keys["n"].col, H.bits(1.5)), (B.F_VAR, pi.keys["m"].col, H.bits(-2.0)),
                   (B.F_DIV, 0, H.bits(3.0))]
    ops, _ = B.compile({"div": {"left": 1, "right": 2}}, DEFAULTS, pi)
    assert ops[2][2] == H.NAN_BITS
    left = 1                                                            # a left-deep sum stays shallow, a right-deep one does not
    for _ in range(100):
        left = {"sum": [left, "$score"]}
    ops, _ = B.compile(left, DEFAULTS, pi)
    assert len(ops) == 201 and B.stack_depth(ops) == 2
    right = 1
    for _ in range(15):
        right = {"sum": ["$score", right]}
    ops, _ = B.compile(right, DEFAULTS, pi)
    assert B.stack_depth(ops) == 16 and len(ops) == 31
    assert B.compile(0.5, DEFAULTS, None) == ([(B.F_CONST, 0, H.bits(0.5))], [])   # no variable, no condition: no index needed


def test_compiler_declines():
    pi, _ = index_over([])

    def declined(f, reason, index=pi, defaults=DEFAULTS):
        before = dict(index.declined) if index is not None else {}
        assert B.compile(f, defaults, index) is None, f
        if index is not None:
            assert index.declined.get(reason, 0) == before.get(reason, 0) + 1, (reason, index.declined)

    declined({"pow": {"base": "$score", "exponent": 2}}, "formula with pow")
    declined({"sum": [1, {"ln": "$score"}]}, "formula with ln")
    declined({"log10": 3}, "formula with log10")
    declined({"sum": ["$score", "n"]}, "formula variable without a live number index", PayloadIndex())
    assert B.compile("n", DEFAULTS, None) is None
    declined({"datetime_key": "n"}, "formula variable without a live datetime index", None)
    pi2, _ = index_over([], live=("n", "ts"))
    pi2.keys["n"].col = None                                             # poisoned
    declined("n", "formula variable without a live number index", pi2)
    declined("ts", "formula variable without a live number index", pi2, {"ts": 0})   # a datetime key as a plain variable
    declined({"datetime_key": "n"}, "formula variable without a live datetime index", pi)
    declined(CONDS[0], "formula condition declined", pi2)                # `tag` is not indexed there
    nine = {"sum": [{"key": "tag", "match": {"value": f"v{i}"}} for i in range(9)]}
    declined(nine, "formula with more than 8 conditions")
    assert B.compile({"sum": nine["sum"][:8]}, DEFAULTS, pi) is not None
    right = 1
    for _ in range(16):
        right = {"sum": ["$score", right]}
    declined(right, "formula program over the limits")                  # depth 17
    assert B.compile({"sum": ["$score"] * 128}, DEFAULTS, pi) is not None   # 255 ops
    declined({"sum": ["$score"] * 129}, "formula program over the limits")  # 257 ops


# ---- the helpers' stage against evaluate + sorted() -------------------------------------------------------------------------------
def stage_by_evaluate(tree, payloads, ids, keys, counts, eligible, threshold, limit):
    out = []
    for b in range(keys.shape[0]):
        n = keys.shape[1] if counts is None else int(counts[b])
        vals = []
        for k in keys[b, :n].tolist():
            r = int(H.key_ids(np.uint64(k)))
            if k == 0 or r >= len(payloads) or (eligible is not None and not eligible[r]):
                vals.append(None)
            else:
                s = float(H.key_scores(np.array([k], np.uint64))[0])
                vals.append(B.value_f32(B.evaluate(tree, DEFAULTS, s, payloads[r], ids[r])))
        live = [(-float(v), i) for i, v in enumerate(vals) if v is not None and math.isfinite(v)
                and not (threshold is not None and v < np.float32(threshold))]
        dropped = sum(1 for v in vals if v is not None and not math.isfinite(v))
        hits = [i for _, i in sorted(live)[:limit]]
        out.append((hits, [vals[i] for i in hits], dropped))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_helpers_stage_equals_evaluate_and_sorted(seed):
    rng = random.Random(900 + seed)
    n_rows = [1, 40, 300][seed % 3]
    payloads = [rand_payload(rng, poison=False) for _ in range(n_rows)]
    ids = [f"p{r}" for r in range(n_rows)]
    pi, columns = index_over(payloads)
    nrng = np.random.default_rng(seed)
    done = 0
    while done < 12:
        tree = rand_tree(rng, rng.randint(1, 4), device_only=True)
        prog = B.compile(tree, DEFAULTS, pi)
        if prog is None:
            continue
        done += 1
        ops, conds = prog
        planes = [np.array([F.matches(p, c, i) for p, i in zip(payloads, ids)], bool) for c in conds]
        Bq, stride = 2, rng.choice([1, 5, 70])
        rows = nrng.integers(0, n_rows + 3, (Bq, stride))                # (some rows past the index)
        keys = H.make_keys(nrng.uniform(-1, 1, (Bq, stride)).astype(np.float32), rows)
        keys[nrng.random((Bq, stride)) < 0.1] = 0
        counts = np.array([stride, max(0, stride - 2)], np.int32)
        eligible = None if done % 2 else nrng.random(n_rows) < 0.7
        threshold = None if done % 3 else rng.choice([0.0, 0.5, -1.0])
        limit = rng.choice([1, 3, 100])
        ok, op_, oc, od = H.formula_stage(ops, planes, keys, counts, eligible, threshold, limit, columns, n_rows)
        want = stage_by_evaluate(tree, payloads, ids, keys, counts, eligible, threshold, limit)
        for b, (hits, vals, dropped) in enumerate(want):
            m = len(hits)
            assert oc[b] == m and od[b] == dropped, (tree, b)
            assert op_[b, :m].tolist() == hits and (op_[b, m:] == -1).all() and (ok[b, m:] == 0).all(), (tree, b)
            assert np.array_equal(H.key_scores(ok[b, :m]).view(np.uint32), np.array(vals, np.float32).view(np.uint32)), (tree, b)
            assert H.key_ids(ok[b, :m]).tolist() == H.key_ids(keys[b, hits]).tolist()


# ---- the handler over stub indexes ---------------------------------------------------------------------------------------------------
class PoolIndex:
    """hybrid_query_host over a fixed pool per mode: rows 0 .. 15 in a shuffled order with descending scores"""

    def __init__(self):
        self.calls = []
        order = np.random.default_rng(3).permutation(16)
        self.rows = order
        self.scores = np.linspace(0.95, 0.2, 16).astype(np.float32)

    def count(self):
        return 16

    def pool(self, B, L, mask):
        keep = np.ones(16, bool) if mask is None else np.unpackbits(np.asarray(mask, np.uint32).view(np.uint8),
                                                                     bitorder="little")[:16].astype(bool)
        sel = [i for i in range(16) if keep[self.rows[i]]][:L]
        scores = np.full((B, L), -np.inf, np.float32)
        ids = np.full((B, L), -1, np.int64)
        scores[:, :len(sel)] = self.scores[sel]
        ids[:, :len(sel)] = self.rows[sel]
        return scores, ids, np.full(B, len(sel), np.int32)

    def hybrid_query_host(self, q, indptr, idx, val, hp, mask=None):
        self.calls.append(("plain", int(hp.mode), int(hp.final_limit), mask is not None))
        return self.pool(q.shape[0], int(hp.final_limit), mask)


class FormulaIndex(PoolIndex):
    """... and hybrid_query_formula_host answered by the helpers over the columns of the stub's payloads"""
    columns = None

    def hybrid_query_formula_host(self, q, indptr, idx, val, hp, ops, limit, planes=(), score_threshold=None,
                                  candidates_limit=0, mask=None, mask_root_only=False):
        self.calls.append(("formula", int(hp.mode), limit, candidates_limit, len(planes), score_threshold, mask is not None,
                           bool(mask_root_only)))
        B = q.shape[0]
        scores, ids, counts = self.pool(B, candidates_limit, None if mask_root_only else mask)
        keys = H.make_keys(scores, np.where(ids < 0, 0, ids))
        keys[ids < 0] = 0
        unpack = lambda w: np.unpackbits(np.asarray(w, np.uint32).view(np.uint8), bitorder="little")[:16].astype(bool)  # noqa: E731
        ok, pos, oc, od = H.formula_stage(ops, [unpack(w) for w in planes], keys, counts,
                                          unpack(mask) if mask_root_only and mask is not None else None, score_threshold,
                                          limit, self.columns, 16)
        base = np.full((B, limit), -np.inf, np.float32)
        for b in range(B):
            base[b, :oc[b]] = scores[b, pos[b, :oc[b]]]
        out_ids = np.where(ok == 0, -1, H.key_ids(ok))
        return H.key_scores(ok), out_ids, base, oc, od


def stub_handler(index_cls):
    rng = random.Random(77)
    h = QdrantHandler()
    col = _Collection.__new__(_Collection)
    col.dim, col.msizes, col.sparse_enabled = 4, (), True
    col.index = index_cls()
    col.ids = [f"p{r}" for r in range(16)]
    col.payloads = [rand_payload(rng, poison=False) for _ in range(16)]
    col.payloads[3]["n"] = -1                                           # sqrt("n") is a NaN there
    col._masks, col.tokens = {}, None
    col.pindex, columns = index_over(col.payloads)
    col.index.columns = columns
    h._collections["u"] = col
    return h, col


def search(h, formula, B=2, **kw):
    qs = [[0.1, 0.2, 0.3, 0.4]] * B
    sv = [{"indices": [1, 5], "values": [1.0, 0.5]}] * B
    kw.setdefault("search_params", P)
    kw.setdefault("defaults", DEFAULTS)
    return asyncio.run(h.hybrid_search_boost("u", qs, sv, formula, **kw))


RECENCY = {"sum": ["$score", {"mult": [0.2, {"exp_decay": {"x": {"datetime_key": "ts"}, "target": {"datetime": T0},
                                                          "scale": 10 * 86400}}]}]}
TWO_CONDS = {"mult": ["$score", {"sum": [1, {"mult": [0.5, CONDS[0]]}, {"mult": [-0.5, CONDS[2]]}, CONDS[0]]}]}
NEEDS_DROP = {"sum": ["$score", {"sqrt": "n"}]}
EVEN_TAG = {"must": [{"key": "tag", "match": {"value": "chat"}}]}


def test_handler_device_path_and_python_path_agree(caplog):
    hd, cd = stub_handler(FormulaIndex)
    hp_, cp = stub_handler(PoolIndex)
    for formula in (RECENCY, TWO_CONDS, NEEDS_DROP, "$score", 0.5, {"neg": "$score"}):
        for kw in (dict(), dict(limit=3), dict(mode="h1", candidates_limit=None), dict(score_threshold=0.6),
                   dict(filters=EVEN_TAG), dict(filters=EVEN_TAG, filter_stages="all", mode="h1"), dict(candidates_limit=5)):
            dev, py = search(hd, formula, **kw), search(hp_, formula, **kw)
            assert cd.index.calls[-1][0] == "formula" and cp.index.calls[-1][0] == "plain", (formula, kw)
            assert len(dev) == len(py) == 2
            for a, b in zip(dev, py):
                assert [p.id for p in a] == [p.id for p in b], (formula, kw)
                assert [H.bits(p.score) for p in a] == [H.bits(p.score) for p in b], (formula, kw)
                assert [H.bits(p.base_score) for p in a] == [H.bits(p.base_score) for p in b], (formula, kw)
                assert all(isinstance(p, BoostedPoint) and isinstance(p, ScoredPoint) for p in a + b)
                assert all(x.payload is cd.payloads[int(x.id[1:])] for x in a)
    assert cp.pindex.declined["boost on an index without the formula query"] == 6 * 7
    # what reaches the engine
    search(hd, TWO_CONDS, B=1, limit=4, candidates_limit=7, filters=EVEN_TAG, score_threshold=0.25)
    assert cd.index.calls[-1] == ("formula", 0, 4, 7, 2, 0.25, True, True)   # a root filter: the mask goes to the stage only
    search(hd, "$score", B=1, mode="h1", candidates_limit=None)
    assert cd.index.calls[-1] == ("formula", 1, 10, 90, 0, None, False, False)
    # a constant formula returns the pool in its own order; the drops are logged
    res = search(hd, 1, B=1, limit=16, candidates_limit=16)[0]
    assert [p.id for p in res] == [f"p{r}" for r in cd.index.rows] and {p.score for p in res} == {1.0}
    caplog.clear()
    with caplog.at_level("WARNING"):
        res = search(hd, NEEDS_DROP, B=1, limit=16, candidates_limit=16)[0]
    neg = {f"p{r}" for r, p in enumerate(cd.payloads) if isinstance(p.get("n"), (int, float)) and p["n"] < 0}
    assert "p3" in neg and not neg & {p.id for p in res} and len(res) == 16 - len(neg)
    assert any(f"dropped {len(neg)} points" in r.getMessage() for r in caplog.records)
    # a formula that does not compile goes the Python way on the formula index too, and is counted
    caplog.clear()
    with caplog.at_level("WARNING"):
        res = search(hd, {"pow": {"base": "$score", "exponent": 2}}, B=1, limit=2)[0]
    assert cd.index.calls[-1][0] == "plain" and cd.pindex.declined["formula with pow"] == 1
    assert [H.bits(p.score) for p in res] == [H.bits(float(B.value_f32(p.base_score ** 2))) for p in res]
    assert any("Python path" in r.getMessage() for r in caplog.records)


def test_handler_refusals():
    h, col = stub_handler(FormulaIndex)
    for limit in (0, -1, 2049, 2.0, True, None):
        with pytest.raises(ValueError, match="limit"):
            search(h, "$score", limit=limit)
    for cl in (0, -5, 1.5, True):
        with pytest.raises(ValueError, match="candidates_limit"):
            search(h, "$score", candidates_limit=cl)
    for thr in (NAN, "0.5", True):
        with pytest.raises(ValueError, match="score_threshold"):
            search(h, "$score", score_threshold=thr)
    with pytest.raises(ValueError, match="defaults"):
        search(h, "$score", defaults=[1])
    with pytest.raises(ValueError, match="defaults"):
        search(h, {"sum": ["$score", "popularity"]})
    with pytest.raises(ValueError, match="scale"):
        search(h, {"exp_decay": {"x": "n", "scale": 0}})
    with pytest.raises(ValueError, match="midpoint"):
        search(h, {"gauss_decay": {"x": "n", "midpoint": 1}})
    with pytest.raises(ValueError, match="unknown expression"):
        search(h, {"geo_distance": {"origin": {}, "to": "loc"}})
    with pytest.raises(ValueError, match="root"):
        search(h, "$score", mode="h1", filters=EVEN_TAG)
    with pytest.raises(ValueError, match="mode"):
        search(h, "$score", mode="flat")
    with pytest.raises(ValueError, match="filter_stages"):
        search(h, "$score", filter_stages="none")
    with pytest.raises(ValueError, match="clause"):
        search(h, "$score", filters={"mustnt": []})
    with pytest.raises(ValueError, match="dimension"):
        asyncio.run(h.hybrid_search_boost("u", [[0.1, 0.2]], [{"indices": [1], "values": [1.0]}], "$score", search_params=P))
    assert col.index.calls == []                                        # refused before the engine is asked
    assert search(h, "$score", search_params=None) == []                # any other failure: logged, [] -- as every search
    assert asyncio.run(h.hybrid_search_boost("nobody", [[0.1] * 4], [{"indices": [1], "values": [1.0]}], "$score",
                                             search_params=P)) == []


def test_a_sharded_collection_is_refused():
    from rag_application_amd.sharded import ShardedHandler
    h = ShardedHandler.__new__(ShardedHandler)                          # (no process group: the refusal comes first)
    h._collections, h._lock = {}, None
    assert ShardedHandler._boost_search is False and QdrantHandler._boost_search is True
    with pytest.raises(ValueError, match="sharded"):
        QdrantHandler._boost_sync(h, "u", [[0.0]], [{"indices": [], "values": []}], "$score", None, 10, 100, None, P, None,
                                  "tree", "root")
