"""Score boosting on the host: the model of hx_formula's arithmetic, the compiler of a formula
into its postfix program, and the path a boosted search takes when its formula does not compile.

Qdrant's `FormulaQuery(formula, defaults)` over the hybrid prefetch, as this project states it (parity unpinned).  An
EXPRESSION is

  a number (an `int` or `float`, not a `bool`)      the constant, as a double;
  "$score"                                          the score the pool carried for the point, as a double;
  any other `str`                                   a payload VARIABLE: the `int` / `float` (not a `bool`, not a NaN) that
                                                    `filters._get(payload, key)` gives, else `defaults[key]`;
  a filter condition or a filter dict               1.0 when `filters.matches` holds for the point, else 0.0 (a dict
                                                    with "must" / "should" / "must_not", or with "key", "has_id",
                                                    "is_empty", "is_null" or "nested");
  {"sum": [e, ...]} / {"mult": [e, ...]}            at least one term, folded from the left: ((e0 + e1) + e2) ...;
  {"neg": e}  {"abs": e}  {"sqrt": e}  {"exp": e}   sqrt of a negative number is a NaN; exp is `hx_exp`;
  {"div": {"left": e, "right": e, "by_zero_default": number}}
                                                    right == 0.0: by_zero_default, a NaN without one;
  {"pow": {"base": e, "exponent": e}}  {"ln": e}  {"log10": e}
                                                    Python path only; outside the function's domain a NaN;
  {"datetime": v}                                   a `datetime.datetime` or RFC 3339 string as SECONDS since the epoch:
                                                    float(microseconds) / 1e6;
  {"datetime_key": key}                             the payload's datetime at `key`, likewise; a value that is no
                                                    datetime gives the default -- `defaults[key]`, a datetime, an RFC
                                                    3339 string or a number of seconds;
  {"lin_decay" | "exp_decay" | "gauss_decay": {"x": e, "target": e = 0, "scale": number = 1, "midpoint": number = 0.5}}
                                                    with d = x + (-target): max(0, 1 - c |d|), c = (1 - midpoint) / scale;
                                                    hx_exp(c |d|), c = ln(midpoint) / scale; hx_exp(c (d d)), c =
                                                    ln(midpoint) / (scale scale).  scale > 0, 0 < midpoint < 1.

Every operation is one IEEE double operation in the order written above (Python's float arithmetic is exactly that), and
`hx_exp` is the engine's own exponential (include/hx.h), so `evaluate` gives the bits k_formula gives for every formula
that compiles.  A NaN stays a NaN through every operation but a `div` by zero.  The VALUE of a point is
`value_f32(evaluate(...))`: the double rounded to fp32, + 0.0f; a point whose value is not finite is dropped; `rank`
orders the rest by value descending, then pool position ascending.

A variable without an entry in `defaults` is a ValueError (Qdrant fails at run time, on the first point that lacks the
field; here the formula is refused up front by `check`), and so are a default that is not a number, a scale <= 0, a
midpoint outside (0, 1), an empty sum or mult, and an unknown expression key.

`compile` DECLINES (returns None, the reason counted in the payload index's `declined`): pow / ln / log10, a variable
whose key has no live "number" index (a datetime_key: no live "datetime" index), a condition `PayloadIndex.compile`
declines, more than 8 distinct conditions, a program of more than 256 ops or deeper than 16 entries."""
from __future__ import annotations

import datetime as _dt
import math
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np

from . import filters as _filters
from . import payload_index as _pindex
from . import scrolling as _scrolling

# hx.h
(F_CONST, F_SCORE, F_VAR, F_COND, F_ADD, F_MUL, F_NEG, F_ABS, F_DIV, F_SQRT, F_EXP, F_LIN_DECAY, F_EXP_DECAY,
 F_GAUSS_DECAY) = range(14)
MAX_OPS, MAX_STACK, MAX_PLANES = 256, 16, 8
MAX_LIMIT = 2048

_NAN = float("nan")
_INF = float("inf")
_LOG2E = 1.4426950408889634
_LN2_HI = 6.93147180369123816490e-01
_LN2_LO = 1.90821492927058770002e-10
_EXP_C = tuple(1.0 / float(math.factorial(i)) for i in range(14))
_FILTER_KEYS = ("must", "should", "must_not", "key", "has_id", "is_empty", "is_null", "nested")
_UNARY = ("neg", "abs", "sqrt", "exp", "ln", "log10")
_DECAYS = {"lin_decay": F_LIN_DECAY, "exp_decay": F_EXP_DECAY, "gauss_decay": F_GAUSS_DECAY}
_KEYS = ("sum", "mult", "div", "pow", "datetime", "datetime_key") + _UNARY + tuple(_DECAYS)


def hx_exp(x: float) -> float:
    """hx.h's exponential on one double."""
    if x != x:
        return x
    if x > 709.0:
        return _INF
    if x < -708.0:
        return 0.0
    k = round(x * _LOG2E)                                  # (round half to even: rint)
    kf = float(k)
    r = (x - kf * _LN2_HI) - kf * _LN2_LO
    p = _EXP_C[13]
    for i in range(12, -1, -1):
        p = p * r + _EXP_C[i]
    return math.ldexp(p, k)


def value_f32(x: float) -> np.float32:
    """The value of a position: the double rounded to fp32 (out of range: +-inf), + 0.0f."""
    with np.errstate(over="ignore"):
        return np.float32(np.float64(x).astype(np.float32) + np.float32(0.0))


def rank(values, limit: int, score_threshold: Optional[float] = None) -> Tuple[List[int], int]:
    """values[i] = the fp32 value of pool position i, or None for a position that is not eligible -> (the positions of
    the hits, value descending then position ascending, at most `limit`; the positions dropped for a value that is
    not finite)."""
    thr = None if score_threshold is None or score_threshold != score_threshold else np.float32(score_threshold)
    live, dropped = [], 0
    for i, v in enumerate(values):
        if v is None:
            continue
        if not math.isfinite(v):
            dropped += 1
        elif thr is None or not v < thr:
            live.append((-float(v), i))
    live.sort()
    return [i for _, i in live[:limit]], dropped


def _number(v, what: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
        raise ValueError(f"{what} must be a number that is not a NaN, got {v!r}")
    return float(v)


def _is_condition(e) -> bool:
    return isinstance(e, dict) and any(k in e for k in _FILTER_KEYS)


def condition_filter(e: Dict[str, Any]) -> Dict[str, Any]:
    """The filter dict of a condition term: itself, or the bare condition under "must"."""
    return e if any(k in e for k in ("must", "should", "must_not")) else {"must": [e]}


def _default(defaults, key) -> float:
    if not isinstance(defaults, dict) or key not in defaults:
        raise ValueError(f"the variable {key!r} has no entry in `defaults`")
    return _number(defaults[key], f"defaults[{key!r}]")


def _default_micros(defaults, key) -> float:
    """The default of a datetime_key as the double of its microseconds."""
    if not isinstance(defaults, dict) or key not in defaults:
        raise ValueError(f"the variable {key!r} has no entry in `defaults`")
    v = defaults[key]
    if isinstance(v, (str, _dt.datetime)):
        us = _scrolling.datetime_micros(v)
        if us is None:
            raise ValueError(f"defaults[{key!r}] is no RFC 3339 datetime: {v!r}")
        return float(us)
    return _number(v, f"defaults[{key!r}]") * 1e6


def _datetime_const(v) -> float:
    us = _scrolling.datetime_micros(v) if isinstance(v, (str, _dt.datetime)) else None
    if us is None:
        raise ValueError(f"datetime must be a datetime or an RFC 3339 string, got {v!r}")
    return float(us) / 1e6


def _one_key(e: Dict[str, Any]) -> str:
    if len(e) != 1 or next(iter(e)) not in _KEYS:
        raise ValueError(f"unknown expression key(s) {sorted(map(str, e))}: an expression holds one of {sorted(_KEYS)}")
    return next(iter(e))


def _terms(v, name: str) -> list:
    if not isinstance(v, (list, tuple)) or not v:
        raise ValueError(f"{name} takes a list of at least one expression")
    return list(v)


def _decay_params(name: str, d) -> Tuple[Any, Any, float]:
    """(x, target, the op's constant) of a decay."""
    if not isinstance(d, dict) or "x" not in d or set(d) - {"x", "target", "scale", "midpoint"}:
        raise ValueError(f'{name} takes {{"x", "target", "scale", "midpoint"}} with an "x"')
    scale = _number(d.get("scale", 1.0), "scale")
    midpoint = _number(d.get("midpoint", 0.5), "midpoint")
    if not scale > 0.0 or scale == _INF:
        raise ValueError(f"scale must be a positive finite number, got {scale!r}")
    if not 0.0 < midpoint < 1.0:
        raise ValueError(f"midpoint must lie in (0, 1), got {midpoint!r}")
    if name == "lin_decay":
        c = (1.0 - midpoint) / scale
    elif name == "exp_decay":
        c = math.log(midpoint) / scale
    else:
        c = math.log(midpoint) / (scale * scale)
    return d["x"], d.get("target", 0.0), c


def _div_params(d) -> Tuple[Any, Any, float]:
    if not isinstance(d, dict) or "left" not in d or "right" not in d or set(d) - {"left", "right", "by_zero_default"}:
        raise ValueError('div takes {"left", "right", "by_zero_default"} with both sides')
    bz = d.get("by_zero_default")
    return d["left"], d["right"], _NAN if bz is None else _number(bz, "by_zero_default")


def _pow_params(d) -> Tuple[Any, Any]:
    if not isinstance(d, dict) or set(d) != {"base", "exponent"}:
        raise ValueError('pow takes {"base", "exponent"}')
    return d["base"], d["exponent"]


def check(formula, defaults=None) -> None:
    """ValueError for a formula no evaluation can serve (the module's docstring lists them); a condition's clause names
    are checked as `filters.matches` checks them."""
    if isinstance(formula, bool) or formula is None:
        raise ValueError(f"an expression is a number, a string or a dict, got {formula!r}")
    if isinstance(formula, (int, float)):
        _number(formula, "a constant")
        return
    if isinstance(formula, str):
        if formula != "$score":
            _default(defaults, formula)
        return
    if not isinstance(formula, dict):
        raise ValueError(f"an expression is a number, a string or a dict, got {formula!r}")
    if _is_condition(formula):
        _filters.matches({}, condition_filter(formula))
        return
    name = _one_key(formula)
    arg = formula[name]
    if name in ("sum", "mult"):
        for t in _terms(arg, name):
            check(t, defaults)
    elif name in _UNARY:
        check(arg, defaults)
    elif name == "div":
        left, right, _ = _div_params(arg)
        check(left, defaults)
        check(right, defaults)
    elif name == "pow":
        for t in _pow_params(arg):
            check(t, defaults)
    elif name == "datetime":
        _datetime_const(arg)
    elif name == "datetime_key":
        if not isinstance(arg, str):
            raise ValueError("datetime_key takes a payload key")
        _default_micros(defaults, arg)
    else:
        x, target, _ = _decay_params(name, arg)
        check(x, defaults)
        check(target, defaults)


def evaluate(formula, defaults, score: float, payload, point_id=None) -> float:
    """The double a formula gives for one point: `score` = the score the pool carried (the fp32 as a Python float)."""
    e = formula
    if isinstance(e, bool) or e is None:
        raise ValueError(f"an expression is a number, a string or a dict, got {e!r}")
    if isinstance(e, (int, float)):
        return _number(e, "a constant")
    if isinstance(e, str):
        if e == "$score":
            return float(score)
        v = _filters._get(payload, e)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
            return _default(defaults, e)
        try:
            return float(v)
        except OverflowError:
            return _default(defaults, e)
    if not isinstance(e, dict):
        raise ValueError(f"an expression is a number, a string or a dict, got {e!r}")
    if _is_condition(e):
        return 1.0 if _filters.matches(payload, condition_filter(e), point_id) else 0.0
    name = _one_key(e)
    arg = e[name]
    ev = lambda x: evaluate(x, defaults, score, payload, point_id)   # noqa: E731
    if name == "sum" or name == "mult":
        terms = _terms(arg, name)
        acc = ev(terms[0])
        for t in terms[1:]:
            acc = acc + ev(t) if name == "sum" else acc * ev(t)
        return acc
    if name == "neg":
        return -ev(arg)
    if name == "abs":
        return abs(ev(arg))
    if name == "sqrt":
        a = ev(arg)
        return _NAN if a < 0.0 else a if a != a or a == _INF else math.sqrt(a)
    if name == "exp":
        return hx_exp(ev(arg))
    if name == "ln" or name == "log10":
        a = ev(arg)
        if a != a or a < 0.0:
            return _NAN
        if a == 0.0:
            return -_INF
        return a if a == _INF else (math.log(a) if name == "ln" else math.log10(a))
    if name == "div":
        left, right, bz = _div_params(arg)
        a, b = ev(left), ev(right)
        return bz if b == 0.0 else a / b
    if name == "pow":
        base, exponent = _pow_params(arg)
        a, b = ev(base), ev(exponent)
        try:
            return math.pow(a, b)
        except ValueError:
            return _NAN
        except OverflowError:
            return _INF
    if name == "datetime":
        return _datetime_const(arg)
    if name == "datetime_key":
        v = _filters._get(payload, arg)
        us = _scrolling.datetime_micros(v) if isinstance(v, (str, _dt.datetime)) else None
        return (_default_micros(defaults, arg) if us is None else float(us)) / 1e6
    x, target, c = _decay_params(name, arg)
    d = ev(x)
    d = d + (-ev(target))
    if name == "lin_decay":
        t = 1.0 - c * abs(d)
        return 0.0 if t < 0.0 else t
    if name == "exp_decay":
        return hx_exp(c * abs(d))
    return hx_exp(c * (d * d))


class _Decline(Exception):
    pass


def compile(formula, defaults, payload_index, id_rows: Optional[Callable[[], Dict[Any, int]]] = None):   # noqa: A001
    """(ops, condition filters) for hx_formula -- ops: (op, arg, imm) triples, a VAR's arg = its engine column, a COND's
    arg = the entry of the filter list whose row mask is its plane -- or None when the formula is declined (the reason
    is counted in payload_index.declined).  ValueError as `check`."""
    check(formula, defaults)
    ops: List[Tuple[int, int, int]] = []
    conds: List[Dict[str, Any]] = []
    cond_keys: Dict[str, int] = {}
    bits = _pindex.f64_bits

    def var(key: str, schema: str, default: float):
        k = payload_index.keys.get(key) if payload_index is not None else None
        if k is None or k.col is None or k.schema != schema or k.array:
            raise _Decline(f"formula variable without a live {schema} index")
        ops.append((F_VAR, k.col, bits(default)))

    def emit(e):
        if isinstance(e, (int, float)):
            ops.append((F_CONST, 0, bits(float(e))))
        elif isinstance(e, str):
            if e == "$score":
                ops.append((F_SCORE, 0, 0))
            else:
                var(e, "number", _default(defaults, e))
        elif _is_condition(e):
            flt = condition_filter(e)
            fk = _filters.filter_key(flt)
            if fk not in cond_keys:
                if payload_index is None or payload_index.compile(flt, id_rows) is None:
                    raise _Decline("formula condition declined")
                if len(conds) >= MAX_PLANES:
                    raise _Decline("formula with more than 8 conditions")
                cond_keys[fk] = len(conds)
                conds.append(flt)
            ops.append((F_COND, cond_keys[fk], 0))
        else:
            name = _one_key(e)
            arg = e[name]
            if name in ("sum", "mult"):
                terms = _terms(arg, name)
                emit(terms[0])
                for t in terms[1:]:
                    emit(t)
                    ops.append((F_ADD if name == "sum" else F_MUL, 0, 0))
            elif name in ("neg", "abs", "sqrt", "exp"):
                emit(arg)
                ops.append(({"neg": F_NEG, "abs": F_ABS, "sqrt": F_SQRT, "exp": F_EXP}[name], 0, 0))
            elif name in ("pow", "ln", "log10"):
                raise _Decline(f"formula with {name}")
            elif name == "div":
                left, right, bz = _div_params(arg)
                emit(left)
                emit(right)
                ops.append((F_DIV, 0, bits(bz)))
            elif name == "datetime":
                ops.append((F_CONST, 0, bits(_datetime_const(arg))))
            elif name == "datetime_key":
                var(arg, "datetime", _default_micros(defaults, arg))
                ops.append((F_CONST, 0, bits(1e6)))
                ops.append((F_DIV, 0, bits(_NAN)))
            else:
                x, target, c = _decay_params(name, arg)
                emit(x)
                emit(target)
                ops.append((F_NEG, 0, 0))
                ops.append((F_ADD, 0, 0))
                ops.append((_DECAYS[name], 0, bits(c)))

    try:
        emit(formula)
        if len(ops) > MAX_OPS or stack_depth(ops) > MAX_STACK:
            raise _Decline("formula program over the limits")
    except _Decline as d:
        if payload_index is not None:
            payload_index.declined[str(d)] = payload_index.declined.get(str(d), 0) + 1
        return None
    return ops, conds


def stack_depth(ops) -> int:
    """The most entries the stack of a program holds."""
    depth = most = 0
    for op, _, _ in ops:
        depth += 1 if op <= F_COND else -1 if op in (F_ADD, F_MUL, F_DIV) else 0
        most = max(most, depth)
    return most
