"""The hazard table of relaxed arithmetic (dsl.relaxed_arithmetic: a / d as a * (1 / d)), shared by tests/test_relaxed_arithmetic_host.py
and tests/test_gpu_relaxed_arithmetic.py: the inputs whose quotient sits ON a step of a rounding or a compare, the consumers that
turn an ulp of the quotient into a whole unit, the same table spelled as traced DSL code and as StableHLO text, and a reference that
never divides in floating point.  TEST INFRASTRUCTURE."""
import functools
import math
from fractions import Fraction

import numpy as np

KS = (1, 2, 3, 7, 100, -1, -7)                                      # x = k * y: the pair list of tests/test_stablehlo_ingest.py and two negative k
YS = (49, 98, 103, 107, 161, 187, 196, 197, 206, 214)               # denominators whose reciprocal, multiplied back, misses k
HALF_KS = (0, 1, 2, 3, 7, -1, -2, -8)                               # x = (2k + 1) * y / 2 for even y: the quotient is k + 1/2, rint's step
CMP_CONSTS = tuple(sorted({s * abs(k) for k in KS for s in (1.0, -1.0)}))      # the constants a wrapped quotient (neg, abs) is compared with
WRAPS = ("id", "neg", "abs")                                        # "directly" includes one neg / abs between quotient and consumer
ROUNDS = ("floor", "ceil", "trunc", "rint")
CMPS = ("GE", "GT", "LE", "LT", "EQ", "NE")
_PY_CMP = {"GE": lambda a, b: a >= b, "GT": lambda a, b: a > b, "LE": lambda a, b: a <= b, "LT": lambda a, b: a < b,
           "EQ": lambda a, b: a == b, "NE": lambda a, b: a != b}


def hazard_denominators(dtype):
    """Ten denominators found in `dtype`: the first five y with y * (1 / y) != 1 and their doubles (even: rint's half-way rows)."""
    one, base = dtype(1), []
    for y in range(3, 1000):
        if dtype(y) * (one / dtype(y)) != one and y % 2:
            base.append(y)
            if len(base) == 5:
                break
    return tuple(sorted(base + [2 * y for y in base]))


def half_pairs(dtype, ys):
    """(k, y) with a half-way quotient k + 1/2, found in `dtype`: 30 on which rint(x * (1 / y)) is wrong and 10 on which it is right."""
    wrong, right = [], []
    for k in range(-8, 9):
        for y in ys:
            if y % 2 == 0:
                x = dtype((2 * k + 1) * y // 2)
                (wrong if np.rint(x * (dtype(1) / dtype(y))) != np.rint(dtype(k + 0.5)) else right).append((k, y))
    return wrong[:30] + right[:10]


def rows(dtype=np.float64, YS=YS, halves=None):
    """-> x, y, c (arrays of `dtype`), kinds: "exact" (x = k y, c = k), "half" (quotient k + 1/2 = c) and "ulp" (x = k y moved by one
    ulp of `dtype` either way, c = k: the true quotient is not representable)."""
    xs, ys, cs, kinds = [], [], [], []
    for k in KS:
        for y in YS:
            xs.append(k * y), ys.append(y), cs.append(k), kinds.append("exact")
    for k, y in (halves if halves is not None else [(k, y) for k in HALF_KS for y in YS if y % 2 == 0]):
        xs.append((2 * k + 1) * y / 2), ys.append(y), cs.append(k + 0.5), kinds.append("half")
    for k in KS:
        for y in YS:
            for toward in (np.inf, -np.inf):
                xs.append(np.nextafter(dtype(k * y), dtype(toward))), ys.append(y), cs.append(k), kinds.append("ulp")
    return np.array(xs, dtype=dtype), np.array(ys, dtype=dtype), np.array(cs, dtype=dtype), kinds


@functools.lru_cache(maxsize=None)
def ieee_quotient(x, y, dtype=np.float64):
    """The correctly rounded x / y without a floating-point divide -> (the value as a Fraction, whether it IS x / y).  f64: Python's
    integer true division rounds correctly; f32: that double rounded once more (53 >= 2 * 24 + 2 bits: no double rounding)."""
    q = Fraction(float(x)) / Fraction(float(y))
    r = q.numerator / q.denominator
    if dtype is np.float32:
        r = float(np.float32(r))
    return Fraction(r), Fraction(r) == q


def specs(front, const_den=False):
    """The consumers of one quotient, (wrap, consumer, parameter) each.  front "dsl": floor-mod (`%`), trunc / astype(int);
    "hlo": remainder with the dividend's sign, the converts to i32 and i64.  const_den: the short list run per constant denominator."""
    out = []
    for wrap in (WRAPS if not const_den or front == "dsl" else ("id",)):
        for r in ROUNDS:
            if front == "dsl" or r != "trunc":
                out.append((wrap, r, None))
        out.extend([(wrap, "astype_int", None)] if front == "dsl" else [(wrap, "convert_i32", None), (wrap, "convert_i64", None)])
        for d in CMPS:
            out.append((wrap, "cmp_col_" + d, None))
            if not const_den:
                out.extend((wrap, "cmp_const_" + d, t) for t in CMP_CONSTS)
        out.append((wrap, "select", None))
        out.append((wrap, "mod_q_1" if front == "dsl" else "rem_q_1", None))
        if not const_den:      # x / D for a D that is not the row's y: 2c / q is a large ratio, where the device's mod (x - floor(x / y) * y)
            out.append((wrap, "mod_2c_q" if front == "dsl" else "rem_2c_q", None))      # rounds its product — nothing of relaxed arithmetic
    return out


def reference(spec, x, y, c, dtype=np.float64):
    """What one consumer gives for one row, in exact arithmetic on the correctly rounded quotient (for an exact quotient: on x / y)."""
    wrap, op, t = spec
    q, _ = ieee_quotient(x, y, dtype)
    q = -q if wrap == "neg" else (abs(q) if wrap == "abs" else q)
    c = Fraction(float(c))
    if op in ("floor", "ceil", "trunc", "astype_int", "convert_i32", "convert_i64"):
        return float({"floor": math.floor, "ceil": math.ceil}.get(op, math.trunc)(q))
    if op == "rint":
        return float(round(q))                                        # Fraction.__round__: half to even
    if op.startswith("cmp_"):
        return float(_PY_CMP[op[-2:]](q, c if t is None else Fraction(t)))
    if op == "select":
        return 10.0 if q >= c else 20.0
    a, b = (q, Fraction(1)) if op.endswith("q_1") else (2 * c, q)
    r = a % b if op.startswith("mod") else (abs(a) % abs(b)) * (-1 if a < 0 else 1)      # the divisor's sign / the dividend's
    return float(r)                                                   # Fraction -> float rounds correctly where the floor-mod is not representable


def numpy_reference(spec, q, c):
    """The documented reference trace for a quotient that is not representable: numpy's IEEE q = x / y, then the op in numpy."""
    wrap, op, t = spec
    q = -q if wrap == "neg" else (np.abs(q) if wrap == "abs" else q)
    if op in ("floor", "ceil", "rint"):
        return getattr(np, op)(q)
    if op in ("trunc", "astype_int", "convert_i32", "convert_i64"):
        return np.trunc(q)
    if op.startswith("cmp_"):
        return _PY_CMP[op[-2:]](q, c if t is None else q.dtype.type(t)).astype(q.dtype)
    if op == "select":
        return np.where(q >= c, 10.0, 20.0).astype(q.dtype)
    a, b = (q, q.dtype.type(1)) if op.endswith("q_1") else (2 * c, q)
    return np.mod(a, b) if op.startswith("mod") else np.fmod(a, b)


def naive(op, x, y):
    """The form relaxed arithmetic must NOT hand a rounding: op(x * (1 / y)) in numpy."""
    one = x.dtype.type(1)
    return {"floor": np.floor, "ceil": np.ceil, "trunc": np.trunc, "rint": np.rint}[op](x * (one / y))


# ---- the table as traced DSL code ------------------------------------------------------------------------------------------------

def dsl_outputs(xp, x, y, c, front_specs):
    """[one traced value per spec] for the quotient x / y (y: a traced column, or a Python number)."""
    out = []
    for wrap, op, t in front_specs:
        q = x / y
        w = -q if wrap == "neg" else (xp.abs(q) if wrap == "abs" else q)
        if op in ROUNDS:
            v = getattr(xp, op)(w)
        elif op == "astype_int":
            v = w.astype(int)
        elif op.startswith("cmp_"):
            other = c if t is None else t
            p = {"GE": lambda: w >= other, "GT": lambda: w > other, "LE": lambda: w <= other, "LT": lambda: w < other,
                 "EQ": lambda: w == other, "NE": lambda: w != other}[op[-2:]]()
            v = xp.where(p, 1.0, 0.0)
        elif op == "select":
            v = xp.where(w >= c, 10.0, 20.0)
        elif op == "mod_q_1":
            v = w % 1.0
        else:
            v = xp.remainder(2.0 * c, w)
        out.append(v)
    return out


# ---- the table as StableHLO text: one world per row (mode "world"), scalar arguments, results packed into columns of <= 64 --------

COLUMN = 64


def hlo_module(front_specs, const_dens=(), const_specs=(), ty="f64"):
    """-> (text, slots, out_slots, labels): @main(x, y, c) applies every spec of `front_specs` to x / y and every spec of `const_specs`
    to x / D for each constant D of `const_dens`; labels[k] = (denominator | None, spec) of packed result k (row-major over the
    result columns out0, out1, ...)."""
    T = f"tensor<{ty}>"
    lines, n = [], [0]

    def emit(rhs, rt=T):
        n[0] += 1
        lines.append(f"    %v{n[0]} = {rhs}" + (f" : {rt}" if rt else ""))      # rt None: the statement carries its own types
        return f"%v{n[0]}"

    def const(v):
        return emit(f"stablehlo.constant dense<{float(v)!r}>")
    one, two, ten, twenty = const(1.0), const(2.0), const(10.0), const(20.0)
    c2 = emit("stablehlo.multiply %c, " + two)
    labels, values = [], []
    for den, group in [(None, front_specs)] + [(d, const_specs) for d in const_dens]:
        q = emit(f"stablehlo.divide %x, {'%y' if den is None else const(den)}")
        wrapped = {"id": q}
        for wrap, op, t in group:
            if wrap not in wrapped:
                wrapped[wrap] = emit(f"stablehlo.{'negate' if wrap == 'neg' else 'abs'} {q}")
            w = wrapped[wrap]
            if op in ("floor", "ceil", "rint"):
                v = emit(f"stablehlo.{'round_nearest_even' if op == 'rint' else op} {w}")
            elif op.startswith("convert_"):
                i = emit(f"stablehlo.convert {w} : ({T}) -> tensor<{op[-3:]}>", None)
                v = emit(f"stablehlo.convert {i} : (tensor<{op[-3:]}>) -> {T}", None)
            elif op.startswith("cmp_") or op == "select":
                d = "GE" if op == "select" else op[-2:]
                p = emit(f"stablehlo.compare  {d}, {w}, {'%c' if t is None else const(t)},  FLOAT : ({T}, {T}) -> tensor<i1>", None)
                v = emit(f"stablehlo.select {p}, {ten}, {twenty} : tensor<i1>, {T}", None) if op == "select" else \
                    emit(f"stablehlo.convert {p} : (tensor<i1>) -> {T}", None)
            elif op == "rem_q_1":
                v = emit(f"stablehlo.remainder {w}, {one}")
            elif op == "rem_2c_q":
                v = emit(f"stablehlo.remainder {c2}, {w}")
            else:
                raise ValueError(op)
            labels.append((den, (wrap, op, t)))
            values.append(emit(f"stablehlo.reshape {v} : ({T}) -> tensor<1x{ty}>", None))
    outs, out_types = [], []
    for k in range(0, len(values), COLUMN):
        part = values[k:k + COLUMN]
        rt = f"tensor<{len(part)}x{ty}>"
        outs.append(emit(f"stablehlo.concatenate {', '.join(part)}, dim = 0 : ({', '.join([f'tensor<1x{ty}>'] * len(part))}) -> {rt}", None))
        out_types.append(rt)
    text = (f"module @relaxed_hazards {{\n  func.func public @main(%x: {T}, %y: {T}, %c: {T}) -> ({', '.join(out_types)}) {{\n"
            + "\n".join(lines) + f"\n    return {', '.join(outs)} : {', '.join(out_types)}\n  }}\n}}\n")
    slots = [("x", (), True), ("y", (), True), ("c", (), True)]
    out_slots = [(f"out{k}", (min(COLUMN, len(values) - k * COLUMN),), True) for k in range(len(outs))]
    return text, slots, out_slots, labels


def hlo_expected(labels, x, y, c, dtype=np.float64):
    """[rows, len(labels)]: the rational reference of every packed result for every row."""
    return np.array([[reference(spec, xi, yi if den is None else den, ci, dtype) for den, spec in labels]
                     for xi, yi, ci in zip(x, y, c)])


def unpack(columns, out_slots, prefix="hlo_"):
    return np.concatenate([np.asarray(columns[prefix + name], dtype=np.float64) for name, _, _ in out_slots], axis=1)
