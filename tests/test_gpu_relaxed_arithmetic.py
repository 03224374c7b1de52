"""Relaxed arithmetic through the generated gfx950 kernel: the hazard table of tests/relaxed_cases.py (a quotient consumed by a rounding,
a convert, a compare, a select or a remainder) in f64 and f32, every row its own case, and the two device primitives of a relaxed
build — m_rcp_relaxed and m_rsqrt_relaxed — against exact arithmetic.  CPU twin: tests/test_relaxed_arithmetic_host.py."""
import math
from fractions import Fraction

import numpy as np
import pytest

import elodin_amd as ea
from elodin_amd import _lib as L
from elodin_amd import codegen, dsl, workloads
from elodin_amd import stablehlo as sh
from tests import relaxed_cases as R

pytestmark = pytest.mark.gpu


def _run(text, slots, out_slots, arith, inputs, dtype=np.float64, want_in_source=()):
    """One world per row (mode "world"): the module's scalar arguments are width-1 columns, its packed results wide ones."""
    system, manifest = sh.world_system(text, slots, out_slots, mode="world", arith=arith)
    assert manifest["mode"] == "world" and manifest.get("arith") == ("relaxed" if arith == "relaxed" else None)
    if want_in_source:
        dsl.Expr.fresh()
        tp = dsl.Program([system], dsl.Pipe([]), []).trace({c["column"]: c["width"] for c in manifest["columns"]})
        src = codegen.generate_source(tp, "float64", 2)
        assert all(w in src for w in want_in_source), want_in_source
    n = len(next(iter(inputs.values())))
    columns = {"hlo_" + k: np.asarray(v, dtype=np.float64).reshape(n, 1) for k, v in inputs.items()}
    columns.update({"hlo_" + name: np.zeros((n, shape[0] if shape else 1)) for name, shape, _ in out_slots})
    w = workloads.independent_bodies(n)
    hip = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], integrator=L.INTEGRATOR_NONE,
                     effectors=dsl.Program([system], dsl.Pipe([]), []), columns=columns, dtype=dtype)
    hip.run(1)
    got = {k: np.asarray(v, dtype=np.float64).copy() for k, v in hip._aux.items()}
    hip.close()
    return got


def _assert_table(got, want, labels, x, y, c, where):
    bad = []
    for j in np.flatnonzero((got != want).any(axis=0)):
        r = np.flatnonzero(got[:, j] != want[:, j])
        bad.append(f"{labels[j]}: {len(r)} rows, first (row {r[0]}) x={x[r[0]]!r} y={y[r[0]]!r} c={c[r[0]]!r} got {got[r[0], j]!r} want {want[r[0], j]!r}")
    print(f"{where}: {got.shape[0]} rows x {got.shape[1]} consumers, {len(bad)} consumers with a wrong row")
    assert not bad, f"{where}: {len(bad)} of {len(labels)} outputs wrong:\n" + "\n".join(bad[:12])


_F64 = {}


def _f64_table():
    if not _F64:
        x, y, c, kinds = R.rows()
        text, slots, out_slots, labels = R.hlo_module(R.specs("hlo"), R.YS, R.specs("hlo", const_den=True))
        _F64.update(x=x, y=y, c=c, text=text, slots=slots, out_slots=out_slots, labels=labels, want=R.hlo_expected(labels, x, y, c))
    return _F64


@pytest.mark.parametrize("arith", ["reference", "relaxed"])
def test_hazard_table_f64_through_the_generated_kernel(arith):
    """Full waves and a ragged one, every consumer of x / y and of x / const in every row, against the rational reference: all exact in
    BOTH builds — the reference build guards the harness itself.  (Every division of the relaxed build is an exact one here: each
    quotient of the table sits under a protected consumer.)"""
    t = _f64_table()
    assert len(t["x"]) >= 65 and len(t["x"]) % 64
    got = _run(t["text"], t["slots"], t["out_slots"], arith, {"x": t["x"], "y": t["y"], "c": t["c"]},
               want_in_source=("fp contract(fast)", "= m_div(") if arith == "relaxed" else ("= m_div(",))
    _assert_table(R.unpack(got, t["out_slots"]), t["want"], t["labels"], t["x"], t["y"], t["c"], f"f64 {arith}")


_F32 = {}


def _f32_table():
    if not _F32:
        ys = R.hazard_denominators(np.float32)
        x, y, c, kinds = R.rows(np.float32, ys, R.half_pairs(np.float32, ys))
        kinds, k = np.array(kinds), c
        # the hazard is real in float32 for these pairs (same sides as the f64 table: tests/test_relaxed_arithmetic_host.py)
        sides = {"floor": (kinds == "exact") & (k > 0), "ceil": (kinds == "exact") & (k < 0), "trunc": kinds == "exact", "rint": kinds == "half"}
        for op, rows in sides.items():
            exact = np.array([R.reference(("id", op, None), a, b, cc, np.float32) for a, b, cc in zip(x[rows], y[rows], c[rows])])
            naive = R.naive(op, x[rows], y[rows])
            assert naive.dtype == np.float32 and 2 * int(np.sum(naive != exact)) >= int(rows.sum()) > 0, (op, int(np.sum(naive != exact)), int(rows.sum()))
        keep = lambda specs: [s for s in specs if s[1] != "convert_i32"]
        text, slots, out_slots, labels = R.hlo_module(keep(R.specs("hlo")), ys, keep(R.specs("hlo", const_den=True)), ty="f32")
        _F32.update(x=x, y=y, c=c, text=text, slots=slots, out_slots=out_slots, labels=labels, want=R.hlo_expected(labels, x, y, c, np.float32))
    return _F32


@pytest.mark.parametrize("arith", ["reference", "relaxed"])
def test_hazard_table_f32_through_the_generated_kernel(arith):
    """The same table in a float32 build (world_system(arith=...) + HipExec(dtype=float32)); denominators, one-ulp neighbours and the
    "hazard is real" check are found in numpy.float32.  Left out: convert f64 -> i32, whose two's-complement wrap the evaluator
    spells as x + 2^31 ... - 2^31 in the program's element type — not exact in float32 in either build, nothing of relaxed arithmetic."""
    t = _f32_table()
    got = _run(t["text"], t["slots"], t["out_slots"], arith, {"x": t["x"], "y": t["y"], "c": t["c"]}, dtype=np.float32)
    _assert_table(R.unpack(got, t["out_slots"]), t["want"], t["labels"], t["x"], t["y"], t["c"], f"f32 {arith}")


# ---- the two primitives ----------------------------------------------------------------------------------------------------------

_PRIM_TEXT = """
module @relaxed_primitives {
  func.func public @main(%a: tensor<f64>, %d: tensor<f64>, %s: tensor<f64>) -> (tensor<f64>, tensor<f64>) {
    %0 = stablehlo.divide %a, %d : tensor<f64>
    %1 = stablehlo.sqrt %s : tensor<f64>
    %2 = stablehlo.divide %a, %1 : tensor<f64>
    return %0, %2 : tensor<f64>, tensor<f64>
  }
}
"""
_LADDER = list(range(-1022, 1024, 64)) + [1023]                     # exponents, steps of 64, both ends


def _rcp_inputs():
    rng = np.random.default_rng(20261019)
    pos = [math.ldexp(1.0, e) for e in _LADDER]
    pos += [math.ldexp(1.0 + float(m), e) for e in _LADDER for m in rng.random(2)]
    pos += [np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 3.0] + [float(y) for y in R.YS]
    pos += [np.finfo(np.float64).max, np.finfo(np.float64).tiny]
    pos += [math.ldexp(1.0, -1074), math.ldexp(1.0, -1040), math.ldexp(1.0, -1023), math.ldexp(3.0, -1025)]
    pos += [0.0, np.inf]
    return np.array([s * v for v in pos for s in (1.0, -1.0)] + [np.nan], dtype=np.float64)


def _rsqrt_inputs():
    """-> (values, class per value).  rsqrt_pos is documented for finite x > 0 only (csrc/spatial.hpp): zero, negatives, subnormals, inf
    and NaN are left out."""
    rng = np.random.default_rng(20261020)
    v = [(math.ldexp(1.0 + float(m), e), "low exponents" if e < -340 else ("high exponents" if e > 340 else "mid exponents"))
         for e in _LADDER for m in [0.0, *rng.random(3)]]
    v += [(float(k * k), "perfect squares") for k in (2, 3, 5, 7, 10, 49, 1000, 94906265)] + [(q, "perfect squares") for q in (0.25, 0.0625, 1.0 / 1024.0)]
    v += [(float(np.nextafter(1.0, 0.0)), "1 +- 1 ulp"), (float(np.nextafter(1.0, 2.0)), "1 +- 1 ulp")]
    v += [(float(np.finfo(np.float64).max), "high exponents"), (float(np.finfo(np.float64).tiny), "low exponents")]
    return np.array([x for x, _ in v], dtype=np.float64), [c for _, c in v]


def _ulps(got, exact):
    """|got - exact| in ulps of the correctly rounded exact value (a Fraction)."""
    return float(abs(Fraction(got) - exact) / Fraction(math.ulp(float(exact))))


def _inv_sqrt(s, bits=160):
    """1 / sqrt(s) = sqrt(p q) / q for 1 / s = p / q, from math.isqrt on scaled integers: relative error below 2^-bits."""
    r = 1 / Fraction(s)
    p, q = r.numerator, r.denominator
    return Fraction(math.isqrt((p * q) << (2 * bits)), q << bits)


def test_relaxed_reciprocal_and_inverse_square_root_against_exact_arithmetic():
    """out = a / d with the column a = 1.0 is m_rcp_relaxed(d) unchanged, out = a / sqrt(s) is m_rsqrt_relaxed(s).
    Reciprocal (fractions.Fraction): a normal result within 1 ulp of 1 / x (the bound codegen.py and csrc/spatial.hpp state);
    +-0 -> +-inf, +-inf -> +-0, NaN -> NaN; a subnormal x whose reciprocal overflows -> +-inf like an IEEE divide; a subnormal x
    with a finite reciprocal: finite, right sign, 1e-9 relative; |x| > 2^1022 (subnormal result): finite, right sign, within 2^-1022.
    Inverse square root (math.isqrt): 2 ulp — the seed's error e leaves (5/16) e^3 < 1/2 ulp of series, plus one rounding inside e and
    one in the closing fma.  Inputs: positive normals only, see _rsqrt_inputs."""
    d, (s, s_classes) = _rcp_inputs(), _rsqrt_inputs()
    n = max(len(d), len(s))
    assert n >= 65
    dd, ss = np.concatenate([d, np.ones(n - len(d))]), np.concatenate([s, np.ones(n - len(s))])
    slots = [("a", (), True), ("d", (), True), ("s", (), True)]
    out_slots = [("rcp", (), True), ("rsqrt", (), True)]
    got = _run(_PRIM_TEXT, slots, out_slots, "relaxed", {"a": np.ones(n), "d": dd, "s": ss},
               want_in_source=("= m_rcp_relaxed(", "= m_rsqrt_relaxed("))
    rcp, rsq = got["hlo_rcp"][:len(d), 0], got["hlo_rsqrt"][:len(s), 0]
    worst, bad = {}, []
    tiny = math.ldexp(1.0, -1022)
    for x, g in zip(d, rcp):
        x, g = float(x), float(g)
        if x != x:
            ok, cls = g != g, "nan"
        elif x == 0.0 or math.isinf(x):
            ok, cls = (g == (math.copysign(math.inf, x) if x == 0.0 else 0.0) and math.copysign(1.0, g) == math.copysign(1.0, x)), "zero / inf"
        else:
            exact = 1 / Fraction(x)
            if abs(exact) >= Fraction(2) ** 1024 - Fraction(2) ** 970:              # rounds to inf: an IEEE divide overflows
                ok, cls = g == math.copysign(math.inf, x), "subnormal x, overflow"
            elif abs(x) < tiny:
                err = _ulps(g, exact)
                ok, cls = math.isfinite(g) and (g > 0) == (x > 0) and abs(Fraction(g) - exact) <= abs(exact) * Fraction(1, 10 ** 9), "subnormal x, finite"
                worst[cls] = max(worst.get(cls, 0.0), err)
            elif abs(exact) < Fraction(tiny):
                ok, cls = math.isfinite(g) and math.copysign(1.0, g) == math.copysign(1.0, x) and abs(Fraction(g) - exact) <= Fraction(tiny), "subnormal result"
                worst[cls] = max(worst.get(cls, 0.0), float(abs(Fraction(g) - exact) / Fraction(math.ldexp(1.0, -1074))))
            else:
                err = _ulps(g, exact) if math.isfinite(g) else math.inf
                ok, cls = err <= 1.0, "normal"
                worst[cls] = max(worst.get(cls, 0.0), err)
        if not ok:
            bad.append(f"m_rcp_relaxed({x!r}) [{cls}] = {g!r}")
    print("m_rcp_relaxed worst error in ulps per input class (subnormal result: in units of 2^-1074): " + repr(worst))
    worst_s = {}
    for x, g, cls in zip(s, rsq, s_classes):
        x, g = float(x), float(g)
        exact = _inv_sqrt(x)
        err = _ulps(g, exact) if math.isfinite(g) else math.inf
        worst_s[cls] = max(worst_s.get(cls, 0.0), err)
        if not err + 2.0 ** -100 <= 2.0:
            bad.append(f"m_rsqrt_relaxed({x!r}) = {g!r}: {err:.3f} ulp")
    print("m_rsqrt_relaxed worst error in ulps per input class: " + repr(worst_s))
    assert not bad, "\n".join(bad)
