"""Relaxed arithmetic (dsl.relaxed_arithmetic, stablehlo.world_system(arith="relaxed")) where a quotient meets a rounding or a compare,
on the CPU: a / d becomes a * (1 / d), an ulp in the quotient, which is a whole unit behind floor / ceil / trunc / rint, a convert to an
integer, a compare, a select's predicate or a mod.  Such a consumer must see the exact IEEE division (tests/relaxed_cases.py: the
table, spelled as traced DSL code with a column and with a constant denominator, and as StableHLO text; the reference is rational
arithmetic, never the reference-mode trace of the code under test).  tests/test_gpu_relaxed_arithmetic.py runs the table through the
generated gfx950 kernel."""
import numpy as np
import pytest

from elodin_amd import codegen, dsl
from elodin_amd import stablehlo as sh
from tests import dsl_numpy
from tests import relaxed_cases as R

X, Y, C, KINDS = R.rows()
EXACT = np.array([k != "ulp" for k in KINDS])


def _walk_exprs(build):
    """The table's traced values (built under relaxed arithmetic over the leaves x, y, c) on the numpy walker -> [rows, outputs]"""
    dsl.Expr.fresh()
    with dsl.relaxed_arithmetic():
        outs = build(dsl.np, dsl.leaf("x"), dsl.leaf("y"), dsl.leaf("c"))
    return np.stack(dsl_numpy._eval([dsl._lift(o) for o in outs], {"x": X, "y": Y, "c": C}, len(X)), axis=1)


def _check(got, labels, where):
    """Every row of every output against the rational reference; the rows whose quotient is not representable also against numpy's
    IEEE x / y followed by the op (what the reference trace is documented to be)."""
    bad = []
    for j, (den, spec) in enumerate(labels):
        d = Y if den is None else np.full(len(X), float(den))
        want = np.array([R.reference(spec, x, yy, c) for x, yy, c in zip(X, d, C)])
        ulp_rows = ~np.array([R.ieee_quotient(x, yy)[1] for x, yy in zip(X, d)])
        assert np.array_equal(R.numpy_reference(spec, X / d, C)[ulp_rows], want[ulp_rows]), (where, den, spec)      # the two references agree
        miss = np.flatnonzero(got[:, j] != want)
        if len(miss):
            r = miss[0]
            bad.append(f"{where} den={den} {spec}: {len(miss)} rows, first x={X[r]!r} y={d[r]!r} c={C[r]!r} got {got[r, j]!r} want {want[r]!r}")
    assert not bad, f"{len(bad)} of {len(labels)} outputs wrong:\n" + "\n".join(bad[:12])


def test_the_hazard_is_real_for_the_table_s_inputs():
    """Keeps the input list from going stale: op(x * (1 / y)) in numpy is wrong for at least half of the exact-quotient pairs on the
    side from which the op meets the step.  x * (1 / y) falls SHORT of k in magnitude, so floor steps down only for k > 0, ceil steps up
    only for k < 0, trunc loses a unit on both sides, and rint only notices at a half-way quotient (k + 1/2, even y)."""
    kinds, k = np.array(KINDS), C
    sides = {"floor": (kinds == "exact") & (k > 0), "ceil": (kinds == "exact") & (k < 0), "trunc": kinds == "exact", "rint": kinds == "half"}
    for op, rows in sides.items():
        exact = np.array([R.reference(("id", op, None), x, y, c) for x, y, c in zip(X[rows], Y[rows], C[rows])])
        assert all(R.ieee_quotient(x, y)[1] for x, y in zip(X[rows], Y[rows]))
        wrong = int(np.sum(R.naive(op, X[rows], Y[rows]) != exact))
        print(f"naive {op}(x * (1 / y)): {wrong} of {int(rows.sum())} exact-quotient pairs wrong")
        assert 2 * wrong >= int(rows.sum()) > 0, (op, wrong)
    # the issue's own count: floor(x * (1 / y)) != x // y for 45 of the 50 pairs of tests/test_stablehlo_ingest.py
    base = (kinds == "exact") & (k > 0)
    assert int(np.sum(np.floor(X[base] * (1.0 / Y[base])) != X[base] // Y[base])) == 45 and int(base.sum()) == 50


def test_hazard_table_traced_dsl_code_with_a_column_denominator():
    front = R.specs("dsl")
    got = _walk_exprs(lambda xp, x, y, c: R.dsl_outputs(xp, x, y, c, front))
    _check(got, [(None, s) for s in front], "dsl, y a column")


@pytest.mark.parametrize("den", R.YS)
def test_hazard_table_traced_dsl_code_with_a_constant_denominator(den):
    front = R.specs("dsl", const_den=True)
    got = _walk_exprs(lambda xp, x, y, c: R.dsl_outputs(xp, x, float(den), c, front))
    _check(got, [(den, s) for s in front], "dsl, y a constant")


def _hlo_walk(text, slots, out_slots, arith, columns):
    system, manifest = sh.world_system(text, slots, out_slots, mode="world", arith=arith)
    assert manifest.get("arith") == ("relaxed" if arith == "relaxed" else None) and manifest["mode"] == "world"
    widths = {c["column"]: c["width"] for c in manifest["columns"]}
    dsl.Expr.fresh()
    tp = dsl.Program([system], dsl.Pipe([]), []).trace(widths)
    n = len(next(iter(columns.values())))
    comps = {"hlo_" + k: np.array(v, dtype=np.float64).reshape(n, 1) for k, v in columns.items()}
    for nm, w in tp.columns:
        comps.setdefault(nm, np.zeros((n, w)))
    pos, vel, acc, inertia = np.tile([0, 0, 0, 1.0, 0, 0, 0], (n, 1)), np.zeros((n, 6)), np.zeros((n, 6)), np.ones((n, 7))
    dsl_numpy.program_tick_systems_only(tp, pos, vel, acc, inertia, comps, 1)
    return tp, comps


def test_hazard_table_stablehlo_text_through_world_system():
    """floor / ceil / round_nearest_even, convert f64 -> i32 and -> i64, compare (six directions, against a constant and a column),
    select, remainder, each also behind negate and abs — with the denominator an argument, and with it a constant of the module."""
    text, slots, out_slots, labels = R.hlo_module(R.specs("hlo"), R.YS, R.specs("hlo", const_den=True))
    _, comps = _hlo_walk(text, slots, out_slots, "relaxed", {"x": X, "y": Y, "c": C})
    _check(R.unpack(comps, out_slots), labels, "stablehlo, relaxed")


# ---- A2: one realistic shape ---------------------------------------------------------------------------------------------------

DT = 1.0 / 128.0                   # exact in binary: tick * DT and 49 * DT are exact, so the IEEE quotient at a multiple of the period is k
PERIOD = 49 * DT


def test_a_cadence_counter_counts_whole_periods_for_200_ticks():
    """floor(tick * dt / period), period = 49 dt: the count steps at ticks 49, 98, 147, 196 — with the period a constant and a column."""
    ticks = np.arange(1, 201, dtype=np.float64)
    naive = np.floor(ticks * DT * (1.0 / PERIOD))
    assert np.array_equal(np.floor(ticks * DT / PERIOD), ticks // 49) and int(np.sum(naive != ticks // 49)) >= 3      # the hazard is real

    @dsl.system(count=1, count_col=1, period=1)
    def cadence(tick, count, count_col, period):
        return {"count": dsl.np.floor(tick * DT / PERIOD), "count_col": dsl.np.floor(tick * DT / period)}
    dsl.Expr.fresh()
    with dsl.relaxed_arithmetic():
        tp = dsl.Program([cadence], dsl.Pipe([]), []).trace({"count": 1, "count_col": 1, "period": 1})
    n = 2
    comps = {"count": np.zeros((n, 1)), "count_col": np.zeros((n, 1)), "period": np.full((n, 1), PERIOD)}
    pos, vel, acc, inertia = np.tile([0, 0, 0, 1.0, 0, 0, 0], (n, 1)), np.zeros((n, 6)), np.zeros((n, 6)), np.ones((n, 7))
    for tick in range(1, 201):
        dsl_numpy.program_tick_systems_only(tp, pos, vel, acc, inertia, comps, tick)
        assert comps["count"][0, 0] == tick // 49 and comps["count_col"][0, 0] == tick // 49, (tick, comps["count"][0, 0], comps["count_col"][0, 0])


# ---- A3: sharing survives ------------------------------------------------------------------------------------------------------

def _nodes(roots):
    seen, todo = {}, list(roots)
    while todo:
        e = todo.pop()
        if id(e) not in seen:
            seen[id(e)] = e
            todo.extend(e.args)
    return list(seen.values())


def test_quotients_of_one_denominator_still_share_one_reciprocal_beside_a_protected_floor():
    dsl.Expr.fresh()
    with dsl.relaxed_arithmetic():
        a, b, c, y = (dsl.leaf(n) for n in ("a", "b", "c", "y"))
        outs = [a / y, b / y, c / y, dsl.np.floor(a / y)]
    divs = [e for e in _nodes(outs) if e.op == "div"]
    shared = [e for e in divs if e.value == dsl.RELAXED_RCP]
    exact = [e for e in divs if e.value != dsl.RELAXED_RCP]
    assert len(divs) == 2 and len(shared) == 1 and len(exact) == 1, [(e.op, e.value) for e in divs]
    assert shared[0].args[0].is_const(1.0) and shared[0].args[1] is y
    assert all(o.op == "mul" and o.args[1] is shared[0] for o in outs[:3])             # three quotients, ONE reciprocal node
    assert outs[3].op == "floor" and outs[3].args[0] is exact[0] and exact[0].args == (a, y)      # the floor sees a / y itself
    leaves = {"a": np.array([49.0, 98.0]), "b": np.array([1.0, 2.0]), "c": np.array([3.0, 5.0]), "y": np.array([49.0, 49.0])}
    got = dsl_numpy._eval(outs, leaves, 2)
    assert np.array_equal(got[3], [1.0, 2.0]) and got[0][0] == 49.0 * (1.0 / 49.0) != 1.0      # ... while the arithmetic use stays relaxed
    # a normalised quaternion's inverse still drops its division by |q^|^2 (dsl._unit_norm_squared reads the tagged reciprocal)
    with dsl.relaxed_arithmetic():
        q = dsl.Vec([dsl.leaf(n) for n in ("q0", "q1", "q2", "q3")])
        unit = q / dsl.np.sqrt(dsl.np.sum(q * q))
        inv = unit / dsl.np.sum(unit * unit)
    assert all(p is r for p, r in zip(inv.e, unit.e))


# ---- A4: which reciprocal a build emits ----------------------------------------------------------------------------------------

_RCP_TEXT = """
module @m {
  func.func public @main(%a: tensor<f64>, %d: tensor<f64>, %x: tensor<f64>, %n: tensor<i64>) -> (tensor<f64>, tensor<f64>, tensor<i64>) {
    %one = stablehlo.constant dense<1.000000e+00> : tensor<f64>
    %ione = stablehlo.constant dense<1> : tensor<i64>
    %0 = stablehlo.divide %a, %d : tensor<f64>
    %1 = stablehlo.divide %one, %x : tensor<f64>
    %2 = stablehlo.divide %ione, %n : tensor<i64>
    return %0, %1, %2 : tensor<f64>, tensor<f64>, tensor<i64>
  }
}
"""


def test_a_relaxed_build_emits_the_relaxed_reciprocal_only_for_the_divisions_it_rewrote():
    """a / d is rewritten: m_rcp_relaxed(d).  A `1.0 / x` of the user's keeps its IEEE divide (dsl.py: "a constant numerator keeps its
    IEEE divide"), and so does the 1 / n an integer divide builds while the evaluator suspends the relaxation."""
    slots = [("a", (), True), ("d", (), True), ("x", (), True), ("n", (), True)]
    out_slots = [("q", (), True), ("r", (), True), ("i", (), True)]
    src = {}
    for arith in ("reference", "relaxed"):
        system, manifest = sh.world_system(_RCP_TEXT, slots, out_slots, mode="world", arith=arith)
        dsl.Expr.fresh()
        tp = dsl.Program([system], dsl.Pipe([]), []).trace({c["column"]: c["width"] for c in manifest["columns"]})
        src[arith] = codegen.generate_source(tp, "float64", 2)
        cols = {c: k for k, (c, _) in enumerate(tp.columns)}
    rel, ref = src["relaxed"], src["reference"]
    d, x = f"r.c{cols['hlo_d']}[0]", f"r.c{cols['hlo_x']}[0]"
    assert rel.count("= m_rcp_relaxed(") == 1 and f"= m_rcp_relaxed({d});" in rel, [l for l in rel.splitlines() if "m_rcp_relaxed(" in l or "m_div(" in l]
    assert rel.count("= m_div(T(1.0), ") == rel.count("= m_div(") == 2 and f"= m_div(T(1.0), {x});" in rel, [l for l in rel.splitlines() if "= m_div(" in l]
    assert ref.count("= m_div(") == 3 and "m_rcp_relaxed" not in ref
