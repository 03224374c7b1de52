"""Effector front-end, CPU side: tracing, code generation (hipcc cross-compiles here) and the numpy
stepper that serves as oracle for user-written effectors."""
import os

import numpy as np
import pytest

from elodin_amd import codegen, dsl, workloads
from oracle import oracle as orc
from tests import dsl_numpy, np_sixdof

np_ = dsl.np


@dsl.effector
def gravity(force, inertia):                                     # examples/ball/sim.py:57-59
    return force + dsl.SpatialForce(linear=np_.array([0.0, 0.0, -9.81]) * inertia.mass())


@dsl.effector(body_torque=3)
def rcs(force, pos, body_torque):                                # apollo-lander/sim.py:396-398
    return force + dsl.SpatialForce(torque=pos.angular() @ body_torque)


def test_numpy_stepper_is_bit_identical_to_the_c_oracle():
    w = workloads.independent_bodies(500)
    ops = [(orc.EFF_UNIFORM_GRAVITY, (0, 0, -9.81), None), (orc.EFF_BODY_TORQUE, (), w["body_torque"])]
    inertia = w["inertia"]

    def eff(xs, vs):
        F = np.zeros((len(xs), 6))
        F[:, 3:] = F[:, 3:] + np.array([0.0, 0.0, -9.81]) * inertia[:, 6:7]
        F[:, :3] = F[:, :3] + np_sixdof.rot(xs[:, :4], w["body_torque"])
        return F
    for integ in (0, 1):
        o = orc.OracleWorld(w["world_pos"], w["world_vel"], inertia, simulation_time_step=workloads.DT_120HZ,
                            integrator=integ, ops=ops)
        pos, vel, acc = w["world_pos"].copy(), w["world_vel"].copy(), np.zeros((500, 6))
        for _ in range(5):
            o.step(1)
            pos, vel, acc, F = np_sixdof.tick(pos, vel, acc, inertia, eff, workloads.DT_120HZ, integrator=integ)
        assert np.array_equal(pos, o.world_pos) and np.array_equal(vel, o.world_vel)
        assert np.array_equal(acc, o.world_accel) and np.array_equal(F, o.force)


def test_trace_flags_columns_and_folding():
    tp = (gravity | rcs).trace()
    assert tp.columns == [("body_torque", 3)] and not tp.reads_velocity
    assert tp.body_torque and not tp.world_torque      # `pos.angular() @ x` torque stays in the body frame
    assert "mass" in tp.leaves and "vx" not in tp.leaves
    only_g = dsl.pipe(gravity).trace()
    assert not only_g.world_torque and only_g.columns == []
    assert only_g.outputs[3].op == "mul"               # 0.0 * mass is NOT folded (IEEE: mass may be inf/NaN)
    assert all(t.is_const(0.0) for t in only_g.outputs[:3]) and not only_g.body_torque

    @dsl.effector(wind=3)
    def drag(wind, vel, force):
        fl = wind - vel.linear()
        return dsl.SpatialForce(linear=force.force() + fl)
    assert (gravity | drag).trace().reads_velocity
    with pytest.raises(TypeError):
        dsl.pipe(dsl.effector(lambda force: 3.0)).trace()
    with pytest.raises(TypeError):
        bool(dsl.leaf("x") < 1.0)


def test_dag_matches_direct_numpy():
    tp = (gravity | rcs).trace()
    w = workloads.independent_bodies(64)
    F = dsl_numpy.evaluate(tp, w["world_pos"], w["world_vel"], w["inertia"], {"body_torque": w["body_torque"]})
    assert np.allclose(F[:, 5], -9.81 * w["inertia"][:, 6]) and np.all(F[:, 3:5] == 0)
    assert np.allclose(F[:, :3], np_sixdof.rot(w["world_pos"][:, :4], w["body_torque"]), rtol=1e-13, atol=1e-15)


def test_generated_source_compiles_for_gfx950():
    tp = (gravity | rcs).trace()
    src = codegen.generate_source(tp, "float64", 0)
    assert "struct PipeCustom" in src and "sixdof_custom_launch" in src
    assert "kWorldTorque = false" in src and "kBodyTorque = true" in src
    so = codegen.build(tp, "float64", 0)
    assert so.exists() and so.suffix == ".so"
    assert codegen.build(tp, "float64", 0) == so          # cached by content hash


# ---- user-written edge_fold functions ------------------------------------------------------------------------------

G_NEWTON = 6.6743e-11


@dsl.edge_fold
def gravity_fn(force, a_pos, a_inertia, b_pos, b_inertia):       # examples/three-body/main.py:61-70, verbatim structure
    r = a_pos.linear() - b_pos.linear()
    m = a_inertia.mass()
    M = b_inertia.mass()
    norm = np_.linalg.norm(r)
    f = G_NEWTON * M * m * r / (norm * norm * norm)
    return dsl.SpatialForce(linear=force.force() - f)


def test_edge_fold_trace_against_the_c_oracle_fold():
    """The traced fold, evaluated with numpy in spawn order, equals the oracle's built-in Newton fold on the golden
    three-body initial state."""
    from tests import golden_util as gu
    g = gu.load("three_body")
    pos = np.stack([g[f"{e}.world_pos"][0] for e in "abc"])
    inertia = np.stack([g[f"{e}.inertia"][0] for e in "abc"])
    src, dst = np.array([0, 1, 0, 1, 2, 2]), np.array([1, 0, 2, 2, 0, 1])
    F = dsl_numpy.fold_force(gravity_fn.trace(), pos, inertia, src, dst)
    assert np.all(F[:, :3] == 0.0) and np.all(np.isfinite(F))
    vel = np.stack([g[f"{e}.world_vel"][0] for e in "abc"])
    ow = orc.OracleWorld(pos, vel, inertia, integrator=orc.SEMI_IMPLICIT, edges=(src, dst),
                         ops=[(orc.EFF_EDGE_GRAVITY_NEWTON, (G_NEWTON,), None)]).step(1)
    assert np.array_equal(F, ow.force)            # semi-implicit: force column = the fold at the initial positions
    # exact check against the formula, edge by edge
    want = np.zeros((3, 3))
    for a, b in zip(src, dst):
        r = pos[a, 4:] - pos[b, 4:]
        nrm = np.sqrt(np.sum(r * r))
        want[a] = want[a] - G_NEWTON * inertia[b, 6] * inertia[a, 6] * r / (nrm * nrm * nrm)
    assert np.allclose(F[:, 3:], want, rtol=1e-15, atol=0.0)


def test_edge_fold_restrictions_and_codegen():
    with pytest.raises(TypeError):
        dsl.edge_fold(lambda acc, a_pos, a_in, b_pos, b_in: dsl.SpatialForce(linear=a_pos.angular() @ b_pos.linear())).trace()
    with pytest.raises(TypeError):
        dsl.edge_fold(lambda acc, a_pos, a_in, b_pos, b_in: dsl.SpatialForce(linear=a_in.inertia_diag())).trace()
    with pytest.raises(TypeError):
        dsl.edge_fold(lambda acc, a, b: acc)
    tf = gravity_fn.trace()
    assert tf.leaves == {"acc3", "acc4", "acc5", "ax", "ay", "az", "ma", "bx", "by", "bz", "mb"}
    src = codegen.generate_pair_source(tf)
    assert "struct PairCustom" in src and "sixdof_custom_pair_launch" in src
    so = codegen.build_pair(tf)
    assert so.exists() and codegen.build_pair(tf) == so


# ---- jax.lax-shaped control flow --------------------------------------------------------------------------------------

def test_lax_cond_switch_select_and_static_fori_loop():
    def f(xp, x, v):
        a = dsl.lax.cond(x < 0.0, lambda t: t * 2.0, lambda t: t + 1.0, x)                     # scalar operand
        b = dsl.lax.cond(x < 0.0, lambda _: v * xp.array([1.0, 1.0, -1.0]), lambda _: v, operand=None)   # closure style
        c = dsl.lax.switch(x, [lambda t: t, lambda t: t * 10.0, lambda t: t * 100.0], x)
        d = dsl.lax.fori_loop(0, 5, lambda i, acc: acc + (i + 1) * x, 0.0 * x)
        e = dsl.lax.select(x > 1.5, v[0], v[1])
        return a, b, c, d, e
    for x, want_a, want_c in ((-2.0, -4.0, -2.0), (0.4, 1.4, 0.4), (1.0, 2.0, 10.0), (2.0, 3.0, 200.0), (7.0, 8.0, 700.0)):
        a, b, c, d, e = dsl_numpy.trace_eval(f, x, [3.0, 4.0, 5.0])
        assert a == want_a and c == want_c and d == 15.0 * x
        assert np.array_equal(b, [3.0, 4.0, -5.0] if x < 0 else [3.0, 4.0, 5.0]) and e == (3.0 if x > 1.5 else 4.0)
    with pytest.raises(TypeError):
        dsl.lax.fori_loop(0, dsl.leaf("n"), lambda i, a: a, 0.0)


def test_lax_cond_over_spatial_values_like_the_ball_examples_bounce():
    """examples/ball/sim.py:64-71: cond(max(z, vz) < 0, v -> SpatialMotion(linear = v * [1, 1, -1] * 0.85), v -> v)."""
    @dsl.system
    def bounce(pos, vel):
        return {"world_vel": dsl.lax.cond(dsl.lax.max(pos.linear()[2], vel.linear()[2]) < 0.0,
                                          lambda _: dsl.SpatialMotion(linear=vel.linear() * np_.array([1.0, 1.0, -1.0]) * 0.85),
                                          lambda _: vel, operand=None)}
    ts = dsl.TracedSystem(bounce, dsl.ColumnTable("c", 48, 16))
    pos = np.array([[0, 0, 0, 1.0, 1.0, 2.0, -0.1], [0, 0, 0, 1.0, 1.0, 2.0, 0.3], [0, 0, 0, 1.0, 0.0, 0.0, -0.2]])
    vel = np.array([[0.1, 0.2, 0.3, 1.0, 2.0, -3.0], [0.1, 0.2, 0.3, 1.0, 2.0, -3.0], [0.0, 0.0, 0.0, 0.0, 0.0, 4.0]])
    inertia = np.ones((3, 7))
    dsl_numpy._run_systems([ts], pos, vel, inertia, {}, dsl.ColumnTable("c", 48, 16), 1)
    assert np.allclose(vel[0], [0, 0, 0, 0.85, 1.7, 2.55])       # below ground and sinking: reflected, spin dropped
    assert np.array_equal(vel[1], [0.1, 0.2, 0.3, 1.0, 2.0, -3.0])  # above ground: untouched
    assert np.array_equal(vel[2], [0.0, 0.0, 0.0, 0.0, 0.0, 4.0])   # below ground but already rising: untouched


# ---- spatial wrappers of SURVEY 8(a) a24 against the reference's own known answers ------------------------------------------

def test_quaternion_and_spatial_wrappers_match_the_reference_known_answers():
    Q = dsl.Quaternion
    ev = lambda fn, *a: dsl_numpy.trace_eval(lambda xp, *t: fn(*t), *a)
    x_axis = [1.0, 0.0, 0.0]
    # quaternion.rs:353-361 test_quat_mult, :364-370 test_quat_inverse, :373-381 test_quat_vec_mult, :384-388 convention
    out = ev(lambda ax, a, b: (Q.from_axis_angle(ax, a) * Q.from_axis_angle(ax, b)).vector(), x_axis, 3.0, 1.0)
    assert np.array_equal(out, [0.9092974268256817, 0.0, 0.0, -0.4161468365471424])
    out = ev(lambda ax, a: Q.from_axis_angle(ax, a).inverse().vector(), x_axis, 3.0)
    assert np.allclose(out, [-0.9974949866040544, 0.0, 0.0, 0.0707372016677029], rtol=1e-15, atol=0)
    out = ev(lambda ax, a, v: Q.from_axis_angle(ax, a) @ v, x_axis, 3.0, [1.0, 2.0, 3.0])
    assert np.allclose(out, [1.0, -2.4033450173804924, -2.6877374736816018], rtol=1e-6)
    out = ev(lambda i, j: (Q(i) * Q(j)).vector(), [1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0])
    assert np.array_equal(out, [0.0, 0.0, 1.0, 0.0])                                     # i * j = k, scalar last
    # spatial.rs:631-650 test_spatial_transform_add (exact), :653-676 test_spatial_transform_integrate (20 steps, 1e-5)
    add = lambda q, p, w, v: (lambda t: dsl.np.concatenate([t.angular().vector(), t.linear()]))(
        dsl.SpatialTransform(Q(q), p) + dsl.SpatialMotion(w, v))
    out = ev(add, [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0])
    assert np.array_equal(out, [0.0, 0.0, 0.4472135954999579, 0.8944271909999159, 0.0, 0.0, 0.0])
    def twenty(q, p, w, v):
        t = dsl.SpatialTransform(Q(q), p)
        t = dsl.lax.fori_loop(0, 20, lambda i, acc: acc + dsl.SpatialMotion(w, v), t)
        return dsl.np.concatenate([t.angular().vector(), t.linear()])
    out = ev(twenty, [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.25 / 20.0], [0.0, 0.0, 0.0])
    assert np.allclose(out, [0.0, 0.0, 0.12467473338522769, 0.992197667229329, 0.0, 0.0, 0.0], atol=1e-5)
    # test_all.py:86-114 test_spatial_integration: integrate_body with w = (pi/2, 0, 0), twice from identity
    def integ(q, w):
        a = Q(q).integrate_body(w)
        return a.integrate_body(w).vector()
    out = ev(integ, [0.0, 0.0, 0.0, 1.0], [np.pi / 2, 0.0, 0.0])
    assert np.allclose(out, [0.97151626, 0.0, 0.0, 0.23697292])
    out = ev(lambda q: Q(q).normalize().vector(), [0.0, 3.0, 0.0, 4.0])
    assert np.allclose(out, [0.0, 0.6, 0.0, 0.8], rtol=1e-15)
    # a NON-unit quaternion (built from an array, or raw spawn data seen on tick 0): the reference's q @ v = q (x) (v,0) (x)
    # conj(q)/|q|^2 is scale-invariant (quaternion.rs:283-305) and inverse() divides by |q|^2 — against the pinned C oracle
    from oracle import oracle as orc
    rng = np.random.default_rng(3)
    for _ in range(5):
        q, v = rng.normal(size=4) * rng.uniform(0.2, 5.0), rng.normal(size=3)
        assert np.allclose(ev(lambda q, v: Q(q) @ v, q, v), orc.quat_rotate(q, v), rtol=1e-13, atol=1e-14)
        assert np.allclose(ev(lambda q, v: Q(q).inverse() @ v, q, v), orc.quat_rotate(orc.quat_inverse(q), v), rtol=1e-13, atol=1e-14)
        assert np.allclose(ev(lambda q: Q(q).inverse().vector(), q), orc.quat_inverse(q), rtol=1e-14)
        assert np.allclose(ev(lambda q, v: Q(q).normalize() @ v, q, v), orc.quat_rotate(q, v), rtol=1e-13, atol=1e-14)


def test_scan_with_stacked_outputs_matches_numpy():
    """lax.scan over a static leading axis, carry + stacked ys (the reference's edge_fold is vmap of scan,
    elodin/__init__.py:524-544): an exponential smoother over 8 samples and a running fold over rows."""
    def smooth(xp, x, alpha):
        carry, ys = dsl.lax.scan(lambda c, xi: ((1.0 - alpha) * c + alpha * xi,) * 2, x[0], x)
        return xp.concatenate([ys, xp.array([carry])])
    x = np.array([1.0, 4.0, 2.0, 8.0, 5.0, 7.0, 1.0, 3.0])
    want, c = [], x[0]
    for xi in x:
        c = 0.7 * c + 0.3 * xi
        want.append(c)
    got = dsl_numpy.trace_eval(smooth, x, 0.3)
    assert np.allclose(got, want + [want[-1]], rtol=1e-15)

    def fold_rows(xp, a, b):            # xs as a tuple of two scanned Vecs; ys are (scalar, Vec) tuples
        def step(acc, ab):
            ai, bi = ab
            acc = acc + ai * bi
            return acc, (acc, xp.array([ai, bi]) * acc)
        total, (running, rows) = dsl.lax.scan(step, 0.0, (a, b))
        return xp.concatenate([xp.array([total]), running, xp.concatenate(rows)])
    a, b = np.array([1.0, 2.0, 3.0]), np.array([0.5, -1.0, 2.0])
    acc, run, rows = 0.0, [], []
    for ai, bi in zip(a, b):
        acc += ai * bi
        run.append(acc)
        rows += [ai * acc, bi * acc]
    assert np.allclose(dsl_numpy.trace_eval(fold_rows, a, b), [acc] + run + rows, rtol=1e-15)
    # length-only form
    got = dsl_numpy.trace_eval(lambda xp, x0: dsl.lax.scan(lambda c, _: (c * 2.0, c), x0, None, length=5)[1], 1.5)
    assert np.allclose(got, [1.5, 3.0, 6.0, 12.0, 24.0])


# ---- data-dependent loops --------------------------------------------------------------------------------------------------------

def kepler(xp, M, ecc):
    """Newton iteration on E - e sin E = M until the step is below 1e-13 (a different trip count per lane)."""
    def cond(c):
        return xp.abs(c[1]) > 1e-13
    def body(c):
        E = c[0]
        d = (E - ecc * xp.sin(E) - M) / (1.0 - ecc * xp.cos(E))
        return (E - d, d, c[2] + 1.0)
    E, _, iters = dsl.lax.while_loop(cond, body, (M, M * 0.0 + 1.0, M * 0.0), max_iter=60)
    return E, iters


def ballistic_impact(xp, alt0, vz0, vx0, cd_s_over_m):
    """The shape of the flight software's impact predictor (examples/falcon9/controller/src/main.rs:746-775): propagate
    a drag-affected arc in 0.5 s steps until it meets the ground, at most 2,400 steps."""
    def cond(c):
        return c[0] > 0.0
    def body(c):
        alt, x, vz, vx, k = c
        speed = xp.sqrt(vz * vz + vx * vx)
        rho = 1.225 * xp.exp(-xp.maximum(alt, 0.0) / 8440.0)
        drag = 0.5 * rho * speed * cd_s_over_m
        vz2 = vz + (-9.81 - drag * vz) * 0.5
        vx2 = vx + (-drag * vx) * 0.5
        return (alt + vz2 * 0.5, x + vx2 * 0.5, vz2, vx2, k + 1.0)
    alt, x, vz, vx, k = dsl.lax.while_loop(cond, body, (alt0, alt0 * 0.0, vz0, vx0, alt0 * 0.0), max_iter=2400)
    return x, k


def test_while_loop_traces_and_evaluates_with_per_lane_trip_counts():
    for M, ecc in ((0.3, 0.1), (2.5, 0.7), (1e-3, 0.95)):
        E, iters = dsl_numpy.trace_eval(kepler, M, ecc)
        assert abs(E - ecc * np.sin(E) - M) < 1e-12 and 2 <= iters <= 60
    # straight Python for the impact predictor
    def py(alt, vz, vx, c):
        x = k = 0.0
        while alt > 0.0 and k < 2400:
            speed = np.sqrt(vz * vz + vx * vx)
            drag = 0.5 * 1.225 * np.exp(-max(alt, 0.0) / 8440.0) * speed * c
            vz = vz + (-9.81 - drag * vz) * 0.5
            vx = vx + (-drag * vx) * 0.5
            alt, x, k = alt + vz * 0.5, x + vx * 0.5, k + 1.0
        return x, k
    for case in ((60_000.0, 900.0, 1200.0, 1e-3), (500.0, -30.0, 10.0, 2e-3), (80_000.0, 1500.0, 500.0, 1e-4)):
        got = dsl_numpy.trace_eval(ballistic_impact, *case)
        want = py(*case)
        assert got[1] == want[1] and abs(got[0] - want[0]) <= 1e-9 * abs(want[0]), (got, want)


def test_while_loop_generates_a_real_loop_and_hoists_invariants():
    @dsl.system
    def solve(m_anom, ecc_anom):
        E, iters = kepler(np_, m_anom[0], m_anom[1])
        return {"ecc_anom": np_.array([E, iters])}
    tp = dsl.Program([solve], dsl.Pipe([]), []).trace({"m_anom": 2, "ecc_anom": 2})
    src = codegen.generate_source(tp, "float64", 2)
    assert "for (int it_" in src and "break;" in src and src.count("m_sin(") == 1 and src.count("m_cos(") == 1
    assert codegen.build(tp, "float64", 2).exists()


# ---- the reference's StableHLO coverage example against its CI baseline CSVs ------------------------------------------------

def test_stablehlo_coverage_example_matches_the_reference_baseline_rows():
    """scripts/ci/baseline/stablehlo (tests/golden/stablehlo.json): 100 ticks of eight systems covering ~50 ops (the int64 bitwise one included, exact) — trig /
    hyperbolic / exp-log family / roots / rounding / erfc / isfinite, sort, static shape ops, while_loop, switch,
    remainder, reductions, select / clamp, a Cholesky solve — traced, evaluated with numpy, compared row by row.
    Six of the seven float columns and the integer column reproduce the baseline to the last bit or two.  `math_state` does not follow the
    example's current `math_step` (no subset of its 24 terms sums to the baseline row; the baseline predates the
    function as checked in), so that system is checked against a direct numpy transcription instead."""
    import json
    from pathlib import Path
    from tests import stablehlo_dsl as S
    gold = json.loads((Path(__file__).parent / "golden" / "stablehlo.json").read_text())["rows"]
    table = dsl.ColumnTable("c", 48, 16, {k: len(v) for k, v in S.INITIAL.items()})
    traced = [dsl.TracedSystem(s, table) for s in S.SYSTEMS]
    comps = {k: np.array([v], dtype=np.float64) for k, v in S.INITIAL.items()}
    pos, vel, inertia = np.array([[0, 0, 0, 1.0, 0, 0, 0]]), np.zeros((1, 6)), np.ones((1, 7))
    worst = {}
    for tick in range(1, 101):
        dsl_numpy._run_systems(traced, pos, vel, inertia, comps, table, tick)
        for name, rows in gold.items():
            if name == "math_state":
                continue
            ref = np.array(rows[tick])
            err = np.max(np.abs(comps[name][0] - ref) / np.maximum(np.abs(ref), 1e-12))
            worst[name] = max(worst.get(name, 0.0), float(err))
    print("stablehlo example vs reference baseline, worst relative error per component:", worst)
    assert max(worst.values()) < 1e-12 and len(worst) == 7 and worst["bitwise_state"] == 0.0, worst
    # math_step: the same 24 terms written directly in numpy / scipy
    from scipy.special import erfc
    x = np.array(S.INITIAL["math_state"])
    comps = {"math_state": x[None, :].copy()}
    tm = dsl.ColumnTable("c", 48, 16, {"math_state": 4})
    t_math = dsl.TracedSystem(S.math_step, tm)
    for tick in range(1, 6):
        r = np.sin(x) + np.cos(x) + np.tanh(x) + np.arctan2(x, 1.0) + np.exp(x * 0.1) + np.log(np.abs(x) + 1) + np.log1p(np.abs(x))
        r = r + np.expm1(x * 0.01) + np.sqrt(np.abs(x) + 1) + 1 / np.sqrt(np.abs(x) + 1) + np.cbrt(np.abs(x) + 1) + np.power(np.abs(x) + 1, 0.5)
        sx = np.clip(x * 0.1, -0.99, 0.99)
        r = r + np.floor(x) + np.ceil(x) + np.sign(x) + np.round(x) + np.abs(x) + np.arcsin(sx) + np.arccos(sx) + np.arctan(x * 0.1)
        r = r + np.sinh(x * 0.1) + np.cosh(x * 0.1) + erfc(x * 0.1) + np.clip(x, -2.0, 2.0)
        x = r * 0.01
        dsl_numpy._run_systems([t_math], pos, vel, inertia, comps, tm, tick)
        assert np.allclose(comps["math_state"][0], x, rtol=1e-14)


def test_construction_cast_and_reduction_helpers_match_numpy():
    """jnp calls the reference's scripts make besides arithmetic: asarray / stack / full / *_like, float and int casts,
    reciprocal / square / mean / degrees, searchsorted over a constant table, linalg.det."""
    from tests import dsl_numpy
    rng = np.random.default_rng(8)
    for _ in range(20):
        v, u, w = rng.normal(size=3), rng.normal(size=3), rng.normal(size=3)
        s = float(rng.normal() * 3.0)
        table = [-2.0, -0.5, 0.0, 0.75, 2.5]
        got = dsl_numpy.trace_eval(lambda np_, v, u, w, s: (
            np_.asarray([s, 1.0, v[0]]), np_.stack([v[0], u[1], s]), np_.full(3, s) + np_.zeros_like(v) + np_.ones_like(v),
            np_.float64(s) + np_.int32(s * 2.0) + np_.int64(-s), np_.reciprocal(v[0]) + np_.square(u[1]) + np_.negative(s),
            np_.mean(v) + np_.degrees(s) - np_.radians(s), np_.searchsorted(table, s), np_.searchsorted(table, s, side="right"),
            np_.linalg.det(np_.stack([v, u, w])), np_.linalg.det([v[:2], u[:2]]), np_.matvec(np_.stack([v, u, w]), w)), v, u, w, s)
        want = (np.array([s, 1.0, v[0]]), np.array([v[0], u[1], s]), np.full(3, s) + 1.0, s + np.trunc(s * 2.0) + np.trunc(-s),
                1.0 / v[0] + u[1] ** 2 - s, v.mean() + np.degrees(s) - np.radians(s), float(np.searchsorted(table, s)),
                float(np.searchsorted(table, s, side="right")), np.linalg.det(np.stack([v, u, w])), np.linalg.det(np.stack([v[:2], u[:2]])),
                np.stack([v, u, w]) @ w)
        for g, e in zip(got, want):
            assert np.allclose(g, e, rtol=1e-13, atol=1e-13), (g, e)
    assert dsl_numpy.trace_eval(lambda np_, s: np_.searchsorted([0.0, 1.0], s), 1.0) == 1.0      # ties: left
    assert dsl_numpy.trace_eval(lambda np_, s: np_.searchsorted([0.0, 1.0], s, side="right"), 1.0) == 2.0


def test_concurrent_builds_of_one_program_share_the_cache_safely():
    """Ranks of one job trace the same program and may all miss the cache at once: every builder writes under its own
    temporary name and publishes with an atomic rename, so all of them end up loading one intact object."""
    import subprocess
    import sys
    import textwrap
    code = textwrap.dedent('''
        import sys, ctypes
        sys.path.insert(0, %r)
        from elodin_amd import dsl, codegen
        @dsl.system(x=2)
        def f(x):
            return {"x": dsl.np.cos(x) * 0.4321 + 0.25}
        so = codegen.build(dsl.Program([f], dsl.Pipe([]), []).trace({"x": 2}), "float64", 2)
        ctypes.CDLL(str(so))
        print(so.name, codegen.last_resources["vgpr_spills"])
    ''') % str(codegen.PKG.parent)
    for stale in codegen.JIT_DIR.glob("pipe_*"):      # this test's program only: force a miss
        if stale.suffix == ".hip" and "0.4321" in stale.read_text():
            for f in codegen.JIT_DIR.glob(stale.stem + ".*"):
                f.unlink()
    procs = [subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for _ in range(3)]
    outs = [p.communicate() + (p.returncode,) for p in procs]
    assert all(rc == 0 for _, _, rc in outs), outs
    assert len({o.strip() for o, _, _ in outs}) == 1 and outs[0][0].split()[1] == "0"
    assert not list(codegen.JIT_DIR.glob("*.tmp*"))


def test_guarded_selects_wrap_only_what_the_expensive_arm_alone_needs():
    """codegen guard_selects: `where(due, fresh, held)` with an expensive `fresh` becomes `T x = held; if (__any(due)) {...}`.
    Nodes another use needs stay outside; selects on the same condition share one branch; constant conditions, loops and the
    default (switch off) are untouched."""
    from elodin_amd import codegen

    @dsl.system
    def sensor(a, b, c):
        due = a[0] > 0.5
        shared = np_.sin(a[1])                                   # also read by `c`: must stay outside the branch
        key = dsl.random.fold_in(dsl.random.key(7), a[2])        # needed by both draws and by nothing else: inside
        n = dsl.random.normal(key, shape=(2,))
        fresh0, fresh1 = b[0] + n[0] * shared, b[1] + n[1] * np_.cos(a[1])
        return {"b": np_.array([np_.where(due, fresh0, b[0]), np_.where(due, fresh1, b[1])]),
                "c": np_.array([shared + c[0], np_.where(a[0] * 0.0 + 1.0 > 2.0, np_.tan(a[1]), 0.0)])}   # (c carried: computed every tick)
    tp = dsl.Program([sensor], dsl.Pipe([]), []).trace({"a": 3, "b": 2, "c": 2})
    plain = codegen.generate_source(tp, "float64", 2)
    src = codegen.generate_source(tp, "float64", 2, guard_selects=True)
    assert "__any(" not in plain and plain == codegen.generate_source(tp, "float64", 2, guard_selects=False)
    body = src[src.index("// sensor"):]
    assert body.count("if (__any(") == 1                          # one branch for the two selects that test `due`
    guard = body[body.index("if (__any("):]
    inside = guard[:guard.index("\n        }")]
    assert inside.count("m_threefry(") >= 3 and inside.count("m_erfinv(") == 2 and "m_cos(" in inside
    assert "m_sin(" not in inside and "m_sin(" in body[:body.index("if (__any(")]            # the shared node: outside, before
    assert inside.count(" ? ") == 2 and "m_tan(" not in inside                                   # cheap arm (tan: cost below the bar) plain
    # evaluation is unchanged by construction (the numpy walk has no notion of the switch); the GPU side is
    # tests/test_gpu_fuzz.py::test_random_programs_with_guarded_selects_f64 and tests/test_gpu_falcon9_unmodified.py


def test_array_surface_added_for_the_unmodified_scripts_matches_numpy():
    """What the reference's falcon9 / cube-sat / stablehlo / apollo scripts needed beyond round 2's surface, each against numpy on
    random data: row-wise cross products and column-condition `where` over matrices, vector-against-matrix broadcasting, stack
    along axis 1, constant fancy indexing, traced gathers from host tables, triangular solves, integer bitwise ops, broadcast_to."""
    import scipy.linalg as sla
    from elodin_amd import dsl_mat
    rng = np.random.default_rng(12)
    A, B, v, cnd = rng.normal(size=(4, 3)), rng.normal(size=(4, 3)), rng.normal(size=3), rng.normal(size=4)

    def mats(xp, a_flat, b_flat, vv, cc):
        a, b = a_flat.reshape(4, 3), b_flat.reshape(4, 3)
        crossed = xp.cross(a - vv, b)                               # [4, 3] - [3] broadcasts; cross row by row
        picked = xp.where(cc[:, None] <= 0.0, a, xp.zeros_like(a))  # a [4, 1] condition against [4, 3] values
        stacked = xp.stack([a[0], b[0]], axis=1)                    # [3, 2]
        return crossed.flatten(), xp.sum(picked, axis=0), stacked.flatten(), vv - a[1], a[2][np.array([2, 0, 0, 1])]
    c_, p_, s_, d_, f_ = dsl_numpy.trace_eval(mats, A.reshape(-1), B.reshape(-1), v, cnd)
    assert np.allclose(c_, np.cross(A - v, B).reshape(-1), rtol=1e-14) and np.allclose(p_, np.where(cnd[:, None] <= 0, A, 0).sum(axis=0))
    assert np.allclose(s_, np.stack([A[0], B[0]], axis=1).reshape(-1)) and np.allclose(d_, v - A[1]) and np.allclose(f_, A[2][[2, 0, 0, 1]])

    L_ = np.tril(rng.normal(size=(4, 4))) + 3.0 * np.eye(4)
    rhs = rng.normal(size=4)
    for lower, trans in ((True, 0), (False, 0), (True, 1)):
        M = L_ if lower else L_.T
        got = dsl_numpy.trace_eval(lambda xp, m, r: dsl_mat.solve_triangular(m.reshape(4, 4), r, lower=lower, trans=trans), M.reshape(-1), rhs)
        assert np.allclose(got, sla.solve_triangular(M, rhs, lower=lower, trans=trans), rtol=1e-13), (lower, trans)

    ints = np.array([0xA5, 0x3C, 0xFF, 0x01], dtype=np.int64)
    def bits(xp, x):
        r = xp.bitwise_and(xp.bitwise_or(xp.bitwise_xor(x, 255.0), 15.0), 4095.0)
        return dsl.lax.shift_right_logical(xp.left_shift(r, 3.0), 2.0)
    assert np.array_equal(dsl_numpy.trace_eval(bits, ints.astype(float)), ((((ints ^ 0xFF) | 0x0F) & 0xFFF) << 3) >> 2)

    table = np.array([10.0, 20.0, 30.0, 40.0])
    def gather(xp, i):
        return dsl._host(table)[i[0]], xp.sum(xp.broadcast_to(i, (3, 2)), axis=0)
    g, bsum = dsl_numpy.trace_eval(gather, np.array([2.0, 5.0]))
    assert g == 30.0 and np.allclose(bsum, [6.0, 15.0])


def test_traced_negative_indices_follow_jax_and_scalar_getitem_takes_traced_keys():
    """jax normalises a dynamic negative index before clamping (x[i] with i = -1 reads the LAST element, x.at[-1].set() updates
    it); a traced key into a one-element value must not trip the membership test (`expr in tuple` would call bool())."""
    v = np.array([10.0, 20.0, 30.0, 40.0])

    def gather(xp, x, i):
        return x[i[0]], x[i[1]], x[i[2]], x[i[3]]
    assert dsl_numpy.trace_eval(gather, v, np.array([-1.0, -4.0, 2.0, 9.0])) == (40.0, 10.0, 30.0, 40.0)
    assert dsl_numpy.trace_eval(gather, v, np.array([-9.0, -2.0, 0.0, 3.0])) == (10.0, 30.0, 10.0, 40.0)    # below -n clamps to 0

    def scatter(xp, x, i):
        return x.at[i[0]].set(-1.0), x.at[i[1]].add(5.0), x.at[i[2]].set(7.0)
    a, b, c = dsl_numpy.trace_eval(scatter, v, np.array([-1.0, -3.0, 11.0]))
    assert np.array_equal(a, [10, 20, 30, -1]) and np.array_equal(b, [10, 25, 30, 40]) and np.array_equal(c, v)   # out of range: dropped
    s, k = dsl.leaf("s"), dsl.leaf("k")
    assert s[k] is s and s[0] is s and s[-1] is s and s[...] is s and s[()] is s
    with pytest.raises(IndexError):
        s[1]


def test_compat_dispatch_probes_with_a_sentinel_and_names_unsupported_keywords():
    from elodin_amd import compat
    compat.install(run="record")
    try:
        import jax.numpy as jnp
        assert jnp.newaxis is None and jnp.pi == np.pi
        with pytest.raises(AttributeError):
            jnp.fft
        x = dsl.Vec([dsl.leaf("a"), dsl.leaf("b")])
        with pytest.raises(NotImplementedError, match="jax.numpy.clip"):
            jnp.clip(x, 0.0, 1.0, out=None)
    finally:
        compat.uninstall()


def test_gather_from_a_constant_device_table_follows_jax_and_generates_a_load():
    """dsl.gather / HostTable: `table[idx, 0]`, `table[rows_vec, 0]` with traced rows over a table too long for a select chain
    (examples/monte-carlo/sim.py:84-97).  jax's gather: negative rows count from the end, then clamp."""
    rng = np.random.default_rng(3)
    table = rng.normal(size=(500, 2))
    tab = dsl.HostTable(table)

    def lookups(xp, i):
        rows = (dsl._host(np.arange(3.0) * 7.0) + i[0]) % 500.0
        return tab[i[0], 0], tab[i[1], 1], tab[i[2], 0], tab[i[3], 1], xp.sum(tab[rows, 0]), tab[i[0]]
    a, b, c, d, e, row = dsl_numpy.trace_eval(lookups, np.array([17.0, -1.0, 900.0, -900.0]))
    assert (a, b, c, d) == (table[17, 0], table[-1, 1], table[499, 0], table[0, 1])
    assert e == table[[17, 24, 31], 0].sum() and np.array_equal(row, table[17])
    assert dsl.gather(table, 3, 1).is_const(table[3, 1])            # a constant row folds

    @dsl.system(x=1, y=1)
    def look(x, y):
        return {"y": tab[dsl.np.clip(dsl.np.abs(x * 10.0).astype(int), 0, 499), 0] + y * 0.0}
    src = codegen.generate_source(dsl.Program([look], dsl.pipe(), []).trace({"x": 1, "y": 1}), "float64", 2)
    assert "m_gather<T>(gtab0," in src and "__device__ const double gtab0[1000]" in src


def test_map_coordinates_follows_jax_on_constant_grids():
    """dsl.map_coordinates (jax.scipy.ndimage.map_coordinates, examples/rocket/main.py:368) against a numpy restatement of
    jax's _map_coordinates — bit for bit, both modes, orders 0 and 1 — and against scipy where the two libraries agree
    (mode="nearest"); a grid of 33+ samples is read from device memory (dsl.gather), a smaller one through selects."""
    import itertools
    from scipy import ndimage

    def jax_mc(g, c, order, mode, cval):
        per = []
        for x, size in zip(c, g.shape):
            if order == 0:
                items = [(np.round(x), 1.0)]
            else:
                lo = np.floor(x)
                uw = x - lo
                items = [(lo, 1 - uw), (lo + 1, uw)]
            per.append([(int(np.clip(i, 0, size - 1)), ((0 <= i) & (i < size)) if mode == "constant" else True, w) for i, w in items])
        out = 0.0
        for items in itertools.product(*per):
            idxs, valids, ws = zip(*items)
            w = ws[0]
            for k in ws[1:]:
                w = w * k
            out = out + (g[idxs] if all(valids) else cval) * w
        return out
    rng = np.random.default_rng(5)
    for shape in ((3, 5, 4), (3, 4), (40,)):
        g = rng.normal(size=shape)
        for _ in range(12):
            c = np.array([rng.uniform(-1.5, s + 0.5) for s in shape])
            for order in (0, 1):
                for mode in ("nearest", "constant"):
                    got = dsl_numpy.trace_eval(lambda xp, cc: dsl.map_coordinates(g, [cc[k] for k in range(len(shape))], order, mode=mode, cval=0.25),
                                               np.concatenate([c, [0.0]]))
                    assert got == jax_mc(g, c, order, mode, 0.25), (shape, order, mode, c)
                    if mode == "nearest":
                        assert abs(got - ndimage.map_coordinates(g, c.reshape(-1, 1), order=order, mode=mode)[0]) < 1e-14
    with pytest.raises(NotImplementedError):
        dsl.map_coordinates(np.zeros((2, 2)), [dsl.leaf("a"), dsl.leaf("b")], 3)


def test_polars_subset_over_pandas_builds_the_rocket_examples_grid():
    """elodin_amd/compat_polars.py: the calls examples/rocket/main.py:150-262 makes, checked on a table of the same shape."""
    from elodin_amd import compat_polars
    pl = compat_polars.module()
    mach, delta, alpha = [0.1, 0.5], [-20.0, 0.0, 20.0], [0.0, 5.0]
    rows = [(m, d, a) for m in mach for d in delta for a in alpha]
    df = pl.from_dict({"Mach": [r[0] for r in rows], "Alphac": [r[2] for r in rows], "Delta": [r[1] for r in rows],
                       "CA": [100 * r[0] + r[1] + 0.1 * r[2] for r in rows], "CZ": [float(k) for k in range(len(rows))]})
    coefs = ["CA", "CZ"]
    grid = np.array([[sub2.group_by(["Alphac"], maintain_order=True).agg(pl.col(coefs).min()).select(pl.col(coefs)).to_numpy()
                      for _, sub2 in sub.group_by(["Delta"], maintain_order=True)] for _, sub in df.group_by(["Mach"], maintain_order=True)])
    assert grid.shape == (2, 3, 2, 2)
    assert grid[1, 2, 1, 0] == 100 * 0.5 + 20.0 + 0.5 and grid[0, 1, 1, 1] == 3.0
    s = df["Delta"]
    assert (s.min(), s.max(), len(s.unique())) == (-20.0, 20.0, 3)
    with pytest.raises(AttributeError):
        pl.scan_csv


def test_fast_math_builds_fold_single_use_products_into_their_sums():
    """codegen's FMA fusion (_Unit.fuse_fma): in a fast-math program `a * b + c`, `a * b - c` and `c - a * b` become one m_fma
    each when the product has no other use; a product used twice, a block output and every exact build stay apart."""
    import re

    @dsl.system(x=3, y=5)
    def sums(x, y):
        a, b, c = x[0], x[1], x[2]
        shared = a * c
        return {"y": dsl.np.array([a * b + c, b * c * 2.0 - a, c - b * b, shared + b, shared - a])}
    tp = dsl.Program([sums], dsl.pipe(), []).trace({"x": 3, "y": 5})
    fast = codegen.generate_source(tp, "float32", 2, fast_math=True)
    body = fast[fast.index("// sums"):]
    fmas = re.findall(r"= (m_fma\([^;]*\));", body)
    assert len(fmas) == 3 and sum("-" in f for f in fmas) == 2, fmas
    assert len(re.findall(r"= r\.c0\[0\] \* r\.c0\[2\];", body)) == 1          # the shared product is a value of its own
    os.environ["SIXDOF_FUSE_FMA"] = "0"
    try:
        assert "= m_fma(" not in codegen.generate_source(tp, "float32", 2, fast_math=True)
    finally:
        del os.environ["SIXDOF_FUSE_FMA"]
    assert "= m_fma(" not in codegen.generate_source(tp, "float32", 2) and "= m_fma(" not in codegen.generate_source(tp, "float64", 2)


def test_columns_nobody_reads_are_evaluated_where_they_are_stored():
    """codegen._store_only_slots: a per-tick (transient) column no system and no effector reads — telemetry derived for the
    database — is computed on the last tick of a launch or while the history ring records it, not on every tick; a column with
    a reader, and a loop-carried one, are computed every tick as before."""
    @dsl.system(x=1, seen=1, unseen=2, acc=1)
    def derive(x, acc):
        return {"seen": x * 2.0, "unseen": dsl.np.array([dsl.np.sin(x[0]), x[0] * x[0]]), "acc": acc + x}

    @dsl.system(seen=1, out=1)
    def use(seen):
        return {"out": seen + 1.0}
    tp = dsl.Program([derive, use], dsl.pipe(), []).trace({"x": 1, "seen": 1, "unseen": 2, "acc": 1, "out": 1})
    src = codegen.generate_source(tp, "float64", 2)
    names = [c for c, _ in tp.columns]
    k = names.index("unseen")
    assert "if (tick == P.tick0 + P.n_ticks || P.hist_ring != 0u) {  // store-only columns of derive" in src
    lazy = src[src.index("// store-only columns of derive"):]
    lazy = lazy[:lazy.index("\n        }")]
    assert "m_sin(" in lazy and f"r.c{k}[1] =" in lazy and f"r.c{names.index('seen')}[0]" not in lazy
    assert src.count("m_sin(") == 1                                   # (the prelude defines it by macro) the one use, inside the block
    os.environ["SIXDOF_NO_STORE_ONLY_COLUMNS"] = "1"
    try:
        assert "store-only" not in codegen.generate_source(tp, "float64", 2)
    finally:
        del os.environ["SIXDOF_NO_STORE_ONLY_COLUMNS"]


def test_lane_exchanges_never_land_in_a_guarded_arm_or_a_divergent_loop():
    """lane_read / lane_read_dyn are __shfl exchanges every lane of the world must execute.  With guard_selects on, an
    exchange that only an expensive select arm needs is still emitted BEFORE the branch, unconditionally (with what only it needs);
    the rest of the arm stays guarded.  A data-dependent while loop whose body exchanges a carried value is refused."""
    from elodin_amd import codegen
    from elodin_amd.dsl import Expr

    @dsl.system
    def world(a, b):
        due = a[0] > 0.5
        mine = np_.sin(a[1]) * 3.0                                        # needed only by the exchange: outside with it
        other = Expr("lane_read", (dsl._lift(mine),), (4, (1, 2, 3, 0)))    # what the next entity of this 4-row world holds
        key = dsl.random.fold_in(dsl.random.key(7), a[2])
        fresh = b[0] + dsl.random.normal(key, shape=(1,))[0] * other      # expensive arm: threefry + erfinv, and the exchange's value
        return {"b": np_.array([np_.where(due, fresh, b[0])])}
    tp = dsl.Program([world], dsl.Pipe([]), []).trace({"a": 3, "b": 1})
    src = codegen.generate_source(tp, "float64", 2, guard_selects=True)
    body = src[src.index("// world"):]
    assert body.count("if (__any(") == 1 and body.count("__shfl(") == 1
    before, guard = body[:body.index("if (__any(")], body[body.index("if (__any("):]
    inside = guard[:guard.index("\n        }")]
    assert "__shfl(" in before and "m_sin(" in before and "__shfl(" not in inside           # the exchange and its operand: every lane
    assert "m_threefry(" in inside and "m_erfinv(" in inside                                    # the draw itself stays guarded

    @dsl.system
    def bad(a, b):
        def cond(s):
            return s[0] < a[0]
        def step(s):
            return (s[0] + Expr("lane_read", (dsl._lift(s[0]),), (4, (1, 2, 3, 0))) + 1.0,)
        return {"b": np_.array([dsl.lax.while_loop(cond, step, (b[0],))[0]])}
    tp2 = dsl.Program([bad], dsl.Pipe([]), []).trace({"a": 1, "b": 1})
    with pytest.raises(NotImplementedError, match="lane exchange"):
        codegen.generate_source(tp2, "float64", 2)


def test_relaxed_arithmetic_rules_at_the_node_level():
    """dsl.relaxed_arithmetic rewrites while the DAG is built: `0 * x` -> 0, `a / d` -> a * (1 / d) with ONE reciprocal node per
    denominator, `a / c` -> a * (1 / c), and the division by the squared norm of a vector that was JUST normalised
    (x_i * (1 / sqrt(sum x_i^2)), the very nodes) is dropped — the reference's `inverse` of a normalised quaternion
    (quaternion.rs:141-155).  Nothing of it happens outside the context, and look-alikes keep their division."""
    x = [dsl.leaf(f"x{k}") for k in range(4)]
    y = dsl.leaf("y")

    def norm2(v):
        return ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]
    with dsl.relaxed_arithmetic():
        assert (x[0] * 0.0).is_const(0.0) and (0.0 * x[1]).is_const(0.0)
        q1, q2 = x[0] / y, x[1] / y
        assert q1.op == "mul" and q2.op == "mul" and q1.args[1] is q2.args[1] and q1.args[1].op == "div" and q1.args[1].args[0].is_const(1.0)
        h = x[0] / 4.0
        assert h.op == "mul" and h.args[1].is_const(0.25)
        assert (3.0 / y).op == "div"                                     # a constant numerator keeps its IEEE divide
        n = dsl.np.sqrt(norm2(x))
        u = [c / n for c in x]                                            # normalise: x_i * (1 / sqrt(S))
        inv = [(-u[0]) / norm2(u), (-u[1]) / norm2(u), (-u[2]) / norm2(u), u[3] / norm2(u)]      # conj / |u|^2
        assert inv[3] is u[3] and inv[0].op == "neg" and inv[0].args[0] is u[0]            # the division is gone
        inv2 = [(-inv[0]) / norm2(inv), inv[3] / norm2(inv)]             # the inverse of THAT (signs stripped inside the squares)
        assert inv2[1] is u[3]
        # look-alikes keep their division: another scale per component, a base that is not the normalised vector, three of four terms
        w = [x[0] / n, x[1] / n, x[2] / n, x[3] / (n * 2.0)]
        assert (y / norm2(w)).op == "mul" and (y / norm2(w)).args[1].op == "div"
        m = dsl.np.sqrt(norm2([x[0], x[1], x[2], y]))
        v = [c / m for c in x]
        assert (y / norm2(v)).args[1].op == "div"
        assert (y / ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])).args[1].op == "div"
    assert (x[0] * 0.0).op == "mul" and (x[0] / y).op == "div"          # outside the context: the program as written
