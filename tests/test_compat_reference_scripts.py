"""Reference scripts run UNMODIFIED under elodin_amd.compat (`import elodin`, `import jax`, `from jax import numpy, lax,
random`, `jax.numpy.linalg`, `jax.scipy.linalg` resolve to this package's front-end).  Build container only — the scripts are
read from the checkout ELODIN_REFERENCE names (tests/reference.py) and never copied:

  examples/ball/sim.py         generates the SAME HIP source, byte for byte, as the respelling examples/ball.py, whose GPU
                               flight lands on the reference's ball baseline (tests/test_gpu_examples.py, test_gpu_frontend.py)
  examples/three-body/main.py  same for the user-written edge_fold (pair kernel source) and the spawned world, vs
                               examples/three_body.py (GPU: the three-body golden CSV)
  examples/linalg/sim.py       traced and stepped 100 ticks on the CPU walker: every component lands on the rows of the
                               reference's CI baseline scripts/ci/baseline/linalg (1e-9; the reference's own CI accepts 1e-4)
  examples/n-body/sim.py       BASELINE configs[2]'s example (sun + nine planets from its truth CSV, complete gravity graph, the
                               user-written softened fold): the spawned world is the one tests/solar_util.py holds, and the
                               traced fold stepped with RK4 equals the C oracle's built-in softened all-pairs op
  examples/falcon9/sim.py      BASELINE configs[4]'s example: the whole powered plant of `build_powered` (engines with their ignition
                               state machine, valves, TVC, grid fins, RCS allocation, tanks, US-76 atmosphere, aero tables, WGS84
                               frames, pad clamp, leg contact, sensors; 23 systems, 62 components) driven the way the reference's
                               own tests drive it, against the trajectories the reference's own functions flew
                               (tests/golden/falcon9_plant.json): 43 columns, three windows
  examples/apollo-lander/sim.py  BASELINE configs[3]'s example: `build(params)` traces and generates (its closed loop needs the
                               example's controller process behind main.py's post_step; the campaign kernel of this repo is
                               pinned on reference-flown descents separately, tests/test_apollo_reference_fixtures.py)
  examples/stablehlo/main.py   the op-coverage example (eight single-component entities, ~50 ops incl. int64 bitwise ones, sort,
                               while_loop / switch, static shape ops, Cholesky + triangular solve): 100 ticks against
                               scripts/ci/baseline/stablehlo, integers exact
  examples/drone/main.py       the closed-loop quadcopter (cascaded attitude / rate PIDs, motor + sensor models, Mahony-style
                               estimator; 300 Hz simulation under a 100 Hz telemetry tick = three semi-implicit sub-steps per
                               tick): traced and stepped 100 ticks on the CPU walker against scripts/ci/baseline/drone-csv
                               (GPU: tests/test_gpu_drone.py runs the same generated kernel from a frozen fixture)
  examples/cube-sat/main.py    the attitude-controlled satellite (MEKF with pseudo-inverses, reaction wheels, sun sensors; eleven
                               entities, four edge folds, everything inside six_dof(sys=..., SemiImplicit)): traced and stepped
                               100 ticks against scripts/ci/baseline/cube-sat-csv with the attitude loop closed and the orbit
                               translation taken from the baseline (its EGM08 gravity tables are a download: tests/cube_sat_util.py)
"""
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import reference

REF = reference.root()
ROOT = Path(__file__).resolve().parents[1]
pytestmark = pytest.mark.skipif(REF is None, reason=reference.SKIP_REASON)


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture()
def compat():
    import elodin_amd.compat as c
    before = set(sys.modules)
    path = list(sys.path)
    c.install(run="record")
    try:
        yield c
    finally:
        c.uninstall()
        sys.path[:] = path
        for name in set(sys.modules) - before:       # the scripts imported meanwhile hold references to the shim modules
            f = getattr(sys.modules[name], "__file__", None) or ""
            if "site-packages" in f or "dist-packages" in f or "/lib/python3" in f:
                continue                             # real libraries first imported during the test (pandas under compat_polars)
            del sys.modules[name]                    # stay imported: purging and re-importing them leaves two copies of their classes


def test_ball_script_generates_the_same_kernel_as_its_respelling(compat):
    sys.path.insert(0, str(REF / "examples" / "ball"))
    ref = _load(REF / "examples" / "ball" / "sim.py", "ref_ball_sim")
    ours = _load(ROOT / "examples" / "ball.py", "our_ball")
    a = ref.world(seed=3).generated_sources(ref.system(), simulation_rate=1.0 / ref.SIM_TIME_STEP)
    b = ours.world(seed=3).generated_sources(ours.system(), simulation_rate=120.0)
    assert set(a) == {"step"} and a == b
    assert "threefry" in a["step"] and "sample_wind" in a["step"] and "bounce" in a["step"]
    wa, wb = ref.world(seed=3), ours.world(seed=3)
    for comp in ("world_pos", "world_vel", "inertia", "seed", "wind"):
        assert np.array_equal(wa.column(comp)[0], wb.column(comp)[0]) and np.array_equal(wa.column(comp)[1], wb.column(comp)[1]), comp


def test_three_body_script_generates_the_same_pair_kernel_and_world(compat):
    ref = _load(REF / "examples" / "three-body" / "main.py", "ref_three_body")       # runs w.run(...) at import: recorded
    run = ref.w.compat_run
    assert run["simulation_rate"] == 120.0 and run["ignored"]["generate_real_time"] is True      # editor-only arguments are recorded, not acted on
    ours = _load(ROOT / "examples" / "three_body.py", "our_three_body")
    w2, sys2 = ours.world_and_system()
    a = ref.w.generated_sources(run["system"], simulation_rate=run["simulation_rate"])
    b = w2.generated_sources(sys2, simulation_rate=120.0)
    assert set(a) == {"pair"} and a == b
    for comp in ("world_pos", "world_vel", "inertia"):
        assert np.array_equal(ref.w.column(comp)[0], w2.column(comp)[0]), comp
    ea, eb = ref.w.edge_pairs("gravity_edge"), w2.edge_pairs("gravity_edge")
    assert np.array_equal(ea[0], eb[0]) and np.array_equal(ea[1], eb[1]) and len(ea[0]) == 6      # spawn order = fold order


def test_linalg_script_unmodified_lands_on_the_reference_baseline(compat):
    from tests import dsl_numpy
    ref = _load(REF / "examples" / "linalg" / "sim.py", "ref_linalg_sim")
    w = ref.world()
    plan = w.build(ref.system(), simulation_rate=ref.SIMULATION_RATE, _dry=True)
    prog, cols = plan["effectors"], plan["columns"]
    tp = prog.trace()
    n = next(iter(cols.values())).shape[0]
    assert n == 6 and dict(tp.columns)["ekf6_cov"] == 36
    comps = {name: np.array(cols[name], dtype=np.float64).reshape(n, -1).copy() for name, _ in tp.columns}
    pos, vel, acc, inertia = np.tile([0, 0, 0, 1.0, 0, 0, 0], (n, 1)), np.zeros((n, 6)), np.zeros((n, 6)), np.ones((n, 7))
    gold = json.loads((ROOT / "tests" / "golden" / "linalg.json").read_text())["rows"]
    worst = {}
    for tick in range(1, 101):
        dsl_numpy.program_tick_systems_only(tp, pos, vel, acc, inertia, comps, tick)
        for name, rows in gold.items():
            row = int(np.argmax(comps["has:" + name][:, 0]))                # the one entity that carries the component
            refv, got = np.asarray(rows[tick]), comps[name][row]
            scale = 1e5 if name == "chol_res_norms" else max(float(np.max(np.abs(refv))), 1e-300)   # residual norms: 1e-14 absolute
            worst[name] = max(worst.get(name, 0.0), float(np.max(np.abs(got - refv))) / scale)
        for name in gold:                                                   # rows of the other entities stay as spawned (query joins)
            others = comps["has:" + name][:, 0] < 0.5
            assert np.all(comps[name][others] == 0.0), name
    print("examples/linalg/sim.py unmodified vs its CI baseline, worst per component:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert len(worst) == 11 and max(worst.values()) < 1e-9, worst


def test_drone_script_unmodified_lands_on_the_reference_baseline(compat):
    from tests import dsl_numpy
    from tests.drone_util import drone_errors, drone_verdict
    compat.install(run="record", inert=("polars",))
    sys.path.insert(0, str(REF / "examples" / "drone"))
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(20000)
    try:
        ref = _load(REF / "examples" / "drone" / "main.py", "ref_drone_main")           # runs world.run(...) at import: recorded
        run = ref.world.compat_run
        assert run["simulation_rate"] == 300.0 and run["telemetry_rate"] == 100.0
        plan = ref.world.build(run["system"], simulation_rate=run["simulation_rate"], telemetry_rate=run["telemetry_rate"], _dry=True)
        tp = plan["effectors"].trace()
        # the reference's schedule: control on the first of three sub-steps, plant + sensors on every one
        assert plan["substeps"] == 3 and plan["integrator"] == 1 and abs(plan["time_step"] * 900.0 - 1.0) < 1e-12
        sched = {s.name: (s.every, s.phase) for s in list(tp.pre) + list(tp.post)}
        assert all(sched[k] == (3, 1) for k in ("attitude_flight_plan", "update_target_attitude", "attitude_control", "rate_control",
                                                 "motor_input_to_pwm"))
        assert all(sched[k] == (1, 0) for k in ("drag", "motor_thrust_response", "body_thrust", "gyro", "accel", "mag"))
        from elodin_amd import codegen
        frozen = json.loads((ROOT / "tests" / "golden" / "drone_program.json").read_text())      # what tests/test_gpu_drone.py runs
        assert codegen.generate_variant(tp, frozen["variant"], "float64", plan["integrator"]) == frozen["source"], "re-run tests/golden/make_drone_program.py"
        assert [list(c) for c in tp.columns] == frozen["columns"] and frozen["substeps"] == 3
        gold = json.loads((ROOT / "tests" / "golden" / "drone.json").read_text())
        body, cols = plan["body"], plan["columns"]
        n = body["world_pos"].shape[0]
        pos, vel, acc, inertia = (np.array(body[k], dtype=np.float64).copy() for k in ("world_pos", "world_vel", "world_accel", "inertia"))
        comps = {name: np.array(cols[name], dtype=np.float64).reshape(n, -1).copy() for name, _ in tp.columns}
        worst, sub = {}, 0
        for tick in range(1, 101):
            for _ in range(plan["substeps"]):
                sub += 1
                dsl_numpy.program_tick(tp, pos, vel, acc, inertia, comps, sub, plan["dt"], plan["integrator"], dt=plan["time_step"])
            if tick in gold["tick"]:
                cur = {k: v[0] for k, v in comps.items()}
                cur.update(world_pos=pos[0], world_vel=vel[0], world_accel=acc[0])
                drone_errors(gold, gold["tick"].index(tick), cur, worst)
    finally:
        sys.setrecursionlimit(limit)
    print("examples/drone/main.py unmodified vs its CI baseline, worst per component:",
          {k: f"{v:.1e}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])})
    drone_verdict(worst)


def test_n_body_script_builds_the_solar_system_and_its_fold_is_the_oracles_pair_op(compat):
    """sim.py only: main.py deletes and recreates the example's database directory before it runs."""
    from oracle import oracle as orc
    from tests import dsl_numpy, np_sixdof, solar_util as su
    from elodin_amd import _lib as L
    sim = _load(REF / "examples" / "n-body" / "sim.py", "ref_nbody_sim")
    w, system = sim.build_world(), sim.build_system()
    plan = w.build(system, simulation_rate=sim.SIMULATION_RATE_HZ, telemetry_rate=sim.TELEMETRY_RATE_HZ, _dry=True)
    d, pos, vel, inertia = su.load()
    body = plan["body"]
    assert plan["dt"] == su.DT and plan["integrator"] == L.RK4
    assert np.array_equal(body["world_pos"], pos) and np.array_equal(body["inertia"], inertia)
    assert np.allclose(body["world_vel"], vel, rtol=1e-15, atol=0.0)             # the example divides by 86,400 s in jnp, the fixture in numpy
    frm, to = plan["edges"]
    ids = [int(e) for e in plan["row_ids"]]
    assert len(frm) == 90 and sorted(zip(frm.tolist(), to.tolist())) == sorted((a, b) for a in ids for b in ids if a != b)
    (fold,) = plan["effectors"]
    tf = fold.trace()
    rows = {e: k for k, e in enumerate(ids)}
    src, dst = [rows[int(e)] for e in frm], [rows[int(e)] for e in to]
    eff = lambda xs, vs: dsl_numpy.fold_force(tf, xs, inertia, src, dst)
    ref = orc.OracleWorld(pos, vel, inertia, simulation_time_step=su.DT, ops=[(L.EFF_ALLPAIRS_GRAVITY_SOFTENED, (su.K_SQUARED, su.SOFTENING_AU2), None)])
    x, v, a = body["world_pos"].copy(), body["world_vel"].copy(), np.zeros((len(ids), 6))
    for _ in range(240):                                                           # ten days of one-hour RK4 ticks
        x, v, a, _f = np_sixdof.tick(x, v, a, inertia, eff, su.DT, integrator=L.RK4)
    ref.step(240)
    err = max(float(np.max(np.abs(x[:, 4:] - ref.world_pos[:, 4:])) / np.max(np.abs(ref.world_pos[:, 4:]))),
              float(np.max(np.abs(v[:, 3:] - ref.world_vel[:, 3:])) / np.max(np.abs(ref.world_vel[:, 3:]))))
    print("examples/n-body/sim.py unmodified: traced fold vs the oracle's softened all-pairs op over 240 ticks:", f"{err:.1e}")
    assert err < 1e-12
    assert set(w.generated_sources(system, simulation_rate=sim.SIMULATION_RATE_HZ)) == {"pair"}


def test_apollo_lander_script_builds_and_generates(compat):
    import elodin as el
    sys.path.insert(0, str(REF / "examples" / "apollo-lander"))
    sim = _load(REF / "examples" / "apollo-lander" / "sim.py", "ref_apollo_sim")
    world, system = sim.build(el.monte_carlo.params(sim.PARAMS))             # main.py:88-90
    plan = world.build(system, simulation_rate=sim.SIMULATION_RATE_HZ, telemetry_rate=sim.TELEMETRY_RATE_HZ, _dry=True)
    tp = plan["effectors"].trace()
    assert plan["integrator"] == 1 and abs(plan["dt"] - 1.0 / 120.0) < 1e-9
    assert [e.__name__ for e in plan["effectors"].effectors.effectors] == ["lunar_gravity", "apply_main_thrust", "apply_rcs_torque"]
    assert [s.name for s in tp.pre] == ["truth_playback", "engine_response", "attitude_control", "mass_props", "thrust_visualization"]
    assert [s.name for s in tp.post] == ["ground_contact", "derive_telemetry"] and len(tp.columns) == 22
    src = world.generated_sources(system, simulation_rate=sim.SIMULATION_RATE_HZ)["step"]
    assert "apply_rcs_torque" in src and "ground_contact" in src


@pytest.mark.parametrize("case", ["pad", "maxq", "coast"])
def test_falcon9_plant_script_unmodified_follows_the_reference_flown_windows(compat, case):
    from tests import dsl_numpy, falcon9_plant_util as pu, falcon9_unmodified_util as fu
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(50000)
    try:
        plan, tp, a = fu.build(case)
        assert plan["integrator"] == 1 and len(tp.columns) == 62
        assert [s.name for s in tp.pre][:3] == ["commands", "attitude_control", "valve_dynamics"] and "imu_model" in [s.name for s in tp.post]
        if case == "maxq":
            from elodin_amd import codegen
            frozen = pu.load_program_fixture()     # what tests/test_gpu_falcon9_unmodified.py runs
            assert codegen.generate_variant(tp, frozen["variant"], "float64", plan["integrator"]) == frozen["source"], \
                "re-run tests/golden/make_falcon9_plant_program.py"
            guarded = codegen.generate_source(tp, "float32", plan["integrator"], fast_math=True, guard_selects=True)
            assert guarded == frozen["source_f32_fast_guarded"] and guarded.count("if (__any(") == 8
            assert codegen.generate_source(tp, "float32", plan["integrator"], fast_math=True) == frozen["source_f32_fast"]      # the switch is off by default
        pos, vel, acc, inertia = a["world_pos"], a["world_vel"], a["world_accel"], a["inertia"]
        comps = {name: a[name] for name, _ in tp.columns}
        worst = {}
        for tick in range(1, 1001):
            force = dsl_numpy.program_tick(tp, pos, vel, acc, inertia, comps, tick, plan["dt"], plan["integrator"], dt=plan["time_step"])
            if tick in (1, 2, 10, 500, 1000):
                body = {"world_pos": pos, "world_vel": vel, "world_accel": acc, "inertia": inertia, "force": force}
                for k, e in pu.compare(case, tick, lambda name: body[name] if name in body else comps[name]).items():
                    worst[k] = max(worst.get(k, 0.0), e)
    finally:
        sys.setrecursionlimit(limit)
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print(f"examples/falcon9/sim.py unmodified, window {case}: worst of {len(worst)} columns over 1,000 ticks:", ", ".join(f"{k} {e:.1e}" for k, e in top))
    assert len(worst) == 43 and max(worst.values()) < 1e-11, top


def test_stablehlo_script_unmodified_lands_on_the_reference_baseline(compat):
    from tests import dsl_numpy, stablehlo_dsl as S
    sys.path.insert(0, str(REF / "examples" / "stablehlo"))
    _load(REF / "examples" / "stablehlo" / "main.py", "ref_stablehlo_main")         # `from sim import ...; world().run(...)`: recorded
    sim = sys.modules["sim"]
    w = sim.world()
    plan = w.build(sim.system(), simulation_rate=sim.SIMULATION_RATE, _dry=True)
    tp = plan["effectors"].trace()
    names = [n for n, _ in tp.columns if not n.startswith("has:")]
    assert len(names) == 8 and plan["integrator"] != 1          # no six_dof in this example: systems only
    gold = json.loads((ROOT / "tests" / "golden" / "stablehlo.json").read_text())["rows"]
    n = next(iter(plan["columns"].values())).shape[0]
    comps = {name: np.array(plan["columns"][name], dtype=np.float64).reshape(n, -1).copy() for name, _ in tp.columns}
    pos, vel, acc, inertia = np.tile([0, 0, 0, 1.0, 0, 0, 0], (n, 1)), np.zeros((n, 6)), np.zeros((n, 6)), np.ones((n, 7))
    # math_state's baseline predates the example's current math_step (tests/test_dsl_host.py): that column is compared with the
    # respelled system's walk, which is itself checked against a numpy transcription there
    from elodin_amd import dsl
    tm = dsl.ColumnTable("c", 48, 16, {"math_state": 4})
    t_math = dsl.TracedSystem(S.math_step, tm)
    math_ref = {"math_state": np.array([S.INITIAL["math_state"]])}
    dummy = (np.array([[0, 0, 0, 1.0, 0, 0, 0]]), np.zeros((1, 6)), np.ones((1, 7)))
    worst = {}
    for tick in range(1, 101):
        dsl_numpy.program_tick_systems_only(tp, pos, vel, acc, inertia, comps, tick)
        dsl_numpy._run_systems([t_math], *dummy, math_ref, tm, tick)
        for name, rows in gold.items():
            row = int(np.argmax(comps["has:" + name][:, 0]))
            ref = math_ref["math_state"][0] if name == "math_state" else np.asarray(rows[tick])
            worst[name] = max(worst.get(name, 0.0), float(np.max(np.abs(comps[name][row] - ref) / np.maximum(np.abs(ref), 1e-12))))
    print("examples/stablehlo/main.py unmodified vs its CI baseline, worst per component:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert len(worst) == 8 and max(worst.values()) < 1e-12 and worst["bitwise_state"] == 0.0, worst


def load_cube_sat(compat):
    """examples/cube-sat/main.py imported unmodified; the one thing replaced is the evaluation of its EGM08 field (compat refuses
    it: the coefficient tables are a download), by a zero field — see tests/cube_sat_util.py for what that leaves pinned."""
    from elodin_amd import dsl
    compat.install(run="record")
    egm = sys.modules["elodin.egm08"].EGM08
    refused = egm.compute_field
    egm.compute_field = lambda self, x, y, z, mass: dsl.np.array([x * 0.0, y * 0.0, z * 0.0])
    try:
        ref = _load(REF / "examples" / "cube-sat" / "main.py", "ref_cube_sat_main")     # runs w.run(...) at import: recorded
        run = ref.w.compat_run
        assert run["simulation_rate"] == 120.0 and run["max_ticks"] == 144000
        plan = ref.w.build(run["system"], simulation_rate=run["simulation_rate"], _dry=True)
    finally:
        egm.compute_field = refused
    row_ids = [int(e) for e in plan["row_ids"]]
    row_of = {name: row_ids.index(e) for name, e in plan["names"].items() if e in row_ids}
    row_of["earth"] = next(k for k in range(len(row_ids)) if plan["columns"]["has:world_pos"][k, 0] > 0.5 and k != row_of["ore_sat"])
    return ref, plan, row_of


def test_cube_sat_script_unmodified_closes_its_attitude_loop_on_the_reference_baseline(compat):
    from tests import cube_sat_util as U, dsl_numpy
    ref, plan, row_of = load_cube_sat(compat)
    tp = plan["effectors"].trace()
    assert plan["integrator"] == 1 and plan["substeps"] == 1 and len(row_of) == 11 and dict(tp.columns)["P"] == 36
    assert [s.name for s in tp.fold_stages] == ["sun_sensor", "sun_sensor_value", "actuator_allocator", "rw_effector"]
    from elodin_amd import codegen
    frozen = json.loads((ROOT / "tests" / "golden" / "cube_sat_program.json").read_text())       # what tests/test_gpu_cube_sat.py runs
    assert codegen.generate_variant(tp, frozen["variant"], "float64", plan["integrator"]) == frozen["source"], "re-run tests/golden/make_cube_sat_program.py"
    g = U.gold()
    body, cols = plan["body"], plan["columns"]
    n = len(plan["row_ids"])
    pos, vel, acc, inertia = (np.array(body[k], dtype=np.float64).copy() for k in ("world_pos", "world_vel", "world_accel", "inertia"))
    comps = {name: (np.array(cols[name], dtype=np.float64).reshape(n, -1).copy() if name in cols else np.zeros((n, w)))
             for name, w in tp.columns}                                          # fold scratch rows start at zero
    worst = {}
    for tick in range(1, 101):
        U.put_translation(g, tick, pos, vel, row_of["ore_sat"])
        force = dsl_numpy.program_tick(tp, pos, vel, acc, inertia, comps, tick, plan["dt"], plan["integrator"], dt=plan["time_step"])
        U.errors(g, tick, row_of, dict(world_pos=pos, world_vel=vel, world_accel=acc, force=force, inertia=inertia), comps.get, worst)
    print("examples/cube-sat/main.py unmodified vs its CI baseline (attitude loop closed), worst per column:",
          {k: f"{v:.1e}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:12]}, f"... {len(worst)} columns")
    U.verdict(worst)


def test_shim_keeps_data_and_traced_code_apart(compat):
    import jax
    import jax.numpy as jnp
    from jax import lax, random
    from elodin_amd import dsl
    a = jnp.array([1.0, 2, 3])
    assert isinstance(a, np.ndarray) and a.dtype == np.float64 and jnp.eye(2).dtype == np.float64 and jnp.int64(5) == 5
    assert jnp.array([1, 2, 3]).dtype == np.int64 and jnp.zeros(3).dtype == np.float64        # jax_enable_x64 rules
    x = dsl.leaf("x")
    assert isinstance(jnp.sin(x), dsl.Expr) and isinstance(jnp.array([1.0, 2.0]) * x, dsl.Vec) and isinstance(jnp.cos(0.5), float)
    with dsl.tracing():
        assert isinstance(jnp.array([1.0, 2.0]), dsl.Vec) and isinstance(jnp.eye(3), list)
    assert isinstance(lax.cond(x > 0.0, lambda _: x, lambda _: -x, operand=None), dsl.Expr)
    assert isinstance(random.normal(random.key(dsl.leaf("seed")), shape=(3,)), dsl.Vec)
    with pytest.raises(NotImplementedError, match="grad"):
        jax.grad(lambda v: v)
    stacked = jax.vmap(lambda row: row * x)(jnp.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]))       # unrolled over the leading axis
    assert isinstance(stacked, list) and len(stacked) == 3 and isinstance(stacked[0], dsl.Vec) and len(stacked[0]) == 2
    table = jnp.asarray(np.array([10.0, 20.0, 30.0]))
    assert isinstance(table[x], dsl.Expr) and table[1] == 20.0                  # a traced index into a host table: a select chain
    with pytest.raises(NotImplementedError, match="traced values"):
        jnp.unwrap(jnp.array([1.0, 2.0]) * x)          # numpy functions without a traced counterpart refuse traced values
    with pytest.raises(AttributeError, match="not provided"):
        jnp.fft


def test_rocket_script_unmodified_lands_on_the_reference_baseline(compat):
    """examples/rocket/main.py as it is: its polars table preparation (elodin_amd/compat_polars.py over pandas), `map_coordinates`
    over the aero grid, the 480 x 3 sample window spelled `concatenate((buffer[1:], row))` (recognised as a push) and
    `lax.scan` over `signal[2:]` with stacked outputs of which only `[-1]` is read (a loop in the kernel, dsl.LazyRows) — 100
    ticks free-running on the CPU walker against scripts/ci/baseline/rocket-csv, all 24 columns + the final window."""
    from elodin_amd import _lib as L
    from tests import dsl_numpy, rocket_util as U
    sys.path.insert(0, str(REF / "examples" / "rocket"))
    main = _load(REF / "examples" / "rocket" / "main.py", "ref_rocket_main")
    world = next(v for v in vars(main).values() if hasattr(v, "compat_run"))
    run = world.compat_run
    plan = world.build(run["system"], simulation_rate=run["simulation_rate"], telemetry_rate=run["telemetry_rate"], _dry=True)
    tp = plan["effectors"].trace()
    assert tp.windows == {"v_rel_accel_buffer": (tp.windows["v_rel_accel_buffer"][0], 480, 3)} and tp.pre_reads_accel
    assert plan["integrator"] == L.RK4 and abs(plan["dt"] - U.GOLDEN["simulation_time_step"]) < 1e-15
    from elodin_amd import codegen
    frozen = json.loads((ROOT / "tests" / "golden" / "rocket_program.json").read_text())      # what tests/test_gpu_rocket.py runs on the GPU box
    assert codegen.generate_variant(tp, frozen["variant"], "float64", plan["integrator"]) == frozen["source"], "re-run tests/golden/make_rocket_program.py"
    body = plan["body"]
    pos, vel, inertia = (np.array(body[k], dtype=np.float64).reshape(1, -1).copy() for k in ("world_pos", "world_vel", "inertia"))
    comps = {name: np.array(plan["columns"][name], dtype=np.float64).reshape(1, -1).copy() for name, _ in tp.columns if not name.endswith("#head")}
    comps["v_rel_accel_buffer#head"] = np.zeros((1, 1))
    acc, worst = np.zeros((1, 6)), {}
    for tick in range(1, 101):
        F = dsl_numpy.program_tick(tp, pos, vel, acc, inertia, comps, tick, plan["dt"], L.RK4)
        got = {k: v[0] for k, v in comps.items()}
        got.update(world_pos=pos[0], world_vel=vel[0], world_accel=acc[0], force=F[0], inertia=inertia[0])
        U.check_row(tick, got, worst)
    print("examples/rocket/main.py unmodified vs its CI baseline, CPU walker:", {k: f"{v:.1e}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:6]})
    U.assert_all_columns(worst)
    window = dsl_numpy.window_rows(comps, "v_rel_accel_buffer", 480, 3)[0].ravel()
    want = np.array(U.GOLDEN["v_rel_accel_buffer_final"])
    assert np.abs(window - want).max() < 1e-9 * np.abs(want).max()


def test_falcon9_full_mission_script_unmodified_flies_the_closed_loop_ascent_window(compat):
    """examples/falcon9/main.py — the FULL mission world (plant + sensors + truth ghost + display scoring: 65 component columns,
    more than the 64 a program could hold before round 4), unmodified.  Its program is stepped on the CPU walker with main.py's
    OWN post_step bridging to the flight software on the server loop's cadence (only the UDP socket is replaced, by
    oracle/falcon9_fsw.c — exactly how tests/golden/make_falcon9_closed_loop.py flew the reference's plant), from the pad through
    navigator initialisation, the ignition command and liftoff (tick 878): every component the fixture holds at its checkpoints up
    to tick 1,000 of flight 0 (the calibrated defaults), and the flight software's own state."""
    from elodin_amd import _lib as L
    from oracle import falcon9_fsw as fsw_mod
    from tests import dsl_numpy, falcon9_closed_loop_util as cu
    if "0" not in cu.FLIGHTS:
        pytest.skip("closed-loop fixture not generated")
    flight = cu.FLIGHTS["0"]
    ex_dir = REF / "examples" / "falcon9"
    sys.path.insert(0, str(ex_dir))
    main = _load(ex_dir / "main.py", "ref_falcon9_main")
    world = main.world
    run = world.compat_run
    assert run["post_step"] is main.post_step and run["simulation_rate"] == 1000.0
    plan = world.build(run["system"], simulation_rate=run["simulation_rate"], telemetry_rate=run["telemetry_rate"], _dry=True)
    tp = plan["effectors"].trace()
    assert len(tp.columns) == 65 and plan["integrator"] == L.SEMI_IMPLICIT
    from elodin_amd import codegen
    frozen = json.loads((ROOT / "tests" / "golden" / "falcon9_main_program.json").read_text())      # what tests/test_gpu_falcon9_main.py runs on the GPU box
    assert codegen.generate_variant(tp, frozen["variant"], "float64", plan["integrator"]) == frozen["source"], "re-run tests/golden/make_falcon9_main_program.py"
    booster = next(e for e, nm in world._names.items() if nm == "booster")

    def row_of(name, width):          # the booster's row of a component (the executor's rows are the Body join = the booster)
        try:
            rows, ids = world.column(name)
        except KeyError:
            return np.zeros((1, width))
        hit = np.nonzero(ids == booster)[0]
        return rows[hit[:1]].astype(np.float64).reshape(1, -1) if len(hit) else np.zeros((1, width))
    comps = {name: (np.array([[1.0 if booster in world.column(name[4:])[1] else 0.0]]) if name.startswith("has:") else row_of(name, w))
             for name, w in tp.columns}
    pos, vel, inertia = (row_of(k, w) for k, w in (("world_pos", 7), ("world_vel", 6), ("inertia", 7)))
    acc = np.zeros((1, 6))
    body = {"world_pos": pos, "world_vel": vel, "world_accel": acc, "inertia": inertia}
    fsw = fsw_mod.Fsw(fsw_mod.read_raw_profile(ex_dir / "data" / "crs12" / "stage1_raw.json"))

    class OracleBridge:                     # main.py:221-243 minus the socket
        def exchange(self, state):
            return fsw.step(np.asarray(state, dtype=np.float64))
    main.bridge = OracleBridge()

    class Ctx:                              # el.StepContext.component_batch_operation over the walker's arrays
        def component_batch_operation(self, reads=None, writes=None):
            if writes:
                for name, v in writes.items():
                    k = name.split(".", 1)[1]
                    (body[k] if k in body else comps[k])[0] = np.asarray(v, dtype=np.float64).reshape(-1)
                return None
            out = {}
            for name in reads:
                k = name.split(".", 1)[1]
                src = body[k] if k in body else (comps[k] if k in comps else row_of(k, 1))
                out[name] = np.array(src[0], dtype=np.float64).reshape(-1)
            return out
    ctx = Ctx()
    # the LIVE bridge the GPU box flies this loop with (tests/falcon9_bridge.py: the packet layout restated as data, the script's
    # constants from the fixture) runs beside main.py's own post_step, on the same reads, with its own flight-software instance:
    # it must write exactly what main.py writes, tick for tick — that is what pins it on the reference's code
    from tests import falcon9_bridge
    assert frozen["exchange"]["reads"] == list(main.READS) and frozen["exchange"]["period_ticks"] == main.guidance_period_ticks
    twin_writes = {}

    class TwinCtx:
        def component_batch_operation(self, reads=None, writes=None):
            if writes:
                twin_writes.clear()
                twin_writes.update({k: np.array(v, dtype=np.float64).reshape(-1) for k, v in writes.items()})
                return None
            return ctx.component_batch_operation(reads=reads)
    twin = falcon9_bridge.Exchange(frozen["exchange"], fsw_mod.Fsw(table=__import__("elodin_amd.models.falcon9", fromlist=["x"]).ascent_profile()))
    twin_ctx, twin_checked = TwinCtx(), 0
    cps = {c["tick"]: c for c in flight["checkpoints"] if c["tick"] <= 1000}
    worst, seen, fsw_worst = {}, 0, 0.0
    for tick in range(1, 1001):
        F = dsl_numpy.program_tick(tp, pos, vel, acc, inertia, comps, tick, plan["dt"], L.SEMI_IMPLICIT)
        twin_writes.clear()
        twin.post_step(tick - 1, twin_ctx)  # reads only (its writes are captured, not applied)
        main.post_step(tick - 1, ctx)       # the server loop's call after the tick (ticks_per_telemetry = 1)
        for name, v in twin_writes.items():
            k = name.split(".", 1)[1]
            assert np.array_equal((body[k] if k in body else comps[k])[0], v), (tick, name)
            twin_checked += 1
        if tick in cps:
            cp = dict(cps[tick], state={k: v for k, v in cps[tick]["state"].items() if k != "fsw"})
            cp["state"]["fsw"] = {}
            state = dict(body, force=F)
            for k, e in cu.compare(flight, cp, lambda name: state[name] if name in state else comps[name]).items():
                worst[k] = max(worst.get(k, 0.0), e)
            pk = fsw.peek()
            for k, want in cps[tick]["state"]["fsw"].items():
                if k in pk and k in cu.FSW_MAP:
                    got, want = np.asarray(pk[k], dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
                    fl = cu.FLOORS.get(k, 1e-300)
                    fsw_worst = max(fsw_worst, float(np.max(np.abs(got - want))) / max(float(np.max(np.abs(want))), fl if not isinstance(fl, tuple) else fl[0]))
            seen += 1
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print(f"examples/falcon9/main.py unmodified, closed loop on the CPU walker: worst of {len(worst)} quantities at {seen} checkpoints:",
          ", ".join(f"{k} {e:.1e}" for k, e in top), f"; flight software state {fsw_worst:.1e}")
    assert seen >= 7 and len(worst) >= 45
    assert max(worst.values()) < 1e-9 and fsw_worst < 1e-9, (top, fsw_worst)
    assert float(comps["lifted"][0, 0]) == 1.0 and fsw.peek()["phase"] == 1.0      # off the pad, vertical rise
    assert twin.exchanges == 100 and twin_checked == 700                            # 100 exchanges x 7 written components, all identical
