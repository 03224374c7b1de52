"""The float32 instantiations of sixdof_step_kernel against the f64 oracle at float32 accuracy: every compile-time pipe
and its interpreter twin, both integrators, ragged and full waves, three launch shapes; then the same matrix in f64.

The reference is the f64 C oracle on the float32-rounded inputs; the tolerance is what the float32 numpy restatement of
the same tick loses against it in the same case and column half, times 4, with a floor of 8 * 2^-24
(tests/f32_parity_util.py; the restatement itself is pinned by tests/test_f32_restatement_host.py).  Figures are printed
in units of 2^-24 and, on a GPU run with a scratch output directory, appended there (profiles/f32_step_parity.md)."""
import numpy as np
import pytest

import elodin_amd as ea
from elodin_amd import _lib as L
from elodin_amd import workloads
from tests import f32_parity_util as fu
from tests import parity

pytestmark = pytest.mark.gpu
NAMES = {L.RK4: "rk4", L.SEMI_IMPLICIT: "semi_implicit"}


def executor(pipe, integrator, cols, dtype=np.float32, params=lambda p: p, **kw):
    eff = [ea.Effector(kind, params(p), aux_name=aux, aux=None if aux is None else cols[aux]) for kind, p, aux in pipe]
    return ea.HipExec(cols["world_pos"], cols["world_vel"], cols["inertia"], dtype=dtype, simulation_time_step=workloads.DT_120HZ,
                      integrator=integrator, effectors=eff, **kw)


def run(pipe, integrator, cols, ticks, **kw):
    """The four columns after `ticks` ticks on a fresh handle, in the executor's own dtype."""
    ex = executor(pipe, integrator, cols, **kw)
    ex.run(ticks)
    assert ex.tick == ticks
    out = {f: getattr(ex, f).copy() for f in parity.FIELDS}
    ex.close()
    return out


def check_gate(what, got, ref, rest, lines, failures):
    """Kernel error <= max(4 x restatement error, 8 * 2^-24) in every column half; both figures go to `lines`."""
    kerr, rerr = fu.half_errors(got, ref), fu.half_errors(rest, ref)
    lines.append(f"{what}: kernel {fu.fmt(kerr)} | restatement {fu.fmt(rerr)}  [2^-24]")
    for half, bound in fu.gate(rerr).items():
        if not kerr[half] <= bound:
            failures.append(f"{what} {half}: kernel {kerr[half] / fu.U32:.2f} > gate {bound / fu.U32:.2f} (restatement {rerr[half] / fu.U32:.2f}) x 2^-24")


@pytest.mark.parametrize("integrator", fu.INTEGRATORS, ids=NAMES.get)
@pytest.mark.parametrize("name", list(fu.PIPES))
def test_f32_step_meets_the_oracle_at_f32_accuracy_in_every_launch_shape(name, integrator):
    pipe = fu.PIPES[name]
    ref, rest = fu.references(name, integrator)
    lines, failures = [], []
    for n in fu.SIZES:
        cols = {k: v[:n] for k, v in fu.world().items()}
        ones = run(pipe, integrator, cols, 4, ticks_per_launch=1)            # four one-tick launches
        fused = run(pipe, integrator, cols, 4, ticks_per_launch=4)           # one fused launch
        split = run(pipe, integrator, cols, 4, ticks_per_launch=3)           # 3 + 1
        for f in parity.FIELDS:
            assert fused[f].dtype == np.float32
            assert ones[f].tobytes() == fused[f].tobytes(), (n, f, "1+1+1+1 vs 4", np.argwhere(ones[f] != fused[f])[:4].tolist())
            assert split[f].tobytes() == fused[f].tobytes(), (n, f, "3+1 vs 4", np.argwhere(split[f] != fused[f])[:4].tolist())
        first = run(pipe, integrator, cols, 1, ticks_per_launch=1)
        for t, got in ((1, first), (4, fused)):
            check_gate(f"{name} {NAMES[integrator]} n {n} ticks {t}", fu.snapshot(fu.SimpleNamespace(**got)),
                       fu.rows_of(ref[t], slice(0, n)), fu.rows_of(rest[t], slice(0, n)), lines, failures)
    fu.record(lines)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("integrator", fu.INTEGRATORS, ids=NAMES.get)
@pytest.mark.parametrize("name", list(fu.PIPES))
def test_f64_step_meets_the_oracle_on_the_same_matrix(name, integrator):
    """The same pipes in f64 at the north-star tolerance: the world-frame pipe under RK4 and the static / interpreter twins
    had no f64 case against the oracle either."""
    n, pipe = 130, fu.PIPES[name]
    cols = {k: v[:n] for k, v in fu.world().items()}
    rounded = lambda p: tuple(float(np.float32(v)) for v in p)       # the oracle helper's parameters, so both see the same doubles
    got = run(pipe, integrator, cols, 4, dtype=np.float64, params=rounded, ticks_per_launch=4)
    ref = fu.run_oracle(pipe, integrator, cols, ticks=(4,), dt=workloads.DT_120HZ)[4]
    errs = parity.state_errors(fu.SimpleNamespace(**got), ref)
    print(f"f64 {name} {NAMES[integrator]} n {n} ticks 4: {errs}")
    assert max(errs.values()) < parity.F64_RTOL, errs
    if name.startswith("interp_") and name[7:] in fu.STATIC_PIPES:       # the twin adds a zero wrench: same state as the static pipe
        twin = run(fu.PIPES[name[7:]], integrator, cols, 4, dtype=np.float64, params=rounded, ticks_per_launch=4)
        errs = parity.state_errors(fu.SimpleNamespace(**got), fu.SimpleNamespace(**twin))
        assert max(errs.values()) < parity.F64_RTOL, ("twin", errs)


@pytest.mark.parametrize("n", [130, 191])       # 191: two slabs and a 63-row tail
@pytest.mark.parametrize("k", [1, 4])
def test_f32_results_do_not_depend_on_which_lane_or_wave_an_entity_lands_in(n, k):
    """The f32 form of test_results_do_not_depend_on_which_lane_or_workgroup_an_entity_lands_in: rows permuted, every entity
    in another lane and wave, the tail elsewhere — the same rows, permuted, bit for bit (gravity + drag, RK4, 8 ticks)."""
    pipe = fu.PIPES["gravity_drag"]
    cols = {key: v[:n] for key, v in fu.world().items()}
    perm = np.random.default_rng(n + k).permutation(n)
    a = run(pipe, L.RK4, cols, 8, ticks_per_launch=k)
    b = run(pipe, L.RK4, {key: v[perm] for key, v in cols.items()}, 8, ticks_per_launch=k)
    for f in parity.FIELDS:
        assert a[f][perm].tobytes() == b[f].tobytes(), (f, np.argwhere(a[f][perm] != b[f])[:4].tolist())
    assert np.isfinite(a["world_pos"]).all() and not np.array_equal(a["world_vel"], fu.f32(cols["world_vel"]))


def test_f32_entity_set_joins_vs_the_oracle():
    """The 4-byte gather / scatter instantiations, built the way test_random_entity_set_joins_vs_the_oracle builds its worlds:
    100 bodies; world_vel bound on a superset of 110 ids in scrambled order; inertia on a subset of 70 ids, which makes the
    Body join 70 rows (one slab and a tail of 6); the torque column on those 70 ids, scrambled.  (An effector column takes
    no part in the join, and one that does not cover it is refused — that is why the 70-id set arrives through a Body
    column.)  Entity e carries row e - 1 of the shared world in every column, so the joined rows meet the shared reference
    under the same gate; rows outside the join come back byte for byte."""
    w, rng = fu.world(), np.random.default_rng(70)
    ids = {"world_pos": np.arange(1, 101, dtype=np.uint64), "world_vel": rng.permutation(np.arange(1, 111)).astype(np.uint64),
           "inertia": np.sort(rng.choice(np.arange(1, 101), size=70, replace=False)).astype(np.uint64)}
    ids["world_accel"] = ids["force"] = ids["world_pos"]
    ids["body_torque"] = rng.permutation(ids["inertia"])
    joined = ids["inertia"]
    data = {k: fu.f32(w[k][(ids[k] - 1).astype(np.int64)]) for k in ("world_pos", "world_vel", "inertia", "body_torque")}
    outside = ~np.isin(ids["world_pos"], joined)
    for k in ("world_accel", "force"):          # a sentinel where the kernel has no business; zeros (the reference's input) on the join
        data[k] = np.zeros((100, 6), dtype=np.float32)
        data[k][outside] = 7.0
    eff = [ea.Effector(L.EFF_UNIFORM_GRAVITY, fu.GRAVITY[1]), ea.Effector(L.EFF_BODY_TORQUE, (), aux_name="body_torque", aux=data["body_torque"])]
    hip = ea.HipExec(data["world_pos"], data["world_vel"], data["inertia"], world_accel=data["world_accel"], force=data["force"],
                     entity_ids=ids["world_pos"], dtype=np.float32, simulation_time_step=workloads.DT_120HZ, effectors=eff,
                     ticks_per_launch=4, column_entity_ids=ids)
    assert hip.n == 70
    hip.run(4)
    rows = {k: hip.join_rows(k) for k in ids}
    for k in ids:
        where = {int(e): r for r, e in enumerate(ids[k])}
        assert rows[k].tolist() == [where[int(j)] for j in joined], k
    got = fu.snapshot(fu.SimpleNamespace(**{f: getattr(hip, f)[rows[f]] for f in parity.FIELDS}))
    ref, rest = fu.references("gravity_torque", L.RK4)
    sel = (joined - 1).astype(np.int64)
    lines, failures = [], []
    check_gate("join 70 of 100, gravity_torque rk4 ticks 4", got, fu.rows_of(ref[4], sel), fu.rows_of(rest[4], sel), lines, failures)
    fu.record(lines)
    assert not failures, "\n".join(failures)
    for k in ("world_pos", "world_vel", "world_accel", "force", "inertia"):
        others = np.setdiff1d(np.arange(len(ids[k])), rows[k])
        assert len(others) == len(ids[k]) - 70
        assert getattr(hip, k)[others].tobytes() == data[k][others].tobytes(), k          # not in the join: untouched
    assert hip.inertia.tobytes() == data["inertia"].tobytes()
    hip.close()


def finite_rows(state):
    return np.isfinite(np.concatenate([getattr(state, f) for f in parity.FIELDS], axis=1)).all(axis=1)


def check_patterns_and_gate(what, pipe, integrator, cols, world_accel=None):
    """1 and 4 ticks: NaN and finiteness patterns equal the oracle's in all four columns; the rows the oracle keeps finite
    pass the gate.  Returns {ticks: kernel state}."""
    ref = fu.run_oracle(pipe, integrator, cols, world_accel=world_accel)
    rest = fu.run_restatement(pipe, integrator, cols, world_accel=world_accel)
    lines, failures, out = [], [], {}
    for t in fu.TICKS:
        got = fu.snapshot(fu.SimpleNamespace(**run(pipe, integrator, cols, t, ticks_per_launch=t, world_accel=world_accel)))
        for f in parity.FIELDS:
            g, r = getattr(got, f), getattr(ref[t], f)
            assert np.array_equal(np.isnan(g), np.isnan(r)), (what, t, f, np.argwhere(np.isnan(g) != np.isnan(r))[:5].tolist())
            assert np.array_equal(np.isfinite(g), np.isfinite(r)), (what, t, f, np.argwhere(np.isfinite(g) != np.isfinite(r))[:5].tolist())
        ok = finite_rows(ref[t])
        assert finite_rows(rest[t])[ok].all()
        check_gate(f"{what} ticks {t}, {int(ok.sum())} finite rows", fu.rows_of(got, ok), fu.rows_of(ref[t], ok), fu.rows_of(rest[t], ok), lines, failures)
        out[t] = (got, ok)
    fu.record(lines)
    assert not failures, "\n".join(failures)
    return out


@pytest.mark.parametrize("integrator", fu.INTEGRATORS, ids=NAMES.get)
def test_f32_infinite_and_zero_mass_rows_follow_the_reference_division(integrator):
    """The f32 form of test_infinite_and_zero_mass_rows_follow_the_reference_division (spatial.hpp `recip(float)`: same rule in
    both dtypes): the same four rows, the same constant world-frame force + body-frame torque."""
    n = 200
    cols = {k: v[:n].copy() for k, v in fu.world().items()}
    cols["inertia"][3, 6] = np.inf                 # infinite mass only
    cols["inertia"][50, [0, 1, 2, 6]] = np.inf     # a static anchor
    cols["inertia"][120, 1] = np.inf               # one infinite principal moment
    cols["inertia"][199, 6] = 0.0                  # zero mass under a force
    pipe = [(L.EFF_CONST_WRENCH, (0.0, 0.0, 0.0, 1.0, -2.0, 3.0), None), fu.TORQUE]
    for t, (got, ok) in check_patterns_and_gate(f"division edges {NAMES[integrator]}", pipe, integrator, cols).items():
        assert ok[[3, 50, 120]].all() and not ok[199] and ok.sum() == n - 1
        assert np.isnan(got.world_accel[199, 3:]).all()
        assert np.all(got.world_accel[50] == 0.0) and np.all(got.world_accel[3, 3:] == 0.0)      # the anchor does not accelerate


@pytest.mark.parametrize("name", ["gravity_drag", "gravity_torque"])
def test_f32_poisoned_rows_end_where_the_reference_does(name):
    """The reference's NaN semantics in f32, RK4, 100 rows: a NaN world_accel row at upload (read once, by the first
    launch's CHECK kernel: v_s = v0 + 0 * a_in), a quaternion row [inf, 0, nan, 1], and — with the drag — a row whose wind
    equals its linear velocity exactly (0 / 0 in the drag, as in the reference)."""
    n = 100
    cols = {k: v[:n].copy() for k, v in fu.world().items()}
    accel = np.zeros((n, 6))
    accel[7, 4] = np.nan
    cols["world_pos"][40, :4] = [np.inf, 0.0, np.nan, 1.0]
    cols["wind"][66] = cols["world_vel"][66, 3:]
    out = check_patterns_and_gate(f"poisoned rows {name}", fu.PIPES[name], L.RK4, cols, world_accel=accel)
    for t, (got, ok) in out.items():
        bad = [7, 40] + ([66] if name == "gravity_drag" else [])
        assert not ok[bad].any() and ok.sum() == n - len(bad), (t, np.argwhere(~ok).ravel().tolist())
        assert np.isnan(got.world_pos[7, 5]) and np.isnan(got.world_accel[40]).all()


def test_f64_velocity_reading_pipe_carries_a_nan_attitude_into_the_force_column():
    """What the f32 poisoned rows found, in f64: with a drag in the pipe the reference's last RK4 stage sees
    v_s = v0 + dt * A_2 with A_2 = NaN for a non-finite attitude, so the `force` column of that row is NaN from the first
    tick on, not only world_accel and the state."""
    n, pipe = 100, fu.PIPES["gravity_drag"]
    cols = {k: v[:n].copy() for k, v in fu.world().items()}
    cols["world_pos"][40, :4] = [np.inf, 0.0, np.nan, 1.0]
    rounded = lambda p: tuple(float(np.float32(v)) for v in p)
    for t in fu.TICKS:
        got = fu.SimpleNamespace(**run(pipe, L.RK4, cols, t, dtype=np.float64, params=rounded, ticks_per_launch=t))
        ref = fu.run_oracle(pipe, L.RK4, cols, ticks=(t,), dt=workloads.DT_120HZ)[t]
        for f in parity.FIELDS:
            assert np.array_equal(np.isnan(getattr(got, f)), np.isnan(getattr(ref, f))), (t, f)
        ok = finite_rows(ref)
        assert not ok[40] and ok.sum() == n - 1 and np.isnan(got.force[40, 3:]).all()
        errs = parity.state_errors(fu.rows_of(got, ok), fu.rows_of(ref, ok))
        assert max(errs.values()) < parity.F64_RTOL, (t, errs)
