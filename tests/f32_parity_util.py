"""Float32 step parity: the case matrix, the numpy restatement of the built-in per-entity effectors, and the gate that
tests/test_f32_restatement_host.py (CPU) and tests/test_gpu_f32_step_parity.py (GPU) share.  TEST INFRASTRUCTURE.

Reference of every comparison: the f64 C oracle fed the float32-ROUNDED inputs converted back to double (state, inertia,
aux columns, op parameters, float(np.float32(dt))).  The float32 restatement (tests/np_sixdof.py on float32 columns with
`builtin_effectors` below) only measures what that rounding costs an honest implementation in the reference's operation
order; the kernel is then allowed a small multiple of it (`gate`).  No tolerance comes from the kernel."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from elodin_amd import _lib as L
from elodin_amd import workloads
from oracle import oracle as orc
from tests import np_sixdof, parity

U32 = 2.0 ** -24                     # unit roundoff of float32: every figure below is reported in these
RESTATEMENT_CAP = 32 * U32           # host test: the restatement is never further than this from the oracle
KERNEL_FACTOR, KERNEL_FLOOR = 4.0, 8 * U32
NMAX = 200                           # rows of the shared world; row i depends on i alone, so a case of n rows is its first n
SIZES = (1, 63, 64, 65, 130)         # lone ragged wave, largest ragged wave, one DMA slab, slab + 1 tail row, 2 slabs + 2 tail rows
TICKS = (1, 4)
INTEGRATORS = (L.RK4, L.SEMI_IMPLICIT)
HALVES = tuple(f"{f}.{h}" for f in parity.FIELDS for h in ("a", "b"))   # a: quaternion / angular half, b: position / linear half

GRAVITY = (L.EFF_UNIFORM_GRAVITY, (0.0, 0.0, -9.81), None)
TORQUE = (L.EFF_BODY_TORQUE, (), "body_torque")
THRUST = (L.EFF_BODY_FORCE, (), "thrust")
DRAG = (L.EFF_BALL_DRAG, (0.5, 1.2, 0.3), "wind")
ZERO_WRENCH = (L.EFF_CONST_WRENCH, (0.0,) * 6, None)      # adds nothing, but no compile-time pipe has it: the interpreter runs
_STATIC = {"none": [], "gravity": [GRAVITY], "gravity_torque": [GRAVITY, TORQUE], "gravity_drag": [GRAVITY, DRAG],
           "gravity_thrust_torque": [GRAVITY, THRUST, TORQUE]}
PIPES = dict(_STATIC)
PIPES.update({f"interp_{k}": v + [ZERO_WRENCH] for k, v in _STATIC.items()})
PIPES["interp_four_aux"] = [TORQUE, THRUST, (L.EFF_WORLD_TORQUE, (), "world_torque"), DRAG]   # the drag clears the torques, as in the reference
PIPES["interp_world_frame"] = [(L.EFF_CONST_WRENCH, (0.1, -0.2, 0.3, 1.0, -2.0, 3.0), None), (L.EFF_WORLD_TORQUE, (), "world_torque"),
                               (L.EFF_WORLD_FORCE, (), "world_force")]
STATIC_PIPES = tuple(_STATIC)

f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
DT32 = float(np.float32(workloads.DT_120HZ))


@lru_cache(maxsize=None)
def world():
    """workloads.independent_bodies(NMAX) with seeded aux columns, every value rounded to float32 (held as float64)."""
    w = workloads.independent_bodies(NMAX)
    rng = np.random.default_rng(0xF32)
    cols = dict(world_pos=w["world_pos"], world_vel=w["world_vel"], inertia=w["inertia"], body_torque=w["body_torque"],
                wind=rng.normal(size=(NMAX, 3)) * 3.0, thrust=rng.normal(size=(NMAX, 3)) * 50.0,
                world_torque=rng.normal(size=(NMAX, 3)), world_force=rng.normal(size=(NMAX, 3)) * 50.0)
    out = {k: f32(v).astype(np.float64) for k, v in cols.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def builtin_effectors(ops, inertia):
    """numpy restatement of the seven built-in per-entity effectors in the oracle's operation order (oracle/sixdof_oracle.c
    `effectors`): ops = [(kind, params, aux [n,3] or None)] in the dtype of the state; returns the effectors(xs, vs)
    callback np_sixdof.tick expects.  (The oracle's `+ 0.0` on the untouched half can only change the sign of a zero.)"""
    def effectors(xs, vs):
        T = xs.dtype.type
        F = np.zeros((len(xs), 6), dtype=xs.dtype)
        for kind, p, aux in ops:
            p = np.array(p, dtype=xs.dtype)
            if kind == L.EFF_CONST_WRENCH:
                F = F + p[None, :6]
            elif kind == L.EFF_UNIFORM_GRAVITY:
                F[:, 3:] = F[:, 3:] + p[None, :3] * inertia[:, 6:7]
            elif kind == L.EFF_BODY_TORQUE:
                F[:, :3] = F[:, :3] + np_sixdof.rot(xs[:, :4], aux)
            elif kind == L.EFF_BODY_FORCE:
                F[:, 3:] = F[:, 3:] + np_sixdof.rot(xs[:, :4], aux)
            elif kind == L.EFF_WORLD_TORQUE:
                F[:, :3] = F[:, :3] + aux
            elif kind == L.EFF_WORLD_FORCE:
                F[:, 3:] = F[:, 3:] + aux
            elif kind == L.EFF_BALL_DRAG:
                fl = aux - vs[:, 3:]
                V = np.sqrt(fl[:, 0] * fl[:, 0] + fl[:, 1] * fl[:, 1] + fl[:, 2] * fl[:, 2])
                drag = T(0.5) * ((p[0] * p[1]) * (V * V) * p[2])
                F[:, :3] = T(0.0)       # el.SpatialForce(linear=...) has zero torque
                F[:, 3:] = F[:, 3:] + drag[:, None] * (fl / V[:, None])
            else:
                raise ValueError(f"not a built-in per-entity effector: {kind}")
        return F
    return effectors


def snapshot(src):
    return SimpleNamespace(**{f: np.array(getattr(src, f), dtype=np.float64) for f in parity.FIELDS})


def rows_of(state, rows):
    return SimpleNamespace(**{f: getattr(state, f)[rows] for f in parity.FIELDS})


def half_errors(got, ref):
    """parity.state_errors with the two halves of each column kept apart: {"world_pos.a": ..., "world_pos.b": ..., ...}."""
    errs = {}
    for f in parity.FIELDS:
        cut = 4 if f == "world_pos" else 3
        g, r = getattr(got, f), getattr(ref, f)
        errs[f + ".a"] = parity.field_rel_err(g[:, :cut], r[:, :cut])
        errs[f + ".b"] = parity.field_rel_err(g[:, cut:], r[:, cut:])
    return errs


def oracle_ops(pipe, cols, rows=slice(None)):
    return [(kind, tuple(float(np.float32(v)) for v in p), None if aux is None else cols[aux][rows]) for kind, p, aux in pipe]


def run_oracle(pipe, integrator, cols, ticks=TICKS, dt=DT32, world_accel=None):
    """{ticks: state} of the f64 C oracle on `cols` (already float32-rounded)."""
    ref = orc.OracleWorld(cols["world_pos"], cols["world_vel"], cols["inertia"], world_accel=world_accel, simulation_time_step=dt,
                          integrator=integrator, ops=oracle_ops(pipe, cols))
    out, done = {}, 0
    for t in ticks:
        ref.step(t - done)
        out[t], done = snapshot(ref), t
    return out


def run_restatement(pipe, integrator, cols, ticks=TICKS, dt=DT32, dtype=np.float32, world_accel=None):
    """{ticks: state} of tests/np_sixdof.py in `dtype` arithmetic on the same inputs."""
    c = {k: np.ascontiguousarray(v, dtype=dtype) for k, v in cols.items()}
    n = len(c["world_pos"])
    eff = builtin_effectors(oracle_ops(pipe, c), c["inertia"])      # parameters float32-rounded, like the oracle's
    pos, vel = c["world_pos"], c["world_vel"]
    acc = np.zeros((n, 6), dtype=dtype) if world_accel is None else np.ascontiguousarray(world_accel, dtype=dtype)
    out = {}
    with np.errstate(all="ignore"):      # edge rows divide by zero and rotate infinities on purpose
        for t in range(1, max(ticks) + 1):
            pos, vel, acc, F = np_sixdof.tick(pos, vel, acc, c["inertia"], eff, dt, integrator=integrator)
            assert pos.dtype == vel.dtype == acc.dtype == F.dtype == np.dtype(dtype)
            if t in ticks:
                out[t] = SimpleNamespace(world_pos=pos.astype(np.float64), world_vel=vel.astype(np.float64),
                                         world_accel=acc.astype(np.float64), force=F.astype(np.float64))
    return out


@lru_cache(maxsize=None)
def references(pipe_name, integrator):
    """(oracle, float32 restatement) of one matrix case on all NMAX rows of the shared world, computed once per process:
    rows are independent, so the first n rows of each are the case of size n."""
    cols = world()
    return run_oracle(PIPES[pipe_name], integrator, cols), run_restatement(PIPES[pipe_name], integrator, cols)


def gate(restatement_errs):
    """Per column half: what the kernel may be off by, given what the float32 restatement is off by in the same case."""
    return {k: max(KERNEL_FACTOR * v, KERNEL_FLOOR) for k, v in restatement_errs.items()}


def fmt(errs):
    """The four columns (worse half of each) in units of 2^-24."""
    return " ".join(f"{f} {max(errs[f + '.a'], errs[f + '.b']) / U32:.2f}" for f in parity.FIELDS)


def record(lines, name="f32_step_parity.txt"):
    """Print the figures; on a GPU run with a scratch output directory they are appended there (parity.Worst.report)."""
    if lines:
        parity.Worst.report("\n".join(lines), name)
