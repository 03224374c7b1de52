"""The step kernels after their slab movement was re-addressed (csrc/step_kernel.hpp: slabs_dma_in in every kernel; slab_flush
and the ragged wave's late flush in the RK4 kernels): one address per column, the 1-KiB chunks as immediate offsets, the lanes
of the partial last chunk masked once, and under RK4 no early store by the ragged wave.  The semi-implicit kernels keep their
one-column flush.  No arithmetic changed, so every path computes what it did.

Sizes: the ragged wave alone (1, 31, 32, 33, 47, 48, 49, 63: around the remainder-lane boundaries 32 and 48 of the partial
chunks, although the ragged wave itself moves element-wise), one full wave (64), and full waves with a ragged one (65, 128,
129).  Per dtype, integrator and pipe: 8 ticks straight after the upload, so the first launch is the accel-check kernel,
stepped
  * as one-tick launches with graph replay on (the AQL chain),
  * the same with SIXDOF_AQL=0 (hipGraph replay),
  * the same eagerly,
  * as fused 4-tick launches.
All four columns are byte-identical among the four handles, and the AQL handle's lie within the parity tolerance of the oracle:
f64 at parity.F64_RTOL of the f64 C oracle; f32 under the gate of tests/f32_parity_util.py (4 x what the float32 numpy
restatement loses against the oracle on the float32-rounded inputs, floor 8 * 2^-24).

Pipes: gravity | body_torque (the benchmark's compile-time pipe) and body_torque | world_force (no compile-time pipe: the
interpreter runs).

The f64 RK4 gravity | body_torque case again under the other two shipped cache policies (SIXDOF_STREAMING=0: plain stores,
=9: non-temporal loads too), and once recording into a 4-slot history ring: a recording launch flushes late, through the
non-temporal ring policy, so after every tick the ring's rows of that tick are compared with the live columns."""
from functools import lru_cache

import numpy as np
import pytest

import elodin_amd as ea
from elodin_amd import _lib as L
from elodin_amd import workloads
from tests import f32_parity_util as fu
from tests import parity

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 47, 48, 49, 63, 64, 65, 128, 129)
TICKS = 8
FUSED = 4
PIPES = {
    "gravity_torque": fu.PIPES["gravity_torque"],
    "torque_world_force": [fu.TORQUE, (L.EFF_WORLD_FORCE, (), "world_force")],
}
NAMES = {L.RK4: "rk4", L.SEMI_IMPLICIT: "semi_implicit"}
PATHS = ("aql", "hipgraph", "eager", "fused")
rounded = lambda p: tuple(float(np.float32(v)) for v in p)      # the oracle helper's op parameters: both sides see the same doubles


@lru_cache(maxsize=None)
def references(pipe_name, integrator, dtype_name):
    """(oracle state, float32 restatement or None) after TICKS ticks on all rows of the shared world, once per process: rows
    are independent, so a case of n rows is the first n."""
    cols, pipe = fu.world(), PIPES[pipe_name]
    if dtype_name == "f64":
        return fu.run_oracle(pipe, integrator, cols, ticks=(TICKS,), dt=workloads.DT_120HZ)[TICKS], None
    return fu.run_oracle(pipe, integrator, cols, ticks=(TICKS,))[TICKS], fu.run_restatement(pipe, integrator, cols, ticks=(TICKS,))[TICKS]


def handle(monkeypatch, path, pipe, integrator, dtype, cols):
    if path == "hipgraph":
        monkeypatch.setenv("SIXDOF_AQL", "0")          # read when the handle is created
    else:
        monkeypatch.delenv("SIXDOF_AQL", raising=False)
    eff = [ea.Effector(kind, rounded(p), aux_name=aux, aux=None if aux is None else cols[aux]) for kind, p, aux in pipe]
    ex = ea.HipExec(cols["world_pos"], cols["world_vel"], cols["inertia"], dtype=dtype, simulation_time_step=workloads.DT_120HZ,
                    integrator=integrator, effectors=eff, device=0, ticks_per_launch=FUSED if path == "fused" else 1,
                    use_graph=path in ("aql", "hipgraph"))
    monkeypatch.delenv("SIXDOF_AQL", raising=False)
    want = {"aql": "aql", "hipgraph": "hipgraph: SIXDOF_AQL=0"}.get(path)
    assert ex.step_path == want if want else ex.step_path.startswith("eager") or path == "fused", (path, ex.step_path)
    return ex


def run_paths(monkeypatch, pipe, integrator, dtype, n, what):
    """TICKS ticks from a fresh upload on every path; the four columns byte-identical among them.  -> the AQL handle's columns."""
    cols = {k: v[:n] for k, v in fu.world().items()}
    ex = {path: handle(monkeypatch, path, pipe, integrator, dtype, cols) for path in PATHS}
    try:
        for path, e in ex.items():
            if path in ("aql", "hipgraph"):
                e.prepare(TICKS)
            t = e.invoke_batch(TICKS)
            assert t.launches == (TICKS // FUSED if path == "fused" else TICKS), (what, path, t.launches)
            assert e.tick == TICKS
            e.download()
        for f in parity.FIELDS:
            want = ex["fused"]
            assert getattr(want, f).dtype == dtype
            for path in PATHS[:3]:
                a, b = getattr(ex[path], f), getattr(want, f)
                assert a.tobytes() == b.tobytes(), (what, f, f"{path} differs from the fused launches", np.argwhere(a != b)[:4].tolist())
        return fu.snapshot(ex["aql"])
    finally:
        for e in ex.values():
            e.close()


def check_f64(got, ref, n, what, lines, failures):
    errs = parity.state_errors(got, fu.rows_of(ref, slice(0, n)))
    lines.append(f"{what}: {errs}")
    if not max(errs.values()) < parity.F64_RTOL:
        failures.append(f"{what}: {errs}")


@pytest.mark.parametrize("integrator", (L.RK4, L.SEMI_IMPLICIT), ids=NAMES.get)
@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("pipe_name", list(PIPES))
def test_every_path_agrees_bytewise_and_with_the_oracle_at_the_slab_boundaries(monkeypatch, pipe_name, dtype_name, integrator):
    monkeypatch.delenv("SIXDOF_STREAMING", raising=False)
    pipe, dtype = PIPES[pipe_name], {"f64": np.float64, "f32": np.float32}[dtype_name]
    ref, rest = references(pipe_name, integrator, dtype_name)
    lines, failures = [], []
    for n in SIZES:
        what = f"{pipe_name} {dtype_name} {NAMES[integrator]} n {n} ticks {TICKS}"
        got = run_paths(monkeypatch, pipe, integrator, dtype, n, what)
        if dtype_name == "f64":
            check_f64(got, ref, n, what, lines, failures)
        else:
            want = fu.rows_of(ref, slice(0, n))
            kerr, rerr = fu.half_errors(got, want), fu.half_errors(fu.rows_of(rest, slice(0, n)), want)
            lines.append(f"{what}: kernel {fu.fmt(kerr)} | restatement {fu.fmt(rerr)}  [2^-24]")
            for half, bound in fu.gate(rerr).items():
                if not kerr[half] <= bound:
                    failures.append(f"{what} {half}: kernel {kerr[half] / fu.U32:.2f} > gate {bound / fu.U32:.2f} x 2^-24")
    fu.record(lines, "step_slab_issue_parity.txt")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("policy", ["0", "9"])
def test_the_other_shipped_cache_policies(monkeypatch, policy):
    """f64 RK4 gravity | body_torque under plain stores (0) and under non-temporal loads and stores (9)."""
    monkeypatch.setenv("SIXDOF_STREAMING", policy)
    pipe = PIPES["gravity_torque"]
    ref, _ = references("gravity_torque", L.RK4, "f64")
    lines, failures = [], []
    for n in SIZES:
        what = f"gravity_torque f64 rk4 SIXDOF_STREAMING={policy} n {n} ticks {TICKS}"
        check_f64(run_paths(monkeypatch, pipe, L.RK4, np.float64, n, what), ref, n, what, lines, failures)
    fu.record(lines, "step_slab_issue_parity.txt")
    assert not failures, "\n".join(failures)


def test_a_recording_launch_writes_the_ring_rows_it_leaves_in_the_live_columns(monkeypatch):
    """f64 RK4 gravity | body_torque with a 4-slot history ring, one tick per launch, TICKS ticks (the ring wraps once): after
    every tick the ring's rows of that tick equal the live columns byte for byte, and the last state is the oracle's."""
    monkeypatch.delenv("SIXDOF_STREAMING", raising=False)
    monkeypatch.delenv("SIXDOF_AQL", raising=False)
    pipe = PIPES["gravity_torque"]
    ref, _ = references("gravity_torque", L.RK4, "f64")
    lines, failures = [], []
    for n in SIZES:
        what = f"gravity_torque f64 rk4 ring 4 n {n}"
        cols = {k: v[:n] for k, v in fu.world().items()}
        eff = [ea.Effector(kind, rounded(p), aux_name=aux, aux=None if aux is None else cols[aux]) for kind, p, aux in pipe]
        ex = ea.HipExec(cols["world_pos"], cols["world_vel"], cols["inertia"], dtype=np.float64, simulation_time_step=workloads.DT_120HZ,
                        integrator=L.RK4, effectors=eff, device=0)
        try:
            ex.enable_history(4)
            for tick in range(1, TICKS + 1):
                ex.invoke_batch(1)
                ex.download()
                for f in parity.FIELDS:
                    ring, live = ex.history(f, tick, tick)[0], getattr(ex, f)
                    assert ring.tobytes() == live.tobytes(), (what, f, tick, np.argwhere(ring != live)[:4].tolist())
            check_f64(fu.snapshot(ex), ref, n, what, lines, failures)
        finally:
            ex.close()
    fu.record(lines, "step_slab_issue_parity.txt")
    assert not failures, "\n".join(failures)
