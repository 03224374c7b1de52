"""The built-in step kernels after their argument reads moved to kernel entry and their aux rows lost the run-time width
(csrc/step_kernel.hpp: read_entry_args, load_aux): entry, ragged-tail and aux code at the sizes where each can go wrong.

Per pipe, dtype and integrator, at n in {1, 63, 64, 65, 129} (a lone ragged wave, the largest ragged wave, one DMA slab,
a slab and one tail row, two slabs and one tail row): 5 ticks straight after the upload — the first launch is the
accel-check kernel — and then 5 more, stepped
  * as one-tick launches with graph replay on (the AQL chain),
  * the same with SIXDOF_AQL=0 (hipGraph replay),
  * the same eagerly,
  * as one fused 5-tick launch per batch.
After each batch all four columns are byte-identical among the four handles and within the parity tolerance of the oracle:
f64 at parity.F64_RTOL of the f64 C oracle; f32 under the gate of tests/f32_parity_util.py (4 x what the float32 numpy
restatement loses against the oracle on the float32-rounded inputs, floor 8 * 2^-24).

Pipes: gravity | body_torque (the benchmark's compile-time pipe, one aux column); gravity | thrust | body_torque (compile-time,
two aux columns); body_torque | world_force (two aux columns, no compile-time pipe: the interpreter runs)."""
from functools import lru_cache

import numpy as np
import pytest

import elodin_amd as ea
from elodin_amd import _lib as L
from elodin_amd import workloads
from tests import f32_parity_util as fu
from tests import parity

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 129)
BATCHES = (5, 10)          # tick counts at which the columns are compared: after the batch behind the upload, and after one more
PIPES = {
    "gravity_torque": fu.PIPES["gravity_torque"],
    "gravity_thrust_torque": fu.PIPES["gravity_thrust_torque"],
    "torque_world_force": [fu.TORQUE, (L.EFF_WORLD_FORCE, (), "world_force")],
}
NAMES = {L.RK4: "rk4", L.SEMI_IMPLICIT: "semi_implicit"}
PATHS = ("aql", "hipgraph", "eager", "fused")
rounded = lambda p: tuple(float(np.float32(v)) for v in p)      # the oracle helper's op parameters: both sides see the same doubles


@lru_cache(maxsize=None)
def references(pipe_name, integrator, dtype_name):
    """({ticks: oracle state}, {ticks: float32 restatement} or None) on all rows of the shared world, once per process: rows are
    independent, so a case of n rows is the first n."""
    cols, pipe = fu.world(), PIPES[pipe_name]
    if dtype_name == "f64":
        return fu.run_oracle(pipe, integrator, cols, ticks=BATCHES, dt=workloads.DT_120HZ), None
    return fu.run_oracle(pipe, integrator, cols, ticks=BATCHES), fu.run_restatement(pipe, integrator, cols, ticks=BATCHES)


def handle(monkeypatch, path, pipe, integrator, dtype, cols):
    if path == "hipgraph":
        monkeypatch.setenv("SIXDOF_AQL", "0")          # read when the handle is created
    else:
        monkeypatch.delenv("SIXDOF_AQL", raising=False)
    eff = [ea.Effector(kind, rounded(p), aux_name=aux, aux=None if aux is None else cols[aux]) for kind, p, aux in pipe]
    ex = ea.HipExec(cols["world_pos"], cols["world_vel"], cols["inertia"], dtype=dtype, simulation_time_step=workloads.DT_120HZ,
                    integrator=integrator, effectors=eff, device=0, ticks_per_launch=5 if path == "fused" else 1,
                    use_graph=path in ("aql", "hipgraph"))
    monkeypatch.delenv("SIXDOF_AQL", raising=False)
    want = {"aql": "aql", "hipgraph": "hipgraph: SIXDOF_AQL=0"}.get(path)
    assert ex.step_path == want if want else ex.step_path.startswith("eager") or path == "fused", (path, ex.step_path)
    return ex


@pytest.mark.parametrize("integrator", (L.RK4, L.SEMI_IMPLICIT), ids=NAMES.get)
@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("pipe_name", list(PIPES))
def test_one_tick_launches_on_every_path_match_a_fused_launch_and_the_oracle(monkeypatch, pipe_name, dtype_name, integrator):
    pipe, dtype = PIPES[pipe_name], {"f64": np.float64, "f32": np.float32}[dtype_name]
    ref, rest = references(pipe_name, integrator, dtype_name)
    lines, failures = [], []
    for n in SIZES:
        cols = {k: v[:n] for k, v in fu.world().items()}
        ex = {path: handle(monkeypatch, path, pipe, integrator, dtype, cols) for path in PATHS}
        try:
            done = 0
            for ticks in BATCHES:
                what = f"{pipe_name} {dtype_name} {NAMES[integrator]} n {n} ticks {done}..{ticks}"
                for path, e in ex.items():
                    if path in ("aql", "hipgraph"):
                        e.prepare(ticks - done)
                    t = e.invoke_batch(ticks - done)
                    assert t.launches == (1 if path == "fused" else ticks - done), (what, path, t.launches)
                    assert e.tick == ticks
                    e.download()
                done = ticks
                for f in parity.FIELDS:
                    want = ex["fused"]
                    assert getattr(want, f).dtype == dtype
                    for path in PATHS[:3]:
                        a, b = getattr(ex[path], f), getattr(want, f)
                        assert a.tobytes() == b.tobytes(), (what, f, f"{path} differs from the fused launch", np.argwhere(a != b)[:4].tolist())
                got = fu.snapshot(ex["aql"])
                want = fu.rows_of(ref[ticks], slice(0, n))
                if dtype_name == "f64":
                    errs = parity.state_errors(got, want)
                    lines.append(f"{what}: {errs}")
                    if not max(errs.values()) < parity.F64_RTOL:
                        failures.append(f"{what}: {errs}")
                else:
                    kerr, rerr = fu.half_errors(got, want), fu.half_errors(fu.rows_of(rest[ticks], slice(0, n)), want)
                    lines.append(f"{what}: kernel {fu.fmt(kerr)} | restatement {fu.fmt(rerr)}  [2^-24]")
                    for half, bound in fu.gate(rerr).items():
                        if not kerr[half] <= bound:
                            failures.append(f"{what} {half}: kernel {kerr[half] / fu.U32:.2f} > gate {bound / fu.U32:.2f} x 2^-24")
        finally:
            for e in ex.values():
                e.close()
    fu.record(lines, "step_entry_loads_parity.txt")
    assert not failures, "\n".join(failures)
