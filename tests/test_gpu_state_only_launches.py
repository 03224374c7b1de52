"""State-only launches (StepParams::state_only, csrc/sixdof_capi.cpp state_only_eligible): inside one sixdof_step call
every launch but the last leaves world_accel and force unwritten, and after every call all four columns are, byte for byte,
what a handle stepped one tick per call holds — each of its launches closes its call, so it never uses the flag — and what a
SIXDOF_STATE_ONLY=0 handle stepped with the same batches holds.  On the AQL, hipGraph and eager paths."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COLUMNS = ("world_pos", "world_vel", "world_accel", "force")

# n = 1: the ragged-tail path only; 64: one full wave (LDS-DMA slabs); 100: a full wave and a ragged 36-row one
SIZES = [1, 64, 100]
PATHS = ["aql", "hipgraph", "eager"]

# K = 1 batches, in this order on one handle, the first straight after the upload (it opens with the accel-check launch):
# closing launch only | 2 | all eager | smallest chain, which closes the batch | 32-chain + one eager closing launch |
# two 32-chains, the second closing | chain + 3 eager | nothing
K1_BATCHES = [1, 2, 3, 4, 33, 64, 35, 0]
K1_AFTER_UPLOAD = 20        # after a fresh upload: the check launch, then a chain
# K = 4: no remainder (the last full launch closes) | the remainder launch closes | a batch shorter than K
K4_BATCHES = [8, 103, 3]


def _exec(monkeypatch, path, n, k=1, state_only=True, kind="f64_rk4", world=None):
    import elodin_amd as ea
    from elodin_amd import _lib as L
    from elodin_amd import workloads
    kw = {"f64_rk4": {}, "f32_rk4": {"dtype": np.float32}, "f64_semi_implicit": {"integrator": L.SEMI_IMPLICIT}}[kind]
    for name, off in (("SIXDOF_AQL", path == "hipgraph"), ("SIXDOF_STATE_ONLY", not state_only)):
        if off:
            monkeypatch.setenv(name, "0")        # both are read when the handle is created
        else:
            monkeypatch.delenv(name, raising=False)
    w = workloads.independent_bodies(n) if world is None else world
    eff = workloads.gravity_torque_effectors(w["body_torque"])
    ex = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], world_accel=w.get("world_accel"),
                    entity_ids=w["entity_ids"], simulation_time_step=workloads.DT_120HZ, effectors=eff, device=0,
                    ticks_per_launch=k, use_graph=path != "eager", **kw)
    monkeypatch.delenv("SIXDOF_AQL", raising=False)
    monkeypatch.delenv("SIXDOF_STATE_ONLY", raising=False)
    return ex


def _trio(monkeypatch, path, n, k=1, kind="f64_rk4", world=None):
    """The handle under test, the same with SIXDOF_STATE_ONLY=0, and the yardstick stepped one tick per call."""
    ex = [_exec(monkeypatch, path, n, k, True, kind, world), _exec(monkeypatch, path, n, k, False, kind, world),
          _exec(monkeypatch, "eager", n, 1, True, kind, world)]
    want = {"aql": "aql", "hipgraph": "hipgraph: SIXDOF_AQL=0"}.get(path)
    for e in ex[:2]:
        assert e.step_path == want if want else e.step_path.startswith("eager"), e.step_path
    return ex


def _batch_and_compare(ex, ticks, what, prepare=True):
    test, off, yard = ex
    counts = []
    for e in (test, off):
        if prepare:
            e.prepare(ticks)
        t = e.invoke_batch(ticks)
        counts.append((t.launches, t.graph_launches))
    assert counts[0] == counts[1], (what, counts)
    for _ in range(ticks):
        t = yard.invoke_batch(1)
        assert (t.launches, t.graph_launches) == (1, 0)
    assert test.tick == off.tick == yard.tick
    for e in ex:
        e.download()
    for f in COLUMNS:
        a, b, c = (getattr(e, f).tobytes() for e in ex)
        assert a == c, (what, f, "differs from the tick-by-tick handle")
        assert a == b, (what, f, "differs from the SIXDOF_STATE_ONLY=0 handle")
    return counts[0]


def _close(ex):
    for e in ex:
        e.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", SIZES)
def test_k1_batches_leave_the_bytes_of_tick_by_tick_stepping(monkeypatch, n, path):
    ex = _trio(monkeypatch, path, n)
    try:
        for i, ticks in enumerate(K1_BATCHES):
            before = {f: getattr(ex[0], f).tobytes() for f in COLUMNS}
            launches, _ = _batch_and_compare(ex, ticks, (n, path, ticks), prepare=i % 2 == 0)
            assert launches == ticks
            if ticks == 0:
                assert all(getattr(ex[0], f).tobytes() == before[f] for f in COLUMNS), "an empty batch changed a column"
        for e in ex:
            e.upload()
        _batch_and_compare(ex, K1_AFTER_UPLOAD, (n, path, "after upload"))
    finally:
        _close(ex)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", SIZES)
def test_k4_batches_leave_the_bytes_of_tick_by_tick_stepping(monkeypatch, n, path):
    ex = _trio(monkeypatch, path, n, k=4)
    try:
        for ticks in K4_BATCHES:
            launches, _ = _batch_and_compare(ex, ticks, (n, path, ticks))
            assert launches == -(-ticks // 4)
    finally:
        _close(ex)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", ["f32_rk4", "f64_semi_implicit"])
def test_other_kernels_leave_the_bytes_of_tick_by_tick_stepping(monkeypatch, kind, path):
    ex = _trio(monkeypatch, path, 100, kind=kind)
    try:
        for ticks in K1_BATCHES[:5]:
            _batch_and_compare(ex, ticks, (kind, path, ticks))
    finally:
        _close(ex)


# Neither is a GPU fault: both are the reference's NaN semantics (rk4.rs:96-100: stage 0 forms v0 + 0 * a_in from the
# uploaded world_accel; a non-finite quaternion poisons its row), and the NaNs must come out byte-identical too.
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", ["nan_world_accel_row", "non_finite_quaternion_row"])
def test_non_finite_rows_leave_the_bytes_of_tick_by_tick_stepping(monkeypatch, case, path):
    from elodin_amd import workloads
    w = dict(workloads.independent_bodies(100))
    if case == "nan_world_accel_row":
        w["world_accel"] = np.zeros((100, 6))
        w["world_accel"][70] = np.nan
    else:
        w["world_pos"] = np.array(w["world_pos"], copy=True)
        w["world_pos"][37, :4] = [np.inf, 0.0, np.nan, 1.0]
    ex = _trio(monkeypatch, path, 100, world=w)
    try:
        _batch_and_compare(ex, 20, (case, path))
        poisoned = 70 if case == "nan_world_accel_row" else 37
        bad = ~np.isfinite(ex[0].world_vel).all(axis=1) | ~np.isfinite(ex[0].world_pos).all(axis=1)
        assert bad[poisoned] and bad.sum() == 1, np.flatnonzero(bad)
    finally:
        _close(ex)
