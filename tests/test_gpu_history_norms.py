"""Ring norms (sixdof_history_norms): per probe and run, over the sampled ticks of a range, the smallest and the largest squared
Euclidean norm of 1 to 4 elements of a row — or of their difference to as many elements of another row of the run — with the
earliest sampled tick that holds each, the count of finite samples and the earliest non-finite tick, reduced on the device out of
the telemetry ring.

The reference is always numpy over the [ticks, n, w] blocks HipExec.history reads from the same ring: d = A - B in f64, the sum of
squares left to right (numpy's multiply and add are separate roundings, as the kernel's, which is compiled without FMA
contraction), argmin / argmax on the integer keys of the doubles so that the first occurrence wins.  Nothing else is rounded, so
every comparison is np.array_equal (NaN equal to NaN) and no tolerance appears.

Every values case asserts ON THE REFERENCE that it can tell a wrong answer from a right one: min_sq < max_sq in every run, and
argmin takes more than one value across the runs.  Two cases cannot by their own definition — one sample has min_sq == max_sq,
one run has one argmin — and assert the part that can hold."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import elodin_amd as ea
from elodin_amd import _lib as L
from tests.test_gpu_history_watch import _exec

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
INT_KEYS = ("count", "argmin", "argmax", "first_nonfinite")
F64_KEYS = ("min_sq", "max_sq", "min", "max")

SPEED = ea.Norm("world_vel", 3, 3)                                               # |v|
SEPARATION = ea.Norm("world_pos", 4, 3, group=0, minus="world_pos", minus_group=1)    # |r_0 - r_1| of the run's rows 0 and 1
CROSS = ea.Norm("world_pos", 4, 3, minus="world_vel", minus_element=3)            # across components
QUATERNION = ea.Norm("world_pos", 0, 4)                                          # |q|
VERTICAL = ea.Norm("world_vel", 5, 1)                                            # count 1: v_z squared
EIGHT = [SPEED, SEPARATION, CROSS, QUATERNION, VERTICAL, ea.Norm("world_vel", 0, 3, group=1),                      # |omega| of row 1
         ea.Norm("world_vel", 4, 2, group=1, minus="world_accel", minus_element=3, minus_group=0),                 # (v_y, v_z) of row 1 against (a_x, a_y) of row 0
         ea.Norm("force", 0, 3, group=1, minus="force", minus_group=0)]                                            # the torques of the two rows


def _reference(hip, norms, first, last, every, period):
    """The dict of HipExec.history_norms out of HipExec.history."""
    ticks = np.arange(first, last + 1, every)
    names = {c for v in norms for c in (v.component, v.minus) if c is not None}
    blocks = {name: hip.history(name, first, last)[::every] for name in names}
    out = {k: [] for k in INT_KEYS + ("min_sq", "max_sq")}
    for v in norms:
        d = blocks[v.component][:, v.group::period, v.element:v.element + v.count].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            if v.minus is not None:
                e = v.element if v.minus_element is None else v.minus_element
                g = v.group if v.minus_group is None else v.minus_group
                d = d - blocks[v.minus][:, g::period, e:e + v.count].astype(np.float64)
            s = d[..., 0] * d[..., 0]
            for k in range(1, v.count):
                s = s + d[..., k] * d[..., k]                     # [samples, runs], left to right
        finite = np.isfinite(s)
        key = np.ascontiguousarray(s).view(np.int64)              # s is +0.0 or above where it is finite: the bit pattern is the order
        at_min = np.argmin(np.where(finite, key, np.iinfo(np.int64).max), axis=0)       # the first occurrence wins
        at_max = np.argmax(np.where(finite, key, -1), axis=0)
        count = finite.sum(axis=0)
        some, runs = count > 0, np.arange(s.shape[1])
        out["count"].append(count.astype(np.int64))
        out["min_sq"].append(np.where(some, s[at_min, runs], np.nan))
        out["max_sq"].append(np.where(some, s[at_max, runs], np.nan))
        out["argmin"].append(np.where(some, ticks[at_min], 0).astype(np.int64))
        out["argmax"].append(np.where(some, ticks[at_max], 0).astype(np.int64))
        out["first_nonfinite"].append(np.where(np.all(finite, axis=0), 0, ticks[np.argmax(~finite, axis=0)]).astype(np.int64))
    out = {k: np.stack(v) for k, v in out.items()}
    out["min"], out["max"] = np.sqrt(out["min_sq"]), np.sqrt(out["max_sq"])
    return out


def _same(got, want, what=""):
    assert sorted(got) == sorted(INT_KEYS + F64_KEYS), what
    for k in INT_KEYS + F64_KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, got[k].dtype)
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)
    for k in F64_KEYS:
        assert not np.any(np.signbit(got[k][~np.isnan(got[k])])), (what, k, "a square is never -0.0")


def _proves_something(want, n_samples, runs, what):
    """The reference itself shows that the case can fail: extremes that differ in every run, argmin not the same tick everywhere."""
    if n_samples > 1:
        assert np.all(want["min_sq"] < want["max_sq"]), (what, "min_sq < max_sq in every run")
    if n_samples > 1 and runs > 1:
        for p in range(want["argmin"].shape[0]):
            assert len(np.unique(want["argmin"][p])) > 1, (what, p, "argmin takes one value only")


def _recorded(n, dtype=np.float64, ticks_per_launch=4, ring=64, run=40):
    hip, _ = _exec(n, ticks_per_launch, dtype)
    hip.enable_history(ring)
    hip.run(run)
    return hip


def _buffer(hip, n_norms, period, fill=123.0):
    return np.full((n_norms, L.NORMS_PLANES, hip.n // period), fill)


def _raw(hip, norms, period, first, n_samples, every, buf, flags=0):
    probes = ea.HipExec._norm_probes(norms)
    return hip._lib.sixdof_history_norms(hip._h, probes, len(probes), period, first, n_samples, every, None if buf is None else buf.ctypes.data, flags)


# ---- 1. values ---------------------------------------------------------------------------------------------------------------
# (what, n, period, dtype, norms, ring, ticks run, first, last, every)
VALUES = [
    ("1 run", 2, 2, np.float64, [SPEED, SEPARATION], 64, 40, 1, 40, 1),
    ("63 runs", 126, 2, np.float32, [SPEED, SEPARATION], 64, 40, 1, 40, 1),                  # a wavefront's edge
    ("65 runs", 130, 2, np.float64, [SPEED, SEPARATION], 64, 40, 1, 40, 1),
    ("257 runs", 514, 2, np.float32, [SPEED, SEPARATION], 64, 40, 1, 40, 1),                 # a block's edge
    ("3 rows per run", 195, 3, np.float64, [ea.Norm("world_pos", 4, 3, group=2, minus="world_pos", minus_group=0), ea.Norm("world_vel", 3, 3, group=1)], 64, 40, 1, 40, 1),
    ("speed", 130, 2, np.float32, [SPEED], 64, 40, 1, 40, 1),
    ("separation", 130, 2, np.float64, [SEPARATION], 64, 40, 1, 40, 1),
    ("cross-component", 130, 2, np.float32, [CROSS], 64, 40, 1, 40, 1),
    ("quaternion", 130, 2, np.float64, [QUATERNION], 64, 40, 1, 40, 1),
    ("count 1", 130, 2, np.float32, [VERTICAL], 64, 40, 1, 40, 1),
    ("eight probes", 130, 2, np.float64, EIGHT, 64, 40, 1, 40, 1),
    ("wraps the ring", 130, 2, np.float64, [SPEED, SEPARATION], 10, 27, 18, 27, 1),         # ticks 18 .. 27 sit in slots 7 8 9 0 .. 6
    ("every 3", 130, 2, np.float32, [SPEED, SEPARATION], 64, 40, 2, 38, 3),
    ("13 samples", 130, 2, np.float64, [SPEED, SEPARATION, QUATERNION], 64, 40, 28, 40, 1),  # no multiple of a load depth (4, 2)
    ("a single sample", 130, 2, np.float32, [SPEED, SEPARATION], 64, 40, 17, 17, 1),
]


@pytest.mark.parametrize("what,n,period,dtype,norms,ring,run,first,last,every", VALUES, ids=[v[0] for v in VALUES])
def test_norms_equal_numpy_over_the_history_blocks(what, n, period, dtype, norms, ring, run, first, last, every):
    hip = _recorded(n, dtype, ring=ring, run=run)
    runs, n_samples = n // period, (last - first) // every + 1
    got = hip.history_norms(norms, first, last, every, period=period)
    assert got["count"].shape == (len(norms), runs) and got["count"].dtype == np.int64 and got["min_sq"].dtype == np.float64
    want = _reference(hip, norms, first, last, every, period)
    _proves_something(want, n_samples, runs, what)
    _same(got, want, what)
    assert np.all(got["count"] == n_samples) and np.all(got["first_nonfinite"] == 0)
    assert np.all((got["argmin"] - first) % every == 0) and np.all((got["argmin"] >= first) & (got["argmax"] <= last))
    hip.close()


# ---- 2. ties --------------------------------------------------------------------------------------------------------------
def test_a_row_against_itself_is_zero_from_the_first_sample_on():
    hip = _recorded(130, np.float32, ring=10, run=27)
    norms = [ea.Norm("world_vel", 3, 3, group=1, minus="world_vel"), ea.Norm("world_pos", 0, 4, minus="world_pos", minus_element=0, minus_group=0), SPEED]
    got = hip.history_norms(norms, 18, 27, every=3, period=2)                   # samples 18 21 24 27
    _same(got, _reference(hip, norms, 18, 27, 3, 2), "ties")
    for p in (0, 1):
        assert np.all(got["min_sq"][p] == 0.0) and np.all(got["max_sq"][p] == 0.0) and not np.any(np.signbit(got["min_sq"][p]))
        assert np.all(got["argmin"][p] == 18) and np.all(got["argmax"][p] == 18) and np.all(got["count"][p] == 4)
    assert np.all(got["min_sq"][2] < got["max_sq"][2])                          # the probe beside them is no tie
    hip.close()


# ---- 3. non-finite samples -------------------------------------------------------------------------------------------------
def test_non_finite_samples_are_skipped_and_dated():
    n, period = 130, 2
    hip, _ = _exec(n, 2)
    hip.world_vel[128] = np.nan                               # run 64, row 0: never finite
    hip.upload()
    hip.enable_history(16)
    hip.run(6)
    hip.world_vel[[0, 63]] = np.nan                           # run 0 row 0 and run 31 row 1: finite up to tick 6
    hip.world_vel[10, 4] = np.inf                             # run 5 row 0: one infinite element from tick 7 on
    hip.upload()
    hip.run(6)
    norms = [SPEED, ea.Norm("world_vel", 3, 3, group=1), SEPARATION]
    got = hip.history_norms(norms, 1, 12, period=period)
    want = _reference(hip, norms, 1, 12, 1, period)
    _same(got, want, "non-finite")
    speed0, speed1, separation = range(3)
    assert want["count"][speed0, 0] == 6 and want["first_nonfinite"][speed0, 0] == 7          # on the reference: skipped from tick 7 on
    assert want["count"][speed1, 31] == 6 and want["first_nonfinite"][speed1, 31] == 7
    assert want["count"][speed0, 5] == 6 and want["first_nonfinite"][speed0, 5] == 7          # the infinite element
    assert np.all(got["argmin"][speed0, [0, 5]] <= 6) and np.all(got["argmax"][speed0, [0, 5]] <= 6)
    assert got["count"][speed0, 64] == 0 and got["first_nonfinite"][speed0, 64] == 1          # none finite
    assert np.isnan(got["min_sq"][speed0, 64]) and np.isnan(got["max_sq"][speed0, 64]) and np.isnan(got["min"][speed0, 64])
    assert got["argmin"][speed0, 64] == 0 and got["argmax"][speed0, 64] == 0
    assert got["count"][separation, 64] < 12 and got["first_nonfinite"][separation, 64] > 0   # the NaN reaches the position
    others = np.setdiff1d(np.arange(n // period), [0, 5, 31, 64])
    assert np.all(got["count"][:, others] == 12) and np.all(got["first_nonfinite"][:, others] == 0)
    hip.close()


# ---- 4. cut invariance ------------------------------------------------------------------------------------------------------
CUT_CASE = dict(n=130, period=2, first=3, last=60, every=1)


def _cut_exec():
    hip = _recorded(CUT_CASE["n"], np.float64, ring=64, run=60)
    return hip


def _child(out_path):
    """What a child process of the cut-invariance test runs: SIXDOF_NORMS_SEGMENTS is what its environment says."""
    hip = _cut_exec()
    got = hip.history_norms(EIGHT, CUT_CASE["first"], CUT_CASE["last"], CUT_CASE["every"], period=CUT_CASE["period"])
    np.savez(out_path, **got)
    hip.close()


def test_forced_segment_counts_give_identical_arrays(tmp_path):
    children = {}
    for segments in ("1", "2", "3", "5", None):                # a fresh process per value: the library reads the variable per call,
        env = dict(os.environ)                                # but no process that holds the GPU changes its own environment here
        env.pop("SIXDOF_NORMS_SEGMENTS", None)
        if segments is not None:
            env["SIXDOF_NORMS_SEGMENTS"] = segments
        out = tmp_path / f"segments_{segments}.npz"
        code = f"import sys; sys.path.insert(0, {str(ROOT)!r}); from tests.test_gpu_history_norms import _child; _child({str(out)!r})"
        children[segments] = (subprocess.Popen([sys.executable, "-c", code], env=env, cwd=str(ROOT), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), out)
    hip = _cut_exec()
    want = _reference(hip, EIGHT, CUT_CASE["first"], CUT_CASE["last"], CUT_CASE["every"], CUT_CASE["period"])
    _proves_something(want, 58, 65, "cut invariance")
    hip.close()
    for segments, (proc, out) in children.items():
        text, _ = proc.communicate(timeout=120)
        assert proc.returncode == 0, (segments, text[-2000:])
        with np.load(out) as got:
            _same({k: got[k] for k in got.files}, want, f"SIXDOF_NORMS_SEGMENTS={segments}")


# ---- 5. longer than the ring ------------------------------------------------------------------------------------------------
def test_streamed_norms_over_a_ring_one_batch_deep_equal_one_read_of_a_whole_ring():
    n, period = 130, 2
    a, _ = _exec(n, 4)
    b, _ = _exec(n, 4)
    with pytest.raises(ValueError):
        a.stream_norms(EIGHT, 3, 8, every=3, period=period)
    wall, got = a.stream_norms(EIGHT, 3, 8, every=2, period=period)
    assert wall > 0.0 and a.tick == 24 and a._ring_ticks == 8
    b.enable_history(24)
    b.run(24)
    want = b.history_norms(EIGHT, 2, 24, every=2, period=period)
    _same(want, _reference(b, EIGHT, 2, 24, 2, period), "the twin")
    _same(got, want, "streamed")
    assert got["argmax"].max() > 16 and got["argmin"].min() < 8                # extremes in the last batch and in the first
    a.run(2)                                                 # the caller's flags are back: a blocking step, and the state a plain run leaves
    b.run(2)
    assert a.tick == 26
    for c in ("world_pos", "world_vel"):
        assert np.array_equal(getattr(a, c), getattr(b, c)), c
    for h in (a, b):
        h.close()


def test_hold_delivers_nothing_and_a_changed_probe_cannot_continue():
    n, period = 130, 2
    hip = _recorded(n, np.float32, ring=32, run=24)
    norms = [SPEED, SEPARATION]
    whole = hip.history_norms(norms, 1, 24, period=period)
    _same(whole, _reference(hip, norms, 1, 24, 1, period), "one call")
    buf = _buffer(hip, 2, period)
    bad = L.ERR_INVALID_ARGUMENT
    assert _raw(hip, norms, period, 1, 8, 1, buf, L.NORMS_HOLD) == L.OK and _raw(hip, norms, period, 9, 8, 1, buf, L.NORMS_HOLD | L.NORMS_CONTINUE) == L.OK
    assert np.all(buf == 123.0)                                                   # held: nothing is delivered
    changed = [SPEED, ea.Norm("world_pos", 4, 3, group=0, minus="world_pos", minus_element=3, minus_group=1)]
    assert _raw(hip, changed, period, 17, 8, 1, buf, L.NORMS_CONTINUE) == bad    # another minus_element
    assert _raw(hip, norms[::-1], period, 17, 8, 1, buf, L.NORMS_CONTINUE) == bad
    assert _raw(hip, norms, 1, 17, 8, 1, _buffer(hip, 2, 1), L.NORMS_CONTINUE) == bad        # another period
    assert _raw(hip, norms, period, 16, 9, 1, buf, L.NORMS_CONTINUE) == bad      # tick 16 is accumulated already
    assert b"16" in hip._lib.sixdof_last_error(hip._h)
    assert _raw(hip, norms, period, 17, 8, 1, None, 0) == bad and _raw(hip, norms, period, 17, 8, 1, buf, 8) == bad
    assert _raw(hip, [ea.Norm("world_vel", 4, 3)], period, 17, 8, 1, buf) == bad and b"width" in hip._lib.sixdof_last_error(hip._h)
    assert _raw(hip, [ea.Norm("world_vel", 3, 3, group=2)], period, 17, 8, 1, buf) == bad
    assert _raw(hip, [ea.Norm("inertia", 0, 3)], period, 17, 8, 1, buf) == L.ERR_COMPONENT_NOT_FOUND
    assert _raw(hip, norms, period, 17, 0, 1, buf, L.NORMS_CONTINUE) == L.OK     # no samples: a no-op
    assert np.all(buf == 123.0)                                                   # nothing was copied
    assert _raw(hip, norms, period, 17, 8, 1, buf, L.NORMS_CONTINUE) == L.OK     # the accumulator is what the held calls left
    _same(hip._norms_dict(buf), whole, "after the refusals")
    with pytest.raises(ValueError, match="period"):
        hip.history_norms(norms, 1, 24, period=7)
    with pytest.raises(KeyError):
        hip.history_norms([ea.Norm("inertia", 0, 3)], 1, 24, period=period)
    empty = hip.history_norms(norms, 24, 23, period=period)                       # no samples
    assert np.all(empty["count"] == 0) and np.all(np.isnan(empty["min"])) and np.all(empty["argmax"] == 0) and empty["max_sq"].shape == (2, 65)
    hip.close()


# ---- 6. upper layers ----------------------------------------------------------------------------------------------------------
def test_front_end_norms_of_one_entity_are_the_norms_of_its_series():
    spec = importlib.util.spec_from_file_location("ball", ROOT / "examples" / "ball.py")
    ball = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ball)
    six = ball.el.six_dof(sys=ball.gravity | ball.apply_drag)      # the same stage three times: three executor ticks per world tick
    ex = ball.world(0).build(ball.sample_wind | ball.bounce | six | six | six, simulation_rate=120.0, telemetry_rate=40.0, history=True)
    assert ex._substeps == 3
    ex.enable_history(128)
    ex.run(30)
    norms = [ea.Norm("world_vel", 3, 3), ea.Norm("world_pos", 4, 3, minus="world_vel", minus_element=3), ea.Norm("world_pos", 6, 1)]
    series = ex.history_series(["ball.world_pos", "ball.world_vel"], 2, 30, every=2)
    got = ex.history_norms(norms, 2, 30, every=2)
    ticks = np.arange(2, 31, 2)
    pos, vel = series["ball.world_pos"].astype(np.float64), series["ball.world_vel"].astype(np.float64)
    d = [vel[:, 3:6], pos[:, 4:7] - vel[:, 3:6], pos[:, 6:7]]
    for p, x in enumerate(d):
        s = x[:, 0] * x[:, 0]
        for k in range(1, x.shape[1]):
            s = s + x[:, k] * x[:, k]
        assert np.all(np.isfinite(s)) and s.min() < s.max()
        assert got["min_sq"][p, 0] == s.min() and got["max_sq"][p, 0] == s.max()
        assert got["argmin"][p, 0] == ticks[np.argmin(s)] and got["argmax"][p, 0] == ticks[np.argmax(s)]      # world ticks
        assert got["min"][p, 0] == np.sqrt(s.min()) and got["max"][p, 0] == np.sqrt(s.max())
    assert got["count"].shape == (3, 1) and np.all(got["count"] == 15) and np.all(got["first_nonfinite"] == 0)
    dt = ex._dt
    assert np.array_equal(got["t_min"], got["argmin"] * dt) and np.array_equal(got["t_max"], got["argmax"] * dt)
    assert np.all(np.isnan(got["t_first_nonfinite"]))                                                       # tick 0: no such time
    assert len({int(got["argmin"][p, 0]) for p in range(3)} | {int(got["argmax"][p, 0]) for p in range(3)}) > 1
    with pytest.raises(KeyError):
        ex.history_norms([ea.Norm("nothing", 0, 1)], 2, 30)
    with pytest.raises(ValueError):
        ex.history_norms(norms, 0, 30)                               # tick 0 is not in the ring
    with pytest.raises(ValueError):
        ex.history_norms(norms, 2, 30, every=0)


def test_campaign_norms_equal_numpy_over_the_runs_columns():
    """A 17-run campaign of the Monte-Carlo example: Campaign.norms against numpy over Campaign.column after each tick."""
    from tests.test_gpu_monte_carlo_example import GOLDEN, example
    from elodin_amd import vectorize
    ex = example(0)
    doc = json.loads((GOLDEN / "monte_carlo_example.json").read_text())
    params = [r["params"] for r in doc["runs"] if r["probe_rows"] == 0]
    c = vectorize.Campaign(ex.build, vectorize.plan_of((params * 17)[:17]), ex.PARAMS, simulation_rate=ex.SIMULATION_RATE_HZ)
    assert c.n_runs == 17 and c.entities_per_run == 1
    comps = ["position", "velocity"]
    c.exec.enable_history(16)
    cols = {name: [] for name in comps}
    for _ in range(12):
        c.exec.run(1)
        for name in comps:
            cols[name].append(np.array(c.column(name), dtype=np.float64).reshape(17, -1))
    ticks = np.arange(1, 13)
    pos, vel = np.stack(cols["position"]), np.stack(cols["velocity"])          # [tick, run, w]
    k = min(pos.shape[2], vel.shape[2], 4)
    norms = [ea.Norm("position", 0, min(pos.shape[2], 4)), ea.Norm("position", 0, k, minus="velocity"), ea.Norm("velocity", 0, 1)]
    got = c.norms(norms, 1, 12)
    rows = c.exec.history_norms(norms, 1, 12)
    for p, x in enumerate([pos[:, :, :min(pos.shape[2], 4)], pos[:, :, :k] - vel[:, :, :k], vel[:, :, :1]]):
        s = x[..., 0] * x[..., 0]
        for e in range(1, x.shape[2]):
            s = s + x[..., e] * x[..., e]
        assert np.all(np.isfinite(s))
        key = np.ascontiguousarray(s).view(np.int64)
        run = np.arange(17)
        assert np.array_equal(got["min_sq"][p], s[np.argmin(key, axis=0), run]) and np.array_equal(got["max_sq"][p], s[np.argmax(key, axis=0), run]), p
        assert np.array_equal(got["argmin"][p], ticks[np.argmin(key, axis=0)]) and np.array_equal(got["argmax"][p], ticks[np.argmax(key, axis=0)]), p
    for key in INT_KEYS + F64_KEYS + ("t_min", "t_max", "t_first_nonfinite"):
        assert got[key].shape == (3, 17) and np.array_equal(got[key], rows[key], equal_nan=True), key
    assert np.all(got["count"] == 12) and np.array_equal(got["t_min"], got["argmin"] * c.exec._dt)
    assert np.any(got["min_sq"] < got["max_sq"])
