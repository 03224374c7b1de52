"""Ring extremes (sixdof_history_extremes): per row and component element, over the sampled ticks of a range, the count of finite
samples, the smallest and largest finite value with the EARLIEST sampled tick that holds each, and the earliest sampled tick at
which the element is not finite — reduced on the device out of the telemetry ring.

The reference is always numpy over the [ticks, n, w] blocks HipExec.history reads from the same ring.  It forms the integer keys
on the host — the bit pattern viewed as unsigned, the order-preserving transform of csrc/quantile_plan.hpp, non-finite elements
masked — and takes argmin / argmax on the keys, which return the first occurrence.  Nothing is rounded anywhere, so every
comparison is np.array_equal on all six fields (and on the sign of a zero)."""
import ctypes as C
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

import elodin_amd as ea
from elodin_amd import _lib as L
from elodin_amd import dsl, workloads
from tests.test_gpu_history_watch import _exec

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FIELDS = ("world_pos", "world_vel", "world_accel", "force")
KEYS = ("count", "min", "argmin", "max", "argmax", "first_nonfinite")
U64P = C.POINTER(C.c_uint64)
WIDTH = lambda c: 7 if c == "world_pos" else 6


def _reference(blocks, ticks):
    """The six fields as [n, w] out of [s, n, w] blocks sampled at `ticks`."""
    ticks = np.asarray(ticks, dtype=np.int64)
    if blocks.dtype == np.float32:
        u = blocks.view(np.uint32).astype(np.uint64)
        negative, finite = (u >> np.uint64(31)) != 0, (u & np.uint64(0x7f800000)) != np.uint64(0x7f800000)
        key = np.where(negative, ~u & np.uint64(0xffffffff), u | np.uint64(1 << 31))
    else:
        u = np.ascontiguousarray(blocks).view(np.uint64)
        negative, finite = (u >> np.uint64(63)) != 0, (u & np.uint64(0x7ff0000000000000)) != np.uint64(0x7ff0000000000000)
        key = np.where(negative, ~u, u | np.uint64(1 << 63))
    count = finite.sum(axis=0).astype(np.int64)
    first_min = np.where(finite, key, np.uint64(0xffffffffffffffff)).argmin(axis=0)
    first_max = np.where(finite, key, np.uint64(0)).argmax(axis=0)
    x = blocks.astype(np.float64)
    some = count > 0
    pick = lambda at: np.where(some, np.take_along_axis(x, at[None], axis=0)[0], np.nan)
    return {"count": count, "min": pick(first_min), "argmin": np.where(some, ticks[first_min], 0), "max": pick(first_max),
            "argmax": np.where(some, ticks[first_max], 0), "first_nonfinite": np.where((~finite).any(axis=0), ticks[(~finite).argmax(axis=0)], 0)}


def _same_fields(got, want, what):
    assert sorted(got) == sorted(KEYS), what
    for k in KEYS:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape)
        assert got[k].dtype == (np.float64 if k in ("min", "max") else np.int64), (what, k)
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)
    for k in ("min", "max"):
        assert np.array_equal(np.signbit(got[k]), np.signbit(want[k])), (what, k, "the sign of a zero")


def _check_all(hip, names, got, first, last, every, what=""):
    assert sorted(got) == sorted(set(names))
    ticks = np.arange(first, last + 1, every)
    for name in names:
        _same_fields(got[name], _reference(hip.history(name, first, last)[::every], ticks), f"{what} {name}")


def _same(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        _same_fields(a[name], b[name], name)


def _buffers(hip, names, fill=123.0):
    return [np.full((L.EXTREMES_PLANES, hip.n, hip._recorded_width(c)), fill) for c in names]


def _raw(hip, names, first, n_samples, every, bufs, flags=0):
    comp = np.array([L.component_id(n) for n in names], dtype=np.uint64)
    ptrs = None if bufs is None else (C.c_void_p * max(1, len(bufs)))(*[b.ctypes.data for b in bufs])
    return hip._lib.sixdof_history_extremes(hip._h, comp.ctypes.data_as(U64P), len(names), first, n_samples, every, ptrs, flags)


# ---- 1. values, range shapes, dtypes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,ring,run,first,every,dtype", [
    (300, 8, 10, 27, 18, 3, np.float64),       # ticks 18 .. 27 sit in slots 7 8 9 0 .. 6: the range wraps the ring
    (4099, 7, 64, 50, 1, 7, np.float64),       # a ragged last block
    (64, 1, 8, 8, 1, 1, np.float32),
    (1, 1, 4, 4, 4, 1, np.float64),            # one sample each: one row, one short of a wavefront, one past it
    (63, 4, 4, 4, 4, 1, np.float64),
    (65, 4, 4, 4, 4, 1, np.float64),
    (300, 1, 16, 16, 4, 1, np.float64),        # 13 samples: no multiple of the load depth nor of a segment count
])
def test_extremes_equal_numpy_over_the_history_blocks(n, k, ring, run, first, every, dtype):
    hip, _ = _exec(n, k, dtype)
    hip.enable_history(ring)
    hip.run(run)
    last = first + (run - first) // every * every
    got = hip.history_extremes(FIELDS, first, run, every)             # the four columns in one call
    assert [got[c]["min"].shape for c in FIELDS] == [(n, 7)] + [(n, 6)] * 3
    _check_all(hip, FIELDS, got, first, last, every, what=f"n {n} {np.dtype(dtype).name}")
    samples = (last - first) // every + 1
    assert np.all(got["world_pos"]["count"] == samples) and np.all(got["world_pos"]["first_nonfinite"] == 0)
    if samples > 1:                                                    # the ticks differ: the extremes are not all at one tick
        assert len(np.unique(got["world_vel"]["argmin"])) > 1 or len(np.unique(got["world_vel"]["argmax"])) > 1
    one = hip.history_extremes("world_vel", run, run)                 # one name, one sample
    assert sorted(one) == ["world_vel"] and np.all(one["world_vel"]["argmax"] == run)
    _check_all(hip, ["world_vel"], one, run, run, 1, what=f"n {n} single sample")
    hip.close()


# ---- 2. ties and zeros ---------------------------------------------------------------------------------------------------
def test_ties_report_the_first_sampled_tick_and_zeros_keep_their_sign():
    """Uniform gravity on bodies thrown upwards that do not spin: the vertical world_accel and force hold one value at every tick,
    the vertical velocity crosses zero, and the angular elements are zeros of either sign (whatever signs the data has, the
    reference has them too)."""
    n = 130
    w = workloads.independent_bodies(n)
    vel = np.zeros((n, 6))
    vel[:, 5] = np.linspace(1.0, 4.0, n)                   # upwards: crosses zero 12 .. 49 ticks of 1 / 120 s later
    vel[::2, 0] = -0.0
    hip = ea.HipExec(w["world_pos"], vel, w["inertia"], entity_ids=w["entity_ids"], simulation_time_step=workloads.DT_120HZ,
                     effectors=[ea.Effector(L.EFF_UNIFORM_GRAVITY, (0.0, 0.0, -9.81))], ticks_per_launch=4)
    hip.enable_history(64)
    hip.run(60)
    got = hip.history_extremes(FIELDS, 5, 60, 5)
    _check_all(hip, FIELDS, got, 5, 60, 5, what="ties")
    for c in ("world_accel", "force"):
        assert np.all(got[c]["argmin"][:, 5] == 5) and np.all(got[c]["argmax"][:, 5] == 5), c      # one value at every tick: the first sample
        assert np.array_equal(got[c]["min"][:, 5], got[c]["max"][:, 5]) and np.all(got[c]["min"][:, 5] < 0.0), c
    wx = got["world_vel"]
    assert np.all(wx["min"][:, :3] == 0.0) and np.all(wx["max"][:, :3] == 0.0)         # zeros of either sign
    assert np.all(wx["max"][:, 5] > 0) and np.all(wx["min"][:, 5] < 0)                 # the vertical velocity crossed zero
    assert np.all(wx["argmax"][:, 5] == 5) and np.all(wx["argmin"][:, 5] == 60)
    hip.close()


# ---- 3. non-finite elements ------------------------------------------------------------------------------------------------
def test_non_finite_elements_are_counted_out_and_dated():
    n = 300
    hip, _ = _exec(n, 8)
    hip.world_vel[[0, 63, 64, 299]] = np.nan
    hip.world_vel[150, 4] = np.inf
    hip.upload()
    hip.enable_history(8)
    hip.run(8)
    got = hip.history_extremes(FIELDS, 2, 8, 2)
    _check_all(hip, FIELDS, got, 2, 8, 2, what="diverged rows")
    v = got["world_vel"]
    rows = [0, 63, 64, 299]
    assert np.all(v["count"][rows] == 0) and np.all(v["first_nonfinite"][rows] == 2)            # from the first sampled tick on
    assert np.all(np.isnan(v["min"][rows])) and np.all(np.isnan(v["max"][rows]))
    assert np.all(v["argmin"][rows] == 0) and np.all(v["argmax"][rows] == 0)
    assert v["count"][150, 4] == 0 and v["first_nonfinite"][150, 4] == 2 and v["count"][150, 3] == 4
    assert np.all(v["count"][1:63] == 4) and np.all(v["first_nonfinite"][1:63] == 0)
    assert np.all(got["world_pos"]["first_nonfinite"][rows, 4:] > 0)                            # the NaN reaches the position
    hip.close()


def _program_exec(n=200, a_nan=False):
    """The f32 program of tests/test_gpu_history_envelope.py::_program_exec."""
    np_ = dsl.np

    @dsl.system(a=1, b=2, c=3, buf=dsl.window(4, 2))
    def plant(a, b, c, buf):
        s = a * 0.5 + b[1]
        return {"a": s * 0.25 + 1.0,
                "b": np_.array([b[1] * 0.99 + c[2] * 1e-3, b[0] + 0.125]),
                "c": np_.array([c[1], c[2] * 0.999, c[0] + a * 1e-3]),
                "buf": buf.push(b)}
    rng = np.random.default_rng(3)
    w = workloads.independent_bodies(n)
    a0 = np.full((n, 1), np.nan) if a_nan else rng.uniform(-1, 1, (n, 1))
    hip = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], entity_ids=w["entity_ids"], dtype=np.float32, integrator=L.SEMI_IMPLICIT,
                     effectors=dsl.Program([plant], dsl.Pipe([]), []), ticks_per_launch=12,
                     columns={"a": a0, "b": rng.uniform(-1, 1, (n, 2)), "c": rng.uniform(-1, 1, (n, 3)), "buf": np.zeros((n, 4, 2))})
    return hip


def test_a_nan_that_spreads_through_a_program_is_dated_per_element():
    hip = _program_exec(a_nan=True)
    hip.enable_history(16)
    hip.run(12)
    names = ["a", "b", "c", "world_pos"]
    got = hip.history_extremes(names, 1, 6)
    _check_all(hip, names, got, 1, 6, 1, what="NaN column")
    # a is NaN from the start; it reaches c[2] in tick 1, b[0] and c[1] in tick 2, c[0] and b[1] in tick 3
    assert np.all(got["a"]["count"] == 0) and np.all(got["a"]["first_nonfinite"] == 1) and np.all(np.isnan(got["a"]["min"]))
    assert np.all(got["c"]["first_nonfinite"] == [3, 2, 1]) and np.all(got["c"]["count"] == [2, 1, 0])
    assert np.all(got["b"]["first_nonfinite"] == [2, 3]) and np.all(got["b"]["count"] == [1, 2])
    assert np.all(got["world_pos"]["first_nonfinite"] == 0)
    whole = _program_exec()
    whole.enable_history(16)
    whole.run(12)
    _check_all(whole, ["c", "a", "world_vel", "b"], whole.history_extremes(["c", "a", "world_vel", "b"], 2, 12, 5), 2, 12, 5, what="program columns")
    with pytest.raises(ValueError, match="window component"):
        whole.history_extremes(["buf"], 2, 12)
    for h in (hip, whole):
        h.close()


# ---- 4. cut-independence -----------------------------------------------------------------------------------------------
def test_one_call_equals_the_range_in_three_calls_and_under_forced_segments(monkeypatch):
    n = 300
    hip, _ = _exec(n, 8)
    hip.world_vel[[7, 200]] = np.nan
    hip.upload()
    hip.enable_history(10)
    hip.run(27)                                               # ticks 18 .. 27 sit in slots 7 8 9 0 .. 6
    whole = hip.history_extremes(FIELDS, 18, 27)
    _check_all(hip, FIELDS, whole, 18, 27, 1, what="one call")
    # 18 .. 20 | 21 .. 24 | 25 .. 27: the first cut falls at the ring's wrap
    bufs = _buffers(hip, FIELDS)
    assert _raw(hip, FIELDS, 18, 3, 1, None, L.EXTREMES_HOLD) == L.OK
    assert _raw(hip, FIELDS, 21, 4, 1, bufs, L.EXTREMES_HOLD | L.EXTREMES_CONTINUE) == L.OK
    assert all(np.all(b == 123.0) for b in bufs)                                            # held: nothing is delivered
    assert _raw(hip, FIELDS, 25, 3, 1, bufs, L.EXTREMES_CONTINUE) == L.OK
    _same(hip._extremes_dict(FIELDS, bufs), whole)
    for segments in ("1", "2", "3", "10", "0"):
        monkeypatch.setenv("SIXDOF_EXTREMES_SEGMENTS", segments)
        _same(hip.history_extremes(FIELDS, 18, 27), whole)
        bufs = _buffers(hip, FIELDS)                                                        # segments and calls together
        assert _raw(hip, FIELDS, 18, 5, 1, None, L.EXTREMES_HOLD) == L.OK and _raw(hip, FIELDS, 23, 5, 1, bufs, L.EXTREMES_CONTINUE) == L.OK
        _same(hip._extremes_dict(FIELDS, bufs), whole)
    monkeypatch.delenv("SIXDOF_EXTREMES_SEGMENTS")
    other = hip.history_extremes(FIELDS[::-1], 18, 27)                                      # another order of the component list
    _same({c: other[c] for c in FIELDS}, whole)
    _same(hip.history_extremes(["force"], 18, 27), {"force": whole["force"]})
    # a campaign-sized read in which the plan cuts the samples itself: 64 samples of 40 rows
    small, _ = _exec(40, 8)
    small.enable_history(64)
    small.run(64)
    _check_all(small, FIELDS, small.history_extremes(FIELDS, 1, 64), 1, 64, 1, what="the plan's own segments")
    for h in (hip, small):
        h.close()


# ---- 5. streaming ---------------------------------------------------------------------------------------------------------
def test_streamed_extremes_over_a_ring_one_batch_deep_equal_one_read_of_a_whole_ring():
    n = 300
    a, _ = _exec(n, 8)
    b, _ = _exec(n, 8)
    for h in (a, b):
        h.world_vel[[5, 77]] = np.nan
        h.upload()
    with pytest.raises(ValueError):
        a.stream_extremes(FIELDS, 6, 8, every=3)
    wall, got = a.stream_extremes(FIELDS, 6, 8, every=2)
    assert wall > 0.0 and a.tick == 48 and a._ring_ticks == 8
    b.enable_history(48)
    b.run(48)
    want = b.history_extremes(FIELDS, 2, 48, 2)
    _check_all(b, FIELDS, want, 2, 48, 2, what="the twin")
    _same(got, want)
    assert np.all(got["world_pos"]["count"][0] == 24) and got["world_vel"]["argmax"].max() > 8       # beyond the first batch
    a.run(2)                                                 # the caller's flags are back: a blocking step, and the state a plain run leaves
    b.run(2)
    assert a.tick == 50
    for c in FIELDS:
        assert np.array_equal(getattr(a, c), getattr(b, c), equal_nan=True), c
    for h in (a, b):
        h.close()


# ---- 6. asynchronous delivery ------------------------------------------------------------------------------------------
def test_async_read_equals_the_blocking_read_though_the_slots_are_overwritten_at_once():
    n = 500
    hip, _ = _exec(n, 8)
    hip.enable_history(8)
    hip.run(8)
    want = hip.history_extremes(FIELDS, 1, 8)
    bufs = _buffers(hip, FIELDS)
    assert _raw(hip, FIELDS, 1, 8, 1, bufs, L.EXTREMES_ASYNC) == L.OK
    hip.invoke_batch(8)                                      # overwrites every slot the read took its samples from
    hip.download_wait()
    _same(hip._extremes_dict(FIELDS, bufs), want)
    hip.sync()
    assert hip.tick == 16
    _check_all(hip, FIELDS, hip.history_extremes(FIELDS, 9, 16), 9, 16, 1, what="after the overwrite")
    hip.close()


# ---- 7. more components than one launch covers -----------------------------------------------------------------------------
def test_33_component_entries_in_one_call():
    hip, _ = _exec(65, 4)
    hip.enable_history(8)
    hip.run(8)
    names = [FIELDS[k % 4] for k in range(33)]
    many, four = _buffers(hip, names, -7.0), _buffers(hip, FIELDS, -9.0)
    assert _raw(hip, names, 2, 3, 1, None, L.EXTREMES_HOLD) == L.OK and _raw(hip, names, 5, 4, 1, many, L.EXTREMES_CONTINUE) == L.OK
    assert _raw(hip, FIELDS, 2, 7, 1, four) == L.OK
    assert all(np.all(b[0] == 7) for b in four)              # filled: seven samples
    for k, b in enumerate(many):
        assert b.tobytes() == four[k % 4].tobytes(), (k, names[k])
    hip.close()


# ---- 8. refusals copy nothing -------------------------------------------------------------------------------------------
def test_refused_reads_copy_nothing_and_leave_the_accumulator():
    hip, _ = _exec(300, 8)
    buf = _buffers(hip, ["world_vel"])
    sentinel = buf[0].copy()
    raw_read = lambda first, n_samples, every, flags=0, names=("world_vel",), bufs=buf: _raw(hip, list(names), first, n_samples, every, bufs, flags)
    assert raw_read(1, 1, 1) == L.ERR_INVALID_ARGUMENT                         # no ring
    hip.run(5)
    hip.enable_history(10)                                                       # recording starts at tick 6
    hip.run(25)                                                                  # the ring keeps 21 .. 30
    assert raw_read(21, 4, 1, L.EXTREMES_CONTINUE) == L.ERR_INVALID_ARGUMENT    # nothing to continue
    want = hip.history_extremes(["world_vel"], 21, 30)
    assert raw_read(21, 4, 1, L.EXTREMES_HOLD, bufs=None) == L.OK              # the accumulator the refusals must leave alone
    assert raw_read(25, 4, 0) == L.ERR_INVALID_ARGUMENT                         # every = 0
    assert raw_read(20, 4, 1) == L.ERR_INVALID_ARGUMENT                         # has fallen out of the ring
    assert raw_read(28, 4, 1) == L.ERR_INVALID_ARGUMENT                         # runs beyond `tick`
    assert raw_read(24, 4, 3) == L.ERR_INVALID_ARGUMENT                         # its last sample does
    assert raw_read(31, 1, 1) == L.ERR_INVALID_ARGUMENT
    assert raw_read(25, 4, 1, 8) == L.ERR_INVALID_ARGUMENT                      # unknown flags
    assert raw_read(25, 4, 1, bufs=None) == L.ERR_INVALID_ARGUMENT              # a null buffer list without HOLD
    null = (C.c_void_p * 1)(None)
    comp = np.array([L.component_id("world_vel")], dtype=np.uint64)
    assert hip._lib.sixdof_history_extremes(hip._h, comp.ctypes.data_as(U64P), 1, 25, 4, 1, null, 0) == L.ERR_INVALID_ARGUMENT     # a null buffer
    assert hip._lib.sixdof_history_extremes(hip._h, None, 1, 25, 4, 1, null, L.EXTREMES_HOLD) == L.ERR_INVALID_ARGUMENT           # null component ids
    assert raw_read(25, 4, 1, names=("inertia",)) == L.ERR_COMPONENT_NOT_FOUND
    assert raw_read(25, 6, 1, L.EXTREMES_CONTINUE, names=("force",)) == L.ERR_INVALID_ARGUMENT          # another component list
    assert raw_read(24, 7, 1, L.EXTREMES_CONTINUE) == L.ERR_INVALID_ARGUMENT                            # tick 24 is accumulated already
    assert b"24" in hip._lib.sixdof_last_error(hip._h)
    assert raw_read(21, 0, 1) == L.OK and raw_read(99, 0, 7, L.EXTREMES_CONTINUE) == L.OK              # no samples: a no-op
    assert np.array_equal(buf[0], sentinel)                                     # nothing was copied
    assert raw_read(25, 6, 1, L.EXTREMES_CONTINUE) == L.OK                     # the accumulator is what the held call left
    _same(hip._extremes_dict(["world_vel"], buf), want)
    for bad in ((20, 30, 1), (21, 31, 1), (21, 30, 0)):
        with pytest.raises(ValueError):
            hip.history_extremes(["world_vel"], *bad)
    with pytest.raises(KeyError):
        hip.history_extremes(["world_pos", "inertia"], 21, 30)
    empty = hip.history_extremes(["world_vel"], 30, 29)["world_vel"]            # no samples: count 0, NaN, no ticks
    assert np.all(empty["count"] == 0) and np.all(np.isnan(empty["min"])) and np.all(empty["argmax"] == 0) and empty["max"].shape == (300, 6)
    hip.enable_history(10)                                                       # a ring that starts over: the accumulator went with the old one
    hip.run(3)                                                                   # 31 .. 33
    buf[0][...] = 123.0
    assert raw_read(31, 3, 1, L.EXTREMES_CONTINUE) == L.ERR_INVALID_ARGUMENT
    assert raw_read(30, 4, 1) == L.ERR_INVALID_ARGUMENT                         # starts before the ring's first tick
    assert np.array_equal(buf[0], sentinel)
    _check_all(hip, ["world_vel"], hip.history_extremes(["world_vel"], 31, 33), 31, 33, 1, what="the new ring")
    hip.enable_history(0)
    with pytest.raises(ValueError, match="no history ring"):
        hip.history_extremes(["world_vel"], 31, 33)
    hip.close()


# ---- 9. front end ---------------------------------------------------------------------------------------------------------
def test_front_end_extremes_of_one_entity_are_the_extremes_of_its_series():
    spec = importlib.util.spec_from_file_location("ball", ROOT / "examples" / "ball.py")
    ball = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ball)
    six = ball.el.six_dof(sys=ball.gravity | ball.apply_drag)      # the same stage three times: three executor ticks per world tick
    ex = ball.world(0).build(ball.sample_wind | ball.bounce | six | six | six, simulation_rate=120.0, telemetry_rate=40.0, history=True)
    assert ex._substeps == 3
    ex.enable_history(64)
    ex.run(30)
    comps = ["world_pos", "world_vel", "wind", "force"]
    series = ex.history_series(["ball." + c for c in comps], 3, 30, every=3)
    got = ex.history_extremes(comps, 3, 30, every=3)
    ticks = np.arange(3, 31, 3)
    assert sorted(got) == sorted(comps)
    for c in comps:
        x = series["ball." + c].reshape(10, -1)
        d = got[c]
        assert d["min"].shape == (1, x.shape[1]) and np.all(d["count"] == 10) and np.all(d["first_nonfinite"] == 0), c
        assert np.array_equal(d["min"][0], x.min(axis=0)) and np.array_equal(d["max"][0], x.max(axis=0)), c
        assert np.array_equal(d["argmin"][0], ticks[x.argmin(axis=0)]) and np.array_equal(d["argmax"][0], ticks[x.argmax(axis=0)]), c       # world ticks
        assert np.array_equal(d["t_min"][0], series["time"][x.argmin(axis=0)]) and np.array_equal(d["t_max"][0], d["argmax"][0] * ex._dt), c
        assert np.all(np.isnan(d["t_first_nonfinite"])), c
    assert len(np.unique(got["world_pos"]["argmin"])) > 1 or len(np.unique(got["world_pos"]["argmax"])) > 1
    with pytest.raises(KeyError):
        ex.history_extremes("nothing", 3, 30)
    with pytest.raises(ValueError):
        ex.history_extremes("world_pos", 0, 30)              # tick 0 is not in the ring
    with pytest.raises(ValueError):
        ex.history_extremes("world_pos", 3, 30, every=0)


def test_campaign_extremes_equal_numpy_over_the_runs_columns():
    """A 17-run campaign of the Monte-Carlo example: Campaign.extremes against numpy over Campaign.column after each tick."""
    from tests.test_gpu_monte_carlo_example import GOLDEN, example
    from elodin_amd import vectorize
    ex = example(0)
    doc = json.loads((GOLDEN / "monte_carlo_example.json").read_text())
    params = [r["params"] for r in doc["runs"] if r["probe_rows"] == 0]
    c = vectorize.Campaign(ex.build, vectorize.plan_of((params * 17)[:17]), ex.PARAMS, simulation_rate=ex.SIMULATION_RATE_HZ)
    assert c.n_runs == 17 and c.entities_per_run == 1
    comps = ["position", "velocity", "specific_force"]
    c.exec.enable_history(16)
    cols = {name: [] for name in comps}
    for _ in range(12):
        c.exec.run(1)
        for name in comps:
            cols[name].append(np.array(c.column(name), dtype=np.float64).reshape(17, -1))
    got = c.extremes(comps, 2, 12, every=5)                  # ticks 2, 7, 12
    ticks = np.array([2, 7, 12])
    rows = c.exec.history_extremes(comps, 2, 12, every=5)
    for name in comps:
        ref = _reference(np.stack([cols[name][t - 1] for t in ticks]), ticks)
        w = ref["min"].shape[1]
        for k in KEYS:
            assert got[name][k].shape == (17, 1, w), (name, k)
            assert np.array_equal(got[name][k][:, 0], ref[k], equal_nan=True), (name, k)
            assert np.array_equal(got[name][k][:, 0], rows[name][k], equal_nan=True), (name, k)
        assert np.allclose(got[name]["t_min"], got[name]["argmin"] / ex.SIMULATION_RATE_HZ) and got[name]["t_max"].shape == (17, 1, w)
    assert len(np.unique(got["position"]["max"])) > 1        # the runs differ
