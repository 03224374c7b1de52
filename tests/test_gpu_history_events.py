"""Ring events (sixdof_history_events): per event and run, over the sampled ticks of a range, the first tick at which one element
of one recorded component meets a threshold — as a level or as a crossing — the element's value there, tick and value of the
finite sample before, and the rows of other components at that tick, found and captured on the device out of the telemetry ring.

The reference is always numpy over the [ticks, n, w] blocks HipExec.history reads from the same ring: a loop over the samples,
vectorised over the runs, that says the issue's words — a non-finite sample is skipped as if it had not been sampled, LEVEL fires
at the earliest finite sample that holds, CROSSING at the earliest that holds after a finite sample that did not.  Nothing is
rounded anywhere, so every comparison is np.array_equal (NaN equal to NaN) and no tolerance appears."""
import ctypes as C
import importlib.util
import json
import operator
from pathlib import Path

import numpy as np
import pytest

import elodin_amd as ea
from elodin_amd import _lib as L
from elodin_amd import workloads

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
OPS = {"<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}
KEYS = ("tick", "value", "tick_before", "value_before")
Z0 = 5.0


def _reference_one(x, ticks, ev):
    """tick, value, tick_before, value_before as [runs] out of the event element's samples x [s, runs]."""
    runs = x.shape[1]
    x = x.astype(np.float64)
    tick, before = np.zeros(runs, dtype=np.int64), np.zeros(runs, dtype=np.int64)
    value, value_before = np.full(runs, np.nan), np.full(runs, np.nan)
    seen, prev_holds = np.zeros(runs, dtype=bool), np.zeros(runs, dtype=bool)
    prev_tick, prev = np.zeros(runs, dtype=np.int64), np.full(runs, np.nan)
    for j, t in enumerate(ticks):
        live = np.isfinite(x[j]) & (tick == 0)
        with np.errstate(invalid="ignore"):
            holds = OPS[ev.op](x[j], ev.level)
        fires = live & holds & ((seen & ~prev_holds) if ev.mode == "crossing" else True)
        tick[fires], value[fires] = t, x[j][fires]
        with_before = fires & seen
        before[with_before], value_before[with_before] = prev_tick[with_before], prev[with_before]
        rest = live & ~fires
        seen[rest], prev_holds[rest], prev_tick[rest], prev[rest] = True, holds[rest], t, x[j][rest]
    return {"tick": tick, "value": value, "tick_before": before, "value_before": value_before}


def _reference(hip, events, capture, first, last, every, period=1):
    """The dict of HipExec.history_events out of HipExec.history."""
    ticks = np.arange(first, last + 1, every)
    blocks = {name: hip.history(name, first, last)[::every] for name in {e.component for e in events} | set(capture)}
    per_event = [_reference_one(blocks[e.component][:, e.group::period, e.element], ticks, e) for e in events]
    out = {k: np.stack([d[k] for d in per_event]) for k in KEYS}
    out["capture"] = {}
    for name in capture:
        b = blocks[name].astype(np.float64)
        cap = np.full((len(events),) + b.shape[1:], np.nan)
        for e, d in enumerate(per_event):
            at = np.repeat(d["tick"], period)                       # the event tick of every row's run
            rows = np.nonzero(at)[0]
            cap[e, rows] = b[(at[rows] - first) // every, rows]
        out["capture"][name] = cap
    return out


def _same(got, want, what=""):
    assert sorted(got) == sorted(KEYS + ("capture",)), what
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, got[k].dtype)
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)
    for k in ("value", "value_before"):
        assert np.array_equal(np.signbit(got[k]), np.signbit(want[k])), (what, k, "the sign of a zero")
    assert list(got["capture"]) == list(want["capture"]), what
    for name in want["capture"]:
        a, b = got["capture"][name], want["capture"][name]
        assert a.shape == b.shape and a.dtype == np.float64 and np.array_equal(a, b, equal_nan=True), (what, name)


def _thrown(n, dtype=np.float64, ring=64, nan_rows=()):
    """test_gpu_history_extremes.py test 2's set-up: bodies thrown upwards from height Z0 under uniform gravity, without spin."""
    w = workloads.independent_bodies(n)
    pos = np.array(w["world_pos"], dtype=dtype)
    pos[:, 6] = Z0
    vel = np.zeros((n, 6), dtype=dtype)
    vel[:, 5] = np.linspace(1.0, 4.0, n)                   # upwards: apogee 12 .. 49 ticks of 1 / 120 s later, back at Z0 after twice that
    vel[list(nan_rows)] = np.nan
    hip = ea.HipExec(pos, vel, np.array(w["inertia"], dtype=dtype), entity_ids=w["entity_ids"], simulation_time_step=workloads.DT_120HZ,
                     effectors=[ea.Effector(L.EFF_UNIFORM_GRAVITY, (0.0, 0.0, -9.81))], ticks_per_launch=4, dtype=dtype)
    hip.enable_history(ring)
    return hip


APOGEE = ea.Event("world_vel", 5, "<=", 0.0)
FALL_BACK = ea.Event("world_pos", 6, "<=", Z0)
RISING_LEVEL = ea.Event("world_vel", 5, ">", 0.0, mode="level")
RISING_CROSSING = ea.Event("world_vel", 5, ">", 0.0, mode="crossing")
EVENTS = [APOGEE, FALL_BACK, RISING_LEVEL, RISING_CROSSING]
CAPTURE = ["world_pos", "world_vel"]


def _triggers(events):
    return ea.HipExec._event_triggers(events)


def _buffers(hip, n_events, capture, period=1, fill=123.0):
    return np.full((n_events, L.EVENTS_PLANES, hip.n // period), fill), [np.full((n_events, hip.n, hip._recorded_width(c)), fill) for c in capture]


def _raw(hip, events, capture, period, first, n_samples, every, bufs, flags=0):
    trig = _triggers(events)
    comp = np.array([L.component_id(c) for c in capture], dtype=np.uint64)
    ev, caps = bufs if bufs is not None else (None, None)
    ptrs = None if caps is None else (C.c_void_p * max(1, len(caps)))(*[b.ctypes.data for b in caps])
    return hip._lib.sixdof_history_events(hip._h, trig, len(trig), comp.ctypes.data_as(C.POINTER(C.c_uint64)), len(capture), period, first, n_samples, every,
                                          None if ev is None else ev.ctypes.data, ptrs, flags)


# ---- 1. values and shapes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dtype", [(1, np.float64), (63, np.float64), (65, np.float64), (130, np.float64), (300, np.float64), (64, np.float32)])
def test_events_equal_numpy_over_the_history_blocks(n, dtype):
    hip = _thrown(n, dtype)
    hip.run(60)
    got = hip.history_events(EVENTS, CAPTURE, 1, 60)
    assert got["tick"].shape == (4, n) and got["tick"].dtype == np.int64 and got["value"].dtype == np.float64
    assert got["capture"]["world_pos"].shape == (4, n, 7) and got["capture"]["world_vel"].shape == (4, n, 6)
    _same(got, _reference(hip, EVENTS, CAPTURE, 1, 60, 1), f"n {n} {np.dtype(dtype).name}")
    apogee, fall_back, level, crossing = range(4)
    assert np.all(got["tick"][apogee] > 1) and np.all(got["tick_before"][apogee] == got["tick"][apogee] - 1)
    assert np.all(got["value"][apogee] <= 0.0) and np.all(got["value_before"][apogee] > 0.0)
    assert np.any(got["tick"][fall_back] > 0) and np.all(got["tick"][fall_back][got["tick"][fall_back] > 0] > got["tick"][apogee][got["tick"][fall_back] > 0])
    if n > 1:
        assert len(np.unique(got["tick"][apogee])) > 1                       # the event ticks differ between rows
        assert np.any(got["tick"][fall_back] == 0)                           # the fastest are not back within 60 ticks
    vel = hip.history("world_vel", 1, 60).astype(np.float64)
    for r in range(n):                                                       # every row's capture is the history row at ITS OWN tick
        assert np.array_equal(got["capture"]["world_vel"][apogee, r], vel[got["tick"][apogee, r] - 1, r]), r
    # holding from the first sample on: LEVEL fires there with nothing before it, CROSSING never fires
    assert np.all(got["tick"][level] == 1) and np.all(got["tick_before"][level] == 0) and np.all(np.isnan(got["value_before"][level]))
    assert np.array_equal(got["capture"]["world_vel"][level], vel[0])
    assert np.all(got["tick"][crossing] == 0) and np.all(np.isnan(got["value"][crossing]))
    assert np.all(np.isnan(got["capture"]["world_pos"][crossing])) and np.all(np.isnan(got["capture"]["world_vel"][crossing]))
    one = hip.history_events(APOGEE, [], 1, 60)                              # one event, no capture
    assert one["capture"] == {} and np.array_equal(one["tick"], got["tick"][:1]) and np.array_equal(one["value"], got["value"][:1])
    hip.close()


# ---- 2. ring wrap and every ----------------------------------------------------------------------------------------------
def test_a_range_that_wraps_the_ring_and_takes_every_third_tick():
    hip = _thrown(300, ring=10)
    hip.run(27)                                                # ticks 18 .. 27 sit in slots 7 8 9 0 .. 6
    got = hip.history_events(EVENTS, CAPTURE, 18, 27, every=3)
    _same(got, _reference(hip, EVENTS, CAPTURE, 18, 27, 3), "wrap")
    fired = got["tick"][0] > 0
    assert np.any(fired) and np.any(~fired)                    # past their apogee at tick 18, or not there by tick 27: no crossing in range
    assert set(np.unique(got["tick"][0][fired])) <= {21, 24, 27} and len(np.unique(got["tick"][0][fired])) > 1
    assert np.all(got["tick_before"][0][fired] == got["tick"][0][fired] - 3)
    rising = hip.history("world_vel", 18, 18)[0, :, 5] > 0.0    # still rising at the first sample: the LEVEL event is there; the others
    assert np.array_equal(got["tick"][2], np.where(rising, 18, 0)) and np.any(rising) and np.any(~rising)      # only fall from here on
    hip.close()


# ---- 3. runs of several rows -----------------------------------------------------------------------------------------------
def test_runs_of_four_rows_are_captured_at_the_tick_of_their_watched_row():
    n, period = 260, 4                                         # 65 runs: one past a wavefront
    hip = _thrown(n)
    hip.run(60)
    events = [ea.Event("world_vel", 5, "<=", 0.0, group=3), ea.Event("world_pos", 6, "<=", Z0, group=0), ea.Event("world_vel", 5, ">", 0.0, mode="level", group=2)]
    got = hip.history_events(events, CAPTURE, 1, 60, period=period)
    assert got["tick"].shape == (3, 65) and got["capture"]["world_pos"].shape == (3, n, 7)
    _same(got, _reference(hip, events, CAPTURE, 1, 60, 1, period), "period 4")
    vel = hip.history("world_vel", 1, 60)
    for run in (0, 31, 64):                                    # all four rows of a run, at the tick of row 3
        t = got["tick"][0, run]
        assert t > 0 and np.array_equal(got["capture"]["world_vel"][0, 4 * run: 4 * run + 4], vel[t - 1, 4 * run: 4 * run + 4])
        assert vel[t - 1, 4 * run + 3, 5] <= 0.0 < vel[t - 2, 4 * run + 3, 5]   # row 3 of the run is at its apogee
    assert len(np.unique(got["tick"][0])) > 1
    with pytest.raises(ValueError, match="period"):
        hip.history_events(events, CAPTURE, 1, 60, period=7)
    with pytest.raises(ValueError, match="group"):
        hip.history_events([ea.Event("world_vel", 5, "<=", 0.0, group=4)], CAPTURE, 1, 60, period=period)
    hip.close()


# ---- 4. non-finite rows --------------------------------------------------------------------------------------------------------
def test_rows_that_are_nan_never_fire_and_leave_the_others_alone():
    n, rows = 130, [0, 63, 64, 129]
    hip, clean = _thrown(n, nan_rows=rows), _thrown(n)
    for h in (hip, clean):
        h.run(60)
    got, want = hip.history_events(EVENTS, CAPTURE, 1, 60), clean.history_events(EVENTS, CAPTURE, 1, 60)
    _same(got, _reference(hip, EVENTS, CAPTURE, 1, 60, 1), "NaN rows")
    others = np.setdiff1d(np.arange(n), rows)
    for e in (0, 2, 3):                                        # the world_vel events: every sample of these rows is skipped
        assert np.all(got["tick"][e][rows] == 0) and np.all(np.isnan(got["value"][e][rows])) and np.all(got["tick_before"][e][rows] == 0)
        assert np.all(np.isnan(got["capture"]["world_pos"][e][rows])) and np.all(np.isnan(got["capture"]["world_vel"][e][rows]))
    for k in KEYS:
        assert np.array_equal(got[k][:, others], want[k][:, others], equal_nan=True), k
    for name in CAPTURE:
        assert np.array_equal(got["capture"][name][:, others], want["capture"][name][:, others], equal_nan=True), name
    for h in (hip, clean):
        h.close()


# ---- 5. cut-independence ---------------------------------------------------------------------------------------------------
def test_one_call_equals_three_continued_calls_and_forced_segments(monkeypatch):
    n = 300
    hip = _thrown(n)
    hip.run(60)
    whole = hip.history_events(EVENTS, CAPTURE, 1, 60)
    _same(whole, _reference(hip, EVENTS, CAPTURE, 1, 60, 1), "one call")
    # the second call starts ON row 0's apogee tick: its "before" sample is the last sample of the first call
    cut = int(whole["tick"][0, 0])
    assert 2 < cut <= 40 and whole["tick_before"][0, 0] == cut - 1
    cuts = [(1, cut - 1), (cut, 20), (cut + 20, 60 - cut - 19)]
    assert sum(c[1] for c in cuts) == 60

    def in_three_calls():
        bufs = _buffers(hip, 4, CAPTURE)
        assert _raw(hip, EVENTS, CAPTURE, 1, *cuts[0], 1, None, L.EVENTS_HOLD) == L.OK
        assert _raw(hip, EVENTS, CAPTURE, 1, *cuts[1], 1, bufs, L.EVENTS_HOLD | L.EVENTS_CONTINUE) == L.OK
        assert np.all(bufs[0] == 123.0) and all(np.all(b == 123.0) for b in bufs[1])           # held: nothing is delivered
        assert _raw(hip, EVENTS, CAPTURE, 1, *cuts[2], 1, bufs, L.EVENTS_CONTINUE) == L.OK
        return hip._events_dict(CAPTURE, *bufs)
    _same(in_three_calls(), whole, "three calls")
    for segments in ("1", "2", "3", "5", "0"):
        monkeypatch.setenv("SIXDOF_EVENTS_SEGMENTS", segments)
        _same(hip.history_events(EVENTS, CAPTURE, 1, 60), whole, f"{segments} segments")
        _same(in_three_calls(), whole, f"{segments} segments in three calls")                  # segments and calls together
    monkeypatch.delenv("SIXDOF_EVENTS_SEGMENTS")
    other = hip.history_events(EVENTS[::-1], CAPTURE[::-1], 1, 60)                             # another order of events and captures
    for k in KEYS:
        assert np.array_equal(other[k][::-1], whole[k], equal_nan=True), k
    assert np.array_equal(other["capture"]["world_vel"][::-1], whole["capture"]["world_vel"], equal_nan=True)
    # a campaign-sized read in which the plan cuts the samples itself: 64 samples of 40 runs
    small = _thrown(40)
    small.run(64)
    _same(small.history_events(EVENTS, CAPTURE, 1, 64), _reference(small, EVENTS, CAPTURE, 1, 64, 1), "the plan's own segments")
    for h in (hip, small):
        h.close()


# ---- 6. streaming ---------------------------------------------------------------------------------------------------------
def test_streamed_events_over_a_ring_one_batch_deep_equal_one_read_of_a_whole_ring():
    n = 300
    a, b = _thrown(n, ring=0, nan_rows=[5, 77]), _thrown(n, ring=48, nan_rows=[5, 77])
    with pytest.raises(ValueError):
        a.stream_events(EVENTS, CAPTURE, 6, 8, every=3)
    wall, got = a.stream_events(EVENTS, CAPTURE, 6, 8, every=2)
    assert wall > 0.0 and a.tick == 48 and a._ring_ticks == 8
    b.run(48)
    want = b.history_events(EVENTS, CAPTURE, 2, 48, every=2)
    _same(want, _reference(b, EVENTS, CAPTURE, 2, 48, 2), "the twin")
    _same(got, want, "streamed")
    assert got["tick"][0].max() > 8 and len(np.unique(got["tick"][0] // 8)) > 2       # events in several batches, beyond the first
    a.run(2)                                                 # the caller's flags are back: a blocking step, and the state a plain run leaves
    b.run(2)
    assert a.tick == 50
    for c in ("world_pos", "world_vel", "world_accel", "force"):
        assert np.array_equal(getattr(a, c), getattr(b, c), equal_nan=True), c
    for h in (a, b):
        h.close()


# ---- 7. asynchronous delivery ------------------------------------------------------------------------------------------
def test_async_read_equals_the_blocking_read_though_the_slots_are_overwritten_at_once():
    hip = _thrown(500, ring=32)
    hip.run(32)
    want = hip.history_events(EVENTS, CAPTURE, 1, 32)
    assert np.any(want["tick"][0] > 0)
    bufs = _buffers(hip, 4, CAPTURE)
    assert _raw(hip, EVENTS, CAPTURE, 1, 1, 32, 1, bufs, L.EVENTS_ASYNC) == L.OK
    hip.invoke_batch(32)                                     # overwrites every slot the read took its samples from
    hip.download_wait()
    _same(hip._events_dict(CAPTURE, *bufs), want, "async")
    hip.sync()
    assert hip.tick == 64
    _same(hip.history_events(EVENTS, CAPTURE, 33, 64), _reference(hip, EVENTS, CAPTURE, 33, 64, 1), "after the overwrite")
    hip.close()


# ---- 8. refusals copy nothing -------------------------------------------------------------------------------------------
def test_refused_reads_copy_nothing_and_leave_the_accumulator():
    hip = _thrown(300, ring=0)
    ev, cap = [APOGEE], ["world_vel"]
    bufs = _buffers(hip, 1, cap)
    untouched = lambda: np.all(bufs[0] == 123.0) and np.all(bufs[1][0] == 123.0)
    bad = L.ERR_INVALID_ARGUMENT
    raw = lambda first, n_samples, every, flags=0, events=ev, capture=cap, period=1, b=bufs: _raw(hip, events, capture, period, first, n_samples, every, b, flags)
    assert raw(1, 1, 1) == bad                                                   # no ring
    hip.run(5)
    hip.enable_history(30)                                                       # recording starts at tick 6
    hip.run(45)                                                                  # the ring keeps 21 .. 50
    assert raw(21, 4, 1, L.EVENTS_CONTINUE) == bad                               # nothing to continue
    want = hip.history_events(ev, cap, 21, 50)
    assert np.any(want["tick"] > 24)
    assert raw(21, 4, 1, L.EVENTS_HOLD, b=None) == L.OK                          # the accumulator the refusals must leave alone
    assert raw(25, 4, 0) == bad                                                  # every = 0
    assert raw(20, 4, 1) == bad                                                  # has fallen out of the ring
    assert raw(48, 4, 1) == bad                                                  # runs beyond `tick`
    assert raw(44, 4, 3) == bad                                                  # its last sample does
    assert raw(25, 4, 1, 8) == bad                                               # unknown flags
    assert raw(25, 4, 1, b=None) == bad                                          # null buffers without HOLD
    assert raw(25, 4, 1, b=(None, bufs[1])) == bad and raw(25, 4, 1, b=(bufs[0], None)) == bad
    assert raw(25, 4, 1, period=0) == bad and raw(25, 4, 1, period=7) == bad    # 300 rows are no multiple of 7
    assert raw(25, 4, 1, events=[ea.Event("world_vel", 5, "<=", 0.0, group=2)], period=2) == bad
    assert raw(25, 4, 1, events=[ea.Event("world_vel", 6, "<=", 0.0)]) == bad    # element = width
    assert b"width" in hip._lib.sixdof_last_error(hip._h)
    assert raw(25, 4, 1, events=[ea.Event("world_vel", 5, "<=", float("nan"))]) == bad and raw(25, 4, 1, events=[ea.Event("world_vel", 5, "<=", float("inf"))]) == bad
    nine, one = (L.EventTrigger * 9)(), _triggers(ev)
    comp = np.array([L.component_id("world_vel")], dtype=np.uint64)
    ptrs = (C.c_void_p * 1)(bufs[1][0].ctypes.data)
    call = lambda trig, n_trig: hip._lib.sixdof_history_events(hip._h, trig, n_trig, comp.ctypes.data_as(C.POINTER(C.c_uint64)), 1, 1, 25, 4, 1, bufs[0].ctypes.data, ptrs, 0)
    assert call(nine, 9) == bad and call(one, 0) == bad and call(None, 1) == bad
    one[0].op = 4
    assert call(one, 1) == bad
    one[0].op, one[0].mode = L.EVENT_LE, 2
    assert call(one, 1) == bad
    assert raw(25, 4, 1, events=[ea.Event("inertia", 0, "<=", 0.0)]) == L.ERR_COMPONENT_NOT_FOUND
    assert raw(25, 4, 1, capture=["inertia"], b=(bufs[0], [np.full((1, 300, 7), 123.0)])) == L.ERR_COMPONENT_NOT_FOUND
    assert raw(25, 6, 1, L.EVENTS_CONTINUE, capture=["force"]) == bad            # another capture list
    assert raw(25, 6, 1, L.EVENTS_CONTINUE, events=[FALL_BACK]) == bad           # another trigger
    assert raw(24, 7, 1, L.EVENTS_CONTINUE) == bad                               # tick 24 is accumulated already
    assert b"24" in hip._lib.sixdof_last_error(hip._h)
    assert raw(21, 0, 1) == L.OK and raw(99, 0, 7, L.EVENTS_CONTINUE) == L.OK   # no samples: a no-op
    assert untouched()                                                           # nothing was copied
    assert raw(25, 26, 1, L.EVENTS_CONTINUE) == L.OK                             # the accumulator is what the held call left
    _same(hip._events_dict(cap, *bufs), want, "after the refusals")
    for wrong in ((20, 50, 1), (21, 51, 1), (21, 50, 0)):
        with pytest.raises(ValueError):
            hip.history_events(ev, cap, *wrong)
    with pytest.raises(KeyError):
        hip.history_events(ev, ["world_pos", "inertia"], 21, 50)
    with pytest.raises(ValueError):
        hip.history_events([], cap, 21, 50)
    empty = hip.history_events(ev, cap, 50, 49)                                  # no samples: no event
    assert np.all(empty["tick"] == 0) and np.all(np.isnan(empty["value"])) and np.all(np.isnan(empty["capture"]["world_vel"])) and empty["tick"].shape == (1, 300)
    hip.enable_history(30)                                                       # a ring that starts over: the accumulator went with the old one
    hip.run(3)                                                                   # 51 .. 53
    bufs[0][...] = 123.0
    bufs[1][0][...] = 123.0
    assert raw(51, 3, 1, L.EVENTS_CONTINUE) == bad and raw(50, 4, 1) == bad     # and a range that starts before the ring's first tick
    assert untouched()
    _same(hip.history_events(ev, cap, 51, 53), _reference(hip, ev, cap, 51, 53, 1), "the new ring")
    hip.enable_history(0)
    with pytest.raises(ValueError, match="no history ring"):
        hip.history_events(ev, cap, 51, 53)
    hip.close()


# ---- 9. front end ---------------------------------------------------------------------------------------------------------
def test_front_end_events_of_one_entity_are_the_events_of_its_series():
    spec = importlib.util.spec_from_file_location("ball", ROOT / "examples" / "ball.py")
    ball = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ball)
    six = ball.el.six_dof(sys=ball.gravity | ball.apply_drag)      # the same stage three times: three executor ticks per world tick
    ex = ball.world(0).build(ball.sample_wind | ball.bounce | six | six | six, simulation_rate=120.0, telemetry_rate=40.0, history=True)
    assert ex._substeps == 3
    ex.enable_history(128)
    ex.run(30)
    # dropped from rest at z = 6: below 5 m after about 0.45 s, faster than 3 m/s downwards after about 0.3 s
    events = [ea.Event("world_pos", 6, "<=", 5.0), ea.Event("world_vel", 5, "<=", -3.0), ea.Event("world_pos", 6, ">", 0.0, mode="level"),
              ea.Event("world_pos", 6, "<=", -100.0)]
    series = ex.history_series(["ball.world_pos", "ball.world_vel"], 2, 30, every=2)
    got = ex.history_events(events, ["world_vel", "wind"], 2, 30, every=2)
    ticks = np.arange(2, 31, 2)
    x = [series["ball.world_pos"][:, 6], series["ball.world_vel"][:, 5], series["ball.world_pos"][:, 6], series["ball.world_pos"][:, 6]]
    for e, event in enumerate(events):
        ref = _reference_one(x[e][:, None], ticks, event)
        for k in KEYS:
            assert got[k].shape == (4, 1) and np.array_equal(got[k][e], ref[k], equal_nan=True), (e, k)      # world ticks
    dt = ex._dt
    assert np.all(got["tick"][:2, 0] > 2) and got["tick"][2, 0] == 2 and got["tick"][3, 0] == 0
    assert np.array_equal(got["t"][:3, 0], got["tick"][:3, 0] * dt) and np.isnan(got["t"][3, 0])
    assert np.array_equal(got["t_before"][:2, 0], got["tick_before"][:2, 0] * dt) and np.all(np.isnan(got["t_before"][2:, 0]))
    for e in range(2):                                              # the crossing time: between the two samples, the numpy interpolation
        t0, t1, v0, v1 = got["t_before"][e, 0], got["t"][e, 0], got["value_before"][e, 0], got["value"][e, 0]
        assert t0 <= got["t_cross"][e, 0] <= t1
        want = min(max(t0 + (events[e].level - v0) / (v1 - v0) * (t1 - t0), t0), t1)
        assert got["t_cross"][e, 0] == want and t0 < want
    assert got["t_cross"][2, 0] == got["t"][2, 0] and np.isnan(got["t_cross"][3, 0])        # no sample before: t itself; no event: NaN
    at = int(got["tick"][0, 0] - 2) // 2
    assert np.array_equal(got["capture"]["world_vel"][0, 0], series["ball.world_vel"][at])
    assert got["capture"]["wind"].shape == (4, 1, 3) and np.all(np.isnan(got["capture"]["wind"][3]))
    with pytest.raises(KeyError):
        ex.history_events([ea.Event("nothing", 0, "<", 0.0)], [], 2, 30)
    with pytest.raises(ValueError):
        ex.history_events(events, [], 0, 30)                         # tick 0 is not in the ring
    with pytest.raises(ValueError):
        ex.history_events(events, [], 2, 30, every=0)


def test_campaign_events_equal_numpy_over_the_runs_columns():
    """A 17-run campaign of the Monte-Carlo example: Campaign.events against numpy over Campaign.column after each tick."""
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
    ticks = np.arange(1, 13)
    pos = np.stack(cols["position"])[:, :, 0]                                  # [tick, run]
    level = float(np.median(pos[5]))                                           # a level the runs reach at different ticks, if at all
    events = [ea.Event("position", 0, ">=", level), ea.Event("position", 0, "<=", level), ea.Event("position", 0, ">=", level, mode="level"),
              ea.Event("position", 0, "<=", level, mode="level")]
    got = c.events(events, comps, 1, 12)
    rows = c.exec.history_events(events, comps, 1, 12)
    for e, event in enumerate(events):
        ref = _reference_one(pos, ticks, event)
        for k in KEYS:
            assert got[k].shape == (4, 17) and np.array_equal(got[k][e], ref[k], equal_nan=True), (e, k)
        for name in comps:
            w = cols[name][0].shape[1]
            assert got["capture"][name].shape == (4, 17, 1, w), name
            want = np.full((17, w), np.nan)
            hit = np.nonzero(ref["tick"])[0]
            want[hit] = np.stack(cols[name])[ref["tick"][hit] - 1, hit]
            assert np.array_equal(got["capture"][name][e, :, 0], want, equal_nan=True), (e, name)
            assert np.array_equal(got["capture"][name][e, :, 0], rows["capture"][name][e], equal_nan=True), (e, name)
    assert np.all((got["tick"][2] > 0) | (got["tick"][3] > 0))                # every run is on one side of the level at some tick
    assert np.array_equal(got["t"], np.where(got["tick"] == 0, np.nan, got["tick"] * c.exec._dt), equal_nan=True)
    assert got["t_cross"].shape == (4, 17)
