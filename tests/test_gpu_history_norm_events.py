"""Ring norm events (sixdof_history_norm_events): per event and run, over the sampled ticks of a range, the first tick at which the
squared Euclidean norm of 1 to 4 elements of a row — or of their difference to as many elements of another row of the run — meets a
squared level, as a level or as a crossing, the squared norm there, tick and squared norm of the finite sample before, and the rows
of other components at that tick, found and captured on the device out of the telemetry ring.

The reference is always numpy over the [ticks, n, w] blocks HipExec.history reads from the same ring: the value loop of
tests/test_gpu_history_norms.py (d = A - B in f64, the sum of squares left to right, multiply and add rounded separately as the
kernel's, which is compiled without FMA contraction) fed into the rule of tests/test_gpu_history_events.py (_reference_one: a
non-finite sample is skipped as if it had not been sampled, LEVEL fires at the earliest finite sample that holds, CROSSING at the
earliest that holds after a finite sample that did not), against level * level as the ABI receives it.  Nothing else is rounded,
so every comparison is np.array_equal (NaN equal to NaN) and no tolerance appears — but for one crossing TIME, whose bound is
derived where it is used.

The world is the events tests' thrown bodies — Z0, uniform gravity, no spin, 4 ticks per launch, v_z = linspace(1, 4, n) — with one
change, so that separations differ per run: the rows of the last group of each run are thrown with 5 - v_z.  Every values case
asserts ON THE REFERENCE that it can tell a wrong answer from a right one (_proves_something)."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np
import pytest

import elodin_amd as ea
from elodin_amd import _lib as L
from elodin_amd import workloads
from tests.test_gpu_history_events import _reference_one

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
INT_KEYS = ("tick", "tick_before")
SQ_KEYS = ("value_sq", "value_before_sq")
F64_KEYS = SQ_KEYS + ("value", "value_before")
RULE_KEYS = {"tick": "tick", "value": "value_sq", "tick_before": "tick_before", "value_before": "value_before_sq"}
Z0 = 5.0
Squared = namedtuple("Squared", "op level mode")           # what _reference_one reads of an event: here the level is the squared one


def _squared_norm(blocks, v, period):
    """[samples, runs]: the squared norm of Norm v out of the history blocks, in f64, left to right."""
    d = blocks[v.component][:, v.group::period, v.element:v.element + v.count].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if v.minus is not None:
            e = v.element if v.minus_element is None else v.minus_element
            g = v.group if v.minus_group is None else v.minus_group
            d = d - blocks[v.minus][:, g::period, e:e + v.count].astype(np.float64)
        s = d[..., 0] * d[..., 0]
        for k in range(1, v.count):
            s = s + d[..., k] * d[..., k]
    return s


def _reference(hip, events, capture, first, last, every, period):
    """The dict of HipExec.history_norm_events out of HipExec.history."""
    ticks = np.arange(first, last + 1, every)
    names = {c for e in events for c in (e.norm.component, e.norm.minus) if c is not None} | set(capture)
    blocks = {name: hip.history(name, first, last)[::every] for name in names}
    per_event = [_reference_one(_squared_norm(blocks, e.norm, period), ticks, Squared(e.op, float(e.level) * float(e.level), e.mode)) for e in events]
    out = {new: np.stack([d[old] for d in per_event]) for old, new in RULE_KEYS.items()}
    out["value"], out["value_before"] = np.sqrt(out["value_sq"]), np.sqrt(out["value_before_sq"])
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
    assert sorted(got) == sorted(INT_KEYS + F64_KEYS + ("capture",)), what
    for k in INT_KEYS + F64_KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, got[k].dtype)
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)
    for k in F64_KEYS:
        assert not np.any(np.signbit(got[k][~np.isnan(got[k])])), (what, k, "a square is never -0.0")
    assert list(got["capture"]) == list(want["capture"]), what
    for name in want["capture"]:
        a, b = got["capture"][name], want["capture"][name]
        assert a.shape == b.shape and a.dtype == np.float64 and np.array_equal(a, b, equal_nan=True), (what, name)


def _proves_something(want, runs, what, one_value=()):
    """The reference itself shows that the case can fail.  With more than one run every event's ticks take more than one value —
    but for the events listed in `one_value`, which by the case's own definition cannot (a crossing needs two samples) and must
    then not fire at all — and at least one event has both firing and non-firing runs.  One run can show neither: there at
    least one event fires and at least one does not."""
    fired = want["tick"] > 0
    print(what, "fired per event:", fired.sum(axis=1).tolist(), "of", runs, "distinct ticks:", [len(np.unique(t[t > 0])) for t in want["tick"]])
    if runs == 1:
        assert np.any(fired) and np.any(~fired), (what, "one run: an event that fires and one that does not")
        return
    for e in range(want["tick"].shape[0]):
        if e in one_value:
            assert not np.any(fired[e]), (what, e, "cannot fire by definition, and yet fires on the reference")
        else:
            assert len(np.unique(want["tick"][e])) > 1, (what, e, "the event ticks take one value only")
    assert any(np.any(fired[e]) and np.any(~fired[e]) for e in range(fired.shape[0])), (what, "no event with both firing and non-firing runs")


def _thrown(n, period, dtype=np.float64, ring=64, nan_rows=()):
    """Bodies thrown upwards from height Z0 under uniform gravity, without spin; the last row of every run with 5 - v_z."""
    w = workloads.independent_bodies(n)
    pos = np.array(w["world_pos"], dtype=dtype)
    pos[:, 6] = Z0
    vel = np.zeros((n, 6), dtype=dtype)
    vel[:, 5] = np.linspace(1.0, 4.0, n)
    vel[period - 1::period, 5] = 5.0 - vel[period - 1::period, 5]
    vel[list(nan_rows)] = np.nan
    hip = ea.HipExec(pos, vel, np.array(w["inertia"], dtype=dtype), entity_ids=w["entity_ids"], simulation_time_step=workloads.DT_120HZ,
                     effectors=[ea.Effector(L.EFF_UNIFORM_GRAVITY, (0.0, 0.0, -9.81))], ticks_per_launch=4, dtype=dtype)
    hip.enable_history(ring)
    return hip


SPEED = ea.Norm("world_vel", 3, 3)                                                # |v|


def _separation(period):
    return ea.Norm("world_pos", 6, 1, group=0, minus="world_pos", minus_group=period - 1)     # |z_0 - z_last| of the run


def _five(period):
    """The issue's triggers a to e."""
    return [ea.NormEvent(SPEED, "<", 0.5), ea.NormEvent(SPEED, ">=", 2.0), ea.NormEvent(_separation(period), ">", 0.3),
            ea.NormEvent(_separation(period), ">=", 0.1, mode="level"), ea.NormEvent(SPEED, ">=", 2.0, mode="level")]


def _eight(period):
    """a to e and three more shapes: count 4, |A - B| of 3 elements across components (load depth 2: v + g, near 9.81 + v_z), count 2."""
    return _five(period) + [ea.NormEvent(ea.Norm("world_vel", 2, 4, group=period - 1), "<", 0.25),
                            ea.NormEvent(ea.Norm("world_vel", 3, 3, minus="world_accel"), "<=", 9.81 + 0.3),
                            ea.NormEvent(ea.Norm("world_vel", 4, 2, group=period - 1), ">=", 1.5, mode="level")]


CAPTURE = ["world_pos", "world_vel"]


def _buffers(hip, n_events, capture, period=1, fill=123.0):
    return np.full((n_events, L.NORM_EVENTS_PLANES, hip.n // period), fill), [np.full((n_events, hip.n, hip._recorded_width(c)), fill) for c in capture]


def _raw(hip, events, capture, period, first, n_samples, every, bufs, flags=0):
    trig = events if isinstance(events, C.Array) else ea.HipExec._norm_triggers(events)
    comp = np.array([L.component_id(c) for c in capture], dtype=np.uint64)
    ev, caps = bufs if bufs is not None else (None, None)
    ptrs = None if caps is None else (C.c_void_p * max(1, len(caps)))(*[b.ctypes.data for b in caps])
    return hip._lib.sixdof_history_norm_events(hip._h, trig, len(trig), comp.ctypes.data_as(C.POINTER(C.c_uint64)), len(capture), period, first, n_samples, every,
                                               None if ev is None else ev.ctypes.data, ptrs, flags)


# ---- 1. values ---------------------------------------------------------------------------------------------------------------
# (what, n, period, dtype, events of period, ring, ticks run, first, last, every, events that cannot fire)
VALUES = [
    ("1 run", 2, 2, np.float64, _five, 64, 60, 1, 60, 1, ()),
    ("63 runs", 126, 2, np.float32, _five, 64, 60, 1, 60, 1, ()),                              # a wavefront's edge
    ("65 runs", 130, 2, np.float64, _five, 64, 60, 1, 60, 1, ()),
    ("257 runs", 514, 2, np.float32, _five, 64, 60, 1, 60, 1, ()),                             # a block's edge
    ("3 rows per run", 195, 3, np.float64, _five, 64, 60, 1, 60, 1, ()),
    ("count 1", 130, 2, np.float32, lambda p: [ea.NormEvent(ea.Norm("world_vel", 5, 1), "<", 0.5), ea.NormEvent(ea.Norm("world_vel", 5, 1, group=1), ">=", 2.0)], 64, 60, 1, 60, 1, ()),
    ("count 2", 130, 2, np.float64, lambda p: [ea.NormEvent(ea.Norm("world_vel", 4, 2), "<", 0.5), ea.NormEvent(ea.Norm("world_vel", 4, 2, group=1), ">=", 2.0)], 64, 60, 1, 60, 1, ()),
    ("count 3", 130, 2, np.float32, lambda p: [ea.NormEvent(SPEED, "<", 0.5), ea.NormEvent(ea.Norm("world_vel", 3, 3, group=1), ">=", 2.0)], 64, 60, 1, 60, 1, ()),
    ("count 4", 130, 2, np.float64, lambda p: [ea.NormEvent(ea.Norm("world_vel", 2, 4), "<", 0.5), ea.NormEvent(ea.Norm("world_vel", 2, 4, group=1), ">=", 2.0)], 64, 60, 1, 60, 1, ()),
    ("minus within a component", 130, 2, np.float32, lambda p: [ea.NormEvent(_separation(p), ">", 0.3), ea.NormEvent(ea.Norm("world_pos", 4, 3, group=1, minus="world_pos", minus_group=1), ">=", 0.0)],
     64, 60, 1, 60, 1, (1,)),                                                                   # a row against itself: +0.0 >= 0 from the first sample on never crosses
    ("minus across components", 130, 2, np.float64, lambda p: [ea.NormEvent(ea.Norm("world_pos", 6, 1, minus="world_vel", minus_element=5), ">=", 7.5),
                                                               ea.NormEvent(ea.Norm("world_vel", 2, 4, group=1, minus="world_accel"), "<=", 9.81 + 0.3)], 64, 60, 1, 60, 1, ()),
    ("eight triggers", 130, 2, np.float64, _eight, 64, 60, 1, 60, 1, ()),
    ("wraps the ring", 130, 2, np.float64, _five, 10, 47, 38, 47, 1, ()),                      # ticks 38 .. 47 sit in slots 7 8 9 0 .. 6
    ("every 3", 130, 2, np.float32, _five, 64, 60, 2, 59, 3, ()),
    ("13 samples", 130, 2, np.float64, _eight, 64, 40, 28, 40, 1, ()),                         # no multiple of a load depth (4, 2)
    ("a single sample", 130, 2, np.float32, _five, 64, 40, 17, 17, 1, (0, 1, 2)),              # a crossing needs two samples
]


@pytest.mark.parametrize("what,n,period,dtype,events_of,ring,run,first,last,every,one_value", VALUES, ids=[v[0] for v in VALUES])
def test_norm_events_equal_numpy_over_the_history_blocks(what, n, period, dtype, events_of, ring, run, first, last, every, one_value):
    hip = _thrown(n, period, dtype, ring=ring)
    hip.run(run)
    events, runs = events_of(period), n // period
    got = hip.history_norm_events(events, CAPTURE, first, last, every, period=period)
    assert got["tick"].shape == (len(events), runs) and got["tick"].dtype == np.int64 and got["value_sq"].dtype == np.float64
    assert got["capture"]["world_pos"].shape == (len(events), n, 7) and got["capture"]["world_vel"].shape == (len(events), n, 6)
    want = _reference(hip, events, CAPTURE, first, last, every, period)
    _proves_something(want, runs, what, one_value)
    _same(got, want, what)
    fired = got["tick"] > 0
    assert np.all((got["tick"][fired] - first) % every == 0) and np.all((got["tick"][fired] >= first) & (got["tick"][fired] <= last))
    assert np.all(got["tick_before"][fired] < got["tick"][fired]) and np.all(np.isnan(got["value_sq"][~fired])) and np.all(got["tick_before"][~fired] == 0)
    vel = hip.history("world_vel", first, last).astype(np.float64)
    for e in range(len(events)):                                # every row's capture is the history row at ITS RUN'S OWN tick
        for row in range(n):
            t = got["tick"][e, row // period]
            if t:
                assert np.array_equal(got["capture"]["world_vel"][e, row], vel[t - first, row]), (what, e, row)
            else:
                assert np.all(np.isnan(got["capture"]["world_vel"][e, row])) and np.all(np.isnan(got["capture"]["world_pos"][e, row])), (what, e, row)
    bare = hip.history_norm_events(events[0], [], first, last, every, period=period)       # one event, no capture
    assert bare["capture"] == {}
    for k in INT_KEYS + F64_KEYS:
        assert np.array_equal(bare[k], got[k][:1], equal_nan=True), (what, k)
    hip.close()


# ---- 2. modes ------------------------------------------------------------------------------------------------------------------
def test_level_fires_at_once_and_a_crossing_only_after_the_predicate_has_failed():
    n, period = 130, 2
    hip = _thrown(n, period)
    hip.run(60)
    events = [ea.NormEvent(SPEED, ">=", 0.9, mode="level"),        # every row starts at 1 m/s or more: holds at tick 1
              ea.NormEvent(SPEED, ">=", 2.0),                      # trigger b
              ea.NormEvent(SPEED, ">=", 0.0),                      # holds throughout: never crosses
              ea.NormEvent(_separation(period), ">=", 0.0)]
    got = hip.history_norm_events(events, CAPTURE, 1, 60, period=period)
    want = _reference(hip, events, CAPTURE, 1, 60, 1, period)
    _same(got, want, "modes")
    level, b, always, always_sep = range(4)
    vel = hip.history("world_vel", 1, 60).astype(np.float64)
    assert np.all(got["tick"][level] == 1) and np.all(got["tick_before"][level] == 0) and np.all(np.isnan(got["value_before_sq"][level]))
    assert np.array_equal(got["value_sq"][level], vel[0, 0::period, 5] * vel[0, 0::period, 5])
    assert np.array_equal(got["capture"]["world_vel"][level], vel[0])
    v0 = np.linspace(1.0, 4.0, n)[0::period]
    fast = v0 >= 2.1                                               # |v| >= 2 from the first sample on: fires only once it has dropped below 2 and is back
    assert np.any(fast & (got["tick"][b] > 0)) and np.any(fast & (got["tick"][b] == 0)) and np.any(~fast & (got["tick"][b] > 0))
    for run in np.nonzero(fast & (got["tick"][b] > 0))[0]:
        t = got["tick"][b, run]
        speed = np.abs(vel[:, run * period, 5])
        assert speed[0] >= 2.0 and np.any(speed[:t - 1] < 2.0) and speed[t - 2] < 2.0 <= speed[t - 1] and vel[t - 1, run * period, 5] < 0.0, run
        assert got["tick_before"][b, run] == t - 1
    for e in (always, always_sep):
        assert np.all(got["tick"][e] == 0) and np.all(np.isnan(got["value_sq"][e])) and np.all(np.isnan(got["value"][e]))
        assert np.all(np.isnan(got["capture"]["world_pos"][e])) and np.all(np.isnan(got["capture"]["world_vel"][e]))
    hip.close()


# ---- 3. non-finite samples -------------------------------------------------------------------------------------------------
def test_non_finite_samples_are_skipped_and_are_never_a_before_sample():
    n, period = 130, 2
    start_nan = [128]                                              # run 64, row 0: never finite
    hip, clean = _thrown(n, period, nan_rows=start_nan), _thrown(n, period)
    for h in (hip, clean):
        h.run(8)
    hip.world_vel[[0, 63]] = np.nan                                # run 0 row 0 and run 31 row 1: finite up to tick 8
    hip.world_vel[8, 4] = np.inf                                   # run 4 row 0: one infinite element in ticks 9 .. 12
    hip.world_vel[20, 5] = 1e200                                   # run 10 row 0: finite, its square is not, from tick 9 on
    hip.world_vel[41, 5] = -np.inf                                 # run 20 row 1
    hip.upload()
    for h in (hip, clean):
        h.run(4)
    hip.world_pos[8], hip.world_vel[8] = clean.world_pos[8], clean.world_vel[8]      # run 4 is finite again from tick 13 on
    hip.upload()
    for h in (hip, clean):
        h.run(48)
    events = _five(period)
    got, other = hip.history_norm_events(events, CAPTURE, 1, 60, period=period), clean.history_norm_events(events, CAPTURE, 1, 60, period=period)
    want = _reference(hip, events, CAPTURE, 1, 60, 1, period)
    _same(got, want, "non-finite")
    a, b, c, d, e = range(5)
    speed_sq = _squared_norm({"world_vel": hip.history("world_vel", 1, 60)}, SPEED, period)
    # on the reference and the history: what the poisoned runs were made to show
    assert not np.any(np.isfinite(speed_sq[:, 64])) and np.all(np.isfinite(speed_sq[:8, 0])) and not np.any(np.isfinite(speed_sq[8:, 0]))
    assert np.all(np.isinf(speed_sq[8:, 10])) and np.isfinite(hip.history("world_vel", 9, 9)[0, 20, 5])        # an overflowing square of a finite element
    assert np.all(np.isinf(speed_sq[8:12, 4])) and np.all(np.isfinite(speed_sq[12:, 4]))
    for ev in (a, b, e):
        assert got["tick"][ev, 64] == 0 and np.isnan(got["value_sq"][ev, 64]) and got["tick_before"][ev, 64] == 0       # no finite sample: no event
        assert np.all(np.isnan(got["capture"]["world_vel"][ev, 128:130]))
    assert got["tick"][a, 0] == other["tick"][a, 0] <= 8           # an event before the NaN stays
    assert got["tick"][b, 0] == 0 and other["tick"][b, 0] > 8      # one after it never comes
    assert got["tick"][e, 10] == 0 and got["tick"][b, 10] == 0     # +inf >= 4 does not hold: the sample is skipped, it neither holds nor fails
    assert other["tick"][a, 10] > 8 and got["tick"][a, 10] == 0
    assert got["tick"][c, 20] == 0 or got["tick"][c, 20] <= 8      # the separation of run 20 is not finite from tick 9 on
    # run 4: |v| < 0.5 would have been crossed in ticks 9 .. 12, which are skipped: the event is tick 13, the sample before it tick 8
    assert 9 <= other["tick"][a, 4] <= 12
    assert got["tick"][a, 4] == 13 and got["tick_before"][a, 4] == 8 and got["value_before_sq"][a, 4] == speed_sq[7, 4] and got["value_sq"][a, 4] == speed_sq[12, 4]
    others = np.setdiff1d(np.arange(n // period), [0, 4, 10, 20, 31, 64])
    for k in INT_KEYS + F64_KEYS:
        assert np.array_equal(got[k][:, others], other[k][:, others], equal_nan=True), k
    rows = np.concatenate([others * period, others * period + 1])
    for name in CAPTURE:
        assert np.array_equal(got["capture"][name][:, rows], other["capture"][name][:, rows], equal_nan=True), name
    for h in (hip, clean):
        h.close()


def test_nan_rows_in_an_f32_world_never_fire():
    n, period, rows = 126, 2, [0, 63, 125]
    hip = _thrown(n, period, np.float32, nan_rows=rows)
    hip.run(60)
    events = _five(period)
    got = hip.history_norm_events(events, CAPTURE, 1, 60, period=period)
    _same(got, _reference(hip, events, CAPTURE, 1, 60, 1, period), "f32 NaN rows")
    assert np.all(got["tick"][[0, 1, 4], 0] == 0) and np.all(got["tick"][2:4, [31, 62]] == 0) and np.any(got["tick"][0] > 0)
    hip.close()


# ---- 4. the norms reader and this one agree -----------------------------------------------------------------------------------
def test_a_level_at_the_extreme_of_history_norms_fires_at_its_tick():
    hip = _thrown(2, 2)                                             # one run
    hip.run(60)
    probes = [SPEED, ea.Norm("world_pos", 6, 1, minus="world_vel", minus_element=5)]
    norms = hip.history_norms(probes, 1, 60, period=2)
    assert np.all(norms["count"] == 60) and np.all(norms["min_sq"] < norms["max_sq"]) and np.all(norms["argmin"] != norms["argmax"])
    for p, probe in enumerate(probes):
        for op, key, at in ((L.EVENT_GE, "max_sq", "argmax"), (L.EVENT_LE, "min_sq", "argmin")):
            trig = ea.HipExec._norm_triggers([ea.NormEvent(probe, ">=", 0.0, mode="level")])
            trig[0].level_sq, trig[0].op = norms[key][p, 0], op     # through the raw ABI: the squared level is the other reader's double, bit for bit
            bufs = _buffers(hip, 1, [], period=2)
            assert _raw(hip, trig, [], 2, 1, 60, 1, bufs) == L.OK
            out = hip._norm_events_dict([], *bufs)
            assert out["tick"][0, 0] == norms[at][p, 0], (p, key)
            assert out["value_sq"][0, 0].tobytes() == norms[key][p, 0].tobytes(), (p, key)
    hip.close()


# ---- 5. cut invariance ------------------------------------------------------------------------------------------------------
CUT_CASE = dict(n=130, period=2, first=3, last=60, every=1)


def _cut_exec():
    hip = _thrown(CUT_CASE["n"], CUT_CASE["period"])
    hip.run(60)
    return hip


def _child(out_path):
    """What a child process of the cut-invariance test runs: SIXDOF_NORM_EVENTS_SEGMENTS is what its environment says."""
    hip = _cut_exec()
    got = hip.history_norm_events(_eight(CUT_CASE["period"]), CAPTURE, CUT_CASE["first"], CUT_CASE["last"], CUT_CASE["every"], period=CUT_CASE["period"])
    flat = {k: v for k, v in got.items() if k != "capture"}
    flat.update({"capture_" + name: v for name, v in got["capture"].items()})
    np.savez(out_path, **flat)
    hip.close()


def test_forced_segment_counts_give_identical_arrays(tmp_path):
    hip = _cut_exec()
    events = _eight(CUT_CASE["period"])
    want = _reference(hip, events, CAPTURE, CUT_CASE["first"], CUT_CASE["last"], CUT_CASE["every"], CUT_CASE["period"])
    _proves_something(want, 65, "cut invariance")
    hip.close()
    for segments in ("1", "2", "3", "5", None):                # a fresh process per value, one after another: the first that fails ends the test
        env = dict(os.environ)
        env.pop("SIXDOF_NORM_EVENTS_SEGMENTS", None)
        if segments is not None:
            env["SIXDOF_NORM_EVENTS_SEGMENTS"] = segments
        out = tmp_path / f"segments_{segments}.npz"
        code = f"import sys; sys.path.insert(0, {str(ROOT)!r}); from tests.test_gpu_history_norm_events import _child; _child({str(out)!r})"
        proc = subprocess.run([sys.executable, "-c", code], env=env, cwd=str(ROOT), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert proc.returncode == 0, (segments, proc.returncode, proc.stdout[-2000:])
        with np.load(out) as z:
            got = {k: z[k] for k in z.files if not k.startswith("capture_")}
            got["capture"] = {name: z["capture_" + name] for name in CAPTURE}
        _same(got, want, f"SIXDOF_NORM_EVENTS_SEGMENTS={segments}")


# ---- 6. longer than the ring ------------------------------------------------------------------------------------------------
def test_streamed_norm_events_over_a_ring_one_batch_deep_equal_one_read_of_a_whole_ring():
    n, period = 130, 2
    events = _eight(period)
    a, b = _thrown(n, period, ring=0, nan_rows=[5, 77]), _thrown(n, period, ring=48, nan_rows=[5, 77])
    with pytest.raises(ValueError):
        a.stream_norm_events(events, CAPTURE, 6, 8, every=3, period=period)
    wall, got = a.stream_norm_events(events, CAPTURE, 6, 8, every=2, period=period)
    assert wall > 0.0 and a.tick == 48 and a._ring_ticks == 8
    b.run(48)
    want = b.history_norm_events(events, CAPTURE, 2, 48, every=2, period=period)
    _same(want, _reference(b, events, CAPTURE, 2, 48, 2, period), "the twin")
    _same(got, want, "streamed")
    batches = np.unique(got["tick"][0][got["tick"][0] > 0] // 8)
    assert len(batches) > 2 and got["tick"][0].max() > 16          # events in several batches, beyond the first
    early = np.nonzero((got["tick"][0] > 0) & (got["tick"][0] <= 16))[0]
    assert len(early) > 0                                           # a capture taken in an early batch survives the later ones
    vel = b.history("world_vel", 1, 48).astype(np.float64)
    for run in early:
        assert np.array_equal(got["capture"]["world_vel"][0, run * period], vel[got["tick"][0, run] - 1, run * period]), run
    a.run(2)                                                 # the caller's flags are back: a blocking step, and the state a plain run leaves
    b.run(2)
    assert a.tick == 50
    for c in ("world_pos", "world_vel"):
        assert np.array_equal(getattr(a, c), getattr(b, c), equal_nan=True), c
    for h in (a, b):
        h.close()


# ---- 7. HOLD and CONTINUE -----------------------------------------------------------------------------------------------------
def test_hold_delivers_nothing_and_a_changed_request_cannot_continue():
    n, period = 130, 2
    hip = _thrown(n, period, np.float32, ring=64)
    hip.run(60)
    events, cap = _five(period)[:3], ["world_vel"]
    whole = hip.history_norm_events(events, cap, 1, 60, period=period)
    _same(whole, _reference(hip, events, cap, 1, 60, 1, period), "one call")
    assert np.any(whole["tick"] > 40) and np.any((whole["tick"] > 0) & (whole["tick"] <= 20))
    bufs = _buffers(hip, 3, cap, period)
    untouched = lambda: np.all(bufs[0] == 123.0) and np.all(bufs[1][0] == 123.0)
    bad, hold, cont = L.ERR_INVALID_ARGUMENT, L.NORM_EVENTS_HOLD, L.NORM_EVENTS_CONTINUE
    raw = lambda first, n_samples, flags=0, ev=events, capture=cap, per=period, b=bufs, every=1: _raw(hip, ev, capture, per, first, n_samples, every, b, flags)
    assert raw(1, 20, hold) == L.OK and raw(21, 20, hold | cont) == L.OK
    assert untouched()                                                            # held: nothing is delivered

    def changed(change):
        trig = ea.HipExec._norm_triggers(events)
        change(trig[2])
        return trig
    one_bit = np.nextafter(np.float64(0.3) * np.float64(0.3), 1.0)
    refused = [("a changed probe", dict(ev=changed(lambda t: setattr(t.probe, "minus_element", 5)))),
               ("a changed element", dict(ev=changed(lambda t: setattr(t.probe, "element", 5)))),
               ("a changed op", dict(ev=changed(lambda t: setattr(t, "op", L.EVENT_GE)))),
               ("a changed mode", dict(ev=changed(lambda t: setattr(t, "mode", L.EVENT_LEVEL)))),
               ("a level changed in one bit", dict(ev=changed(lambda t: setattr(t, "level_sq", float(one_bit))))),
               ("a changed capture list", dict(capture=["world_pos"], b=(bufs[0], [np.full((3, n, 7), 123.0)]))),
               ("no capture list", dict(capture=[], b=(bufs[0], []))),
               ("another order", dict(ev=events[::-1])),
               ("another period", dict(per=1, b=_buffers(hip, 3, cap, 1))),
               ("a first_tick that is accumulated already", dict(first=40, n_samples=21))]
    for what, kw in refused:
        first, n_samples = kw.pop("first", 41), kw.pop("n_samples", 20)
        assert raw(first, n_samples, cont, **kw) == bad, what
        assert hip._lib.sixdof_last_error(hip._h), what
    assert b"40" in hip._lib.sixdof_last_error(hip._h)
    # the refusals of the ABI return their status
    assert raw(41, 20, 0, b=None) == bad and raw(41, 20, 8) == bad and raw(41, 20, 0, every=0) == bad and raw(41, 21) == bad and raw(41, 20, per=7) == bad
    assert raw(41, 20, ev=[ea.NormEvent(ea.Norm("world_vel", 4, 3), "<", 1.0)]) == bad and b"width" in hip._lib.sixdof_last_error(hip._h)
    assert raw(41, 20, ev=[ea.NormEvent(ea.Norm("world_vel", 3, 3, group=2), "<", 1.0)]) == bad
    for level_sq in (-1.0, float("nan"), float("inf"), -5e-324):
        assert raw(41, 20, ev=changed(lambda t: setattr(t, "level_sq", level_sq))) == bad, level_sq
        assert b"level" in hip._lib.sixdof_last_error(hip._h)
    assert raw(41, 20, ev=changed(lambda t: setattr(t, "op", 4))) == bad and raw(41, 20, ev=changed(lambda t: setattr(t, "mode", 2))) == bad
    assert raw(41, 20, ev=changed(lambda t: setattr(t.probe, "count", 5))) == bad and raw(41, 20, ev=changed(lambda t: setattr(t.probe, "flags", 2))) == bad
    assert raw(41, 20, ev=(L.NormTrigger * 9)()) == bad
    assert raw(41, 20, ev=[ea.NormEvent(ea.Norm("inertia", 0, 3), "<", 1.0)]) == L.ERR_COMPONENT_NOT_FOUND
    assert raw(41, 20, capture=["inertia"], b=(bufs[0], [np.full((3, n, 7), 123.0)])) == L.ERR_COMPONENT_NOT_FOUND
    assert raw(41, 0, cont) == L.OK                                               # no samples: a no-op
    assert untouched()                                                            # nothing was copied
    assert raw(41, 20, cont) == L.OK                                              # the accumulator is what the held calls left
    _same(hip._norm_events_dict(cap, *bufs), whole, "after the refusals")
    with pytest.raises(ValueError, match="period"):
        hip.history_norm_events(events, cap, 1, 60, period=7)
    with pytest.raises(KeyError):
        hip.history_norm_events(events, ["inertia"], 1, 60, period=period)
    empty = hip.history_norm_events(events, cap, 60, 59, period=period)          # no samples: no event
    assert np.all(empty["tick"] == 0) and np.all(np.isnan(empty["value"])) and np.all(np.isnan(empty["capture"]["world_vel"])) and empty["tick"].shape == (3, 65)
    hip.close()


# ---- 8. upper layers ----------------------------------------------------------------------------------------------------------
def test_front_end_norm_events_of_one_entity_are_the_events_of_its_series():
    spec = importlib.util.spec_from_file_location("ball", ROOT / "examples" / "ball.py")
    ball = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ball)
    six = ball.el.six_dof(sys=ball.gravity | ball.apply_drag)      # the same stage three times: three executor ticks per world tick
    ex = ball.world(0).build(ball.sample_wind | ball.bounce | six | six | six, simulation_rate=120.0, telemetry_rate=40.0, history=True)
    assert ex._substeps == 3
    ex.enable_history(128)
    ex.run(30)
    # dropped from rest at z = 6: faster than 3 m/s after about 0.3 s, closer than 5 m to the origin's height after about 0.45 s
    events = [ea.NormEvent(ea.Norm("world_vel", 3, 3), ">=", 3.0), ea.NormEvent(ea.Norm("world_pos", 6, 1), "<=", 5.0),
              ea.NormEvent(ea.Norm("world_pos", 6, 1), ">", 0.0, mode="level"), ea.NormEvent(ea.Norm("world_pos", 6, 1, minus="world_vel", minus_element=5), ">=", 1000.0)]
    series = ex.history_series(["ball.world_pos", "ball.world_vel"], 2, 30, every=2)
    got = ex.history_norm_events(events, ["world_vel", "wind"], 2, 30, every=2)
    ticks = np.arange(2, 31, 2)
    pos, vel = series["ball.world_pos"].astype(np.float64), series["ball.world_vel"].astype(np.float64)
    s = [vel[:, 3] * vel[:, 3] + vel[:, 4] * vel[:, 4] + vel[:, 5] * vel[:, 5], pos[:, 6] * pos[:, 6], pos[:, 6] * pos[:, 6], (pos[:, 6] - vel[:, 5]) * (pos[:, 6] - vel[:, 5])]
    for e, event in enumerate(events):
        ref = _reference_one(s[e][:, None], ticks, Squared(event.op, float(event.level) * float(event.level), event.mode))
        for old, new in RULE_KEYS.items():
            assert got[new].shape == (4, 1) and np.array_equal(got[new][e], ref[old], equal_nan=True), (e, new)      # world ticks
    assert np.array_equal(got["value"], np.sqrt(got["value_sq"]), equal_nan=True) and np.array_equal(got["value_before"], np.sqrt(got["value_before_sq"]), equal_nan=True)
    dt = ex._dt
    assert np.all(got["tick"][:2, 0] > 2) and got["tick"][2, 0] == 2 and got["tick"][3, 0] == 0
    assert np.array_equal(got["t"][:3, 0], got["tick"][:3, 0] * dt) and np.isnan(got["t"][3, 0])
    assert np.array_equal(got["t_before"][:2, 0], got["tick_before"][:2, 0] * dt) and np.all(np.isnan(got["t_before"][2:, 0]))
    for e in range(2):                                              # the crossing time: between the two samples, the numpy interpolation of the NORMS
        t0, t1, v0, v1 = got["t_before"][e, 0], got["t"][e, 0], got["value_before"][e, 0], got["value"][e, 0]
        assert t0 <= got["t_cross"][e, 0] <= t1
        want = min(max(t0 + (events[e].level - v0) / (v1 - v0) * (t1 - t0), t0), t1)
        assert got["t_cross"][e, 0] == want and t0 < want
    assert got["t_cross"][2, 0] == got["t"][2, 0] and np.isnan(got["t_cross"][3, 0])        # no sample before: t itself; no event: NaN
    at = int(got["tick"][0, 0] - 2) // 2
    assert np.array_equal(got["capture"]["world_vel"][0, 0], series["ball.world_vel"][at])
    assert got["capture"]["wind"].shape == (4, 1, 3) and np.all(np.isnan(got["capture"]["wind"][3]))
    with pytest.raises(KeyError):
        ex.history_norm_events([ea.NormEvent(ea.Norm("nothing", 0, 1), "<", 1.0)], [], 2, 30)
    with pytest.raises(ValueError):
        ex.history_norm_events(events, [], 0, 30)                    # tick 0 is not in the ring
    with pytest.raises(ValueError):
        ex.history_norm_events(events, [], 2, 30, every=0)


def test_the_crossing_time_of_a_linearly_growing_separation_is_exact():
    """The two rows of a run start at the same height with speeds that differ by dv under the same gravity: their z-separation is
    |dv| t, a straight line through the origin, so the line through the two samples around the level meets it at level / |dv|.
    The bound: a z carries the roundings of at most 60 steps, each at most half an ulp of a height below 8 (8.9e-16), so a
    separation is off by at most 1.1e-13 m and the crossing time, divided by |dv| >= 0.3 / 0.5 m/s (an event within 60 ticks),
    by at most 2e-13 s; the interpolation itself adds a few ulps of 0.5 s.  1e-12 s is asked for."""
    from elodin_amd.api import Exec
    n, period, level = 130, 2, 0.3
    hip = _thrown(n, period)
    hip.run(60)
    event = ea.NormEvent(_separation(period), ">", level)
    got = dict(hip.history_norm_events([event], [], 1, 60, period=period))
    dt = workloads.DT_120HZ
    for tick_field, seconds in (("tick", "t"), ("tick_before", "t_before")):
        got[seconds] = np.where(got[tick_field] == 0, np.nan, got[tick_field].astype(np.float64) * dt)
    t_cross = Exec._crossing_time(np.array([level]), got)[0]
    lin = np.linspace(1.0, 4.0, n)
    dv = np.abs(lin[0::2] - (5.0 - lin[1::2]))
    fired = got["tick"][0] > 0
    assert np.sum(fired) > 40 and np.any(~fired) and len(np.unique(got["tick"][0][fired])) > 10
    assert np.all(got["tick_before"][0][fired] == got["tick"][0][fired] - 1)
    assert np.all((got["t_before"][0][fired] <= t_cross[fired]) & (t_cross[fired] <= got["t"][0][fired]))
    error = np.abs(t_cross[fired] - level / dv[fired])
    print("largest error of the crossing time:", error.max(), "s")
    assert np.all(error < 1e-12)
    assert np.all(np.isnan(t_cross[~fired]))
    hip.close()


def test_campaign_norm_events_equal_numpy_over_the_runs_columns():
    """A 17-run campaign of the Monte-Carlo example: Campaign.norm_events against numpy over Campaign.column after each tick."""
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
    kp = min(pos.shape[2], 4)

    def squared(x):
        s = x[..., 0] * x[..., 0]
        for e in range(1, x.shape[2]):
            s = s + x[..., e] * x[..., e]
        return s
    s_pos, s_sep = squared(pos[:, :, :kp]), squared(pos[:, :, :k] - vel[:, :, :k])
    level_pos, level_sep = float(np.sqrt(np.median(s_pos[5]))), float(np.sqrt(np.median(s_sep[5])))      # levels the runs reach at different ticks, if at all
    events = [ea.NormEvent(ea.Norm("position", 0, kp), ">=", level_pos), ea.NormEvent(ea.Norm("position", 0, kp), "<=", level_pos),
              ea.NormEvent(ea.Norm("position", 0, k, minus="velocity"), ">=", level_sep, mode="level"), ea.NormEvent(ea.Norm("position", 0, k, minus="velocity"), "<=", level_sep, mode="level")]
    got = c.norm_events(events, comps, 1, 12)
    rows = c.exec.history_norm_events(events, comps, 1, 12)
    for e, (event, s) in enumerate(zip(events, (s_pos, s_pos, s_sep, s_sep))):
        ref = _reference_one(s, ticks, Squared(event.op, float(event.level) * float(event.level), event.mode))
        for old, new in RULE_KEYS.items():
            assert got[new].shape == (4, 17) and np.array_equal(got[new][e], ref[old], equal_nan=True), (e, new)
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
    assert got["t_cross"].shape == (4, 17) and np.array_equal(got["value"], np.sqrt(got["value_sq"]), equal_nan=True)
