"""sixdof_history_events (csrc/sixdof_capi.cpp) without a GPU, under AddressSanitizer + UBSan: built with g++ against the fake
runtime (csrc/hip_fake.cpp), whose launchers walk, merge and capture through csrc/events_plan.hpp — the record, the rule and the
time segments the kernels run — and driven by csrc/events_host_test.cpp: the rule exhaustively over every sequence of up to 8
samples and every cut into 2 and 3 parts, every plane and capture bitwise against a plain loop over random and crafted blocks,
one call against the same range in 2 and 3 calls (one cut placed on a crossing) and under forced segment counts, every refusal
with nothing copied and the accumulator untouched, the conditions of SIXDOF_EVENTS_CONTINUE, 33 captured components, every
fallible runtime call failed once.

The raw -> dict conversion of HipExec.history_events, the constants, the trigger struct and the host-side crossing time are pinned
here too: they need no device."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "elodin_amd" / "csrc"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_events_entry_point_over_the_fake_runtime():
    build = subprocess.run(["make", "-C", str(CSRC), "events_test"], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(CSRC / "build" / "events_host_test")], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert "events_host_test: ok" in run.stdout, run.stdout[-500:]
    merges = re.findall(r"events_host_test: (\d+) merges of every sequence", run.stdout)
    assert len(merges) == 1 and int(merges[0]) >= 1_000_000, run.stdout[-500:]
    faults = re.findall(r"events_host_test: (\d+) fallible calls", run.stdout)
    assert len(faults) == 1 and int(faults[0]) >= 14, run.stdout[-500:]      # allocations, three launches, copies, events, waits
    assert len(re.findall(r"^refusal: ", run.stdout, flags=re.M)) >= 40, run.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]


def test_constants_struct_and_symbol_match_the_header():
    from elodin_amd import _lib as L
    header = (ROOT / "include" / "sixdof_hip.h").read_text()
    want = {"EVENT_LT": L.EVENT_LT, "EVENT_LE": L.EVENT_LE, "EVENT_GT": L.EVENT_GT, "EVENT_GE": L.EVENT_GE, "EVENT_LEVEL": L.EVENT_LEVEL,
            "EVENT_CROSSING": L.EVENT_CROSSING, "EVENTS_ASYNC": L.EVENTS_ASYNC, "EVENTS_CONTINUE": L.EVENTS_CONTINUE, "EVENTS_HOLD": L.EVENTS_HOLD,
            "EVENTS_PLANES": L.EVENTS_PLANES, "EVENTS_MAX_TRIGGERS": L.EVENTS_MAX_TRIGGERS}
    for name, value in want.items():
        found = re.findall(rf"#define SIXDOF_{name}\s+(\d+)u?\s", header)
        assert found == [str(value)], (name, found)
    assert (L.EVENT_LT, L.EVENT_LE, L.EVENT_GT, L.EVENT_GE, L.EVENT_LEVEL, L.EVENT_CROSSING) == (0, 1, 2, 3, 0, 1)
    assert (L.EVENTS_ASYNC, L.EVENTS_CONTINUE, L.EVENTS_HOLD, L.EVENTS_PLANES, L.EVENTS_MAX_TRIGGERS) == (1, 2, 4, 4, 8)
    assert C.sizeof(L.EventTrigger) == 32
    assert [(n, getattr(L.EventTrigger, n).offset) for n, _ in L.EventTrigger._fields_] == [
        ("component_id", 0), ("element", 8), ("group", 12), ("op", 16), ("mode", 20), ("level", 24)]
    assert "sixdof_history_events" in L.SYMBOLS and len(L.SYMBOLS["sixdof_history_events"][1]) == 12


def test_events_become_triggers():
    import elodin_amd as ea
    from elodin_amd import _lib as L
    from elodin_amd.exec import HipExec
    arr = HipExec._event_triggers([ea.Event("world_pos", 6, "<=", 0.0), ea.Event("world_vel", 5, ">", 2.5, mode="level", group=3)])
    assert len(arr) == 2
    assert (arr[0].component_id, arr[0].element, arr[0].group, arr[0].op, arr[0].mode, arr[0].level) == (
        L.component_id("world_pos"), 6, 0, L.EVENT_LE, L.EVENT_CROSSING, 0.0)
    assert (arr[1].component_id, arr[1].element, arr[1].group, arr[1].op, arr[1].mode, arr[1].level) == (
        L.component_id("world_vel"), 5, 3, L.EVENT_GT, L.EVENT_LEVEL, 2.5)
    assert len(HipExec._event_triggers(ea.Event("force", 0, "<", 1.0))) == 1
    assert [HipExec._event_triggers(ea.Event("force", 0, op, 1.0))[0].op for op in ("<", "<=", ">", ">=")] == [0, 1, 2, 3]
    for bad in ([], [ea.Event("force", 0, "<", 1.0)] * 9, [ea.Event("force", 0, "==", 1.0)], [ea.Event("force", 0, "<", 1.0, mode="edge")]):
        with pytest.raises(ValueError):
            HipExec._event_triggers(bad)


def test_raw_planes_become_the_dict_of_history_events():
    from elodin_amd.exec import HipExec
    runs, n = 3, 6
    raw = np.empty((2, 4, runs))
    raw[0] = [[2.0 ** 53 - 1, 0.0, 7.0], [-0.0, np.nan, 1.5], [2.0 ** 53 - 2, 0.0, 0.0], [0.25, np.nan, np.nan]]
    raw[1] = np.arange(4 * runs, dtype=np.float64).reshape(4, runs)
    pos, a = np.arange(2 * n * 7, dtype=np.float64).reshape(2, n, 7), np.full((2, n, 1), np.nan)
    got = HipExec._events_dict(["world_pos", "a"], raw, [pos, a])
    assert sorted(got) == ["capture", "tick", "tick_before", "value", "value_before"]
    for key, plane in (("tick", 0), ("tick_before", 2)):
        assert got[key].dtype == np.int64 and got[key].shape == (2, runs)
        assert np.array_equal(got[key], raw[:, plane].astype(np.int64))
    for key, plane in (("value", 1), ("value_before", 3)):
        assert got[key].dtype == np.float64 and got[key].shape == (2, runs)
        assert np.array_equal(got[key], raw[:, plane], equal_nan=True)
    assert got["tick"][0, 0] == 2 ** 53 - 1 and got["tick_before"][0, 0] == 2 ** 53 - 2      # ticks survive the double exactly
    assert np.signbit(got["value"][0, 0]) and got["value"][0, 0] == 0.0                       # -0.0 stays -0.0
    assert got["tick"][0, 1] == 0 and np.isnan(got["value"][0, 1]) and got["tick_before"][0, 1] == 0
    assert list(got["capture"]) == ["world_pos", "a"]
    assert got["capture"]["world_pos"] is pos and got["capture"]["a"] is a


def test_crossing_time_is_the_linear_interpolation_at_the_level():
    from elodin_amd.api import Exec
    dt = 1.0 / 120.0
    tick = np.array([[10, 0, 4, 9], [6, 3, 0, 2]], dtype=np.int64)
    before = np.array([[9, 0, 0, 6], [5, 2, 0, 0]], dtype=np.int64)
    ev = {"tick": tick, "tick_before": before,
          "t": np.where(tick == 0, np.nan, tick * dt), "t_before": np.where(before == 0, np.nan, before * dt),
          "value": np.array([[-1.0, np.nan, 3.0, -0.5], [2.0, 1.0, np.nan, 7.0]]),
          "value_before": np.array([[3.0, np.nan, np.nan, 1.0], [-2.0, 0.5, np.nan, np.nan]])}
    got = Exec._crossing_time(np.array([0.0, 1.0]), ev)
    assert got.shape == (2, 4)
    assert got[0, 0] == 9 * dt + (0.0 - 3.0) / (-1.0 - 3.0) * (10 * dt - 9 * dt)       # three quarters of the way down
    assert np.isnan(got[0, 1]) and np.isnan(got[1, 2])                                 # no event
    assert got[0, 2] == 4 * dt and got[1, 3] == 2 * dt                                 # no sample before: the event's own time
    assert got[0, 3] == 6 * dt + (0.0 - 1.0) / (-0.5 - 1.0) * (9 * dt - 6 * dt)        # a gap of three ticks (skipped samples)
    assert got[1, 0] == 5 * dt + (1.0 - -2.0) / (2.0 - -2.0) * (6 * dt - 5 * dt)
    assert 2 * dt < got[1, 1] <= 3 * dt and 3 * dt - got[1, 1] <= 1e-17                # the event sits on the level: its own time, to an ulp
    flat = {k: v[:1, :1].copy() for k, v in ev.items()}
    flat["value_before"][0, 0] = flat["value"][0, 0]
    assert Exec._crossing_time(np.array([0.0]), flat)[0, 0] == 10 * dt                 # equal values: the event's own time
