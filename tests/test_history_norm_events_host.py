"""sixdof_history_norm_events (csrc/sixdof_capi.cpp) without a GPU, under AddressSanitizer + UBSan: built with g++ (-ffp-contract=off,
as the kernels are compiled without FMA contraction) against the fake runtime (csrc/hip_fake.cpp), whose launcher walks and merges
through csrc/norm_events_plan.hpp — the norms' value and walk under the events' rule, the function the kernel calls — in the kernels'
time segments and captures through the events' capture, and driven by csrc/norm_events_host_test.cpp, a stand-alone program: every
plane and capture bitwise against a plain loop over the ring (count 1 to 4, with and without MINUS, f32 and f64, +-0, denormals,
NaN, +-inf, overflowing squares, all four ops, both modes), the rule over every cut of random and crafted sequences into 2 and 3
parts, one call against the same range in 2 and 3 CONTINUE calls and under forced segment counts around each load depth, every
refusal with nothing copied and the accumulator untouched, the conditions of SIXDOF_NORM_EVENTS_CONTINUE (a level that differs in
one bit among them), every fallible runtime call failed once.

The constants, the trigger struct, the NormEvent -> trigger conversion and the raw planes -> dict conversion of
HipExec.history_norm_events are pinned here too: they need no device."""
import ctypes as C
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "elodin_amd" / "csrc"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_norm_events_entry_point_over_the_fake_runtime():
    build = subprocess.run(["make", "-C", str(CSRC), "norm_events_test"], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(CSRC / "build" / "norm_events_host_test")], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert "norm_events_host_test: ok" in run.stdout, run.stdout[-500:]
    merges = re.findall(r"norm_events_host_test: (\d+) merges of every cut", run.stdout)
    assert len(merges) == 1 and int(merges[0]) >= 100_000, run.stdout[-500:]
    faults = re.findall(r"norm_events_host_test: (\d+) fallible calls", run.stdout)
    assert len(faults) == 1 and int(faults[0]) >= 16, run.stdout[-500:]      # allocations, three launches, copies, events, waits
    refusals = re.findall(r"^refusal: (.*?): ", run.stdout, flags=re.M)
    assert len(refusals) >= 55, run.stdout[-3000:]
    for what in ("negative level", "NaN level", "infinite level", "count = 5", "unknown op", "unknown mode", "capture of inertia",
                 "continue with a level that differs in one bit", "continue with another mode", "continue with other probe flags"):
        assert what in refusals, what
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]


def test_constants_struct_and_symbol_match_the_header():
    from elodin_amd import _lib as L
    header = (ROOT / "include" / "sixdof_hip.h").read_text()
    want = {"NORM_EVENTS_ASYNC": L.NORM_EVENTS_ASYNC, "NORM_EVENTS_CONTINUE": L.NORM_EVENTS_CONTINUE, "NORM_EVENTS_HOLD": L.NORM_EVENTS_HOLD,
            "NORM_EVENTS_PLANES": L.NORM_EVENTS_PLANES, "NORM_EVENTS_MAX_TRIGGERS": L.NORM_EVENTS_MAX_TRIGGERS}
    for name, value in want.items():
        found = re.findall(rf"#define SIXDOF_{name}\s+(\d+)u?\s", header)
        assert found == [str(value)], (name, found)
    assert (L.NORM_EVENTS_ASYNC, L.NORM_EVENTS_CONTINUE, L.NORM_EVENTS_HOLD, L.NORM_EVENTS_PLANES, L.NORM_EVENTS_MAX_TRIGGERS) == (1, 2, 4, 4, 8)
    assert C.sizeof(L.NormTrigger) == 56
    assert [(n, getattr(L.NormTrigger, n).offset) for n, _ in L.NormTrigger._fields_] == [("probe", 0), ("level_sq", 40), ("op", 48), ("mode", 52)]
    assert L.NormTrigger.probe.size == C.sizeof(L.NormProbe) == 40
    assert "sixdof_history_norm_events" in L.SYMBOLS and len(L.SYMBOLS["sixdof_history_norm_events"][1]) == 12
    assert L.SYMBOLS["sixdof_history_norm_events"][1][1] == C.POINTER(L.NormTrigger)
    # the struct as the header spells it: the probe, the squared level, then op and mode
    body = re.search(r"typedef struct sixdof_norm_trigger \{(.*?)\} sixdof_norm_trigger;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == ["probe", "level_sq", "op", "mode"]
    proto = re.search(r"int sixdof_history_norm_events\((.*?)\);", header, flags=re.S).group(1)
    assert len(proto.split(",")) == 12


def test_norm_events_become_triggers():
    import elodin_amd as ea
    from elodin_amd import _lib as L
    from elodin_amd.exec import HipExec
    assert ea.NormEvent is __import__("elodin_amd.exec", fromlist=["NormEvent"]).NormEvent and "NormEvent" in ea.__all__
    assert ea.NormEvent(ea.Norm("force", 0, 1), "<", 1.0).mode == "crossing"
    arr = HipExec._norm_triggers([ea.NormEvent(ea.Norm("world_vel", 3, 3), ">", 0.1),
                                  ea.NormEvent(ea.Norm("world_pos", 4, 3, group=1, minus="world_pos", minus_group=0), "<=", 3.0, mode="level"),
                                  ea.NormEvent(ea.Norm("world_pos", 0, 4, 2, "world_vel", 1, 3), ">=", 0.0),
                                  ea.NormEvent(ea.Norm("force", 5, 1), "<", 1e154, "level")])
    fields = lambda p: (p.component_id, p.minus_component_id, p.element, p.minus_element, p.group, p.minus_group, p.count, p.flags)
    pos, vel, force = (L.component_id(n) for n in ("world_pos", "world_vel", "force"))
    assert len(arr) == 4
    assert fields(arr[0].probe) == (vel, 0, 3, 0, 0, 0, 3, 0) and (arr[0].op, arr[0].mode) == (L.EVENT_GT, L.EVENT_CROSSING)
    assert arr[0].level_sq == 0.1 * 0.1 and arr[0].level_sq != 0.01                  # the square as the ABI receives it: one rounding of level * level
    assert fields(arr[1].probe) == (pos, pos, 4, 4, 1, 0, 3, L.NORM_MINUS) and (arr[1].op, arr[1].mode, arr[1].level_sq) == (L.EVENT_LE, L.EVENT_LEVEL, 9.0)
    assert fields(arr[2].probe) == (pos, vel, 0, 1, 2, 3, 4, L.NORM_MINUS) and (arr[2].op, arr[2].level_sq) == (L.EVENT_GE, 0.0) and not math.copysign(1.0, arr[2].level_sq) < 0
    assert fields(arr[3].probe) == (force, 0, 5, 0, 0, 0, 1, 0) and (arr[3].op, arr[3].mode, arr[3].level_sq) == (L.EVENT_LT, L.EVENT_LEVEL, 1e154 * 1e154)
    assert len(HipExec._norm_triggers(ea.NormEvent(ea.Norm("force", 0, 1), "<", 1.0))) == 1
    assert len(HipExec._norm_triggers([ea.NormEvent(ea.Norm("force", 0, 1), "<", 1.0)] * 8)) == 8
    good = ea.Norm("force", 0, 1)
    for bad in ([], [ea.NormEvent(good, "<", 1.0)] * 9, [ea.NormEvent(good, "<", -1.0)], [ea.NormEvent(good, "<", -5e-324)], [ea.NormEvent(good, "<", float("nan"))],
                [ea.NormEvent(good, "<", float("inf"))], [ea.NormEvent(good, "<", 1e200)],           # finite, but its square is not
                [ea.NormEvent(good, "==", 1.0)], [ea.NormEvent(good, "<", 1.0, mode="edge")], [ea.NormEvent(ea.Norm("force", 0, 5), "<", 1.0)],
                [ea.NormEvent(ea.Norm("force", 0, 1, minus_group=1), "<", 1.0)], [ea.NormEvent(ea.Norm("force", -1, 1), "<", 1.0)]):
        with pytest.raises(ValueError):
            HipExec._norm_triggers(bad)
    assert HipExec._norm_triggers([ea.NormEvent(good, "<", -0.0)])[0].level_sq == 0.0      # -0.0 is not negative


def test_raw_planes_become_the_dict_of_history_norm_events():
    from elodin_amd.exec import HipExec
    runs = 3
    raw = np.empty((2, 4, runs))
    raw[0] = [[2.0 ** 53 - 1, 0.0, 7.0], [0.0, np.nan, 2.25], [2.0 ** 53 - 2, 0.0, 3.0], [4.0, np.nan, 1e300]]
    raw[1] = np.arange(4 * runs, dtype=np.float64).reshape(4, runs)
    caps = [np.arange(2 * 6 * 7, dtype=np.float64).reshape(2, 6, 7)]
    got = HipExec._norm_events_dict(["world_pos"], raw, caps)
    assert sorted(got) == ["capture", "tick", "tick_before", "value", "value_before", "value_before_sq", "value_sq"]
    for key, plane in (("tick", 0), ("tick_before", 2)):
        assert got[key].dtype == np.int64 and got[key].shape == (2, runs)
        assert np.array_equal(got[key], raw[:, plane].astype(np.int64))
    for key, plane in (("value_sq", 1), ("value_before_sq", 3)):
        assert got[key].dtype == np.float64 and got[key].shape == (2, runs)
        assert np.array_equal(got[key], raw[:, plane], equal_nan=True)
    assert got["tick"][0, 0] == 2 ** 53 - 1 and got["tick_before"][0, 0] == 2 ** 53 - 2                    # exact near 2^53
    assert np.array_equal(got["value"], np.sqrt(raw[:, 1]), equal_nan=True) and np.array_equal(got["value_before"], np.sqrt(raw[:, 3]), equal_nan=True)
    assert got["value"][0, 2] == 1.5 and got["value_before"][0, 0] == 2.0 and got["value_before"][0, 2] == 1e150
    assert np.isnan(got["value"][0, 1]) and np.isnan(got["value_before"][0, 1])                            # NaN stays NaN
    assert got["value"][0, 0] == 0.0 and not np.signbit(got["value"][0, 0])                                # sqrt(+0.0) is +0.0
    assert list(got["capture"]) == ["world_pos"] and got["capture"]["world_pos"] is caps[0]
