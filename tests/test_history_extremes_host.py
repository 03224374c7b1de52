"""sixdof_history_extremes (csrc/sixdof_capi.cpp) without a GPU, under AddressSanitizer + UBSan: built with g++ against the fake
runtime (csrc/hip_fake.cpp), whose launcher walks and merges through csrc/extremes_plan.hpp — the record, the rule and the time
segments the kernels run — and driven by csrc/extremes_host_test.cpp: every plane bitwise against a plain loop over random and
crafted blocks, one call against the same range in 2 and 3 calls and under forced segment counts, every refusal with nothing
copied and the accumulator untouched, the conditions of SIXDOF_EXTREMES_CONTINUE, 33 component entries, every fallible runtime
call failed once.

The raw -> dict conversion of HipExec.history_extremes is pinned here too: it needs no device."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

CSRC = Path(__file__).resolve().parents[1] / "elodin_amd" / "csrc"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_extremes_entry_point_over_the_fake_runtime():
    build = subprocess.run(["make", "-C", str(CSRC), "extremes_test"], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(CSRC / "build" / "extremes_host_test")], capture_output=True, text=True, timeout=120,
                         env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert "extremes_host_test: ok" in run.stdout, run.stdout[-500:]
    faults = re.findall(r"extremes_host_test: (\d+) fallible calls", run.stdout)
    assert len(faults) == 1 and int(faults[0]) >= 12, run.stdout[-500:]      # allocations, launches, copies, events, waits
    assert len(re.findall(r"^refusal: ", run.stdout, flags=re.M)) >= 20, run.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]


def test_raw_planes_become_the_dict_of_history_extremes():
    from elodin_amd import _lib as L
    from elodin_amd.exec import HipExec
    assert (L.EXTREMES_ASYNC, L.EXTREMES_CONTINUE, L.EXTREMES_HOLD, L.EXTREMES_PLANES) == (1, 2, 4, 6)
    assert "sixdof_history_extremes" in L.SYMBOLS
    n = 3
    pos = np.empty((6, n, 7))
    pos[0], pos[1], pos[2], pos[3], pos[4], pos[5] = 4.0, -0.0, 2.0 ** 53 - 1, 7.5, 9.0, 0.0
    pos[:, 1, 2] = [0.0, np.nan, 0.0, np.nan, 0.0, 3.0]          # an element that was never finite, first at tick 3
    a = np.arange(6 * n, dtype=np.float64).reshape(6, n, 1)
    got = HipExec._extremes_dict(["world_pos", "a"], [pos, a])
    assert list(got) == ["world_pos", "a"]
    for name, raw in (("world_pos", pos), ("a", a)):
        d = got[name]
        assert sorted(d) == ["argmax", "argmin", "count", "first_nonfinite", "max", "min"]
        for key, plane in (("count", 0), ("argmin", 2), ("argmax", 4), ("first_nonfinite", 5)):
            assert d[key].dtype == np.int64 and d[key].shape == raw.shape[1:], (name, key)
            assert np.array_equal(d[key], raw[plane].astype(np.int64)), (name, key)
        for key, plane in (("min", 1), ("max", 3)):
            assert d[key].dtype == np.float64 and d[key].shape == raw.shape[1:], (name, key)
            assert np.array_equal(d[key], raw[plane], equal_nan=True), (name, key)
    d = got["world_pos"]
    assert d["argmin"][0, 0] == 2 ** 53 - 1                       # ticks survive the double exactly
    assert np.signbit(d["min"][0, 0]) and d["min"][0, 0] == 0.0   # -0.0 stays -0.0
    assert d["count"][1, 2] == 0 and np.isnan(d["min"][1, 2]) and np.isnan(d["max"][1, 2])
    assert d["argmin"][1, 2] == 0 and d["argmax"][1, 2] == 0 and d["first_nonfinite"][1, 2] == 3
