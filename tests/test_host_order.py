"""Stream order, buffer lifetimes and page-lock extents of the host layer (csrc/sixdof_capi.cpp) without a GPU, under
AddressSanitizer + UBSan: built with g++ against the fake runtime's ordered mode (csrc/hip_fake.cpp: every stream a queue that runs
at forcing points only, host destinations poisoned until their copy has run, frees, unlocks and lock extents checked) and driven by
csrc/order_host_test.cpp — the recorded call sequence of a GPU test that once faulted, two reads in flight per reader, growth under
a pending copy, a longer read into the same pointer, blocking after asynchronous, the scans' flags under forced segment counts,
teardown under load and the Python layer's buffer lifetimes, each with everything completing at once and under three lazy
schedules, the same bytes every time."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "elodin_amd" / "csrc"

READERS = ("watch", "stream", "envelope", "quantiles", "covariance", "extremes", "events")
CASES = (["a"] + [f"{c}-{r}" for c in "bcde" for r in READERS]
         + [f"f-{r}-{s}" for r in ("extremes", "events") for s in (1, 2, 6)]
         + [f"g-{op}-{r}" for op in ("set_history", "set_history_0", "bind_columns", "set_watch", "destroy") for r in ("watch", "stream", "envelope")]
         + ["h-envelope", "h-covariance", "h-extremes"])
SCHEDULES = ("at-once", "minimal", "compute-first", "copy-first")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_stream_order_lifetimes_and_lock_extents_over_the_ordered_fake_runtime():
    assert len(CASES) == 53
    build = subprocess.run(["make", "-C", str(CSRC), "order_test"], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    # the program takes 2 s here: four times that for a loaded machine
    run = subprocess.run([str(CSRC / "build" / "order_host_test")], capture_output=True, text=True, timeout=8,
                         env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert "order_host_test: ok" in run.stdout, run.stdout[-500:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    assert "hip_fake:" not in run.stderr, run.stderr[-3000:]                       # no violation, not even a counted one
    lines = re.findall(r"^order: (\S+) (\S+): ok$", run.stdout, flags=re.M)
    assert len(lines) == 212, run.stdout[-3000:]                                   # 53 cases x 4 schedules
    assert sorted(lines) == sorted((c, s) for c in CASES for s in SCHEDULES), run.stdout[-3000:]
