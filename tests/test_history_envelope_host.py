"""sixdof_history_envelope (csrc/sixdof_capi.cpp) without a GPU, under AddressSanitizer + UBSan: built with g++ against the fake
runtime (csrc/hip_fake.cpp), whose launcher computes the real reduction through csrc/envelope_plan.hpp in the kernels' geometry
and merge order, and driven by csrc/envelope_host_test.cpp — values against a long-double two-pass reference, every refusal
with nothing copied, bit-identity of a range's samples with single-sample reads, every fallible runtime call failed once."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "elodin_amd" / "csrc"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_envelope_entry_point_over_the_fake_runtime():
    build = subprocess.run(["make", "-C", str(CSRC), "envelope_test"], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(CSRC / "build" / "envelope_host_test")], capture_output=True, text=True, timeout=120,
                         env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert "envelope_host_test: ok" in run.stdout, run.stdout[-500:]
    faults = re.findall(r"envelope_host_test: (\d+) fallible calls", run.stdout)     # the envelope sweep, then the watch sweep
    assert len(faults) == 2 and all(int(f) >= 15 for f in faults), run.stdout[-500:]      # allocations, launches, copies, events, waits
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
