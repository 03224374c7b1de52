"""The C ABI's host layer (csrc/sixdof_capi.cpp: handle, setters, copy lane, history ring, watch lists) under AddressSanitizer + UBSan
without a GPU: built with g++ against a fake runtime (csrc/hip_fake.cpp) and a host-only generated program
(csrc/capi_fake_program.cpp), and driven by csrc/capi_lifecycle_test.cpp — one scenario over the whole ABI, run once per fallible
runtime call with that call failing, plus the three failure paths that used to corrupt a handle (double free after a failed
re-bind, a copy lane that never recovered, edge tables that disagreed after a failed sixdof_set_edges)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "elodin_amd" / "csrc"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_handle_survives_every_failed_runtime_call():
    build = subprocess.run(["make", "-C", str(CSRC), "capi_test"], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(CSRC / "build" / "capi_lifecycle_test"), str(CSRC / "build" / "capi_fake_program.so")],
                         capture_output=True, text=True, timeout=120,
                         env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    ok = re.search(r"capi_lifecycle_test: ok \(3 named cases; N = (\d+) fallible calls", run.stdout)
    assert ok and int(ok.group(1)) > 100, run.stdout[-500:]      # the scenario makes well over a hundred calls that can fail
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
