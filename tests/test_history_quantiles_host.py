"""sixdof_history_quantiles (csrc/sixdof_capi.cpp) without a GPU, under AddressSanitizer + UBSan: built with g++ against the fake
runtime (csrc/hip_fake.cpp), whose launcher selects through csrc/quantile_plan.hpp — the keys, the scan step and the lo -> hi rule
the kernels run — and driven by csrc/quantile_host_test.cpp: every value bitwise against std::sort on the keys over random and
crafted blocks, every refusal with nothing copied, bit-identity of a range's samples with single-sample reads, a range cut into
several launches, every fallible runtime call failed once."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "elodin_amd" / "csrc"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_quantile_entry_point_over_the_fake_runtime():
    build = subprocess.run(["make", "-C", str(CSRC), "quantile_test"], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(CSRC / "build" / "quantile_host_test")], capture_output=True, text=True, timeout=120,
                         env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert "quantile_host_test: ok" in run.stdout, run.stdout[-500:]
    faults = re.findall(r"quantile_host_test: (\d+) fallible calls", run.stdout)
    assert len(faults) == 1 and int(faults[0]) >= 15, run.stdout[-500:]      # allocations, clears, launches, copies, events, waits
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
