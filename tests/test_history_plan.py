"""The read side of the telemetry ring as pure host arithmetic (csrc/history_plan.hpp): which sampled ranges
(first_tick, n_samples, every) are wholly in the ring, at the rule's edges, and the slot of every sample of wrapping, strided
ranges against a twin that simulates the recorder slot by slot.  csrc/history_plan_test.cpp; no GPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "elodin_amd" / "csrc"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_history_plan():
    build = subprocess.run(["make", "-C", str(CSRC), "history_plan_test"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(CSRC / "build" / "history_plan_test")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "history plan test ok" in run.stdout, (run.stdout[-500:], run.stderr[-2000:])
