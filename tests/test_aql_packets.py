"""The AQL packet builder of the step chains (csrc/aql_packets.cpp), as pure host code: header bits and fence scopes by position
in the chain, grid in work-items, segment sizes, argument-block address and alignment, ring wrap-around and flow control on the
read index.  csrc/aql_packet_test.cpp drives it through a fake ring; no GPU, no HSA runtime.  The same binary checks the batch
plan (csrc/step_plan.hpp) against the launch counts the GPU tests pin."""
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "elodin_amd" / "csrc"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_packet_builder():
    build = subprocess.run(["make", "-C", str(CSRC), "aql_test"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(CSRC / "build" / "aql_packet_test")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "aql packet test ok" in run.stdout, (run.stdout[-500:], run.stderr[-2000:])
