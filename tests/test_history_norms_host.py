"""sixdof_history_norms (csrc/sixdof_capi.cpp) without a GPU, under AddressSanitizer + UBSan: built with g++ (-ffp-contract=off, as
the kernels are compiled without FMA contraction) against the fake runtime (csrc/hip_fake.cpp), whose launcher walks and merges
through csrc/norms_plan.hpp — the value function and the walk the kernel calls — and csrc/extremes_plan.hpp's rule in the kernels'
time segments, and driven by csrc/norms_host_test.cpp, a stand-alone program: the value function bitwise against a plain loop
(count 1 to 4, with and without MINUS, f32 and f64, +-0, denormals, overflowing squares, NaN, +-inf), the rule over every cut of
random and crafted sequences into 2 and 3 parts, every plane bitwise against a plain loop over the ring, one call against the same
range in 2 and 3 CONTINUE calls and under forced segment counts, every refusal with nothing copied and the accumulator untouched,
the conditions of SIXDOF_NORMS_CONTINUE, every fallible runtime call failed once.

The constants, the probe struct, the Norm -> probe conversion and the raw planes -> dict conversion of HipExec.history_norms are
pinned here too: they need no device."""
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
def test_norms_entry_point_over_the_fake_runtime():
    build = subprocess.run(["make", "-C", str(CSRC), "norms_test"], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(CSRC / "build" / "norms_host_test")], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert "norms_host_test: ok" in run.stdout, run.stdout[-500:]
    values = re.findall(r"norms_host_test: (\d+) (f32|f64) values agree", run.stdout)
    assert sorted(kind for _, kind in values) == ["f32", "f64"] and all(int(count) >= 50_000 for count, _ in values), run.stdout[-500:]
    merges = re.findall(r"norms_host_test: (\d+) merges of every cut", run.stdout)
    assert len(merges) == 1 and int(merges[0]) >= 10_000, run.stdout[-500:]
    faults = re.findall(r"norms_host_test: (\d+) fallible calls", run.stdout)
    assert len(faults) == 1 and int(faults[0]) >= 12, run.stdout[-500:]      # allocations, two launches, copies, events, waits
    assert len(re.findall(r"^refusal: ", run.stdout, flags=re.M)) >= 40, run.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]


def test_constants_struct_and_symbol_match_the_header():
    from elodin_amd import _lib as L
    header = (ROOT / "include" / "sixdof_hip.h").read_text()
    want = {"NORM_MINUS": L.NORM_MINUS, "NORM_MAX_COUNT": L.NORM_MAX_COUNT, "NORMS_ASYNC": L.NORMS_ASYNC, "NORMS_CONTINUE": L.NORMS_CONTINUE,
            "NORMS_HOLD": L.NORMS_HOLD, "NORMS_PLANES": L.NORMS_PLANES, "NORMS_MAX_PROBES": L.NORMS_MAX_PROBES}
    for name, value in want.items():
        found = re.findall(rf"#define SIXDOF_{name}\s+(\d+)u?\s", header)
        assert found == [str(value)], (name, found)
    assert (L.NORM_MINUS, L.NORM_MAX_COUNT, L.NORMS_ASYNC, L.NORMS_CONTINUE, L.NORMS_HOLD, L.NORMS_PLANES, L.NORMS_MAX_PROBES) == (1, 4, 1, 2, 4, 6, 8)
    assert C.sizeof(L.NormProbe) == 40
    assert [(n, getattr(L.NormProbe, n).offset) for n, _ in L.NormProbe._fields_] == [
        ("component_id", 0), ("minus_component_id", 8), ("element", 16), ("minus_element", 20), ("group", 24), ("minus_group", 28), ("count", 32), ("flags", 36)]
    assert "sixdof_history_norms" in L.SYMBOLS and len(L.SYMBOLS["sixdof_history_norms"][1]) == 9
    # the struct as the header spells it: two 64-bit ids, then six 32-bit fields in this order
    body = re.search(r"typedef struct sixdof_norm_probe \{(.*?)\} sixdof_norm_probe;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in L.NormProbe._fields_]


def test_norms_become_probes():
    import elodin_amd as ea
    from elodin_amd import _lib as L
    from elodin_amd.exec import HipExec
    assert ea.Norm is __import__("elodin_amd.exec", fromlist=["Norm"]).Norm and "Norm" in ea.__all__
    arr = HipExec._norm_probes([ea.Norm("world_vel", 3, 3), ea.Norm("world_pos", 4, 3, group=1, minus="world_pos", minus_group=0),
                                ea.Norm("world_pos", 0, 4, 2, "world_vel", 1, 3), ea.Norm("force", 5, 1, minus="force")])
    fields = lambda p: (p.component_id, p.minus_component_id, p.element, p.minus_element, p.group, p.minus_group, p.count, p.flags)
    pos, vel, force = (L.component_id(n) for n in ("world_pos", "world_vel", "force"))
    assert len(arr) == 4
    assert fields(arr[0]) == (vel, 0, 3, 0, 0, 0, 3, 0)                         # without minus the minus_ fields stay 0
    assert fields(arr[1]) == (pos, pos, 4, 4, 1, 0, 3, L.NORM_MINUS)            # minus_element defaults to element
    assert fields(arr[2]) == (pos, vel, 0, 1, 2, 3, 4, L.NORM_MINUS)
    assert fields(arr[3]) == (force, force, 5, 5, 0, 0, 1, L.NORM_MINUS)        # a row against itself: both default
    assert len(HipExec._norm_probes(ea.Norm("force", 0, 1))) == 1
    assert len(HipExec._norm_probes([ea.Norm("force", 0, 1)] * 8)) == 8
    for bad in ([], [ea.Norm("force", 0, 1)] * 9, [ea.Norm("force", 0, 0)], [ea.Norm("force", 0, 5)], [ea.Norm("force", 0, 1, minus_element=2)],
                [ea.Norm("force", 0, 1, minus_group=1)], [ea.Norm("force", -1, 1)], [ea.Norm("force", 0, 1, group=-1)],
                [ea.Norm("force", 0, 1, minus="force", minus_group=-1)]):
        with pytest.raises(ValueError):
            HipExec._norm_probes(bad)


def test_raw_planes_become_the_dict_of_history_norms():
    from elodin_amd.exec import HipExec
    runs = 3
    raw = np.empty((2, 6, runs))
    raw[0] = [[2.0 ** 53 - 1, 0.0, 7.0], [0.0, np.nan, 2.25], [2.0 ** 53 - 2, 0.0, 3.0], [4.0, np.nan, 1e300], [2.0 ** 53 - 1, 0.0, 9.0],
              [0.0, 2.0 ** 53 - 3, 5.0]]
    raw[1] = np.arange(6 * runs, dtype=np.float64).reshape(6, runs)
    got = HipExec._norms_dict(raw)
    assert sorted(got) == ["argmax", "argmin", "count", "first_nonfinite", "max", "max_sq", "min", "min_sq"]
    for key, plane in (("count", 0), ("argmin", 2), ("argmax", 4), ("first_nonfinite", 5)):
        assert got[key].dtype == np.int64 and got[key].shape == (2, runs)
        assert np.array_equal(got[key], raw[:, plane].astype(np.int64))
    for key, plane in (("min_sq", 1), ("max_sq", 3)):
        assert got[key].dtype == np.float64 and got[key].shape == (2, runs)
        assert np.array_equal(got[key], raw[:, plane], equal_nan=True)
    assert got["count"][0, 0] == 2 ** 53 - 1 and got["argmin"][0, 0] == 2 ** 53 - 2 and got["argmax"][0, 0] == 2 ** 53 - 1      # exact near 2^53
    assert got["first_nonfinite"][0, 1] == 2 ** 53 - 3
    assert np.array_equal(got["min"], np.sqrt(raw[:, 1]), equal_nan=True) and np.array_equal(got["max"], np.sqrt(raw[:, 3]), equal_nan=True)
    assert got["min"][0, 2] == 1.5 and got["max"][0, 0] == 2.0 and got["max"][0, 2] == 1e150 and np.isnan(got["min"][0, 1]) and np.isnan(got["max"][0, 1])
    assert got["min"][0, 0] == 0.0 and not np.signbit(got["min"][0, 0])
