"""sixdof_history_covariance (csrc/sixdof_capi.cpp) without a GPU, under AddressSanitizer + UBSan: built with g++ against the fake
runtime (csrc/hip_fake.cpp), whose launcher reduces through csrc/covariance_plan.hpp — the update, the merge, the geometry and
the merge order the kernels run, compiled without FMA contraction as they are — and driven by csrc/covariance_host_test.cpp:
update and merge against a long-double two-pass reference under the GPU tests' bounds, merging with the empty record, a channel
listed twice, the entry point bit for bit against a serial walk of the plan over row counts, periods, channel counts and both
dtypes, forced small sample chunks, every refusal with nothing copied, every fallible runtime call failed once.

The constants, the channel struct, the raw -> dict conversion of HipExec.history_covariance and dispersion_ellipse are pinned here
too: they need no device."""
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
def test_covariance_entry_point_over_the_fake_runtime():
    build = subprocess.run(["make", "-C", str(CSRC), "covariance_test"], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(CSRC / "build" / "covariance_host_test")], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert "covariance_host_test: ok" in run.stdout, run.stdout[-500:]
    worst = re.findall(r"arithmetic: worst error / bound: mean ([\d.]+), co-moment ([\d.]+)", run.stdout)
    assert len(worst) == 1 and float(worst[0][0]) <= 1.0 and float(worst[0][1]) <= 1.0, run.stdout[-500:]
    faults = re.findall(r"covariance_host_test: (\d+) fallible calls", run.stdout)
    assert len(faults) == 1 and int(faults[0]) >= 10, run.stdout[-500:]      # allocations, two launches, copies, events, waits
    refusals = re.findall(r"^refusal: ([^:]+): ", run.stdout, flags=re.M)
    for what in ("every = 0", "period = 0", "period does not divide n", "no channel", "one channel", "seven channels", "null channels", "null buffer",
                 "element beyond the width", "reserved != 0", "fallen out of the ring", "unknown flags", "inertia is not recorded", "no ring",
                 "period beyond the limit"):
        assert what in refusals, (what, run.stdout[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]


def test_constants_struct_and_symbol_match_the_header():
    from elodin_amd import _lib as L
    header = (ROOT / "include" / "sixdof_hip.h").read_text()
    for name, value in {"COVARIANCE_ASYNC": L.COVARIANCE_ASYNC, "COVARIANCE_MAX_CHANNELS": L.COVARIANCE_MAX_CHANNELS}.items():
        found = re.findall(rf"#define SIXDOF_{name}\s+(\d+)u?\s", header)
        assert found == [str(value)], (name, found)
    assert (L.COVARIANCE_ASYNC, L.COVARIANCE_MAX_CHANNELS) == (1, 6)
    plan = (CSRC / "covariance_plan.hpp").read_text()
    assert re.findall(r"#define SIXDOF_COVARIANCE_THREADS (\d+)", plan) == [str(L.COVARIANCE_MAX_PERIOD)]
    assert "kCovarianceMaxPeriod = kCovarianceThreads" in plan
    assert C.sizeof(L.CovChannel) == 16
    assert [(n, getattr(L.CovChannel, n).offset) for n, _ in L.CovChannel._fields_] == [("component_id", 0), ("element", 8), ("reserved", 12)]
    assert re.search(r"uint64_t component_id;\s+uint32_t element;[^\n]*\n\s+uint32_t reserved;[^\n]*\n} sixdof_cov_channel;", header)
    assert "sixdof_history_covariance" in L.SYMBOLS and len(L.SYMBOLS["sixdof_history_covariance"][1]) == 9
    assert re.search(r"int sixdof_history_covariance\(sixdof_handle\* h, const sixdof_cov_channel\* channels, size_t n_channels, uint64_t first_tick,\s+"
                     r"uint64_t n_samples, uint64_t every, uint32_t period, double\* host_dst, uint32_t flags\);", header)


def test_raw_entries_become_the_dict_of_history_covariance():
    from elodin_amd.exec import HipExec
    assert [HipExec.covariance_fields(k) for k in (2, 3, 5, 6)] == [6, 10, 21, 28]
    k = 3
    raw = np.empty((2, 2, 10))
    #            count  means            C00  C01   C02  C11  C12   C22
    raw[0, 0] = [4.0, 1.0, -2.0, 0.5,   8.0, -4.0, 0.0, 2.0, 1.0, 16.0]
    raw[0, 1] = [0.0] + [np.nan] * 9                                      # an empty group
    raw[1, 0] = [2.0, 6.4e6, 0.0, 3.0,  0.0, 0.0, 0.0, 0.5, -0.5, 0.5]    # a channel that does not vary; two perfectly anti-correlated
    raw[1, 1] = np.arange(10, dtype=np.float64) + 1.0
    got = HipExec._covariance_dict(raw, k)
    assert sorted(got) == ["comoment", "corr", "count", "cov", "mean"]
    assert got["count"].dtype == np.int64 and got["count"].tolist() == [[4, 0], [2, 1]]
    assert got["mean"].shape == (2, 2, k) and np.array_equal(got["mean"], raw[:, :, 1:4], equal_nan=True)
    for key in ("comoment", "cov", "corr"):
        assert got[key].shape == (2, 2, k, k) and got[key].dtype == np.float64
        assert np.array_equal(got[key], np.swapaxes(got[key], -1, -2), equal_nan=True), key     # symmetric, bit for bit
    assert got["comoment"][0, 0].tolist() == [[8.0, -4.0, 0.0], [-4.0, 2.0, 1.0], [0.0, 1.0, 16.0]]
    assert got["comoment"][1, 1].tolist() == [[5.0, 6.0, 7.0], [6.0, 8.0, 9.0], [7.0, 9.0, 10.0]]      # row-major upper triangle
    assert got["cov"][0, 0].tolist() == [[2.0, -1.0, 0.0], [-1.0, 0.5, 0.25], [0.0, 0.25, 4.0]]        # the population form: / count
    assert got["corr"][0, 0].tolist() == [[1.0, -1.0, 0.0], [-1.0, 1.0, 1.0 / math.sqrt(32.0)], [0.0, 1.0 / math.sqrt(32.0), 1.0]]
    for key in ("mean", "comoment", "cov", "corr"):
        assert np.isnan(got[key][0, 1]).all(), key                                                    # count 0: NaN, without a warning
    corr = got["corr"][1, 0]
    assert np.isnan(corr[0]).all() and np.isnan(corr[:, 0]).all()                                      # a zero diagonal: NaN in its row and column
    assert corr[1:, 1:].tolist() == [[1.0, -1.0], [-1.0, 1.0]]
    assert got["cov"][1, 0][0].tolist() == [0.0, 0.0, 0.0]


def test_dispersion_ellipse_on_known_answers():
    import elodin_amd as ea
    major, minor, angle = ea.dispersion_ellipse([[4.0, 0.0], [0.0, 1.0]], prob=1.0 - math.exp(-0.5))      # scale sqrt(-2 ln e^(-1/2)) = 1
    assert abs(major - 2.0) <= 4e-16 and abs(minor - 1.0) <= 2e-16 and angle == 0.0
    scale = math.sqrt(-2.0 * math.log(0.01))
    major, minor, angle = ea.dispersion_ellipse([[2.0, 1.0], [1.0, 2.0]])                                # eigenvalues 3 and 1
    assert abs(major - scale * math.sqrt(3.0)) <= 1e-15 * major and abs(minor - scale) <= 1e-15 * minor and abs(angle - math.pi / 4) <= 1e-16
    major, minor, angle = ea.dispersion_ellipse([[1.0, 0.0], [0.0, 9.0]], prob=1.0 - math.exp(-0.5))      # the major axis is y
    assert abs(major - 3.0) <= 1e-15 and abs(minor - 1.0) <= 1e-15 and abs(angle - math.pi / 2) <= 1e-16
    major, minor, angle = ea.dispersion_ellipse([[2.0, -1.0], [-1.0, 2.0]], prob=1.0 - math.exp(-0.5))
    assert abs(major - math.sqrt(3.0)) <= 1e-15 and abs(minor - 1.0) <= 1e-15 and abs(angle + math.pi / 4) <= 1e-16
    # broadcasting over leading axes; a degenerate matrix is a segment, a zero matrix a point
    stack = np.array([[[[4.0, 0.0], [0.0, 1.0]], [[2.0, 1.0], [1.0, 2.0]], [[1.0, 1.0], [1.0, 1.0]]],
                      [[[0.0, 0.0], [0.0, 0.0]], [[9.0, 0.0], [0.0, 9.0]], [[np.nan, 0.0], [0.0, 1.0]]]])
    major, minor, angle = ea.dispersion_ellipse(stack, prob=1.0 - math.exp(-0.5))
    assert major.shape == minor.shape == angle.shape == (2, 3)
    assert np.allclose(major[0], [2.0, math.sqrt(3.0), math.sqrt(2.0)], rtol=1e-15, atol=0) and np.allclose(minor[0], [1.0, 1.0, 0.0], rtol=1e-15, atol=0)
    assert (major[1, 0], minor[1, 0]) == (0.0, 0.0) and (major[1, 1], minor[1, 1]) == (3.0, 3.0) and np.isnan(major[1, 2])
    for prob in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ea.dispersion_ellipse(np.eye(2), prob=prob)
    for bad in (np.eye(3), np.ones(4), np.ones((2, 2, 3)), 1.0):
        with pytest.raises(ValueError):
            ea.dispersion_ellipse(bad)


def test_channel_lists_are_checked_before_the_library_is_called():
    from elodin_amd.exec import HipExec

    class Stub:      # what _covariance_channels reads of an executor
        _windows = {"w": None}
        _aux = {"a": np.zeros((4, 2))}
        _refuse_window = HipExec._refuse_window
        _recorded_width = HipExec._recorded_width
    stub = Stub()
    for bad in ([], [("world_pos", 4)], [("world_pos", 4)] * 7, [("world_pos", 7), ("world_vel", 0)], [("world_vel", 0), ("world_vel", 6)],
                [("a", 2), ("a", 0)], [("world_vel", -1), ("a", 0)], [("w", 0), ("a", 0)]):
        with pytest.raises(ValueError):
            HipExec._covariance_channels(stub, "history_covariance", bad)
    with pytest.raises(ValueError, match="envelope"):
        HipExec._covariance_channels(stub, "history_covariance", [("world_pos", 4)])
