"""sixdof_history_dwell (csrc/sixdof_capi.cpp) without a GPU, under AddressSanitizer + UBSan: built with g++ (-ffp-contract=off, as
the kernels are compiled without FMA contraction) against the fake runtime (csrc/hip_fake.cpp), whose launcher walks and merges
through csrc/dwell_plan.hpp — the value, the walk and the rule the kernels call — in the kernels' time segments, and driven by
csrc/dwell_host_test.cpp, a stand-alone program: the rule against a plain loop (every sequence over {holds, fails, skipped} up to
length 8 and random ones up to 200, every cut into 2 and 3 parts in both association orders, accumulate against the merge of a
one-sample record, crafted ties), value and predicate bitwise against a plain loop (both kinds, all six ops, f32 and f64, MINUS,
+-0 at a level of 0, denormals, an overflowing difference and square, NaN, +-inf, values that equal a level), all twelve planes
against a plain loop over the ring, one call against the same range in 2 and 3 CONTINUE calls and under forced segment counts,
every refusal with nothing copied and the accumulator untouched, the conditions of SIXDOF_DWELL_CONTINUE, every fallible runtime
call failed once.

The constants, the condition struct, the Dwell -> condition conversion and the raw planes -> dict conversion of
HipExec.history_dwell are pinned here too: they need no device."""
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
def test_dwell_entry_point_over_the_fake_runtime():
    build = subprocess.run(["make", "-C", str(CSRC), "dwell_test"], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(CSRC / "build" / "dwell_host_test")], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert "dwell_host_test: ok" in run.stdout, run.stdout[-500:]
    # every sequence over three states up to length 8, and every cut of each into three parts (401,041 cut pairs)
    exhaustive = re.findall(r"dwell_host_test: (\d+) sequences up to length 8, (\d+) cut pairs exhaustively", run.stdout)
    assert exhaustive == [(str(sum(3 ** k for k in range(9))), "401041")], run.stdout[-500:]
    merges = re.findall(r"dwell_host_test: (\d+) merges of every cut", run.stdout)
    assert len(merges) == 1 and int(merges[0]) >= 2 * 401_041, run.stdout[-500:]        # both association orders
    values = re.findall(r"dwell_host_test: (\d+) (f32|f64) values and predicates agree", run.stdout)
    assert sorted(kind for _, kind in values) == ["f32", "f64"] and all(int(count) >= 50_000 for count, _ in values), run.stdout[-500:]
    faults = re.findall(r"dwell_host_test: (\d+) fallible calls", run.stdout)
    assert len(faults) == 1 and int(faults[0]) >= 12, run.stdout[-500:]      # allocations, two launches, copies, events, waits
    assert len(re.findall(r"^refusal: ", run.stdout, flags=re.M)) >= 60, run.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]


def test_constants_struct_and_symbol_match_the_header():
    from elodin_amd import _lib as L
    header = (ROOT / "include" / "sixdof_hip.h").read_text()
    want = {"DWELL_ELEMENT": L.DWELL_ELEMENT, "DWELL_NORM_SQ": L.DWELL_NORM_SQ, "DWELL_INSIDE": L.DWELL_INSIDE, "DWELL_OUTSIDE": L.DWELL_OUTSIDE,
            "DWELL_ASYNC": L.DWELL_ASYNC, "DWELL_CONTINUE": L.DWELL_CONTINUE, "DWELL_HOLD": L.DWELL_HOLD, "DWELL_PLANES": L.DWELL_PLANES,
            "DWELL_MAX_CONDITIONS": L.DWELL_MAX_CONDITIONS}
    for name, value in want.items():
        found = re.findall(rf"#define SIXDOF_{name}\s+(\d+)u?\s", header)
        assert found == [str(value)], (name, found)
    assert (L.DWELL_ELEMENT, L.DWELL_NORM_SQ, L.DWELL_INSIDE, L.DWELL_OUTSIDE, L.DWELL_ASYNC, L.DWELL_CONTINUE, L.DWELL_HOLD, L.DWELL_PLANES,
            L.DWELL_MAX_CONDITIONS) == (0, 1, 4, 5, 1, 2, 4, 12, 8)
    assert (L.EVENT_LT, L.EVENT_LE, L.EVENT_GT, L.EVENT_GE) == (0, 1, 2, 3)        # the one-sided ops, below INSIDE and OUTSIDE
    assert C.sizeof(L.DwellCondition) == 64
    assert [(n, getattr(L.DwellCondition, n).offset) for n, _ in L.DwellCondition._fields_] == [("probe", 0), ("lo", 40), ("hi", 48), ("kind", 56), ("op", 60)]
    assert L.DwellCondition._fields_[0][1] is L.NormProbe and C.sizeof(L.NormProbe) == 40
    assert "sixdof_history_dwell" in L.SYMBOLS and len(L.SYMBOLS["sixdof_history_dwell"][1]) == 9
    # the struct as the header spells it: the probe, two doubles, two 32-bit fields in this order
    body = re.search(r"typedef struct sixdof_dwell_condition \{(.*?)\} sixdof_dwell_condition;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in L.DwellCondition._fields_]


def test_dwells_become_conditions():
    import elodin_amd as ea
    from elodin_amd import _lib as L
    from elodin_amd.exec import HipExec
    exec_module = __import__("elodin_amd.exec", fromlist=["Dwell"])
    assert ea.Dwell is exec_module.Dwell and ea.Element is exec_module.Element and "Dwell" in ea.__all__ and "Element" in ea.__all__
    arr = HipExec._dwell_conditions([
        ea.Dwell(ea.Element("world_pos", 6), ">", 120.5),
        ea.Dwell(ea.Element("world_pos", 4, group=1, minus="world_pos", minus_group=0), "inside", -2.0, 3.0),
        ea.Dwell(ea.Element("world_vel", 5, 2, "force", 1, 3), "outside", -1.0, -1.0),
        ea.Dwell(ea.Norm("world_vel", 3, 3), "<=", 1.5),
        ea.Dwell(ea.Norm("world_pos", 4, 3, 0, "world_pos", 4, 1), "inside", 0.0, 3.0),
        ea.Dwell(ea.Norm("world_pos", 0, 4), "outside", 0.5, 2.0),
        ea.Dwell(ea.Element("force", 0), "<", -0.0),
        ea.Dwell(ea.Norm("force", 0, 1), ">=", 0.0)])
    fields = lambda c: (c.kind, c.op, c.lo, c.hi)
    probe = lambda c: (c.probe.component_id, c.probe.minus_component_id, c.probe.element, c.probe.minus_element, c.probe.group, c.probe.minus_group,
                       c.probe.count, c.probe.flags)
    pos, vel, force = (L.component_id(n) for n in ("world_pos", "world_vel", "force"))
    assert len(arr) == 8
    assert fields(arr[0]) == (L.DWELL_ELEMENT, L.EVENT_GT, 120.5, 0.0) and probe(arr[0]) == (pos, 0, 6, 0, 0, 0, 1, 0)     # an Element: kind 0, count 1, levels as they are
    assert fields(arr[1]) == (L.DWELL_ELEMENT, L.DWELL_INSIDE, -2.0, 3.0) and probe(arr[1]) == (pos, pos, 4, 4, 1, 0, 1, L.NORM_MINUS)
    assert fields(arr[2]) == (L.DWELL_ELEMENT, L.DWELL_OUTSIDE, -1.0, -1.0) and probe(arr[2]) == (vel, force, 5, 1, 2, 3, 1, L.NORM_MINUS)
    assert fields(arr[3]) == (L.DWELL_NORM_SQ, L.EVENT_LE, 2.25, 0.0) and probe(arr[3]) == (vel, 0, 3, 0, 0, 0, 3, 0)          # a Norm: kind 1, squared levels
    assert fields(arr[4]) == (L.DWELL_NORM_SQ, L.DWELL_INSIDE, 0.0, 9.0) and probe(arr[4]) == (pos, pos, 4, 4, 0, 1, 3, L.NORM_MINUS)
    assert fields(arr[5]) == (L.DWELL_NORM_SQ, L.DWELL_OUTSIDE, 0.25, 4.0) and probe(arr[5])[6] == 4
    assert fields(arr[6]) == (L.DWELL_ELEMENT, L.EVENT_LT, 0.0, 0.0) and fields(arr[7]) == (L.DWELL_NORM_SQ, L.EVENT_GE, 0.0, 0.0)
    assert [Dwell_op for Dwell_op in ea.Dwell.OPS] == ["<", "<=", ">", ">=", "inside", "outside"]
    assert len(HipExec._dwell_conditions(ea.Dwell(ea.Element("force", 0), ">", 1.0))) == 1
    assert len(HipExec._dwell_conditions([ea.Dwell(ea.Element("force", 0), ">", 1.0)] * 8)) == 8
    el, nm = ea.Element("force", 0), ea.Norm("force", 0, 2)
    for bad in ([], [ea.Dwell(el, ">", 1.0)] * 9, [ea.Dwell(el, "==", 1.0)], [ea.Dwell(el, ">", 1.0, 2.0)], [ea.Dwell(el, "inside", 1.0)],
                [ea.Dwell(el, "outside", 1.0)], [ea.Dwell(el, "inside", 2.0, 1.0)], [ea.Dwell(el, ">", float("nan"))], [ea.Dwell(el, ">", float("inf"))],
                [ea.Dwell(el, "inside", 0.0, float("inf"))], [ea.Dwell(nm, ">", -1.0)], [ea.Dwell(nm, "inside", -1.0, 1.0)], [ea.Dwell(nm, ">", 1e200)],
                [ea.Dwell(nm, "outside", 1.0, 1e200)], [ea.Dwell("force", ">", 1.0)], [ea.Dwell(ea.Element("force", -1), ">", 1.0)],
                [ea.Dwell(ea.Element("force", 0, group=-1), ">", 1.0)], [ea.Dwell(ea.Element("force", 0, minus_element=2), ">", 1.0)],
                [ea.Dwell(ea.Norm("force", 0, 5), ">", 1.0)], [ea.Dwell(ea.Norm("force", 0, 0), ">", 1.0)]):
        with pytest.raises(ValueError):
            HipExec._dwell_conditions(bad)


def test_raw_planes_become_the_dict_of_history_dwell():
    from elodin_amd.exec import HipExec
    runs, top = 3, 2.0 ** 53
    raw = np.zeros((2, 12, runs))
    #            count    held     entries  first    last     pre_len  pre_end  suf_len  suf_start longest  l_start  l_end
    raw[0, :, 0] = [top - 1, top - 2, 1.0,    2.0,     top - 1, 0.0,     0.0,     top - 2, 2.0,      top - 2, 2.0,     top - 1]      # values near 2^53
    raw[0, :, 1] = 0.0                                                                                                          # no finite sample
    raw[0, :, 2] = [8.0,     5.0,     3.0,    10.0,    31.0,    2.0,     13.0,    1.0,     31.0,     2.0,     10.0,    13.0]
    raw[1] = np.arange(12 * runs, dtype=np.float64).reshape(12, runs)
    got = HipExec._dwell_dict(raw)
    assert sorted(got) == ["count", "entries", "first_held", "fraction", "held", "last_held", "longest", "longest_end", "longest_start", "open_at_end", "open_at_start"]
    for key, plane in (("count", 0), ("held", 1), ("entries", 2), ("first_held", 3), ("last_held", 4), ("longest", 9), ("longest_start", 10), ("longest_end", 11)):
        assert got[key].dtype == np.int64 and got[key].shape == (2, runs)
        assert np.array_equal(got[key], raw[:, plane].astype(np.int64))
    assert got["count"][0, 0] == 2 ** 53 - 1 and got["held"][0, 0] == 2 ** 53 - 2 and got["last_held"][0, 0] == 2 ** 53 - 1      # exact near 2^53
    assert got["longest"][0, 0] == 2 ** 53 - 2 and got["longest_end"][0, 0] == 2 ** 53 - 1
    for key, plane in (("open_at_start", 5), ("open_at_end", 7)):
        assert got[key].dtype == np.bool_ and got[key].shape == (2, runs) and np.array_equal(got[key], raw[:, plane] > 0)
    assert got["open_at_start"][0].tolist() == [False, False, True] and got["open_at_end"][0].tolist() == [True, False, True]
    assert got["fraction"].dtype == np.float64 and got["fraction"].shape == (2, runs)
    assert got["fraction"][0, 0] == (2.0 ** 53 - 2) / (2.0 ** 53 - 1) and np.isnan(got["fraction"][0, 1]) and got["fraction"][0, 2] == 5 / 8
    assert np.isnan(got["fraction"][1, 0]) and got["fraction"][1, 1] == 4.0 and got["count"][0, 1] == 0      # count == 0: NaN
