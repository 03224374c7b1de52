"""Where the built-in step kernels fetch their arguments and their aux rows, read off the machine code of the built library.

At one tick per launch the launch is a latency chain, and the scalar cache is empty at every launch: an argument fetched where
it is first used is a miss that the wave waits for on its own, and aux loads split by a wait pay a second memory round trip.
csrc/step_kernel.hpp (read_entry_args, load_aux) therefore reads every argument in the entry block and issues the loads of the
aux rows back to back beside the slab DMA.  This pins both on EVERY instantiation of sixdof_step_kernel in the library (84:
f64 / f32, RK4 / semi-implicit / accel-check, the five compile-time pipes and the interpreter, three cache policies), and says
which of them do not reach the shape.  It looks for ordinary scalar loads, vector loads and waits only.

In linear instruction order:
  * the window from the first `global_load_lds_*` (the slab DMA) to the first `ds_read*` (the lanes fetch their rows):
      (a) holds no `s_load_*`;
      (b) every `global_load_*` in it (the DMA, the aux rows) comes before every `s_waitcnt` in it that names vmcnt;
  * the last-tick body.  Where the compiler puts the copies of the tick body is its own business, so the body is not
    delimited by position: it is everything behind the first `ds_read`, to the end of the kernel.
      (c) it holds no `s_load_*`, except a run of consecutive scalar loads that re-reads the history ring's arguments
          (hist_ring .. hist_force, StepParams 0x4c..0x77, and n at 0x28, the ring's row stride) AND in which at least one load
          reads an argument that only a recording launch uses (hist_slot0, hist_vel, hist_accel, hist_force, n).  hist_ring and
          hist_pos decide `record` in every launch, so on their own they are not excused.  Such a run sits inside
          `if (record)`: the register allocator prefers fetching these again to keeping them over a thousand instructions.

Instantiations that do not reach the shape, and what is asked of them instead:
  * the semi-implicit interpreter (6 kernels): so short of scalar registers that an entry burst is thrown away whole.  It
    keeps the parent's fetch-on-demand code (kEntryArgs in the kernel); only (b) is asked of it.
  * gravity | drag under RK4 (8 kernels): (a) and (b) hold; behind the first `ds_read` the drag's three constants
    (ops[1].p[0..2], 0xd8..0xef) are fetched again in front of the tick body.  Nothing else may be.
  * the accel-check kernels (12, one launch per upload): the tick count (0x2c) is read again after the check tick.  Nothing
    else may be (the drag's constants in the drag's check kernel, as above).
"""
import re
from functools import lru_cache
from pathlib import Path

import pytest

from elodin_amd import isa_check

LIB = Path(isa_check.__file__).resolve().parent / "libsixdof_hip.so"
# sixdof_step_kernel<double, kRk4 = 0, PIPE, kPolNtStores = 1, CHECK = false, ROWS = 64>
KERNELS = {
    "gravity_torque": "_ZN6sixdof18sixdof_step_kernelIdLi0ENS_10PipeStaticIJLi2ELi3EEEELi1ELb0ELi64EEEvNS_10StepParamsE",
    "interpreter": "_ZN6sixdof18sixdof_step_kernelIdLi0ENS_11PipeGenericELi1ELb0ELi64EEEvNS_10StepParamsE",
}


@lru_cache(maxsize=None)
def instructions(lib=LIB):
    """{kernel name: [mnemonic and operands, ...]} of the step kernels in `lib`, labels and comments dropped."""
    out = {}
    for name, lines in isa_check.kernels(isa_check.disassemble(lib)).items():
        if "sixdof_step_kernel" not in name:
            continue
        insts = [ln.split("//")[0].strip() for ln in lines if not re.match(r"^<L\d+>:$", ln.strip())]
        out[name] = [s for s in insts if s]
    return out


def findings(insts, allowed=()):
    """What the kernel's instruction list has against the three rules of the module docstring (empty: nothing).
    allowed: [(lo, hi)] StepParams byte ranges this instantiation may fetch again behind the first ds_read."""
    op = [s.split()[0] for s in insts]
    dma = next((i for i, o in enumerate(op) if o.startswith("global_load_lds_")), None)
    if dma is None:
        return ["no global_load_lds_* instruction: not the slab-DMA kernel this test is about"]
    rows = next((i for i in range(dma, len(op)) if op[i].startswith("ds_read")), None)
    if rows is None:
        return ["no ds_read* behind the slab DMA"]
    bad = [f"(a) scalar load between the slab DMA and the first ds_read: `{insts[i]}` at {i}"
           for i in range(dma, rows) if op[i].startswith("s_load_")]
    waits = [i for i in range(dma, rows) if op[i] == "s_waitcnt" and "vmcnt" in insts[i]]
    loads = [i for i in range(dma, rows) if op[i].startswith("global_load_")]
    if not waits:
        bad.append("(b) no vmcnt wait between the slab DMA and the first ds_read")
    bad += [f"(b) `{insts[i]}` at {i} is issued behind the vmcnt wait at {waits[0]}" for i in loads if waits and i > waits[0]]
    i = rows
    while i < len(op):
        if not op[i].startswith("s_load_"):
            i += 1
            continue
        j = i
        while j < len(op) and op[j].startswith("s_load_"):
            j += 1
        run = [kernarg_range(insts[k]) for k in range(i, j)]            # a run of consecutive scalar loads
        recording = any(r and within(r, RING_ARGUMENTS) and overlaps(r, RECORDING_ONLY) for r in run)
        bad += [f"(c) last-tick body: scalar load of a non-ring argument: `{insts[k]}` at {k}"
                for k, r in zip(range(i, j), run) if not (r and (within(r, allowed) or (recording and within(r, RING_ARGUMENTS))))]
        i = j
    return bad


RING_ARGUMENTS = [(0x28, 0x2c), (0x4c, 0x78)]      # n | hist_ring, hist_slot0, hist_pos, hist_vel, hist_accel, hist_force (kernels.hpp)
RECORDING_ONLY = [(0x28, 0x2c), (0x50, 0x58), (0x60, 0x78)]      # of these, what only `if (record)` regions read: not hist_ring, hist_pos
N_TICKS = [(0x2c, 0x30)]
DRAG_CONSTANTS = [(0xd8, 0xf0)]                     # ops[1].p[0..2]


def kernarg_range(inst):
    """(lo, hi) byte range of `s_load_dword[xN] sD, s[..], 0xOFF`, None for any other addressing form (never excused)."""
    m = re.match(r"^s_load_dword(?:x(\d+))?\s+\S+,\s*s\[\d+:\d+\],\s*(0x[0-9a-f]+|\d+)\s*$", inst)
    if not m:
        return None
    lo = int(m.group(2), 0)
    return lo, lo + 4 * int(m.group(1) or 1)


def within(r, ranges):
    return any(a <= r[0] and r[1] <= b for a, b in ranges)


def overlaps(r, ranges):
    return any(r[0] < b and a < r[1] for a, b in ranges)


NAME = re.compile(r"^_ZN6sixdof18sixdof_step_kernelI([df])Li(\d)ENS_(?:10PipeStaticIJ((?:Li\d+E)*)EEE|11PipeGenericE)Li(\d+)ELb([01])ELi64EEEvNS_10StepParamsE$")


def expectation(name):
    """(rules asked of this instantiation, extra StepParams ranges it may fetch again) — the module docstring's list."""
    m = NAME.match(name)
    assert m, f"not a step kernel name this test can read: {name}"
    dtype, integrator, kinds, _policy, check = m.groups()
    interpreter = kinds is None
    if interpreter and integrator == "1":
        return "b", []
    allowed = []
    if check == "1":
        allowed += N_TICKS
    if kinds == "Li2ELi5E" and integrator == "0":
        allowed += DRAG_CONSTANTS
    return "abc", allowed


def check(name, insts):
    rules, allowed = expectation(name)
    return [f for f in findings(insts, allowed) if f[1] in rules or not f.startswith("(")]


def test_every_instantiation_is_checked():
    names = [n for n in instructions() if NAME.match(n)]
    assert len(names) == 84 and all(n in names for n in KERNELS.values()), len(names)
    asked = [expectation(n) for n in names]
    assert sum(r == "b" for r, _ in asked) == 6 and sum(r == "abc" and not a for r, a in asked) == 60


def test_arguments_are_read_at_entry_and_aux_rows_beside_the_slab_dma_in_every_instantiation():
    assert LIB.exists(), f"{LIB} is not built"
    bad = {n: check(n, insts) for n, insts in instructions().items() if NAME.match(n)}
    bad = {n: f for n, f in bad.items() if f}
    assert not bad, "\n".join(f"{n}:\n  " + "\n  ".join(f[:6]) for n, f in bad.items())


@pytest.mark.parametrize("pipe", list(KERNELS))
def test_arguments_are_read_at_entry_and_aux_rows_beside_the_slab_dma(pipe):
    assert LIB.exists(), f"{LIB} is not built"
    insts = instructions().get(KERNELS[pipe])
    assert insts, f"{KERNELS[pipe]} is not in {LIB.name}"
    assert any(s.startswith("s_load_") for s in insts), "no scalar load at all: the disassembly is not what this test reads"
    bad = findings(insts)
    assert not bad, "\n".join(bad)


def test_the_rules_see_a_late_scalar_load_and_a_split_aux_row():
    """The checker on two hand-made instruction lists, so that a rule that can no longer fail is noticed."""
    good = ["s_load_dwordx8 s[16:23], s[0:1], 0x0", "s_waitcnt lgkmcnt(0)", "global_load_lds_dwordx4 v1, s[2:3]",
            "global_load_dwordx4 v[4:7], v[8:9], off", "global_load_dwordx2 v[10:11], v[8:9], off offset:16",
            "s_waitcnt vmcnt(0)", "s_waitcnt vmcnt(0) lgkmcnt(0)", "ds_read_b64 v[2:3], v1", "v_add_f64 v[2:3], v[2:3], v[4:5]",
            "global_store_dwordx4 v[0:1], v[2:5], off", "s_endpgm"]
    assert findings(good) == []
    late = good[:3] + ["s_load_dword s4, s[0:1], 0x40", "s_waitcnt lgkmcnt(0)"] + good[3:]
    assert any(f.startswith("(a)") for f in findings(late))
    split = good[:4] + ["s_waitcnt vmcnt(0)"] + good[4:]
    assert any(f.startswith("(b)") for f in findings(split))
    body = good[:8] + ["s_load_dword s4, s[0:1], 0x84"] + good[8:]
    assert any(f.startswith("(c)") for f in findings(body))
    for late in ("s_load_dwordx2 s[4:5], s[0:1], 0x98", "s_load_dwordx4 s[4:7], s[0:1], 0x70", "s_load_dword s4, s[0:1], 0x2c",
                 "s_load_dword s4, s[2:3], 0x50 glc", "s_load_dword s4, s[0:1], s6"):
        assert any(f.startswith("(c)") for f in findings(good[:8] + [late] + good[8:])), late
    for ring in (["s_load_dwordx2 s[4:5], s[0:1], 0x50"], ["s_load_dwordx8 s[4:11], s[0:1], 0x58"], ["s_load_dword s4, s[0:1], 0x28"],
                 ["s_load_dwordx2 s[4:5], s[0:1], 0x50", "s_load_dword s6, s[0:1], 0x4c"],
                 ["s_load_dword s4, s[0:1], 0x28", "s_load_dwordx2 s[6:7], s[0:1], 0x58"]):
        assert findings(good[:8] + ring + good[8:]) == [], ring
    for alone in ("s_load_dword s4, s[0:1], 0x4c", "s_load_dwordx2 s[4:5], s[0:1], 0x58"):      # they decide `record`: every launch
        assert any(f.startswith("(c)") for f in findings(good[:8] + [alone] + good[8:])), alone
    body = good[:8] + ["s_load_dword s4, s[0:1], 0x2c"] + good[8:]
    assert findings(body, N_TICKS) == [] and findings(body, DRAG_CONSTANTS) != []
