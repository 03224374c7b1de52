"""How many instructions the step kernels spend on moving their slabs, read off the machine code of the built library.

At one tick per launch a launch is 1,024 waves, one per SIMD, and a lone wave's time is its instruction count
(profiles/r04_ubench_issue_mix.md).  csrc/step_kernel.hpp therefore addresses a slab once per column (column base, lane * 16
and, for the LDS-DMA, the column's LDS base in M0) and names the 1-KiB chunks by the instructions' immediate offsets.  This
pins the shape on every instantiation of sixdof_step_kernel in the library (84; all of them move Body slabs), with the
disassembly and the kernel list of tests/test_step_kernel_entry_loads.py.  Rules (1) and (2), the way in, are asked of all 84;
the way out is re-addressed in the RK4 kernels only (the semi-implicit ones keep the one-column flush: it holds the f32
gravity | body_torque kernel at 78 VGPRs and 6 waves per SIMD) and rules (3) and (4) are asked of the benchmark's kernel:

  (1) the number of `global_load_lds_*` instructions is the sum over world_pos, world_vel and inertia of
      ceil(64 * width * sizeof(T) / 1024): 4 + 3 + 4 = 11 for f64, 2 + 2 + 2 = 6 for f32, times ENTRY_COPIES;
  (2) from the first to the last of them: at most one 64-bit vector address computation and at most two M0 writes per column
      (three columns), and no `s_cmp_lg_u64` (the null check of a generic -> LDS pointer cast).  The parent computed an address
      and wrote M0 per chunk: 10 of each in the f64 kernels, and 5 null checks;
  (3) on the benchmark's kernel no flush issues more `global_store_dwordx4` than its column has chunks.  The wave barrier in
      front of a flush is no instruction in a single-wave workgroup, so the disassembly cannot be cut there; a flush is cut
      where it begins instead, at the first `ds_read_b128` behind a `global_store_dwordx4` (a flush reads its column's
      chunks, one `ds_read_b128` each, then stores them).  In every such piece the stores are no more than the reads, a
      piece that read at most 4 chunks (one column) stores at most 4, and the 7-wide column's flush (4 reads, 4 stores) is there.
      The parent split the 7-wide flush by lane class: 3 reads and 3 stores, then 1 read and 4 stores;
  (4) the benchmark kernel's static instruction count is below the parent's 2,272.  This tree: 1,954.  Pinned with 12
      instructions of slack: the test is to catch a return to the old shape, not the compiler's noise.
"""
import re

import pytest

from tests.test_step_kernel_entry_loads import KERNELS, LIB, NAME, instructions

# One copy of the slab DMA per kernel.  The ragged wave (rows < 64, at most one per launch) does not get a top-level copy of
# the kernel: that doubles the benchmark kernel's code.  It branches once around the DMA to its element-wise movers, which sit
# out of line, and under RK4 it stores nothing on the early path and leaves through the late flush that every kernel has anyway.
ENTRY_COPIES = 1
CHUNKS = {"d": 4 + 3 + 4, "f": 2 + 2 + 2}
COLUMNS = 3
PARENT_BENCH_INSTRUCTIONS = 2272
BENCH_INSTRUCTIONS = 1954
SLACK = 12
ADDRESS_64 = ("v_lshl_add_u64", "v_mad_u64_u32", "v_addc_co_u32_e32", "v_addc_co_u32_e64")
BENCH = KERNELS["gravity_torque"]


def code(insts):
    return [s for s in insts if s != "..."]      # the disassembler's mark for the padding behind a function


def dma_findings(dtype, insts):
    """What a kernel's instruction list has against rules (1) and (2) (empty: nothing)."""
    op = [s.split()[0] for s in insts]
    dma = [i for i, o in enumerate(op) if o.startswith("global_load_lds_")]
    bad = []
    if len(dma) != CHUNKS[dtype] * ENTRY_COPIES:
        bad.append(f"(1) {len(dma)} global_load_lds instructions, not {CHUNKS[dtype] * ENTRY_COPIES}")
    if not dma:
        return bad
    window = insts[dma[0]:dma[-1] + 1]
    addresses = [s for s in window if s.split()[0] in ADDRESS_64]
    m0 = [s for s in window if re.match(r"^s_\w+\s+m0,", s)]
    null = [s for s in window if s.startswith("s_cmp_lg_u64")]
    if len(addresses) > COLUMNS:
        bad.append(f"(2) {len(addresses)} 64-bit vector address computations among the slab DMA, e.g. `{addresses[0]}`")
    if len(m0) > 2 * COLUMNS:
        bad.append(f"(2) {len(m0)} M0 writes among the slab DMA")
    if null:
        bad.append(f"(2) {len(null)} null checks of an LDS pointer among the slab DMA: `{null[0]}`")
    return bad


def flushes(insts):
    """[(ds_read_b128 count, global_store_dwordx4 count)] of the pieces that rule (3) cuts the kernel into."""
    out, reads, stores = [], 0, 0
    for s in insts:
        o = s.split()[0]
        if o == "ds_read_b128":
            if stores:
                out.append((reads, stores))
                reads = stores = 0
            reads += 1
        elif o == "global_store_dwordx4":
            stores += 1
    if reads or stores:
        out.append((reads, stores))
    return out


def flush_findings(insts):
    pieces = flushes(insts)
    bad = [f"(3) a flush stores {s} times what it read {r} times" for r, s in pieces if s > r or (r <= 4 and s > 4)]
    if (4, 4) not in pieces:
        bad.append(f"(3) no flush of a 7-wide column with 4 reads and 4 stores: {pieces}")
    return bad


def test_every_instantiation_issues_its_slab_dma_once_per_column():
    assert LIB.exists(), f"{LIB} is not built"
    names = [n for n in instructions() if NAME.match(n)]
    assert len(names) == 84, len(names)
    bad = {n: dma_findings(NAME.match(n).group(1), code(instructions()[n])) for n in names}
    bad = {n: f for n, f in bad.items() if f}
    assert not bad, "\n".join(f"{n}:\n  " + "\n  ".join(f) for n, f in bad.items())


def test_no_flush_of_the_benchmark_kernel_stores_more_than_its_chunks():
    insts = instructions().get(BENCH)
    assert insts, f"{BENCH} is not in {LIB.name}"
    bad = flush_findings(code(insts))
    assert not bad, "\n".join(bad)


def test_the_benchmark_kernel_is_shorter_than_the_parents():
    insts = instructions().get(BENCH)
    assert insts, f"{BENCH} is not in {LIB.name}"
    count = len(code(insts))
    print(f"benchmark kernel: {count} instructions (parent {PARENT_BENCH_INSTRUCTIONS}, pinned {BENCH_INSTRUCTIONS} + {SLACK})")
    assert count < PARENT_BENCH_INSTRUCTIONS
    assert count <= BENCH_INSTRUCTIONS + SLACK, count


def test_the_rules_see_the_parents_shape():
    """The checkers on hand-made instruction lists, so that a rule that can no longer fail is noticed."""
    dma = lambda k, addr="v66, s[48:49]": [f"global_load_lds_dwordx4 {addr} offset:{1024 * i}" for i in range(k)]
    good = ["s_mov_b32 m0, 0"] + dma(3) + ["s_movk_i32 m0, 0xe00"] + dma(3) + ["s_movk_i32 m0, 0x1a00"] + dma(3) + \
           ["s_and_saveexec_b64 s[4:5], vcc", "s_movk_i32 m0, 0x1a00", "s_nop 0"] + dma(1) + ["s_mov_b32 m0, 0", "s_nop 0"] + dma(1) + \
           ["s_or_b64 exec, exec, s[4:5]", "s_endpgm", "..."]
    assert dma_findings("d", code(good)) == []
    assert any(f.startswith("(1)") for f in dma_findings("f", code(good)))
    assert any(f.startswith("(1)") for f in dma_findings("d", code(good + dma(1))))
    old = []
    for i in range(11):      # the parent: an address, a null check and an M0 write per chunk
        old += [f"v_lshl_add_u64 v[2:3], s[48:49], 0, v[{4 + i}:{5 + i}]", "s_cmp_lg_u64 src_shared_base, 0", "s_cselect_b32 m0, s3, -1",
                "s_nop 0", "global_load_lds_dwordx4 v[2:3], off"]
    found = dma_findings("d", old)
    assert sum(f.startswith("(2)") for f in found) == 3 and not any(f.startswith("(1)") for f in found), found
    rd = lambda k: [f"ds_read_b128 v[{4 * i}:{4 * i + 3}], v66 offset:{1024 * i}" for i in range(k)]
    st = lambda k: [f"global_store_dwordx4 v66, v[{4 * i}:{4 * i + 3}], s[2:3] offset:{1024 * i} nt" for i in range(k)]
    assert flush_findings(rd(4) + st(3) + ["s_and_saveexec_b64 s[4:5], vcc"] + st(1) + rd(3) + st(3)) == []
    assert flushes(rd(4) + st(4) + rd(3) + st(3) + rd(7) + st(7)) == [(4, 4), (3, 3), (7, 7)]
    parent = rd(3) + st(3) + rd(1) + st(4) + rd(3) + st(3)      # the 7-wide flush split by lane class
    assert any("stores 4 times what it read 1 times" in f for f in flush_findings(parent))
    assert any("no flush of a 7-wide column" in f for f in flush_findings(rd(3) + st(3)))
    assert any(f.startswith("(3)") for f in flush_findings(rd(4) + st(5)))
