"""CPU side of fold stages that read their edges from device memory (dsl.Program.trace(fold_tables="device")): no cap on the edge
count, nothing about the graph in the generated text, the walker unchanged, the library's host-side table builder (CSR by source in
spawn order, the lane / wave partition, row checks) and the CLI's sidecar."""
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest

from elodin_amd import _lib as L, codegen, dsl
from elodin_amd import stablehlo as sh
from tests import dsl_numpy, fold_tables_common as ft
from tests.golden import hlo_world_builder as hb
from tests.test_program_folds_host import EDGES, add_one, double, fold_test


def _ring(n):
    return {"e": (list(range(n)), [(i + 1) % n for i in range(n)])}


def test_a_device_flavour_trace_has_no_edge_cap():
    big = {"e": (list(range(70000)), list(range(70000)))}
    tp = dsl.Program([fold_test], dsl.pipe(), []).trace({"x": 1}, fold_edges=big, fold_tables="device")
    fs = tp.fold_stages[0]
    assert tp.fold_tables == "device" and fs.device_tables and tp.device_fold_components == ["e"]
    assert fs.src_rows.dtype == fs.row_start.dtype == fs.dst.dtype == np.uint32
    assert len(fs.dst) == 70000 and np.array_equal(fs.row_start, np.arange(70001)) and np.array_equal(fs.dst, np.arange(70000))
    with pytest.raises(ValueError, match="bake their edges"):                       # the default flavour keeps its cap ...
        dsl.Program([fold_test], dsl.pipe(), []).trace({"x": 1}, fold_edges=big)
    with pytest.raises(ValueError, match='fold_tables="device"'):                  # ... and now names the way out
        dsl.Program([fold_test], dsl.pipe(), []).trace({"x": 1}, fold_edges=big, fold_tables="baked")
    assert dsl.Program([fold_test], dsl.pipe(), []).trace({"x": 1}, fold_edges=EDGES).fold_tables == "baked"
    with pytest.raises(ValueError, match="fold_tables"):
        dsl.Program([fold_test], dsl.pipe(), []).trace({"x": 1}, fold_edges=EDGES, fold_tables="hbm")
    # spawn order per source, as the baked trace builds it
    tp = dsl.Program([fold_test], dsl.pipe(), []).trace({"x": 1}, fold_edges={"e": ([2, 0, 2, 0, 2], [1, 2, 0, 1, 2])}, fold_tables="device")
    fs = tp.fold_stages[0]
    assert fs.src_rows.tolist() == [0, 2] and fs.row_start.tolist() == [0, 2, 5] and fs.dst.tolist() == [2, 1, 1, 0, 2]


def test_the_generated_text_does_not_depend_on_the_graph():
    prog = lambda: dsl.Program([double, fold_test, add_one], dsl.pipe(), [])
    a = codegen.generate_source(prog().trace({"x": 1, "n": 1}, fold_edges=EDGES, fold_tables="device"), "float64", 2)
    b = codegen.generate_source(prog().trace({"x": 1, "n": 1}, fold_edges=_ring(70000), fold_tables="device"), "float64", 2)
    assert a == b
    for name in ("fold0_dst[", "fold0_start[", "fold0_src["):
        assert name not in a
    assert 'extern "C" int sixdof_custom_set_fold_table(unsigned fold, const sixdof::FoldTable* t)' in a
    assert 'extern "C" unsigned sixdof_custom_fold_count() { return 1u; }' in a and "sixdof_custom_fold_info" in a
    assert "fold0_kernel(const StepParams P, const FoldTable F)" in a and "// tick = [double] | fold:fold_test | [add_one]" in a
    assert "70000" not in b and "edges," not in a                                   # no counts, not in comments either
    baked = codegen.generate_source(prog().trace({"x": 1, "n": 1}, fold_edges=EDGES), "float64", 2)
    assert "__device__ const uint32_t fold0_dst[3] = {1, 2, 2};" in baked and "sixdof_custom_set_fold_table" not in baked and "FoldTable" not in baked
    # replicas are part of the text (count and stride are what the object is generated for), the graph still is not
    r1 = codegen.generate_source(prog().trace({"x": 1, "n": 1}, fold_edges=EDGES, fold_replicas=(5, 3), fold_tables="device"), "float64", 2)
    r2 = codegen.generate_source(prog().trace({"x": 1, "n": 1}, fold_edges={"e": ([2], [0])}, fold_replicas=(5, 3), fold_tables="device"), "float64", 2)
    assert r1 == r2 and r1 != a and "{1u, 5u, 3u}" in r1
    # a fold that may be regrouped gets the second kernel and says so to the library (info bit 1); one that may not does neither
    w = codegen.generate_source(ft.sum_program(True).trace({"x": 1, "y": 1, "z": 1}, fold_edges=EDGES, fold_tables="device"), "float64", 2)
    s = codegen.generate_source(ft.sum_program(False).trace({"x": 1, "y": 1, "z": 1}, fold_edges=EDGES, fold_tables="device"), "float64", 2)
    d = codegen.generate_source(ft.damped_program().trace({"x": 1, "y": 1, "z": 1}, fold_edges=EDGES, fold_tables="device"), "float64", 2)
    assert "fold0_wave(const StepParams P, const FoldTable F)" in w and "{3u, 1u, 0u}" in w and "__shfl_down(v0, off, 64)" in w
    assert "fold0_wave" not in s and "{1u, 1u, 0u}" in s and "fold0_wave" not in d


def test_forcing_device_tables_on_a_complete_graph_keeps_its_arithmetic_kernel():
    tp = ft.sum_program(False).trace({"x": 1, "y": 1, "z": 1}, fold_edges={"e": ("complete", 128)}, fold_tables="device")
    assert tp.device_fold_components == [None] and not tp.fold_stages[0].device_tables
    src = codegen.generate_source(tp, "float64", 2)
    assert "(e + ((e) >= i ? 1u : 0u))" in src and "{0u, 1u, 0u}" in src and "fold0_kernel(const StepParams P)" in src


def test_device_flavour_programs_compile_without_spills_or_scratch():
    """hipcc cross-compiles for gfx950 here: the sequential kernel and the lane + wave pair read their indices from memory with no
    scratch and no spills (codegen.build refuses spills anyway)."""
    for prog, widths in ((dsl.Program([double, fold_test, add_one], dsl.pipe(), []), {"x": 1, "n": 1}), (ft.sum_program(True), {"x": 1, "y": 1, "z": 1})):
        so = codegen.build(prog.trace(widths, fold_edges=EDGES, fold_tables="device"), "float64", 2)
        res = dict(codegen.last_resources)
        assert so.exists() and res["vgpr_spills"] == 0 and res["sgpr_spills"] == 0 and res["scratch_bytes_per_lane"] == 0, res
        lib = C.CDLL(str(so))
        assert lib.sixdof_custom_fold_count() == 1
        info = (C.c_uint * 4)()
        assert lib.sixdof_custom_fold_info(0, info) == 0 and info[3] == 32 and lib.sixdof_custom_fold_info(1, info) != 0      # sizeof(FoldTable): 3 pointers + 2 counts


def test_the_walker_reads_a_device_flavour_trace_like_a_baked_one():
    tp = dsl.Program([double, fold_test, add_one], dsl.pipe(), []).trace({"x": 1, "n": 1}, fold_edges=EDGES, fold_tables="device")
    pos = np.tile([0.0, 0, 0, 1, 0, 0, 0], (3, 1))
    vel, inertia, acc = np.zeros((3, 6)), np.ones((3, 7)), np.zeros((3, 6))
    comps = {"x": np.array([[1.0], [2.0], [2.0]]), "n": np.zeros((3, 1)), "x#fold0": np.zeros((3, 1))}
    x = np.array([1.0, 2.0, 2.0])
    for tick in range(1, 4):
        dsl_numpy.program_tick_systems_only(tp, pos, vel, acc, inertia, comps, tick)
        x = x * 2.0
        x = np.array([5.0 + (x[0] + x[1]) + (x[0] + x[2]), 5.0 + (x[1] + x[2]), x[2]]) + 1.0
        assert np.array_equal(comps["x"][:, 0], x)


def test_the_numpy_twins_equal_the_walker():
    """tests/test_gpu_fold_tables.py compares 131,072-edge and hub graphs with vectorised numpy twins (the walker evaluates the traced
    DAG once per edge in Python): here the twins are pinned on the walker, on graphs of the same shape small enough for it."""
    n, k = 256, 16
    src, dst = ft.regular_graph(n, k)
    x0 = np.random.default_rng(5).uniform(-1.0, 1.0, n)
    tp = ft.damped_program().trace({"x": 1, "y": 1, "z": 1}, fold_edges={"e": (src, dst)}, fold_tables="device")
    comps = ft.walker_run(tp, {"x": x0[:, None].copy(), "y": np.zeros((n, 1)), "z": np.zeros((n, 1))}, 4)
    x, y, z = ft.damped_twin(x0, src, dst, k, 4)
    assert np.array_equal(comps["x"][:, 0], x) and np.array_equal(comps["y"][:, 0], y) and np.array_equal(comps["z"][:, 0], z)
    assert np.abs(z).max() > 0.1 and not np.array_equal(z, ft.damped_twin(x0, src, dst[::-1].reshape(n, k)[::-1].ravel(), k, 4)[2])      # order matters
    n = 96
    src, dst = ft.hub_and_ring(n)
    x0 = np.random.default_rng(6).uniform(-1.0, 1.0, n)
    tp = ft.sum_program(True).trace({"x": 1, "y": 1, "z": 1}, fold_edges={"e": (src, dst)}, fold_tables="device")
    comps = ft.walker_run(tp, {"x": x0[:, None].copy(), "y": np.zeros((n, 1)), "z": np.zeros((n, 1))}, 3)
    x, y, z, scale = ft.sum_twin(x0, src, dst, 3)
    assert np.array_equal(comps["x"][:, 0], x) and np.array_equal(comps["z"][:, 0], z) and scale[0] > scale[1:].max()


def test_the_table_builder_keeps_spawn_order_and_splits_the_sources():
    rc, src, start, dst, n_lane = ft.build_table([2, 0, 2, 0, 2], [1, 2, 0, 1, 2], 3, 0)
    assert rc == L.OK and src.tolist() == [0, 2] and start.tolist() == [0, 2, 5] and dst.tolist() == [2, 1, 1, 0, 2] and n_lane == 2
    # a star plus a ring: the hub (row 3 here, 99 spokes + its ring edge) goes behind the lane sources when the fold may be regrouped
    n, hub = 100, 3
    s = np.concatenate([np.full(n - 1, hub), np.arange(n)])
    d = np.concatenate([np.delete(np.arange(n), hub), (np.arange(n) + 1) % n])
    rc, src, start, dst, n_lane = ft.build_table(s, d, n, 64)
    assert rc == L.OK and n_lane == n - 1 and src.tolist() == [r for r in range(n) if r != hub] + [hub]
    assert np.array_equal(np.diff(start), [1] * (n - 1) + [n]) and dst[start[-2]:].tolist() == np.delete(np.arange(n), hub).tolist() + [hub + 1]
    assert dst[:n - 1].tolist() == [(r + 1) % n for r in range(n) if r != hub]
    rc, src, start, dst, n_lane = ft.build_table(s, d, n, 0)                          # a fold that does not qualify: one list, sources ascending
    assert rc == L.OK and n_lane == n and src.tolist() == list(range(n)) and start[hub + 1] - start[hub] == n
    assert dst[start[hub]:start[hub + 1]].tolist() == np.delete(np.arange(n), hub).tolist() + [hub + 1]
    # rows are checked: a table never names a row the kernels may not gather
    assert ft.build_table([0, 1], [1, 3], 3, 0)[0] == L.ERR_INVALID_ARGUMENT and ft.build_table([3], [0], 3, 64)[0] == L.ERR_INVALID_ARGUMENT
    rc, src, start, dst, n_lane = ft.build_table([], [], 8, 64)                       # no edges: an empty table, nothing to launch
    assert rc == L.OK and len(src) == 0 and start.tolist() == [0] and n_lane == 0


@pytest.mark.parametrize("n,k,wave_min", [(8192, 16, 0), (4096, 1, 64), (8192, 9, 0)])
def test_the_table_builder_at_the_sizes_the_gpu_tests_run(n, k, wave_min):
    """What can be rehearsed without a GPU, at full size: every target in range, row_start monotone, the two ranges a partition of the
    sources, each source's targets in the order given."""
    if k == 1:
        src, dst = ft.hub_and_ring(n)
    elif k == 9:
        src = np.repeat(np.arange(n), 9)
        dst = (src + np.tile([1, 5, 11, 17, 23, 29, 31, 37, 41], n)) % n
    else:
        src, dst = ft.regular_graph(n, k)
    rc, rows, start, out, n_lane = ft.build_table(src, dst, n, wave_min)
    assert rc == L.OK and start[0] == 0 and start[-1] == len(src) and np.all(np.diff(start.astype(np.int64)) > 0) and out.max() < n
    assert sorted(rows.tolist()) == np.unique(src).tolist() and np.all(np.diff(rows[:n_lane].astype(np.int64)) > 0) and np.all(np.diff(rows[n_lane:].astype(np.int64)) > 0)
    deg = np.diff(start.astype(np.int64))
    if wave_min:
        assert np.all(deg[:n_lane] < wave_min) and np.all(deg[n_lane:] >= wave_min) and len(rows) - n_lane == 1
    else:
        assert n_lane == len(rows)
    for i in (0, len(rows) // 2, len(rows) - 1):
        assert np.array_equal(out[start[i]:start[i + 1]], np.asarray(dst)[np.asarray(src) == rows[i]])
    tp = ft.damped_program().trace({"x": 1, "y": 1, "z": 1}, fold_edges={"e": (src, dst)}, fold_tables="device")      # the trace's CSR: the one-list table
    if not wave_min:
        fs = tp.fold_stages[0]
        assert np.array_equal(fs.src_rows, rows) and np.array_equal(fs.row_start, start) and np.array_equal(fs.dst, out)


def test_set_fold_edges_is_declared_and_refuses_a_null_handle():
    """A handle needs a device, so the refusals on a live handle (no program installed, a baked object, a bad index, a bad row) are in
    tests/test_gpu_fold_tables.py; without one the entry point still answers with a status."""
    lib = L.lib()
    ids = (C.c_uint64 * 2)(1, 2)
    assert lib.sixdof_set_fold_edges(None, 0, ids, ids, 2) == L.ERR_INVALID_ARGUMENT
    header = (L.PKG.parent / "include" / "sixdof_hip.h").read_text()
    assert "int sixdof_set_fold_edges(sixdof_handle* h, uint32_t fold_index, const uint64_t* from_ids, const uint64_t* to_ids, size_t n_edges);" in header


def _cli_world(tmp_path, name, offsets, nb=70):
    targets = {s_: [(s_ + k) % nb for k in offsets] for s_ in range(nb)}
    text, slots = hb.edge_fold_world(nb, targets, "newton", (6.6743e-11,))
    d = tmp_path / name
    d.mkdir()
    (d / "tick.mlir").write_text(text)
    meta = {"arg_ids": [L.component_id(c) for c, _, _ in slots], "ret_ids": [L.component_id(c) for c, _, _ in slots], "names": {str(L.component_id(c)): c for c, _, _ in slots},
            "rows": nb, "arg_slots": [{"component_id": L.component_id(c), "shape": s_, "entity_axis_elided": e_} for c, s_, e_ in slots]}
    (d / "slots.json").write_text(json.dumps(meta))
    return d, targets


def test_the_cli_writes_one_object_for_every_graph_and_the_edges_next_to_it(tmp_path):
    nb = 70
    outs = []
    for name, offsets in (("a", (1, 5, 11)), ("b", (2, 3, 17))):
        d, targets = _cli_world(tmp_path, name, offsets, nb)
        out = d / "pipe.so"
        res = subprocess.run([sys.executable, "-m", "elodin_amd.stablehlo", str(d / "tick.mlir"), "--slots", str(d / "slots.json"), "-o", str(out), "--fold-tables", "device"],
                             capture_output=True, text=True, cwd=str(L.PKG.parent))
        assert res.returncode == 0, res.stderr[-2000:]
        line = json.loads(res.stdout.strip().splitlines()[-1])
        assert line["mode"] == "folds" and line["fold_tables"] == "device" and out.exists()
        prog, manifest = sh.load_world(str(out))
        assert manifest["fold_tables"] == "device" and manifest["fold_stages"] == 4 and manifest["edge_sidecar"]["file"] == "pipe.so.edges"
        assert (d / "pipe.so.edges").stat().st_size == 4 * 3 * nb * 8                # four scans x 210 edges x two uint32
        assert [f["fold"] for f in manifest["edge_sidecar"]["folds"]] == [0, 1, 2, 3] and len(prog.graph_edges) == 4
        for frm, to in prog.graph_edges.values():
            assert frm.tolist() == [s_ for s_ in range(nb) for _ in range(3)] and to.tolist() == [t for s_ in range(nb) for t in targets[s_]]
        assert prog._traced.device_fold_components == [f["edge_component"] for f in manifest["edge_sidecar"]["folds"]]
        outs.append(out)
    assert outs[0].read_bytes() == outs[1].read_bytes()                               # the same generated text, the same cached object
    assert (outs[0].parent / "pipe.so.edges").read_bytes() != (outs[1].parent / "pipe.so.edges").read_bytes()
    # the default stays baked below the cap: no sidecar, the graph in the object
    d, _ = _cli_world(tmp_path, "c", (1, 5, 11), nb)
    res = subprocess.run([sys.executable, "-m", "elodin_amd.stablehlo", str(d / "tick.mlir"), "--slots", str(d / "slots.json"), "-o", str(d / "pipe.so")],
                         capture_output=True, text=True, cwd=str(L.PKG.parent))
    assert res.returncode == 0, res.stderr[-2000:]
    prog, manifest = sh.load_world(str(d / "pipe.so"))
    assert manifest["fold_tables"] == "baked" and not (d / "pipe.so.edges").exists() and prog.graph_edges == {}
    assert (d / "pipe.so").read_bytes() != outs[0].read_bytes()
