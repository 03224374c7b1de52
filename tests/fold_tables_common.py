"""Programs, graphs and numpy twins shared by tests/test_fold_tables_host.py (CPU) and tests/test_gpu_fold_tables.py (GPU): fold
stages whose edges live in device memory (dsl.Program.trace(fold_tables="device"), HipExec(graph_tables=...))."""
import ctypes as C

import numpy as np

from elodin_amd import _lib as L, dsl

np_ = dsl.np


# ---- an ORDER-SENSITIVE fold between two systems: acc * 0.5 + a * b is no sum, so every source is folded sequentially ----
@dsl.system
def spread(x, y):
    return {"y": x * 0.75 + 0.25}


@dsl.graph_fold("e", left=("y",), right=("y",), out="z", init=0.0)
def damped(acc, a, b):
    return acc * 0.5 + a * b


@dsl.system
def relax(x, z):
    return {"x": x * 0.5 + z * 0.0625}


# the same two systems declaring that they touch no Body column: such a chain never looks at the absolute tick or the Body slabs,
# so batches of it replay from a captured graph (codegen: layout bit 17)
@dsl.system
def spread_free(x, y):
    return {"y": x * 0.75 + 0.25}


@dsl.system
def relax_free(x, z):
    return {"x": x * 0.5 + z * 0.0625}


spread_free.body_free = relax_free.body_free = True


def damped_program(body_free=False):
    return dsl.Program([spread_free, damped, relax_free] if body_free else [spread, damped, relax], dsl.pipe(), [])


def regular_graph(n, k, stride=37):
    """Every row lists k targets (s + j * stride + 1) % n, j = 0..k-1 -> (src rows, dst rows), spawn order = slot order."""
    s = np.repeat(np.arange(n, dtype=np.int64), k)
    j = np.tile(np.arange(k, dtype=np.int64), n)
    return s, (s + j * stride + 1) % n


def damped_twin(x, src, dst, k, ticks):
    """damped_program on a regular_graph, vectorised over the sources: per source the same operations in the same order as the
    generated kernel and the walker (one loop trip per edge slot).  x: [n] -> (x, y, z) after `ticks`."""
    n = x.shape[0]
    x = x.copy()
    d = np.asarray(dst).reshape(n, k)
    assert np.array_equal(np.asarray(src).reshape(n, k), np.repeat(np.arange(n)[:, None], k, axis=1))
    y = z = None
    for _ in range(ticks):
        y = x * 0.75 + 0.25
        acc = np.zeros(n)
        for slot in range(k):
            acc = acc * 0.5 + y * y[d[:, slot]]
        z = acc
        x = x * 0.5 + z * 0.0625
    return x, y, z


# ---- a PLAIN SUM that may ask for waves: z = sum over the out-edges of a * b ----
@dsl.system
def drift(x, y):
    return {"y": x * 0.5 + 0.125}


@dsl.system
def settle(x, z):
    return {"x": x * 0.25 + z * 0.0001220703125}


@dsl.system
def wander(x, y):
    return {"y": x * 0.5 + 0.125, "x": x * 0.96875 + 0.015625}


@dsl.system
def collect(w, z):
    return {"w": w * 0.5 + z * 0.0001220703125}


def sum_program(wave_fold, feedback=True):
    """feedback: the fold's result enters the next tick's inputs (x); without it (x wanders on its own, w collects z) every tick's
    fold sees inputs that do not depend on how earlier folds were associated."""
    fold = dsl.GraphFold(lambda acc, a, b: acc + a * b, "e", ("y",), ("y",), "z", 0.0)
    fold.wave_fold = bool(wave_fold)
    return dsl.Program([drift, fold, settle] if feedback else [wander, fold, collect], dsl.pipe(), [])


def hub_and_ring(n):
    """Row 0 lists every other row (n - 1 out-edges, ascending); every row then lists its ring successor."""
    src = np.concatenate([np.zeros(n - 1, dtype=np.int64), np.arange(n, dtype=np.int64)])
    dst = np.concatenate([np.arange(1, n, dtype=np.int64), (np.arange(n, dtype=np.int64) + 1) % n])
    return src, dst


def walker_run(tp, comps, ticks, first_tick=1):
    """tests/dsl_numpy's walker over a systems-only program: comps are updated in place."""
    from tests import dsl_numpy
    n = next(iter(comps.values())).shape[0]
    pos = np.tile([0.0, 0, 0, 1, 0, 0, 0], (n, 1))
    vel, inertia, acc = np.zeros((n, 6)), np.ones((n, 7)), np.zeros((n, 6))
    for fs in tp.fold_stages:
        comps.setdefault(fs.scratch_name, np.zeros((n, fs.out[2])))
    for t in range(first_tick, first_tick + ticks):
        dsl_numpy.program_tick_systems_only(tp, pos, vel, acc, inertia, comps, t)
    return comps


def sum_twin(x, src, dst, ticks):
    """sum_program with every source folded SEQUENTIALLY in spawn order (np.add.at is unbuffered: one addition per edge in the
    order given, per source) -> (x, y, z, scale) with scale[i] = sum of |terms| of source i in the last tick."""
    x = x.copy()
    src, dst = np.asarray(src), np.asarray(dst)
    order = np.argsort(src, kind="stable")
    s, d = src[order], dst[order]
    is_src = np.zeros(x.shape[0], dtype=bool)
    is_src[s] = True
    z = np.zeros_like(x)
    y = scale = None
    for _ in range(ticks):
        y = x * 0.5 + 0.125
        terms = y[s] * y[d]
        acc = np.zeros_like(x)
        np.add.at(acc, s, terms)
        scale = np.zeros_like(x)
        np.add.at(scale, s, np.abs(terms))
        z = np.where(is_src, acc, z)
        x = x * 0.25 + z * 0.0001220703125
    return x, y, z, scale


def build_table(src, dst, row_limit, wave_min_degree):
    """The library's host-side table builder (sixdof_build_fold_table, no GPU) -> (status, src_rows, row_start, dst, n_lane)."""
    lib = L.lib()
    src = np.ascontiguousarray(src, dtype=np.uint32)
    dst = np.ascontiguousarray(dst, dtype=np.uint32)
    n = len(src)
    o_src, o_start, o_dst = np.zeros(max(n, 1), np.uint32), np.zeros(n + 1, np.uint32), np.zeros(max(n, 1), np.uint32)
    n_src, n_lane = C.c_uint32(), C.c_uint32()
    u32 = C.POINTER(C.c_uint32)
    rc = lib.sixdof_build_fold_table(src.ctypes.data_as(u32), dst.ctypes.data_as(u32), n, int(row_limit), int(wave_min_degree),
                                     o_src.ctypes.data_as(u32), o_start.ctypes.data_as(u32), o_dst.ctypes.data_as(u32),
                                     C.byref(n_src), C.byref(n_lane))
    k = int(n_src.value)
    return rc, o_src[:k].copy(), o_start[:k + 1].copy(), o_dst[:n].copy(), int(n_lane.value)
