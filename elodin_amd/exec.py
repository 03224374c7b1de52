"""HipExec — the backend object a `WorldExec::Hip` variant would wrap.

Mirrors the contract of the reference backends (libs/nox-py/src/exec.rs:53-93,
cranelift_exec.rs:129-195 `invoke_batch(world, n, detailed) -> TickTimings`), over columns
held as numpy arrays in the reference's row-major layout.  All compute goes through the C ABI.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import math
import os
from pathlib import Path

import numpy as np

from . import _lib as L


def _raise(h, rc: int, what: str):
    msg = L.lib().sixdof_last_error(h)
    msg = msg.decode() if msg else ""
    if rc == L.ERR_COMPONENT_NOT_FOUND:
        raise KeyError(f"{what}: {msg}")           # Error::ComponentNotFound -> ValueError-class in PyO3
    if rc in (L.ERR_VALUE_SIZE_MISMATCH, L.ERR_INVALID_ARGUMENT, L.ERR_ENTITY_MISMATCH, L.ERR_UNSUPPORTED):
        raise ValueError(f"{what}: {msg}")
    if rc == L.ERR_OUT_OF_MEMORY:
        raise MemoryError(f"{what}: {msg}")
    raise L.BackendError(f"{what}: {msg} (status {rc})")


@dataclass
class Effector:
    """One op of the effector pipe (include/sixdof_hip.h sixdof_effector_kind)."""
    kind: int
    p: Sequence[float] = ()
    aux_name: Optional[str] = None          # component name of a per-entity [n,3] column
    aux: Optional[np.ndarray] = None        # its data


@dataclass
class TickTimings:  # profile.rs TickTimings
    h2d_upload_ms: float = 0.0
    kernel_invoke_ms: float = 0.0
    d2h_download_ms: float = 0.0
    kernel_device_ms: float = 0.0
    launches: int = 0
    ticks: int = 0
    kernel_sum_ms: float = 0.0
    graph_launches: int = 0    # how many of `launches` were replayed from a captured hipGraph


@dataclass(frozen=True)
class Event:
    """One trigger of HipExec.history_events: element `element` of `component` in row `group` of every run meets `op level`.
    mode "level": the earliest finite sample at which it does; "crossing": the earliest at which it does and the previous finite
    sample did not (a condition that holds from the first sample on never fires)."""
    component: str
    element: int
    op: str                 # "<", "<=", ">" or ">="
    level: float
    mode: str = "crossing"
    group: int = 0

    OPS = {"<": L.EVENT_LT, "<=": L.EVENT_LE, ">": L.EVENT_GT, ">=": L.EVENT_GE}
    MODES = {"level": L.EVENT_LEVEL, "crossing": L.EVENT_CROSSING}


@dataclass(frozen=True)
class Norm:
    """One probe of HipExec.history_norms: the Euclidean norm of elements element .. element + count - 1 of `component` in row
    `group` of every run — |r|, |v|, |omega|, |q| — or, with `minus` (a component name, which may be the same), of their
    difference to as many elements of `minus` from minus_element on in row minus_group: a separation, a miss distance, a
    deviation from a commanded state.  minus_element and minus_group default to element and group."""
    component: str
    element: int
    count: int
    group: int = 0
    minus: Optional[str] = None
    minus_element: Optional[int] = None
    minus_group: Optional[int] = None


@dataclass(frozen=True)
class NormEvent:
    """One trigger of HipExec.history_norm_events: the Euclidean norm `norm` (a Norm: |r|, |v|, a separation) meets `op level`, with
    `level` in the norm's own units — finite, not negative, its square finite.  The device compares squared norm and squared
    level; modes as for Event."""
    norm: Norm
    op: str                 # "<", "<=", ">" or ">="
    level: float
    mode: str = "crossing"


@dataclass(frozen=True)
class Element:
    """The signed scalar a Dwell looks at: element `element` of `component` in row `group` of every run or, with `minus` (a
    component name, which may be the same), its difference to element minus_element of `minus` in row minus_group — an altitude, a
    load factor, a cross-track error between two entities of a run.  minus_element and minus_group default to element and group."""
    component: str
    element: int
    group: int = 0
    minus: Optional[str] = None
    minus_element: Optional[int] = None
    minus_group: Optional[int] = None


@dataclass(frozen=True)
class Dwell:
    """One condition of HipExec.history_dwell: `of` (an Element or a Norm) meets `op level`, or lies inside / outside the closed
    band [level, upper].  Levels are in the units of `of`; for a Norm they are finite, not negative, and squared on the host: the
    device compares squared norm and squared level."""
    of: object              # an Element or a Norm
    op: str                 # "<", "<=", ">", ">=", "inside" or "outside"
    level: float
    upper: Optional[float] = None   # the band's upper level: "inside" and "outside" only

    OPS = {**Event.OPS, "inside": L.DWELL_INSIDE, "outside": L.DWELL_OUTSIDE}


def dispersion_ellipse(cov2, prob: float = 0.99):
    """(semi_major, semi_minor, angle) of the ellipse that holds the share `prob` of a bivariate normal population with the
    2 x 2 covariance `cov2` — the landing footprint out of the x / y block of HipExec.history_covariance's "cov".  Closed-form
    eigen-decomposition of the symmetric matrix (its off-diagonals are averaged); the semi-axes are sqrt(eigenvalue) times
    sqrt(-2 ln(1 - prob)), the exact chi-square quantile at two degrees of freedom; angle, in radians in (-pi/2, pi/2], turns
    the first axis onto the major one.  Broadcasts over leading axes: [..., 2, 2] -> three arrays [...].  ValueError: prob
    outside (0, 1), a shape other than [..., 2, 2]."""
    cov2 = np.asarray(cov2, dtype=np.float64)
    if cov2.ndim < 2 or cov2.shape[-2:] != (2, 2):
        raise ValueError(f"dispersion_ellipse: a [..., 2, 2] covariance is needed, not shape {cov2.shape}")
    prob = float(prob)
    if not 0.0 < prob < 1.0:
        raise ValueError(f"dispersion_ellipse: prob {prob!r} is outside (0, 1)")
    a, b, d = cov2[..., 0, 0], 0.5 * (cov2[..., 0, 1] + cov2[..., 1, 0]), cov2[..., 1, 1]
    half_diff = 0.5 * (a - d)
    major = 0.5 * (a + d) + np.hypot(half_diff, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        minor = np.where(major > 0, (a * d - b * b) / major, 0.0)      # the product of the eigenvalues is the determinant: no cancellation
    scale = np.sqrt(-2.0 * np.log1p(-prob))
    angle = 0.5 * np.arctan2(b, half_diff)
    return scale * np.sqrt(np.maximum(major, 0.0)), scale * np.sqrt(np.maximum(minor, 0.0)), angle


@dataclass(frozen=True)
class _Reduction:
    """One reduction over the ring into (group, element) bins, as HipExec._reduce and _stream_reduce call it."""
    fn: str                 # the library entry point
    async_flag: int
    planes: int             # doubles per bin in a raw block [samples, period, planes, w]
    extra: tuple            # its ctypes arguments between `period` and the buffers
    to_dict: Callable       # (names, raw blocks) -> the dict handed to the caller


@dataclass(frozen=True)
class _Scan:
    """One scan of the ring across time per run, as HipExec._scan and _stream_scan call it."""
    fn: str                 # the library entry point
    continue_flag: int
    hold_flag: int
    name: str               # history_<name> / stream_<name>, for the messages
    captures: bool          # whether it takes a capture list and delivers its blocks
    to_dict: Callable       # (capture names, raw block, capture blocks) -> the dict handed to the caller
    buffer: Optional[Callable] = None   # a scan without captures: (executor, items, period) -> its raw block; None: the norms'


class HipExec:
    def __init__(self, world_pos, world_vel, inertia, *, world_accel=None, force=None, entity_ids=None,
                 simulation_time_step: float = 1.0 / 120.0, time_step: Optional[float] = None,
                 integrator: int = L.RK4, dtype=np.float64, effectors: Sequence[Effector] = (),
                 edges=None, ticks_per_launch: int = 1, use_graph: bool = False, device: int = 0,
                 tick: int = 0, column_entity_ids=None, columns=None, fast_math: bool = False, graph_edges=None,
                 graph_replicas=None, guard_selects: Optional[bool] = None, reuse_trace: bool = False,
                 graph_tables: str = "auto"):
        """graph_tables: where the stand-alone folds of a program find their edges (`graph_edges`).  "baked": written into the
        generated code (at most 65,536 edges per fold; the graph is part of the object); "device": read from device memory
        (sixdof_set_fold_edges: any number of edges, one object for every graph, replaceable with set_graph_edges); "auto":
        baked while every listed fold has at most 65,536 edges, device beyond."""
        if graph_tables not in ("auto", "baked", "device"):
            raise ValueError('graph_tables must be "auto", "baked" or "device"')
        lib = L.lib()
        self._lib = lib
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("dtype must be float64 or float32")
        f = lambda a, w: np.array(a, dtype=self.dtype, order="C").reshape(-1, w)
        self.world_pos = f(world_pos, 7)
        self.world_vel = f(world_vel, 6)
        self.inertia = f(inertia, 7)
        nv = self.world_vel.shape[0]
        self.world_accel = np.zeros((nv, 6), self.dtype) if world_accel is None else f(world_accel, 6)
        self.force = np.zeros((nv, 6), self.dtype) if force is None else f(force, 6)
        # ids are sequential from 1 (0 = Globals) unless given: world.rs:193-196.  `column_entity_ids` gives a
        # column its own id vector when components live on different entity sets (six_dof then runs on the
        # intersection, query.rs:136-208)
        self.entity_ids = (np.arange(1, self.world_pos.shape[0] + 1, dtype=np.uint64) if entity_ids is None
                           else np.ascontiguousarray(entity_ids, dtype=np.uint64))
        self._column_ids = {k: np.ascontiguousarray(v, dtype=np.uint64) for k, v in (column_entity_ids or {}).items()}
        n = self.world_pos.shape[0] if not self._column_ids else 0   # 0 = let the library size the join
        # rows the device really steps: with per-column id vectors six_dof runs on the INTERSECTION of the Body columns' entity
        # sets (csrc/sixdof_capi.cpp sixdof_bind_columns, query.rs:136-208) — every build-time choice below that depends on the
        # row count (one-launch pair kernel, cache policy, column layout, whole worlds per executor) uses this, not world_pos's
        self._n_rows = self.world_pos.shape[0]
        if self._column_ids:
            joined = None
            for name in ("world_pos", "world_vel", "world_accel", "force", "inertia"):
                ids = self._column_ids.get(name, self.entity_ids)
                joined = set(ids.tolist()) if joined is None else joined & set(ids.tolist())
            self._n_rows = len(joined)
        self._aux = {}
        self._windows = {}
        self._window_soa = False
        self._column_soa = False
        self._soa = {}            # program column name -> the element-major staging array bound to the C ABI
        self._device_folds = []   # per fold stage of a program with device fold tables: its edge component (None: no table)
        d = L.Desc()
        d.struct_size = C.sizeof(L.Desc)
        d.device_ordinal = device
        d.integrator = integrator
        d.dtype = L.F64 if self.dtype == np.float64 else L.F32
        d.n_entities = n
        d.simulation_time_step = simulation_time_step
        d.has_time_step = 0 if time_step is None else 1
        d.time_step = 0.0 if time_step is None else float(time_step)
        d.ticks_per_launch = ticks_per_launch
        d.flags = L.FLAG_USE_GRAPH if use_graph else 0
        self._h = C.c_void_p()
        try:
            cols = [("world_pos", self.world_pos), ("world_vel", self.world_vel), ("world_accel", self.world_accel),
                    ("force", self.force), ("inertia", self.inertia)]
            custom = None
            from . import dsl as _dsl
            if isinstance(effectors, _dsl.Effector):
                effectors = _dsl.pipe(effectors)
            self._program_columns = []
            if isinstance(effectors, (_dsl.Pipe, _dsl.Program)):
                # user-written effectors / systems: trace -> generate HIP -> hipcc -> sixdof_set_custom_pipe
                from . import codegen
                # [n, w] columns give their row width; an [n, rows, w] column is a window component (dsl.Window)
                widths = {k: (tuple(int(x) for x in np.shape(v)[1:]) if np.ndim(v) == 3 else int(np.atleast_2d(np.asarray(v)).shape[-1]))
                          for k, v in (columns or {}).items()}
                fold_rows = None
                # A Pipe / Program keeps its first trace (`_traced`).  An executor starts from a FRESH one unless the caller promises
                # (reuse_trace=True) that nothing a trace reads has changed since: the program's systems, and every Python value their
                # functions close over (gains, host tables, parameter sentinels).  A frozen program has no functions to trace again.
                if not reuse_trace and not isinstance(effectors, _dsl.FrozenProgram) and getattr(effectors, "_traced", None) is not None:
                    effectors._traced = None
                if isinstance(effectors, _dsl.Program) and effectors.folds:
                    # stand-alone folds inside the program: their edges as row pairs of this executor (spawn order)
                    if self._column_ids:
                        raise ValueError("a program with stand-alone folds needs every column on the executor's own entity ids")
                    row_of = {int(e): k for k, e in enumerate(self.entity_ids)}
                    fold_rows = {}
                    for name, (frm, to) in (graph_edges or {}).items():
                        if isinstance(frm, str) and frm == "complete":      # the complete graph over a world's rows: nothing to resolve
                            fold_rows[name] = (frm, int(to))
                            continue
                        try:
                            fold_rows[name] = ([row_of[int(a)] for a in frm], [row_of[int(b)] for b in to])
                        except KeyError as e:
                            raise KeyError(f"graph_edges[{name!r}]: edge endpoint {e} is not an entity of this executor") from None
                    if graph_replicas is not None and int(graph_replicas[0]) * int(graph_replicas[1]) != len(self.entity_ids):
                        raise ValueError("graph_replicas=(count, rows per replica) must cover the executor's rows exactly")
                    if graph_tables == "auto":
                        graph_tables = "device" if any(not isinstance(frm, str) and len(frm) > 65536 for frm, _ in fold_rows.values()) else "baked"
                    custom = effectors.trace(widths, fold_edges=fold_rows, fold_replicas=graph_replicas, fold_tables=graph_tables)
                    columns = dict(columns or {})
                    for fs in custom.fold_stages:       # scratch rows: a fold reads the values from before it ran
                        columns.setdefault(fs.scratch_name, np.zeros((self.world_pos.shape[0], fs.out[2])))
                else:
                    # executors built again and again from ONE program object (a campaign service: one per block of runs)
                    # trace it and generate its source once per column layout; the objects themselves are cached on disk
                    # — OPT-IN (`reuse_trace=True`): the memo returns the FIRST trace, so the caller promises that neither the
                    # program's systems nor any Python value its functions close over (gains, host tables, parameter
                    # sentinels) changes between the executors.  Without the promise every executor traces again; the object
                    # is still found in the on-disk cache by the digest of the generated source.
                    memo = (effectors.__dict__.setdefault("_exec_memo", {}) if reuse_trace and hasattr(effectors, "__dict__") else None)
                    wkey = (tuple(sorted((k, v) for k, v in widths.items())),
                            tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("SIXDOF_"))),
                            tuple(sorted((str(k), repr(v)) for k, v in getattr(_dsl, "PARAM_SENTINELS", {}).items())))
                    custom = memo.get(("trace", wkey)) if memo is not None else None
                    if custom is None:
                        custom = effectors.trace(widths)
                        if memo is not None:
                            memo[("trace", wkey)] = custom
                rows_multiple = int(getattr(custom, "rows_multiple", 0) or codegen.lane_stride(custom))
                if getattr(custom, "exact_rows", 0) and self._n_rows != int(custom.exact_rows):
                    raise ValueError(f"this object's fold stages were generated for {int(custom.exact_rows)} rows (manifest 'row_count'); the executor has {self._n_rows}")
                if rows_multiple > 1 and self._n_rows % rows_multiple:
                    raise ValueError(f"this program exchanges data between the entities of a world laid out as {rows_multiple} consecutive rows "
                                     f"(a whole-world StableHLO tick in lane mode, manifest 'rows_per_world'): the executor's {self._n_rows} "
                                     f"rows are not a whole number of worlds")
                if isinstance(effectors, _dsl.Program):
                    self._program_columns = [n for n, _ in custom.columns]
                    self._windows = {name: (rows, width) for name, (_, rows, width) in custom.windows.items()}
                    self._mats = dict(custom.table.mats)       # small 2-D components held as register matrices
                    columns = dict(columns or {})
                    for name in self._windows:       # the ring's head (physical index of the oldest row): starts at 0
                        columns.setdefault(name + "#head", np.zeros((np.shape(columns[name])[0], 1)) if name in columns else None)
                self._window_soa = bool(self._windows) and self._n_rows >= codegen.WINDOW_SOA_MIN_ROWS
                # register columns of a large program executor: element-major on the device (codegen.COLUMN_SOA_MIN_ROWS); the
                # host-facing arrays (self._aux) stay in the reference's [n, w] rows, upload / download transpose
                soa_env = os.environ.get("SIXDOF_COLUMN_SOA")
                self._column_soa = (isinstance(effectors, _dsl.Program) and not getattr(custom, "fold_stages", None)
                                    and not self._column_ids and (soa_env == "1" or (soa_env != "0" and
                                                                  self._n_rows >= codegen.COLUMN_SOA_MIN_ROWS)))
                if getattr(custom, "frozen_source", None) is not None or getattr(custom, "prebuilt_so", None) is not None:      # generated for ONE device layout
                    self._column_soa, self._window_soa = bool(custom.column_soa), False
                memo = effectors.__dict__.get("_exec_memo") if reuse_trace and hasattr(effectors, "__dict__") else None
                bkey = ("build", id(custom), self.dtype.name, integrator, bool(fast_math), self._window_soa, self._column_soa, guard_selects,
                        self._n_rows * self.dtype.itemsize * (32 + sum(int(w_) for _, w_ in custom.columns)) <= (768 << 20),
                        tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("SIXDOF_"))))
                so = memo.get(bkey) if memo is not None else None
                if so is None or not Path(so).exists():
                    row_elems = 32 + sum(int(w_) for _, w_ in custom.columns)       # what fill_step_params counts (csrc/sixdof_capi.cpp)
                    so = codegen.build(custom, self.dtype.name, integrator, fast_math=fast_math, window_soa=self._window_soa,
                                       column_soa=self._column_soa, guard_selects=guard_selects,
                                       policy=codegen.policy_for(self._n_rows, row_elems, self.dtype.itemsize))
                    if memo is not None:
                        memo[bkey] = so
                for name, width in custom.columns:
                    if columns is None or columns.get(name) is None:
                        raise KeyError(f"effector reads component {name!r} which was not provided")
                    arr = np.array(columns[name], dtype=self.dtype, order="C").reshape(-1, width)
                    if name in self._windows and self._window_soa:
                        arr = np.ascontiguousarray(arr.T).reshape(arr.shape)   # large executors: element-major [rows*width][n] (codegen.py)
                    self._aux[name] = arr
                    if self._column_soa and name not in self._windows and width > 1:
                        self._soa[name] = np.ascontiguousarray(arr.T).reshape(arr.shape)    # what the device holds
                        cols.append((name, self._soa[name]))
                    else:
                        cols.append((name, arr))
                effectors = ()
            pair_so = None
            effectors = list(effectors)
            if effectors and isinstance(effectors[-1], _dsl.EdgeFold):
                # user-written edge_fold function: trace -> generate the PAIR functor -> hipcc -> sixdof_set_custom_pair
                from . import codegen
                if self.dtype != np.float64:
                    raise ValueError("edge_fold effectors are float64 only")
                if edges is None:
                    raise ValueError("an edge_fold effector needs edges=(from_ids, to_ids)")
                # the object is built for THIS executor: its integrator, and the one-launch small-graph kernel or the multi-kernel
                # tick (pack once per batch, then the fused fold-and-integrate launch per tick) — the rule csrc/sixdof_capi.cpp applies
                # at step time (kPairSmallMax = 256; SIXDOF_PAIR_SMALL=0 forces the multi-kernel path)
                pair_small = self._n_rows <= 256 and os.environ.get("SIXDOF_PAIR_SMALL", "")[:1] != "0"
                pair_so = codegen.build_pair(effectors.pop().trace(), integrator=integrator, small=pair_small)
            if any(isinstance(e, _dsl.EdgeFold) for e in effectors):
                raise ValueError("an edge_fold effector must be last in the pipe")
            ops = (L.EffectorOp * max(1, len(effectors)))()
            for k, e in enumerate(effectors):
                ops[k].kind = e.kind
                for j, v in enumerate(e.p):
                    ops[k].p[j] = float(v)
                if e.aux is not None:
                    name = e.aux_name or f"effector_aux_{k}"
                    arr = np.array(e.aux, dtype=self.dtype, order="C").reshape(-1, 3)
                    self._aux[name] = arr
                    cols.append((name, arr))
                    ops[k].aux_component_id = L.component_id(name)
            # user code is traced and compiled above, before the device is touched: a program that cannot be built fails
            # without a context, and a machine without a GPU can fill the JIT cache (elodin_amd/_jit) for one that has it
            rc = lib.sixdof_create(C.byref(d), C.byref(self._h))
            if rc != L.OK:
                _raise(None, rc, "sixdof_create")
            self._bind(cols)
            rc = lib.sixdof_set_effectors(self._h, ops, len(effectors))
            if rc != L.OK:
                _raise(self._h, rc, "sixdof_set_effectors")
            if custom is not None:
                ids = (C.c_uint64 * max(1, len(custom.columns)))(*[L.component_id(n) for n, _ in custom.columns])
                rc = lib.sixdof_set_custom_pipe(self._h, str(so).encode(), ids, len(custom.columns))
                if rc != L.OK:
                    _raise(self._h, rc, "sixdof_set_custom_pipe")
                # a program with device fold tables: the fold stages that read one, by edge component; install what was given
                self._device_folds = list(getattr(custom, "device_fold_components", None) or [])
                if any(c is not None for c in self._device_folds):
                    if graph_edges is None and getattr(custom, "graph_edge_rows", None):      # a loaded object's sidecar: rows of one world
                        graph_edges = {c: (self.entity_ids[np.asarray(a_, dtype=np.int64)], self.entity_ids[np.asarray(b_, dtype=np.int64)])
                                       for c, (a_, b_) in custom.graph_edge_rows.items()}
                    missing = sorted({c for c in self._device_folds if c is not None} - set(graph_edges or {}))
                    if missing:
                        raise ValueError(f"graph_edges lacks the edges of {missing}: every fold of a program with device fold tables needs a table")
                    self.set_graph_edges({c: (graph_edges or {})[c] for c in self._device_folds if c is not None})
            if pair_so is not None:
                rc = lib.sixdof_set_custom_pair(self._h, str(pair_so).encode())
                if rc != L.OK:
                    _raise(self._h, rc, "sixdof_set_custom_pair")
            if edges is not None:
                frm = np.ascontiguousarray(edges[0], dtype=np.uint64)
                to = np.ascontiguousarray(edges[1], dtype=np.uint64)
                u64p = C.POINTER(C.c_uint64)
                rc = lib.sixdof_set_edges(self._h, frm.ctypes.data_as(u64p), to.ctypes.data_as(u64p), len(frm))
                if rc != L.OK:
                    _raise(self._h, rc, "sixdof_set_edges")
            lib.sixdof_set_tick(self._h, tick)
            self.upload()
        except Exception:
            self.close()
            raise

    def _bind(self, named_arrays):
        cols = (L.Column * len(named_arrays))()
        prim = L.PRIM_F64 if self.dtype == np.float64 else L.PRIM_F32
        for c, (name, arr) in zip(cols, named_arrays):
            c.component_id = L.component_id(name)
            c.prim_type = prim
            c.ndim = 1
            c.dims[0] = arr.shape[1]
            c.n_rows = arr.shape[0]
            ids = self._column_ids.get(name, self.entity_ids)
            if len(ids) != arr.shape[0]:
                raise ValueError(f"column {name}: {arr.shape[0]} rows but {len(ids)} entity ids")
            c.entity_ids = ids.ctypes.data_as(C.POINTER(C.c_uint64))
            c.host_ptr = arr.ctypes.data
        rc = self._lib.sixdof_bind_columns(self._h, cols, len(named_arrays))
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_bind_columns")
        m = C.c_size_t()
        self._lib.sixdof_get_join_rows(self._h, L.component_id("world_pos"), None, 0, C.byref(m))
        self.n = int(m.value)   # size of the joined Body entity set

    # -- reference-shaped surface -------------------------------------------------------------------
    def upload(self):
        for name, dev in self._soa.items():      # [n, w] rows -> [w][n]
            a = self._aux[name]
            dev.reshape(a.shape[1], a.shape[0])[...] = a.T
        rc = self._lib.sixdof_upload(self._h)
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_upload")

    def invoke_batch(self, n_ticks: int) -> TickTimings:
        """cranelift_exec.rs:129-195: run n ticks back to back; state stays in HBM."""
        t = L.Timings()
        rc = self._lib.sixdof_step(self._h, int(n_ticks), C.byref(t))
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_step")
        return TickTimings(t.h2d_upload_ms, t.kernel_invoke_ms, t.d2h_download_ms, t.kernel_device_ms,
                           int(t.launches), int(t.ticks), t.kernel_sum_ms, int(t.graph_launches))

    def set_graph_edges(self, graph_edges) -> None:
        """Replace the edges of stand-alone folds between batches: {edge_component: (from_ids, to_ids)}, entity ids of this
        executor (of replica 0 under graph_replicas), any size and source set.  Only for a program built with device fold
        tables (graph_tables="device", or "auto" beyond 65,536 edges): a baked program's graph is part of its code."""
        if not any(c is not None for c in self._device_folds):
            raise ValueError("set_graph_edges: this executor's program bakes its folds' edges into the generated code; "
                             "build it with graph_tables=\"device\" to replace them")
        unknown = sorted(set(graph_edges) - {c for c in self._device_folds if c is not None})
        if unknown:
            raise KeyError(f"set_graph_edges: no fold of this program with device tables reads {unknown}")
        u64p = C.POINTER(C.c_uint64)
        for k, comp in enumerate(self._device_folds):
            if comp is None or comp not in graph_edges:
                continue
            frm = np.ascontiguousarray(graph_edges[comp][0], dtype=np.uint64)
            to = np.ascontiguousarray(graph_edges[comp][1], dtype=np.uint64)
            if frm.shape != to.shape or frm.ndim != 1:
                raise ValueError(f"graph_edges[{comp!r}]: from / to must be two id vectors of one length")
            rc = self._lib.sixdof_set_fold_edges(self._h, k, frm.ctypes.data_as(u64p), to.ctypes.data_as(u64p), len(frm))
            if rc != L.OK:
                _raise(self._h, rc, "sixdof_set_fold_edges")

    def prepare(self, n_ticks: int):
        """Capture the replay graphs a later invoke_batch(n_ticks) uses (use_graph=True), outside any timed region."""
        rc = self._lib.sixdof_prepare_step(self._h, int(n_ticks))
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_prepare_step")

    @property
    def step_path(self) -> str:
        """Which path the next invoke_batch takes: "aql", "hipgraph: <why not aql>", "eager: <why>", ... (sixdof_step_path)."""
        return self._lib.sixdof_step_path(self._h).decode()

    def download(self, mask: int = L.COL_ALL):
        rc = self._lib.sixdof_download(self._h, mask)
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_download")
        for name in getattr(self, "_program_columns", ()):   # components a generated program writes
            rc = self._lib.sixdof_download_column(self._h, L.component_id(name))
            if rc != L.OK:
                _raise(self._h, rc, "sixdof_download_column")
        for name, dev in self._soa.items():      # [w][n] -> [n, w] rows
            a = self._aux[name]
            a[...] = dev.reshape(a.shape[1], a.shape[0]).T
        return self

    def download_column(self, name: str) -> np.ndarray:
        """D2H of ONE bound column (a Body column or a program component): what StepContext.read_component costs."""
        rc = self._lib.sixdof_download_column(self._h, L.component_id(name))
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_download_column")
        if name in self._soa:
            a = self._aux[name]
            a[...] = self._soa[name].reshape(a.shape[1], a.shape[0]).T
        return getattr(self, name) if name in ("world_pos", "world_vel", "world_accel", "force", "inertia") else self._aux[name]

    def upload_column(self, name: str) -> None:
        """H2D of ONE bound column from its host array (StepContext.write_component; copy_db_to_world's per-component copy): the
        other columns — which the host may never have downloaded — are left alone."""
        if name in self._soa:
            a = self._aux[name]
            self._soa[name].reshape(a.shape[1], a.shape[0])[...] = a.T
        rc = self._lib.sixdof_upload_column(self._h, L.component_id(name))
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_upload_column")

    def component(self, name: str) -> np.ndarray:
        """A generated program's component column as the reference lays it out.  Plain columns: the [n, w] host array
        itself.  Window components (dsl.Window) are kept as a ring on the device: un-rotated here to [n, rows, w], oldest
        row first — what `concatenate((buffer[1:], row))` leaves in the reference's column."""
        if name in getattr(self, "_mats", {}):
            return self._aux[name].reshape(self._aux[name].shape[0], *self._mats[name])
        if name not in self._windows:
            return self._aux[name]
        rows, width = self._windows[name]
        n = self._aux[name].shape[0]
        ring = (self._aux[name].reshape(rows * width, n).T if self._window_soa else self._aux[name]).reshape(n, rows, width)
        head = self._aux[name + "#head"][:, 0].astype(np.int64)
        idx = (head[:, None] + np.arange(rows)[None, :]) % rows
        return ring[np.arange(ring.shape[0])[:, None], idx]

    def run(self, ticks: int = 1) -> TickTimings:
        """PyExec.run (exec.rs:110-172) without the DB commit: step, then refresh the host columns."""
        t = self.invoke_batch(ticks)
        self.download()
        return t

    @property
    def tick(self) -> int:
        v = C.c_uint64()
        self._lib.sixdof_get_tick(self._h, C.byref(v))
        return int(v.value)

    def set_ticks_per_launch(self, k: int):
        rc = self._lib.sixdof_set_ticks_per_launch(self._h, int(k))
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_set_ticks_per_launch")

    def nonfinite_rows(self) -> np.ndarray:
        """Failure sentinel: boolean [n], True where a row's world_pos / world_vel holds NaN or Inf."""
        flags = np.zeros(self.n, dtype=np.uint8)
        cnt = C.c_uint64()
        rc = self._lib.sixdof_count_nonfinite(self._h, C.byref(cnt), flags.ctypes.data)
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_count_nonfinite")
        assert int(cnt.value) == int(flags.sum())
        return flags.astype(bool)

    def checkpoint(self) -> dict:
        """Sim state = the Body columns + tick (World is `Serialize` in the reference, world.rs:41-46)."""
        self.download()
        state = {k: getattr(self, k).copy() for k in ("world_pos", "world_vel", "world_accel", "force", "inertia")}
        state.update({f"aux:{k}": v.copy() for k, v in self._aux.items()})
        state["tick"] = self.tick
        return state

    def restore(self, state: dict):
        for k in ("world_pos", "world_vel", "world_accel", "force", "inertia"):
            getattr(self, k)[...] = state[k]
        for k, v in self._aux.items():
            v[...] = state[f"aux:{k}"]
        self._lib.sixdof_set_tick(self._h, int(state["tick"]))
        self.upload()

    def last_timings(self) -> TickTimings:
        t = L.Timings()
        self._lib.sixdof_last_timings(self._h, C.byref(t))
        return TickTimings(t.h2d_upload_ms, t.kernel_invoke_ms, t.d2h_download_ms, t.kernel_device_ms,
                           int(t.launches), int(t.ticks), t.kernel_sum_ms, int(t.graph_launches))

    def enable_history(self, ring_ticks: int):
        """Record every tick's world_pos/world_vel/world_accel/force in a device ring (sixdof_set_history)."""
        rc = self._lib.sixdof_set_history(self._h, int(ring_ticks))
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_set_history")
        self._ring_ticks = int(ring_ticks)      # what stream_series compares its batch with (stream_history sizes its own ring)

    def _refuse_window(self, name: str) -> None:
        if name in self._windows:
            raise ValueError(f"{name} is a window component: it is its own history (HipExec.component), the ring does not copy it per tick")

    def _recorded_width(self, name: str) -> int:
        """Row width of a component the ring records: a Body column, or a plain component column of a generated program."""
        self._refuse_window(name)
        return 7 if name == "world_pos" else (self._aux[name].shape[1] if name in self._aux else 6)

    @staticmethod
    def _sample_count(first_tick: int, last_tick: int, every: int) -> int:
        """How many of the ticks first_tick, first_tick + every, ... are at most last_tick (0 for an empty or malformed range:
        the library then says what is wrong with it)."""
        return (last_tick - first_tick) // every + 1 if every > 0 and last_tick >= first_tick else 0

    def history(self, name: str, first_tick: int, last_tick: int) -> np.ndarray:
        """exec.history() analogue: [last-first+1, n, w] block of component `name`, row k = state after tick first+k."""
        out = np.empty((last_tick - first_tick + 1, self.n, self._recorded_width(name)), dtype=self.dtype)
        for k, tick in enumerate(range(first_tick, last_tick + 1)):
            rc = self._lib.sixdof_history_read(self._h, L.component_id(name), tick, out[k].ctypes.data)
            if rc != L.OK:
                _raise(self._h, rc, "sixdof_history_read")
        return out

    # ---- watch lists: time series of chosen (entity, component) pairs out of the ring ---------------------------
    def set_watch(self, names: Sequence[str], entity_ids) -> None:
        """Choose what history_series / stream_series read: components `names` (world_pos / world_vel / world_accel / force and
        the plain component columns of a generated program) of the entities `entity_ids`, in that order; duplicates are
        allowed.  Independent of enable_history (either order).  Empty names and ids clear the watch."""
        names = [names] if isinstance(names, str) else list(names)
        for name in names:
            self._refuse_window(name)
        ids = np.ascontiguousarray(entity_ids, dtype=np.uint64).reshape(-1)
        comp = np.array([L.component_id(n) for n in names], dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        rc = self._lib.sixdof_set_watch(self._h, comp.ctypes.data_as(u64p), len(comp), ids.ctypes.data_as(u64p), len(ids))
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_set_watch")
        self._watch = (names, len(ids))

    def _series_buffers(self, n_samples: int):
        names, m = getattr(self, "_watch", ((), 0))
        out = {}
        for name in names:      # a name watched twice shares one entry: its buffer is filled once per occurrence, identically
            out[name] = np.empty((m, n_samples, self._recorded_width(name)), dtype=self.dtype)
        ptrs = (C.c_void_p * max(1, len(names)))(*[out[name].ctypes.data for name in names])
        return out, ptrs

    def history_series(self, first_tick: int, last_tick: int, every: int = 1) -> dict:
        """{name: [m, samples, w]} of the watched pairs: sample j of entity e is the state after tick first_tick + j * every,
        up to last_tick.  The rows are gathered on the device; m rows per sample cross the link, not n."""
        first_tick, last_tick, every = int(first_tick), int(last_tick), int(every)
        n_samples = self._sample_count(first_tick, last_tick, every)
        out, ptrs = self._series_buffers(n_samples)
        rc = self._lib.sixdof_watch_read(self._h, first_tick, n_samples, every, ptrs, 0)
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_watch_read")
        return out

    def stream_series(self, n_batches: int, ticks_per_batch: int, every: int = 1, consume=None, flags: int = 0) -> float:
        """stream_history for a watch: every `every`-th tick of the watched pairs to the host, overlapped with the stepper.
        After batch i is enqueued its samples are gathered on the compute stream and copied on the copy stream into one of two
        host buffer sets while batch i+1 computes; because the ring is read on the compute stream, a ring of one batch is
        enough (enabled here unless enable_history already made one at least that large).  `consume(batch_index, first_tick,
        {name: array [m, ticks_per_batch // every, w]})` sees a batch once it has landed — first_tick is the batch's first
        SAMPLED tick, the last one is the batch's last tick; the arrays are reused two batches later.  Returns the wall time in
        seconds.  (The ring size is the one enable_history was last called with: after a stream_history, which sizes its own
        ring, call enable_history again.)"""
        n_batches, ticks_per_batch, every = int(n_batches), int(ticks_per_batch), int(every)
        n_samples = self._stream_shape("stream_series", ticks_per_batch, every)
        if not getattr(self, "_watch", ((), 0))[0]:
            raise ValueError("stream_series: no watch (set_watch)")
        if getattr(self, "_ring_ticks", 0) < ticks_per_batch:
            self.enable_history(ticks_per_batch)
        bufs, ptrs = zip(*[self._series_buffers(n_samples) for _ in range(2)])

        def read(first_tick, k):
            rc = self._lib.sixdof_watch_read(self._h, first_tick, n_samples, every, ptrs[k], L.WATCH_ASYNC)
            if rc != L.OK:
                _raise(self._h, rc, "sixdof_watch_read")
        self.sync()              # nothing of an earlier streaming run is in flight
        return self._stream_batches(n_batches, ticks_per_batch, every, read, lambda k: bufs[k], consume, flags)   # samples end on the batch's last tick

    # ---- reductions over the ring into (group, element) bins: envelopes and quantiles -----------------------------------
    def _envelope_reduction(self) -> _Reduction:
        return _Reduction("sixdof_history_envelope", L.ENVELOPE_ASYNC, 5, (), self._envelope_dict)

    def _quantile_reduction(self, q) -> _Reduction:
        num, den = self.quantile_ranks(q)
        return _Reduction("sixdof_history_quantiles", L.QUANTILE_ASYNC, 1 + 2 * len(num), ((C.c_uint32 * len(num))(*num), den, len(num)),
                          lambda names, raw: self._quantile_dict(names, raw, num, den))

    @staticmethod
    def _stream_shape(who: str, ticks_per_batch: int, every: int) -> int:
        """Samples per batch of a stream_* call, or its ValueError."""
        if every < 1 or ticks_per_batch < 1 or ticks_per_batch % every != 0:
            raise ValueError(f"{who}: ticks_per_batch ({ticks_per_batch}) must be a positive multiple of every ({every})")
        return ticks_per_batch // every

    def _reduce_buffers(self, red: _Reduction, names, n_samples: int, period: int):
        raw = [np.empty((n_samples, max(period, 1), red.planes, self._recorded_width(name)), dtype=np.float64) for name in names]
        return raw, (C.c_void_p * max(1, len(names)))(*[a.ctypes.data for a in raw])

    def _reduce_read(self, red: _Reduction, comp, first_tick: int, n_samples: int, every: int, period: int, ptrs, flags: int) -> None:
        rc = getattr(self._lib, red.fn)(self._h, comp.ctypes.data_as(C.POINTER(C.c_uint64)), len(comp), first_tick, n_samples, every, period,
                                        *red.extra, ptrs, flags)
        if rc != L.OK:
            _raise(self._h, rc, red.fn)

    def _reduce(self, red: _Reduction, names, first_tick: int, last_tick: int, every: int, period: int) -> dict:
        """One blocking read of the samples first_tick, first_tick + every, ... <= last_tick."""
        names = [names] if isinstance(names, str) else list(names)
        first_tick, last_tick, every, period = int(first_tick), int(last_tick), int(every), int(period)
        n_samples = self._sample_count(first_tick, last_tick, every)
        raw, ptrs = self._reduce_buffers(red, names, n_samples, period)
        comp = np.array([L.component_id(n) for n in names], dtype=np.uint64)
        self._reduce_read(red, comp, first_tick, n_samples, every, max(period, 0), ptrs, 0)
        return red.to_dict(names, raw)

    def _stream_reduce(self, who: str, red: _Reduction, names, n_batches: int, ticks_per_batch: int, every: int, period: int, consume,
                       flags: int) -> float:
        """Every batch's samples read asynchronously into one of two host buffer sets while the next batch computes."""
        names = [names] if isinstance(names, str) else list(names)
        n_batches, ticks_per_batch, every, period = int(n_batches), int(ticks_per_batch), int(every), int(period)
        n_samples = self._stream_shape(who, ticks_per_batch, every)
        if period < 1:
            raise ValueError(f"{who}: period must be at least 1")
        if getattr(self, "_ring_ticks", 0) < ticks_per_batch:
            self.enable_history(ticks_per_batch)
        raw, ptrs = zip(*[self._reduce_buffers(red, names, n_samples, period) for _ in range(2)])
        comp = np.array([L.component_id(n) for n in names], dtype=np.uint64)
        self.sync()              # nothing of an earlier streaming run is in flight
        return self._stream_batches(n_batches, ticks_per_batch, every,
                                    lambda first_tick, k: self._reduce_read(red, comp, first_tick, n_samples, every, period, ptrs[k], red.async_flag),
                                    lambda k: red.to_dict(names, raw[k]), consume, flags)

    # ---- ring envelopes: count / min / max / mean / spread across the rows of every sampled tick -------------------
    ENVELOPE_STATS = ("count", "min", "max", "mean", "m2")

    @classmethod
    def _envelope_dict(cls, names, raw) -> dict:
        """[s, period, 5, w] blocks -> {name: {statistic: [s, period, w]}}, count as int64, std = sqrt(m2 / count) added."""
        out = {}
        for name, a in zip(names, raw):
            d = {k: a[:, :, i, :] for i, k in enumerate(cls.ENVELOPE_STATS)}
            with np.errstate(invalid="ignore", divide="ignore"):
                d["std"] = np.sqrt(d["m2"] / d["count"])
            d["count"] = d["count"].astype(np.int64)
            out[name] = d
        return out

    def history_envelope(self, names: Sequence[str], first_tick: int, last_tick: int, every: int = 1, period: int = 1) -> dict:
        """{name: {"count": int64 [s, period, w], "min", "max", "mean", "m2", "std": f64 [s, period, w]}} over the rows of ticks
        first_tick, first_tick + every, ... <= last_tick, reduced on the device out of the ring: entry [j, g, c] covers element c
        of the rows r with r % period == g (period = 1: all rows).  Non-finite elements are skipped and show as count below
        n / period; count == 0 leaves the statistics NaN.  Accumulated in f64; m2 is the sum of squared deviations from the mean
        and std = sqrt(m2 / count).  Stateless: no watch is involved."""
        return self._reduce(self._envelope_reduction(), names, first_tick, last_tick, every, period)

    def stream_envelope(self, names: Sequence[str], n_batches: int, ticks_per_batch: int, every: int = 1, period: int = 1, consume=None,
                        flags: int = 0) -> float:
        """stream_series for envelopes: every `every`-th tick of every batch reduced on the compute stream and copied on the copy
        stream into one of two host buffer sets while the next batch computes; a ring one batch deep is enough (enabled here
        unless enable_history already made one at least that large).  `consume(batch_index, first_tick, {name: {statistic:
        [ticks_per_batch // every, period, w]}})` sees a batch once it has landed — first_tick is the batch's first SAMPLED
        tick; the arrays are views of buffers reused two batches later.  Returns the wall time in seconds."""
        return self._stream_reduce("stream_envelope", self._envelope_reduction(), names, n_batches, ticks_per_batch, every, period, consume, flags)

    # ---- ring quantiles: exact order statistics across the rows of every sampled tick ---------------------------------
    @staticmethod
    def quantile_ranks(q):
        """(numerators, denominator) of the ranks `q` over one common denominator.  An entry is a fractions.Fraction, a
        (num, den) pair or a float; a float is read through its shortest decimal repr, Fraction(repr(x)), so 0.99 means 99/100
        and not the binary fraction next to it.  ValueError: no rank or more than 16, a rank outside [0, 1], a common
        denominator beyond 32 bits."""
        import math
        from fractions import Fraction
        fr = []
        for x in ([q] if isinstance(q, (int, float, Fraction)) else list(q)):
            if isinstance(x, Fraction):
                f = x
            elif isinstance(x, (tuple, list)):
                num, den = x
                if int(den) < 1:
                    raise ValueError(f"quantiles: rank {x!r} has no positive denominator")
                f = Fraction(int(num), int(den))
            else:
                x = float(x)
                if not math.isfinite(x):
                    raise ValueError(f"quantiles: rank {x!r} is not a number in [0, 1]")
                f = Fraction(repr(x))
            if not 0 <= f <= 1:
                raise ValueError(f"quantiles: rank {x!r} is outside [0, 1]")
            fr.append(f)
        if not 1 <= len(fr) <= L.QUANTILE_MAX_RANKS:
            raise ValueError(f"quantiles: {len(fr)} ranks, 1 to {L.QUANTILE_MAX_RANKS} can be asked for")
        den = 1
        for f in fr:
            den = den * f.denominator // math.gcd(den, f.denominator)
        if den > 0xFFFFFFFF:
            raise ValueError(f"quantiles: the ranks' common denominator {den} does not fit 32 bits")
        return [int(f * den) for f in fr], den

    @staticmethod
    def _quantile_dict(names, raw, num, den) -> dict:
        """[s, period, 1 + 2Q, w] blocks -> {name: {"count": int64 [s, period, w], "lower", "upper", "linear": [s, period, Q, w]}}.
        linear = lower + (upper - lower) * frac with frac = (num * (count - 1) mod den) / den, evaluated here in f64: what
        numpy's default ("linear") interpolation evaluates, up to rounding."""
        out = {}
        for name, a in zip(names, raw):
            count = a[:, :, 0, :].astype(np.int64)
            lower, upper = a[:, :, 1::2, :], a[:, :, 2::2, :]
            m1 = np.maximum(count - 1, 0).astype(object)[:, :, None, :]      # Python integers: num * (m - 1) is exact
            rem = (m1 * np.array(num, dtype=object)[None, None, :, None]) % den
            frac = rem.astype(np.float64) / float(den)
            with np.errstate(invalid="ignore"):
                linear = lower + (upper - lower) * frac
            out[name] = {"count": count, "lower": lower, "upper": upper, "linear": linear}
        return out

    def history_quantiles(self, names: Sequence[str], first_tick: int, last_tick: int, q, every: int = 1, period: int = 1) -> dict:
        """{name: {"count": int64 [s, period, w], "lower", "upper", "linear": f64 [s, period, Q, w]}}: exact order statistics over
        the rows of ticks first_tick, first_tick + every, ... <= last_tick, selected on the device out of the ring.  Entry
        [j, g, i, c] covers element c of the rows r with r % period == g and rank q[i] (quantile_ranks: Fractions, (num, den)
        pairs or floats read as their decimal repr).  With m = count finite elements x(0) <= ... <= x(m-1) (non-finite ones
        are skipped), lower = x(floor(q (m-1))) and upper = x(ceil(q (m-1))), rank arithmetic in integers: both are elements
        of the ring, bit for bit (-0.0 below +0.0).  linear = lower + (upper - lower) * frac, frac = (num (m-1) mod den) / den in
        f64 on the host.  count == 0 leaves the three NaN.  Stateless: no watch is involved."""
        return self._reduce(self._quantile_reduction(q), names, first_tick, last_tick, every, period)

    def stream_quantiles(self, names: Sequence[str], n_batches: int, ticks_per_batch: int, q, every: int = 1, period: int = 1, consume=None,
                         flags: int = 0) -> float:
        """stream_envelope for quantiles: every `every`-th tick of every batch selected on the compute stream and copied on the
        copy stream into one of two host buffer sets while the next batch computes; a ring one batch deep is enough (enabled
        here unless enable_history already made one at least that large).  `consume(batch_index, first_tick, {name: {"count",
        "lower", "upper", "linear"}})` sees a batch once it has landed — first_tick is the batch's first SAMPLED tick; lower and
        upper are views of buffers reused two batches later.  Returns the wall time in seconds."""
        return self._stream_reduce("stream_quantiles", self._quantile_reduction(q), names, n_batches, ticks_per_batch, every, period, consume, flags)

    # ---- ring covariances: count, mean vector and co-moment matrix of a few channels across the rows of every sampled tick -------
    @staticmethod
    def covariance_fields(k: int) -> int:
        """Doubles of one (sample, group) entry of a k-channel read: count, k means, the k (k + 1) / 2 values of the upper triangle."""
        return 1 + k + k * (k + 1) // 2

    def _covariance_channels(self, who: str, channels):
        """[(name, element), ...] -> the ctypes array.  ValueError: fewer than 2 or more than 6 channels, an element outside its
        component's width (the library refuses the same; here the message names the channel)."""
        channels = [(str(name), int(element)) for name, element in channels]
        if len(channels) == 1:
            raise ValueError(f"{who}: one channel has no co-moments: its count, mean and m2 are history_envelope's")
        if not 2 <= len(channels) <= L.COVARIANCE_MAX_CHANNELS:
            raise ValueError(f"{who}: {len(channels)} channels, 2 to {L.COVARIANCE_MAX_CHANNELS} can be asked for")
        arr = (L.CovChannel * len(channels))()
        for i, (name, element) in enumerate(channels):
            w = self._recorded_width(name)
            if not 0 <= element < w:
                raise ValueError(f"{who}: channel {i}: element {element} of {name}, which is {w} wide")
            arr[i].component_id, arr[i].element, arr[i].reserved = L.component_id(name), element, 0
        return channels, arr

    @staticmethod
    def _covariance_dict(raw: np.ndarray, k: int) -> dict:
        """[s, period, 1 + k + k (k + 1) / 2] -> {"count": int64 [s, period], "mean": [s, period, k], "comoment", "cov", "corr":
        [s, period, k, k]}: the upper triangle mirrored into the full symmetric matrix, cov = comoment / count (the population
        form, as the envelope's std = sqrt(m2 / count)), corr = C_ab / sqrt(C_aa C_bb), NaN where a diagonal is 0 or count is 0."""
        s, period = raw.shape[:2]
        count = raw[:, :, 0]
        iu = np.triu_indices(k)
        comoment = np.empty((s, period, k, k), dtype=np.float64)
        comoment[:, :, iu[0], iu[1]] = raw[:, :, 1 + k:]
        comoment[:, :, iu[1], iu[0]] = raw[:, :, 1 + k:]
        diag = np.einsum("spaa->spa", comoment)
        with np.errstate(invalid="ignore", divide="ignore"):
            cov = comoment / count[:, :, None, None]
            scale = np.sqrt(diag[:, :, :, None] * diag[:, :, None, :])
            corr = np.where(scale > 0, comoment / scale, np.nan)
        return {"count": count.astype(np.int64), "mean": raw[:, :, 1:1 + k], "comoment": comoment, "cov": cov, "corr": corr}

    def _covariance_read(self, arr, first_tick: int, n_samples: int, every: int, period: int, raw: np.ndarray, flags: int) -> None:
        rc = self._lib.sixdof_history_covariance(self._h, arr, len(arr), first_tick, n_samples, every, period, raw.ctypes.data, flags)
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_history_covariance")

    def history_covariance(self, channels, first_tick: int, last_tick: int, every: int = 1, period: int = 1) -> dict:
        """Joint moments of 2 to 6 channels — `channels` is a sequence of (component name, element) — over the rows of ticks
        first_tick, first_tick + every, ... <= last_tick, reduced on the device out of the ring: {"count": int64 [s, period],
        "mean": [s, period, k], "comoment", "cov", "corr": [s, period, k, k]}.  Entry [j, g] covers the rows r with r % period == g
        (period = 1: all rows).  Listwise: a row counts only if all k channel values are finite, so the matrix is that of one
        population; count == 0 leaves everything else NaN.  comoment[a, b] = sum (x_a - mean_a)(x_b - mean_b), cov = comoment /
        count, corr the correlation matrix (NaN where a variance is 0).  Accumulated in f64.  Stateless: no watch is involved."""
        first_tick, last_tick, every, period = int(first_tick), int(last_tick), int(every), int(period)
        channels, arr = self._covariance_channels("history_covariance", channels)
        n_samples = self._sample_count(first_tick, last_tick, every)
        raw = np.empty((n_samples, max(period, 1), self.covariance_fields(len(channels))), dtype=np.float64)
        self._covariance_read(arr, first_tick, n_samples, every, max(period, 0), raw, 0)
        return self._covariance_dict(raw, len(channels))

    def stream_covariance(self, channels, n_batches: int, ticks_per_batch: int, every: int = 1, period: int = 1, consume=None, flags: int = 0) -> float:
        """stream_envelope for covariances: every `every`-th tick of every batch reduced on the compute stream and copied on the
        copy stream into one of two host buffers while the next batch computes; a ring one batch deep is enough (enabled here
        unless enable_history already made one at least that large).  `consume(batch_index, first_tick, {"count", "mean",
        "comoment", "cov", "corr"})` sees a batch once it has landed — first_tick is the batch's first SAMPLED tick; mean is a
        view of a buffer reused two batches later.  Returns the wall time in seconds."""
        n_batches, ticks_per_batch, every, period = int(n_batches), int(ticks_per_batch), int(every), int(period)
        channels, arr = self._covariance_channels("stream_covariance", channels)
        n_samples = self._stream_shape("stream_covariance", ticks_per_batch, every)
        if period < 1:
            raise ValueError("stream_covariance: period must be at least 1")
        if getattr(self, "_ring_ticks", 0) < ticks_per_batch:
            self.enable_history(ticks_per_batch)
        raw = [np.empty((n_samples, period, self.covariance_fields(len(channels))), dtype=np.float64) for _ in range(2)]
        self.sync()              # nothing of an earlier streaming run is in flight
        return self._stream_batches(n_batches, ticks_per_batch, every,
                                    lambda first_tick, k: self._covariance_read(arr, first_tick, n_samples, every, period, raw[k], L.COVARIANCE_ASYNC),
                                    lambda k: self._covariance_dict(raw[k], len(channels)), consume, flags)

    # ---- ring extremes: every row collapsed across time, and the ticks its extremes fall on -----------------------------
    EXTREMES_FIELDS = ("count", "min", "argmin", "max", "argmax", "first_nonfinite")      # the six planes, in order

    @staticmethod
    def _extremes_dict(names, raw) -> dict:
        """[6, n, w] blocks -> {name: {"count", "argmin", "argmax", "first_nonfinite": int64 [n, w]; "min", "max": f64 [n, w]}}.
        The integer planes arrive as doubles below 2^53: the conversion is exact."""
        out = {}
        for name, a in zip(names, raw):
            out[name] = {k: a[i] if k in ("min", "max") else a[i].astype(np.int64) for i, k in enumerate(HipExec.EXTREMES_FIELDS)}
        return out

    def _extremes_buffers(self, names):
        """One [6, n, w] block per name, holding what a range without samples reduces to: count 0, NaN extremes, no ticks."""
        raw = [np.zeros((L.EXTREMES_PLANES, self.n, self._recorded_width(name)), dtype=np.float64) for name in names]
        for a in raw:
            a[1], a[3] = np.nan, np.nan
        return raw, (C.c_void_p * max(1, len(names)))(*[a.ctypes.data for a in raw])

    def _extremes_read(self, comp, first_tick: int, n_samples: int, every: int, ptrs, flags: int) -> None:
        rc = self._lib.sixdof_history_extremes(self._h, comp.ctypes.data_as(C.POINTER(C.c_uint64)), len(comp), first_tick, n_samples, every, ptrs, flags)
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_history_extremes")

    def history_extremes(self, names: Sequence[str], first_tick: int, last_tick: int, every: int = 1) -> dict:
        """{name: {"count", "argmin", "argmax", "first_nonfinite": int64 [n, w]; "min", "max": f64 [n, w]}}: every row collapsed
        across the ticks first_tick, first_tick + every, ... <= last_tick, reduced on the device out of the ring.  Per row and
        element: count of the samples at which it is finite, its smallest and largest finite value — elements of the ring, bit
        for bit, -0.0 below +0.0 — with the EARLIEST sampled tick that holds each, and the earliest sampled tick at which it is
        not finite.  0 in a tick field means none; count == 0 leaves min and max NaN.  Stateless: no watch is involved."""
        names = [names] if isinstance(names, str) else list(names)
        first_tick, last_tick, every = int(first_tick), int(last_tick), int(every)
        raw, ptrs = self._extremes_buffers(names)
        comp = np.array([L.component_id(n) for n in names], dtype=np.uint64)
        self._extremes_read(comp, first_tick, self._sample_count(first_tick, last_tick, every), every, ptrs, 0)
        return self._extremes_dict(names, raw)

    def stream_extremes(self, names: Sequence[str], n_batches: int, ticks_per_batch: int, every: int = 1, flags: int = 0):
        """history_extremes over a run longer than the ring: n_batches batches of ticks_per_batch ticks are stepped, and after
        every batch its samples — every `every`-th tick, ending on the batch's last — are merged into the accumulator on the
        device (SIXDOF_EXTREMES_HOLD, SIXDOF_EXTREMES_CONTINUE from the second batch on).  Nothing crosses the link until the last
        batch's call delivers.  The ring is read on the compute stream, so a ring one batch deep is enough (enabled here unless
        enable_history already made one at least that large).  Returns (wall time in seconds, the dict of history_extremes);
        whatever happens, the caller's flags are restored and the handle is drained."""
        names = [names] if isinstance(names, str) else list(names)
        n_batches, ticks_per_batch, every = int(n_batches), int(ticks_per_batch), int(every)
        n_samples = self._stream_shape("stream_extremes", ticks_per_batch, every)
        if n_batches < 1:
            raise ValueError("stream_extremes: at least one batch")
        raw, ptrs = self._extremes_buffers(names)
        comp = np.array([L.component_id(n) for n in names], dtype=np.uint64)
        wall = self._stream_accumulate(n_batches, ticks_per_batch, every, L.EXTREMES_CONTINUE, L.EXTREMES_HOLD, flags,
                                       lambda first, last, fl: self._extremes_read(comp, first, n_samples, every, ptrs if last else None, fl))
        return wall, self._extremes_dict(names, raw)

    def _stream_accumulate(self, n_batches: int, ticks_per_batch: int, every: int, continue_flag: int, hold_flag: int, flags: int, read) -> float:
        """The loop of stream_extremes / stream_events / stream_norms / stream_norm_events: every batch is stepped and its samples — ending on the batch's last tick —
        are merged into an accumulator on the device by `read(first_tick, last, read_flags)`: held unless the batch is the last,
        continuing from the second batch on.  A ring one batch deep is enabled unless there is one at least that large.
        Whatever happens, the caller's flags are restored and the handle is drained.  Returns the wall time in seconds."""
        import time
        if getattr(self, "_ring_ticks", 0) < ticks_per_batch:
            self.enable_history(ticks_per_batch)
        self.sync()              # nothing of an earlier streaming run is in flight
        self.set_flags(flags | L.FLAG_ASYNC_STEP)
        t0 = time.perf_counter()
        try:
            for i in range(n_batches):
                first = self.tick + every                                # samples end on the batch's last tick
                self.invoke_batch(ticks_per_batch)
                last = i + 1 == n_batches
                read(first, last, (continue_flag if i else 0) | (0 if last else hold_flag))
        finally:
            self.set_flags(flags)
            self.sync()
        return time.perf_counter() - t0

    # ---- scans of the ring across time per run: events, norms and norm events -------------------------------------------
    def _scan_buffers(self, scan: _Scan, n_items: int, capture, period: int):
        """The raw block, the capture blocks, their pointers and the captured component ids, holding what a range without samples gives."""
        if not scan.captures:
            return (scan.buffer or HipExec._norms_buffer)(self, n_items, period), [], None, None
        raw, caps, ptrs = self._events_buffers(n_items, capture, period)
        return raw, caps, ptrs, np.array([L.component_id(n) for n in capture], dtype=np.uint64)

    def _scan_read(self, scan: _Scan, items, comp, period: int, first_tick: int, n_samples: int, every: int, raw, ptrs, flags: int) -> None:
        """One call of the scan's entry point for the ctypes array `items`; raw None: a held read, nothing is delivered."""
        captures = (comp.ctypes.data_as(C.POINTER(C.c_uint64)), len(comp)) if scan.captures else ()
        rc = getattr(self._lib, scan.fn)(self._h, items, len(items), *captures, period, first_tick, n_samples, every,
                                         None if raw is None else raw.ctypes.data, *((ptrs,) if scan.captures else ()), flags)
        if rc != L.OK:
            _raise(self._h, rc, scan.fn)

    def _scan(self, scan: _Scan, items, capture, first_tick: int, last_tick: int, every: int, period: int) -> dict:
        """One blocking read of the samples first_tick, first_tick + every, ... <= last_tick."""
        capture = [capture] if isinstance(capture, str) else list(capture)
        first_tick, last_tick, every, period = int(first_tick), int(last_tick), int(every), int(period)
        raw, caps, ptrs, comp = self._scan_buffers(scan, len(items), capture, period)
        self._scan_read(scan, items, comp, max(period, 0), first_tick, self._sample_count(first_tick, last_tick, every), every, raw, ptrs, 0)
        return scan.to_dict(capture, raw, caps)

    def _stream_scan(self, scan: _Scan, items, capture, n_batches: int, ticks_per_batch: int, every: int, period: int, flags: int):
        """Every batch's samples merged into the accumulator on the device, the last batch's call delivering (_stream_accumulate)."""
        capture = [capture] if isinstance(capture, str) else list(capture)
        n_batches, ticks_per_batch, every, period = int(n_batches), int(ticks_per_batch), int(every), int(period)
        n_samples = self._stream_shape(f"stream_{scan.name}", ticks_per_batch, every)
        if n_batches < 1:
            raise ValueError(f"stream_{scan.name}: at least one batch")
        if period < 1:
            raise ValueError(f"stream_{scan.name}: period must be at least 1")
        raw, caps, ptrs, comp = self._scan_buffers(scan, len(items), capture, period)
        wall = self._stream_accumulate(n_batches, ticks_per_batch, every, scan.continue_flag, scan.hold_flag, flags,
                                       lambda first, last, fl: self._scan_read(scan, items, comp, period, first, n_samples, every, raw if last else None,
                                                                               ptrs if last else None, fl))
        return wall, scan.to_dict(capture, raw, caps)

    # ---- ring events: the first threshold crossing of every run, and the state there -----------------------------------
    EVENTS_FIELDS = ("tick", "value", "tick_before", "value_before")      # the four planes, in order

    @staticmethod
    def _events_dict(capture_names, raw_events, raw_captures) -> dict:
        """A [T, 4, runs] block and one [T, n, w] block per captured name -> {"tick", "tick_before": int64 [T, runs]; "value",
        "value_before": f64 [T, runs]; "capture": {name: f64 [T, n, w]}}.  The tick planes arrive as doubles below 2^53: the
        conversion is exact."""
        out = {k: raw_events[:, i] if k.startswith("value") else raw_events[:, i].astype(np.int64) for i, k in enumerate(HipExec.EVENTS_FIELDS)}
        out["capture"] = dict(zip(capture_names, raw_captures))
        return out

    @staticmethod
    def _event_triggers(events):
        """The ctypes array of sixdof_event_trigger for a list of Event, or its ValueError."""
        events = [events] if isinstance(events, Event) else list(events)
        if not 1 <= len(events) <= L.EVENTS_MAX_TRIGGERS:
            raise ValueError(f"history_events: {len(events)} events, 1 to {L.EVENTS_MAX_TRIGGERS} can be asked for")
        arr = (L.EventTrigger * len(events))()
        for t, e in zip(arr, events):
            if e.op not in Event.OPS or e.mode not in Event.MODES:
                raise ValueError(f"history_events: {e!r}: op is one of {list(Event.OPS)}, mode one of {list(Event.MODES)}")
            t.component_id, t.element, t.group = L.component_id(e.component), int(e.element), int(e.group)
            t.op, t.mode, t.level = Event.OPS[e.op], Event.MODES[e.mode], float(e.level)
        return arr

    def _events_buffers(self, n_events: int, capture, period: int):
        """The [T, 4, runs] block and one [T, n, w] block per captured name, holding what a range without samples gives: no event."""
        raw = np.zeros((n_events, L.EVENTS_PLANES, self.n // max(period, 1)), dtype=np.float64)
        raw[:, 1], raw[:, 3] = np.nan, np.nan
        caps = [np.full((n_events, self.n, self._recorded_width(name)), np.nan, dtype=np.float64) for name in capture]
        return raw, caps, (C.c_void_p * max(1, len(caps)))(*[a.ctypes.data for a in caps])

    _EVENTS_SCAN = _Scan("sixdof_history_events", L.EVENTS_CONTINUE, L.EVENTS_HOLD, "events", True,
                         lambda capture, raw, caps: HipExec._events_dict(capture, raw, caps))

    def history_events(self, events, capture: Sequence[str], first_tick: int, last_tick: int, every: int = 1, period: int = 1) -> dict:
        """{"tick", "tick_before": int64 [T, runs]; "value", "value_before": f64 [T, runs]; "capture": {name: f64 [T, n, w]}}: per
        Event and run (period consecutive rows; runs = n // period), over the ticks first_tick, first_tick + every, ... <=
        last_tick, the first sampled tick at which the event's element meets its threshold, the element's value there, and tick
        and value of the finite sample before — found on the device out of the ring.  capture[name][e, r] is row r of `name` at
        the event tick of r's run for event e.  tick 0 means no event: value and the run's captured rows are then NaN;
        tick_before 0 means no sample before it.  Non-finite samples are skipped.  Stateless: no watch is involved."""
        return self._scan(self._EVENTS_SCAN, self._event_triggers(events), capture, first_tick, last_tick, every, period)

    def stream_events(self, events, capture: Sequence[str], n_batches: int, ticks_per_batch: int, every: int = 1, period: int = 1, flags: int = 0):
        """history_events over a run longer than the ring: n_batches batches of ticks_per_batch ticks are stepped, and after every
        batch its samples — every `every`-th tick, ending on the batch's last — are merged into the accumulator on the device
        (SIXDOF_EVENTS_HOLD, SIXDOF_EVENTS_CONTINUE from the second batch on); a run's rows are captured in the batch that sees its
        event.  Nothing crosses the link until the last batch's call delivers.  The ring is read on the compute stream, so a ring
        one batch deep is enough (enabled here unless enable_history already made one at least that large).  Returns (wall time
        in seconds, the dict of history_events); whatever happens, the caller's flags are restored and the handle is drained."""
        return self._stream_scan(self._EVENTS_SCAN, self._event_triggers(events), capture, n_batches, ticks_per_batch, every, period, flags)

    # ---- ring norms: per-run extremes of a vector's length or of a separation ---------------------------------------------
    NORMS_FIELDS = ("count", "min_sq", "argmin", "max_sq", "argmax", "first_nonfinite")      # the six planes, in order

    @staticmethod
    def _norms_dict(raw) -> dict:
        """A [P, 6, runs] block -> {"count", "argmin", "argmax", "first_nonfinite": int64 [P, runs]; "min_sq", "max_sq", "min",
        "max": f64 [P, runs]}.  The integer planes arrive as doubles below 2^53: the conversion is exact.  min and max are the
        square roots of the _sq fields, taken here on the host."""
        out = {k: raw[:, i] if k.endswith("_sq") else raw[:, i].astype(np.int64) for i, k in enumerate(HipExec.NORMS_FIELDS)}
        out["min"], out["max"] = np.sqrt(out["min_sq"]), np.sqrt(out["max_sq"])
        return out

    @staticmethod
    def _norm_probes(norms):
        """The ctypes array of sixdof_norm_probe for a list of Norm, or its ValueError."""
        norms = [norms] if isinstance(norms, Norm) else list(norms)
        if not 1 <= len(norms) <= L.NORMS_MAX_PROBES:
            raise ValueError(f"history_norms: {len(norms)} norms, 1 to {L.NORMS_MAX_PROBES} can be asked for")
        arr = (L.NormProbe * len(norms))()
        for p, v in zip(arr, norms):
            HipExec._norm_probe_fill(p, v, "history_norms")
        return arr

    @staticmethod
    def _norm_probe_fill(p, v, who: str) -> None:
        """Fills the sixdof_norm_probe `p` from the Norm `v`, or raises its ValueError in the name of `who`."""
        if not 1 <= int(v.count) <= L.NORM_MAX_COUNT:
            raise ValueError(f"{who}: {v!r}: count is 1 to {L.NORM_MAX_COUNT}")
        if v.minus is None and (v.minus_element is not None or v.minus_group is not None):
            raise ValueError(f"{who}: {v!r}: minus_element and minus_group need minus, the component they index")
        if min(int(v.element), int(v.group), int(v.element if v.minus_element is None else v.minus_element),
               int(v.group if v.minus_group is None else v.minus_group)) < 0:
            raise ValueError(f"{who}: {v!r}: a negative element or group")
        p.component_id, p.element, p.group, p.count = L.component_id(v.component), int(v.element), int(v.group), int(v.count)
        if v.minus is not None:
            p.flags, p.minus_component_id = L.NORM_MINUS, L.component_id(v.minus)
            p.minus_element = int(v.element if v.minus_element is None else v.minus_element)
            p.minus_group = int(v.group if v.minus_group is None else v.minus_group)

    def _norms_buffer(self, n_norms: int, period: int) -> np.ndarray:
        """The [P, 6, runs] block, holding what a range without samples reduces to: count 0, NaN extremes, no ticks."""
        raw = np.zeros((n_norms, L.NORMS_PLANES, self.n // max(period, 1)), dtype=np.float64)
        raw[:, 1], raw[:, 3] = np.nan, np.nan
        return raw

    _NORMS_SCAN = _Scan("sixdof_history_norms", L.NORMS_CONTINUE, L.NORMS_HOLD, "norms", False, lambda capture, raw, caps: HipExec._norms_dict(raw))

    def history_norms(self, norms, first_tick: int, last_tick: int, every: int = 1, period: int = 1) -> dict:
        """{"count", "argmin", "argmax", "first_nonfinite": int64 [P, runs]; "min_sq", "max_sq", "min", "max": f64 [P, runs]}: per
        Norm and run (period consecutive rows; runs = n // period), over the ticks first_tick, first_tick + every, ... <= last_tick,
        the smallest and the largest squared norm with the EARLIEST sampled tick that holds each, the count of samples at which
        the squared norm is finite and the earliest tick at which it is not — reduced on the device out of the ring.  The
        squared norm is formed in f64, left to right, from the ring's elements widened to double; one that overflows counts as
        non-finite.  0 in a tick field means none; count == 0 leaves the extremes NaN.  Stateless: no watch is involved."""
        return self._scan(self._NORMS_SCAN, self._norm_probes(norms), (), first_tick, last_tick, every, period)

    def stream_norms(self, norms, n_batches: int, ticks_per_batch: int, every: int = 1, period: int = 1, flags: int = 0):
        """history_norms over a run longer than the ring: n_batches batches of ticks_per_batch ticks are stepped, and after every
        batch its samples — every `every`-th tick, ending on the batch's last — are merged into the accumulator on the device
        (SIXDOF_NORMS_HOLD, SIXDOF_NORMS_CONTINUE from the second batch on).  Nothing crosses the link until the last batch's call
        delivers.  The ring is read on the compute stream, so a ring one batch deep is enough (enabled here unless enable_history
        already made one at least that large).  Returns (wall time in seconds, the dict of history_norms); whatever happens, the
        caller's flags are restored and the handle is drained."""
        return self._stream_scan(self._NORMS_SCAN, self._norm_probes(norms), (), n_batches, ticks_per_batch, every, period, flags)

    # ---- ring norm events: the first crossing of a vector's length or of a separation per run, and the state there ------------
    NORM_EVENTS_FIELDS = ("tick", "value_sq", "tick_before", "value_before_sq")      # the four planes, in order

    @staticmethod
    def _norm_events_dict(capture_names, raw_events, raw_captures) -> dict:
        """A [T, 4, runs] block and one [T, n, w] block per captured name -> {"tick", "tick_before": int64 [T, runs]; "value_sq",
        "value_before_sq", "value", "value_before": f64 [T, runs]; "capture": {name: f64 [T, n, w]}}.  The tick planes arrive as
        doubles below 2^53: the conversion is exact.  value and value_before are the square roots of the _sq fields, taken here on
        the host: NaN stays NaN, +0.0 stays +0.0."""
        out = {k: raw_events[:, i] if k.endswith("_sq") else raw_events[:, i].astype(np.int64) for i, k in enumerate(HipExec.NORM_EVENTS_FIELDS)}
        out["value"], out["value_before"] = np.sqrt(out["value_sq"]), np.sqrt(out["value_before_sq"])
        out["capture"] = dict(zip(capture_names, raw_captures))
        return out

    @staticmethod
    def _norm_triggers(events):
        """The ctypes array of sixdof_norm_trigger for a list of NormEvent — level_sq is level * level — or its ValueError."""
        events = [events] if isinstance(events, NormEvent) else list(events)
        if not 1 <= len(events) <= L.NORM_EVENTS_MAX_TRIGGERS:
            raise ValueError(f"history_norm_events: {len(events)} events, 1 to {L.NORM_EVENTS_MAX_TRIGGERS} can be asked for")
        arr = (L.NormTrigger * len(events))()
        for t, e in zip(arr, events):
            if e.op not in Event.OPS or e.mode not in Event.MODES:
                raise ValueError(f"history_norm_events: {e!r}: op is one of {list(Event.OPS)}, mode one of {list(Event.MODES)}")
            level = float(e.level)
            if not (math.isfinite(level) and level >= 0.0 and math.isfinite(level * level)):
                raise ValueError(f"history_norm_events: {e!r}: level is finite, not negative, and its square is finite")
            HipExec._norm_probe_fill(t.probe, e.norm, "history_norm_events")
            t.level_sq, t.op, t.mode = level * level, Event.OPS[e.op], Event.MODES[e.mode]
        return arr

    _NORM_EVENTS_SCAN = _Scan("sixdof_history_norm_events", L.NORM_EVENTS_CONTINUE, L.NORM_EVENTS_HOLD, "norm_events", True,
                              lambda capture, raw, caps: HipExec._norm_events_dict(capture, raw, caps))

    def history_norm_events(self, events, capture: Sequence[str], first_tick: int, last_tick: int, every: int = 1, period: int = 1) -> dict:
        """{"tick", "tick_before": int64 [T, runs]; "value_sq", "value_before_sq", "value", "value_before": f64 [T, runs]; "capture":
        {name: f64 [T, n, w]}}: per NormEvent and run (period consecutive rows; runs = n // period), over the ticks first_tick,
        first_tick + every, ... <= last_tick, the first sampled tick at which the event's norm meets its level, the squared norm
        there, and tick and squared norm of the finite sample before — found on the device out of the ring.  The squared norm is
        history_norms' (f64, left to right); one that is not finite, an overflowing one included, is skipped.  capture[name][e, r]
        is row r of `name` at the event tick of r's run for event e.  tick 0 means no event: the values and the run's captured rows
        are then NaN; tick_before 0 means no sample before it.  Stateless: no watch is involved."""
        return self._scan(self._NORM_EVENTS_SCAN, self._norm_triggers(events), capture, first_tick, last_tick, every, period)

    def stream_norm_events(self, events, capture: Sequence[str], n_batches: int, ticks_per_batch: int, every: int = 1, period: int = 1, flags: int = 0):
        """history_norm_events over a run longer than the ring: n_batches batches of ticks_per_batch ticks are stepped, and after
        every batch its samples — every `every`-th tick, ending on the batch's last — are merged into the accumulator on the
        device (SIXDOF_NORM_EVENTS_HOLD, SIXDOF_NORM_EVENTS_CONTINUE from the second batch on); a run's rows are captured in the
        batch that sees its event.  Nothing crosses the link until the last batch's call delivers.  A ring one batch deep is
        enough (enabled here unless enable_history already made one at least that large).  Returns (wall time in seconds, the
        dict of history_norm_events); whatever happens, the caller's flags are restored and the handle is drained."""
        return self._stream_scan(self._NORM_EVENTS_SCAN, self._norm_triggers(events), capture, n_batches, ticks_per_batch, every, period, flags)

    # ---- ring dwell: per run, how long and how often a condition held -------------------------------------------------------
    DWELL_FIELDS = ("count", "held", "entries", "first_held", "last_held", "prefix_len", "prefix_end", "suffix_len", "suffix_start",
                    "longest", "longest_start", "longest_end")      # the twelve planes, in order

    @staticmethod
    def _dwell_dict(raw) -> dict:
        """A [D, 12, runs] block -> {"count", "held", "entries", "first_held", "last_held", "longest", "longest_start",
        "longest_end": int64 [D, runs]; "open_at_start", "open_at_end": bool [D, runs]; "fraction": f64 [D, runs]}.  The planes
        arrive as doubles below 2^53: the conversion is exact.  open_at_start and open_at_end say whether the first and the last
        finite sample hold; fraction is held / count, NaN where count is 0."""
        words = {k: raw[:, i].astype(np.int64) for i, k in enumerate(HipExec.DWELL_FIELDS)}
        out = {k: words[k] for k in ("count", "held", "entries", "first_held", "last_held", "longest", "longest_start", "longest_end")}
        out["open_at_start"], out["open_at_end"] = words["prefix_len"] > 0, words["suffix_len"] > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            out["fraction"] = np.where(out["count"] == 0, np.nan, out["held"] / np.maximum(out["count"], 1))
        return out

    @staticmethod
    def _dwell_conditions(conditions):
        """The ctypes array of sixdof_dwell_condition for a list of Dwell — an Element becomes SIXDOF_DWELL_ELEMENT with its levels
        as they are, a Norm SIXDOF_DWELL_NORM_SQ with squared levels — or its ValueError."""
        conditions = [conditions] if isinstance(conditions, Dwell) else list(conditions)
        if not 1 <= len(conditions) <= L.DWELL_MAX_CONDITIONS:
            raise ValueError(f"history_dwell: {len(conditions)} conditions, 1 to {L.DWELL_MAX_CONDITIONS} can be asked for")
        arr = (L.DwellCondition * len(conditions))()
        for c, d in zip(arr, conditions):
            if d.op not in Dwell.OPS:
                raise ValueError(f"history_dwell: {d!r}: op is one of {list(Dwell.OPS)}")
            band = d.op in ("inside", "outside")
            if band != (d.upper is not None):
                raise ValueError(f"history_dwell: {d!r}: upper goes with \"inside\" and \"outside\", and only with them")
            lo, hi = float(d.level), float(d.upper) if band else 0.0
            if not (math.isfinite(lo) and math.isfinite(hi)) or (band and lo > hi):
                raise ValueError(f"history_dwell: {d!r}: levels are finite, and level is not above upper")
            if isinstance(d.of, Norm):
                if lo < 0.0 or hi < 0.0 or not (math.isfinite(lo * lo) and math.isfinite(hi * hi)):
                    raise ValueError(f"history_dwell: {d!r}: the levels of a Norm are not negative, and their squares are finite")
                norm, c.kind, lo, hi = d.of, L.DWELL_NORM_SQ, lo * lo, hi * hi
            elif isinstance(d.of, Element):
                e = d.of
                norm, c.kind = Norm(e.component, e.element, 1, e.group, e.minus, e.minus_element, e.minus_group), L.DWELL_ELEMENT
            else:
                raise ValueError(f"history_dwell: {d!r}: `of` is an Element or a Norm")
            HipExec._norm_probe_fill(c.probe, norm, "history_dwell")
            c.lo, c.hi, c.op = lo, hi, Dwell.OPS[d.op]
        return arr

    def _dwell_buffer(self, n_conditions: int, period: int) -> np.ndarray:
        """The [D, 12, runs] block, holding what a range without samples reduces to: nothing counted, no ticks."""
        return np.zeros((n_conditions, L.DWELL_PLANES, self.n // max(period, 1)), dtype=np.float64)

    _DWELL_SCAN = _Scan("sixdof_history_dwell", L.DWELL_CONTINUE, L.DWELL_HOLD, "dwell", False, lambda capture, raw, caps: HipExec._dwell_dict(raw),
                        lambda self, n_conditions, period: self._dwell_buffer(n_conditions, period))

    def history_dwell(self, conditions, first_tick: int, last_tick: int, every: int = 1, period: int = 1) -> dict:
        """{"count", "held", "entries", "first_held", "last_held", "longest", "longest_start", "longest_end": int64 [D, runs];
        "open_at_start", "open_at_end": bool [D, runs]; "fraction": f64 [D, runs]}: per Dwell and run (period consecutive rows;
        runs = n // period), over the ticks first_tick, first_tick + every, ... <= last_tick, how long and how often the condition
        held — counted on the device out of the ring.  count is the samples at which the value is finite (the others are skipped:
        a stretch continues across them), held those at which the condition holds, entries the maximal stretches of consecutive
        held samples, longest the length in samples of the EARLIEST stretch of maximal length, from tick longest_start to tick
        longest_end.  0 in a tick field means none.  Stateless: no watch is involved."""
        return self._scan(self._DWELL_SCAN, self._dwell_conditions(conditions), (), first_tick, last_tick, every, period)

    def stream_dwell(self, conditions, n_batches: int, ticks_per_batch: int, every: int = 1, period: int = 1, flags: int = 0):
        """history_dwell over a run longer than the ring: n_batches batches of ticks_per_batch ticks are stepped, and after every
        batch its samples — every `every`-th tick, ending on the batch's last — are merged into the accumulator on the device
        (SIXDOF_DWELL_HOLD, SIXDOF_DWELL_CONTINUE from the second batch on); a stretch that spans a batch boundary is one stretch.
        Nothing crosses the link until the last batch's call delivers.  A ring one batch deep is enough (enabled here unless
        enable_history already made one at least that large).  Returns (wall time in seconds, the dict of history_dwell); whatever
        happens, the caller's flags are restored and the handle is drained."""
        return self._stream_scan(self._DWELL_SCAN, self._dwell_conditions(conditions), (), n_batches, ticks_per_batch, every, period, flags)

    def set_flags(self, flags: int):
        self._lib.sixdof_set_flags(self._h, int(flags))

    # ---- telemetry commit overlapped with the next batch -------------------------------------------------------
    def download_async(self, mask: int = L.COL_ALL & ~L.COL_INERTIA):
        rc = self._lib.sixdof_download_async(self._h, int(mask))
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_download_async")

    def download_wait(self):
        rc = self._lib.sixdof_download_wait(self._h)
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_download_wait")

    def sync(self):
        rc = self._lib.sixdof_sync(self._h)
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_sync")

    def stream_history(self, n_batches: int, ticks_per_batch: int, consume=None, columns=("world_pos", "world_vel", "world_accel", "force"),
                       flags: int = 0) -> float:
        """EVERY tick of every batch to the host, overlapped with the stepper: the kernel records each tick into the
        device ring (two batches deep), sixdof_history_stream copies batch i's [ticks, n, w] blocks into one of two
        page-locked host buffers on the copy stream while batch i+1 computes.  `consume(batch_index, first_tick,
        {column: array [ticks, n, w]})` sees a batch once it has landed (the arrays are reused two batches later).
        Returns the wall time in seconds."""
        names = ("world_pos", "world_vel", "world_accel", "force")
        rc = self._lib.sixdof_set_history(self._h, 2 * int(ticks_per_batch))
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_set_history")
        bufs = [{c: np.empty((ticks_per_batch, self.n, 7 if c == "world_pos" else 6), dtype=self.dtype) for c in columns}
                for _ in range(2)]
        ptrs = [(C.c_void_p * 4)(*[b[c].ctypes.data if c in b else None for c in names]) for b in bufs]

        def read(first_tick, k):       # batch i was recorded into ring half i % 2
            rc = self._lib.sixdof_history_stream(self._h, first_tick, ticks_per_batch, ptrs[k])
            if rc != L.OK:
                _raise(self._h, rc, "sixdof_history_stream")
        return self._stream_batches(n_batches, ticks_per_batch, 1, read, lambda k: bufs[k], consume, flags)

    def _stream_batches(self, n_batches: int, ticks_per_batch: int, first_offset: int, read, landed, consume, flags: int) -> float:
        """The double-buffered loop of stream_history / stream_series / stream_envelope / stream_quantiles: batch i is enqueued, then batch i-1 is
        waited for and consumed, then batch i's read-back is enqueued into buffer set i % 2, where it overlaps batch i+1.
        `first_offset`: the batch's first sampled tick, counted from the tick before the batch; `read(first_tick, k)` enqueues
        the asynchronous read into buffer set k; `landed(k)` is what `consume(batch_index, first_tick, .)` receives of set k.
        Whatever happens, the caller's flags are restored and the handle is drained.  Returns the wall time in seconds."""
        import time
        self.set_flags(flags | L.FLAG_ASYNC_STEP)
        t0 = time.perf_counter()
        try:
            first = []
            for i in range(n_batches):
                first.append(self.tick + first_offset)
                self.invoke_batch(ticks_per_batch)                       # enqueue batch i
                if i > 0:
                    self.download_wait()                                 # batch i-1 has landed in buffer set (i-1) % 2
                    if consume is not None:
                        consume(i - 1, first[i - 1], landed((i - 1) % 2))
                read(first[i], i % 2)
            self.download_wait()
            if consume is not None and n_batches:
                consume(n_batches - 1, first[-1], landed((n_batches - 1) % 2))
        finally:
            self.set_flags(flags)
            self.sync()          # also drops the page locks on the buffer sets before they go out of scope
        return time.perf_counter() - t0

    def run_streaming(self, n_batches: int, ticks_per_batch: int, consume=None, flags: int = 0) -> float:
        """The run loop of exec.rs:110-172 (`run(ticks)` = batches of ticks_per_telemetry ticks, each followed by a
        commit of the output columns) with the commit off the critical path: batch i+1 is enqueued before batch i's
        columns are waited for, and they travel to the (page-locked) host columns on a second stream meanwhile.
        `consume(batch_index)` is called when the host columns hold that batch's state (the DB commit goes there).
        Returns the wall time in seconds."""
        import time
        self.set_flags(flags | L.FLAG_ASYNC_STEP)
        t0 = time.perf_counter()
        try:
            for i in range(n_batches):
                self.invoke_batch(ticks_per_batch)          # enqueue batch i (returns once batch i-1 has computed)
                if i > 0:
                    self.download_wait()                    # batch i-1 is in the host columns
                    if consume is not None:
                        consume(i - 1)
                self.download_async()                       # snapshot of batch i; its copy overlaps batch i+1
            self.download_wait()
            if consume is not None and n_batches:
                consume(n_batches - 1)
            self.sync()
        finally:
            self.set_flags(flags)
        return time.perf_counter() - t0

    def join_rows(self, name: str) -> np.ndarray:
        """Row of joined entity j inside column `name` (the reference's constant u32 gather indices)."""
        rows = np.zeros(self.n, dtype=np.uint32)
        m = C.c_size_t()
        rc = self._lib.sixdof_get_join_rows(self._h, L.component_id(name), rows.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            self.n, C.byref(m))
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_get_join_rows")
        return rows

    def edge_rows(self):
        n = C.c_size_t()
        self._lib.sixdof_get_edge_rows(self._h, None, None, 0, C.byref(n))
        src = np.zeros(n.value, dtype=np.uint32)
        dst = np.zeros(n.value, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        rc = self._lib.sixdof_get_edge_rows(self._h, src.ctypes.data_as(u32p), dst.ctypes.data_as(u32p), n.value,
                                            C.byref(n))
        if rc != L.OK:
            _raise(self._h, rc, "sixdof_get_edge_rows")
        return src, dst

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.sixdof_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
