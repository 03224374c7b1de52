"""ctypes binding of the C ABI in include/sixdof_hip.h (elodin_amd/libsixdof_hip.so).

This is the same stub a reference maintainer would write in Rust with `extern "C"` (see
INTEGRATION.md).  There is no fallback: if the HIP library is missing or no GPU is present the
product path raises — it never routes through the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["SIXDOF_LIBRARY"]) if os.environ.get("SIXDOF_LIBRARY") else PKG / "libsixdof_hip.so"   # override: A/B of library builds

OK = 0
ERR_INVALID_ARGUMENT, ERR_COMPONENT_NOT_FOUND, ERR_VALUE_SIZE_MISMATCH = -1, -2, -3
ERR_BACKEND, ERR_NO_DEVICE, ERR_UNSUPPORTED, ERR_ENTITY_MISMATCH, ERR_TIME_TRAVEL = -4, -5, -6, -7, -8
ERR_OUT_OF_MEMORY, ERR_INTERNAL = -9, -10      # the exception barrier of the C ABI (csrc/abi_guard.hpp)

RK4, SEMI_IMPLICIT, INTEGRATOR_NONE = 0, 1, 2
F64, F32 = 0, 1
PRIM_F64, PRIM_U64, PRIM_F32 = 0, 1, 2
FLAG_USE_GRAPH = 1
FLAG_TIME_EACH_LAUNCH = 2
FLAG_ASYNC_STEP = 4
WATCH_ASYNC = 1      # sixdof_watch_read flags
ENVELOPE_ASYNC = 1   # sixdof_history_envelope flags
ENVELOPE_MAX_BINS = 512   # period * width one call reduces (csrc/envelope_plan.hpp: kEnvelopeMaxBins)
QUANTILE_ASYNC = 1   # sixdof_history_quantiles flags
QUANTILE_MAX_RANKS = 16   # ranks one call selects (SIXDOF_QUANTILE_MAX_RANKS)
EXTREMES_ASYNC, EXTREMES_CONTINUE, EXTREMES_HOLD = 1, 2, 4   # sixdof_history_extremes flags
EXTREMES_PLANES = 6       # count, min, tick_min, max, tick_max, first_nonfinite (SIXDOF_EXTREMES_PLANES)
EVENT_LT, EVENT_LE, EVENT_GT, EVENT_GE = 0, 1, 2, 3   # sixdof_event_trigger.op
EVENT_LEVEL, EVENT_CROSSING = 0, 1                    # sixdof_event_trigger.mode
EVENTS_ASYNC, EVENTS_CONTINUE, EVENTS_HOLD = 1, 2, 4  # sixdof_history_events flags
EVENTS_PLANES = 4         # tick, value, tick_before, value_before (SIXDOF_EVENTS_PLANES)
EVENTS_MAX_TRIGGERS = 8   # triggers one call walks (SIXDOF_EVENTS_MAX_TRIGGERS)
NORM_MINUS = 1            # sixdof_norm_probe.flags: the probe is |A - B|
NORM_MAX_COUNT = 4        # elements of one probe (SIXDOF_NORM_MAX_COUNT: a quaternion)
NORMS_ASYNC, NORMS_CONTINUE, NORMS_HOLD = 1, 2, 4     # sixdof_history_norms flags
NORMS_PLANES = 6          # count, min_sq, tick_min, max_sq, tick_max, first_nonfinite (SIXDOF_NORMS_PLANES)
NORMS_MAX_PROBES = 8      # probes one call walks (SIXDOF_NORMS_MAX_PROBES)
NORM_EVENTS_ASYNC, NORM_EVENTS_CONTINUE, NORM_EVENTS_HOLD = 1, 2, 4   # sixdof_history_norm_events flags
NORM_EVENTS_PLANES = 4    # tick, value_sq, tick_before, value_before_sq (SIXDOF_NORM_EVENTS_PLANES)
NORM_EVENTS_MAX_TRIGGERS = 8   # triggers one call walks (SIXDOF_NORM_EVENTS_MAX_TRIGGERS)
DWELL_ELEMENT, DWELL_NORM_SQ = 0, 1                   # sixdof_dwell_condition.kind
DWELL_INSIDE, DWELL_OUTSIDE = 4, 5                    # sixdof_dwell_condition.op, after EVENT_LT .. EVENT_GE
DWELL_ASYNC, DWELL_CONTINUE, DWELL_HOLD = 1, 2, 4     # sixdof_history_dwell flags
DWELL_PLANES = 12         # count, held, entries, first_held, last_held, prefix_len, prefix_end, suffix_len, suffix_start, longest_len, longest_start, longest_end
DWELL_MAX_CONDITIONS = 8  # conditions one call walks (SIXDOF_DWELL_MAX_CONDITIONS)
COVARIANCE_ASYNC = 1      # sixdof_history_covariance flags
COVARIANCE_MAX_CHANNELS = 6   # channels one call reduces jointly (SIXDOF_COVARIANCE_MAX_CHANNELS)
COVARIANCE_MAX_PERIOD = 256   # groups one call keeps apart (csrc/covariance_plan.hpp: kCovarianceMaxPeriod)

EFF_CONST_WRENCH = 1
EFF_UNIFORM_GRAVITY = 2
EFF_BODY_TORQUE = 3
EFF_BODY_FORCE = 4
EFF_BALL_DRAG = 5
EFF_EDGE_GRAVITY_NEWTON = 6
EFF_EDGE_GRAVITY_SOFTENED = 7
EFF_ALLPAIRS_GRAVITY_SOFTENED = 8
EFF_EDGE_CUSTOM = 9
EFF_WORLD_TORQUE = 10
EFF_WORLD_FORCE = 11

COL_WORLD_POS, COL_WORLD_VEL, COL_WORLD_ACCEL, COL_FORCE, COL_INERTIA, COL_ALL = 1, 2, 4, 8, 16, 31


class EffectorOp(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("aux_component_id", C.c_uint64),
                ("p", C.c_double * 6)]


class Desc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device_ordinal", C.c_int32), ("integrator", C.c_int32),
                ("dtype", C.c_int32), ("n_entities", C.c_uint64), ("simulation_time_step", C.c_double),
                ("time_step", C.c_double), ("has_time_step", C.c_int32), ("ticks_per_launch", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class Column(C.Structure):
    _fields_ = [("component_id", C.c_uint64), ("prim_type", C.c_int32), ("ndim", C.c_uint32),
                ("dims", C.c_uint64 * 2), ("n_rows", C.c_uint64), ("entity_ids", C.POINTER(C.c_uint64)),
                ("host_ptr", C.c_void_p)]


class Timings(C.Structure):
    _fields_ = [("h2d_upload_ms", C.c_double), ("kernel_invoke_ms", C.c_double), ("d2h_download_ms", C.c_double),
                ("kernel_device_ms", C.c_double), ("launches", C.c_uint64), ("ticks", C.c_uint64),
                ("kernel_sum_ms", C.c_double), ("graph_launches", C.c_uint64)]


class EventTrigger(C.Structure):   # sixdof_event_trigger, 32 bytes
    _fields_ = [("component_id", C.c_uint64), ("element", C.c_uint32), ("group", C.c_uint32), ("op", C.c_uint32), ("mode", C.c_uint32),
                ("level", C.c_double)]


class NormProbe(C.Structure):   # sixdof_norm_probe, 40 bytes
    _fields_ = [("component_id", C.c_uint64), ("minus_component_id", C.c_uint64), ("element", C.c_uint32), ("minus_element", C.c_uint32),
                ("group", C.c_uint32), ("minus_group", C.c_uint32), ("count", C.c_uint32), ("flags", C.c_uint32)]


class NormTrigger(C.Structure):   # sixdof_norm_trigger, 56 bytes
    _fields_ = [("probe", NormProbe), ("level_sq", C.c_double), ("op", C.c_uint32), ("mode", C.c_uint32)]


class DwellCondition(C.Structure):   # sixdof_dwell_condition, 64 bytes
    _fields_ = [("probe", NormProbe), ("lo", C.c_double), ("hi", C.c_double), ("kind", C.c_uint32), ("op", C.c_uint32)]


class CovChannel(C.Structure):   # sixdof_cov_channel, 16 bytes
    _fields_ = [("component_id", C.c_uint64), ("element", C.c_uint32), ("reserved", C.c_uint32)]


class Slot(C.Structure):
    _fields_ = [("component_id", C.c_uint64), ("bytes", C.c_uint64)]


# every symbol include/sixdof_hip.h declares: name -> (restype, argtypes)
_H = C.c_void_p
SYMBOLS = {
    "sixdof_abi_version": (C.c_uint32, []),
    "sixdof_component_id": (C.c_uint64, [C.c_char_p]),
    "sixdof_quantize_time_step": (C.c_double, [C.c_double]),
    "sixdof_device_count": (C.c_int, []),
    "sixdof_create": (C.c_int, [C.POINTER(Desc), C.POINTER(_H)]),
    "sixdof_destroy": (None, [_H]),
    "sixdof_last_error": (C.c_char_p, [_H]),
    "sixdof_bind_columns": (C.c_int, [_H, C.POINTER(Column), C.c_size_t]),
    "sixdof_set_effectors": (C.c_int, [_H, C.POINTER(EffectorOp), C.c_size_t]),
    "sixdof_set_edges": (C.c_int, [_H, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_size_t]),
    "sixdof_get_join_rows": (C.c_int, [_H, C.c_uint64, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t)]),
    "sixdof_get_edge_rows": (C.c_int, [_H, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t,
                                       C.POINTER(C.c_size_t)]),
    "sixdof_upload": (C.c_int, [_H]),
    "sixdof_prepare_step": (C.c_int, [_H, C.c_uint64]),
    "sixdof_step_path": (C.c_char_p, [_H]),
    "sixdof_comm_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
    "sixdof_comm_init": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int]),
    "sixdof_comm_destroy": (None, [C.c_void_p]),
    "sixdof_comm_last_error": (C.c_char_p, [C.c_void_p]),
    "sixdof_shard_range": (None, [C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "sixdof_gather_block_rows": (C.c_uint64, [C.c_uint64, C.c_int]),
    "sixdof_gather_pack": (C.c_int, [C.POINTER(C.c_double), C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "sixdof_gather_unpack": (C.c_int, [C.POINTER(C.c_double), C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_double)]),
    "sixdof_campaign_broadcast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]),
    "sixdof_campaign_gather": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_uint64, C.c_uint64, C.POINTER(C.c_double), C.c_uint64]),
    "sixdof_step": (C.c_int, [_H, C.c_uint64, C.POINTER(Timings)]),
    "sixdof_download": (C.c_int, [_H, C.c_uint32]),
    "sixdof_get_tick": (C.c_int, [_H, C.POINTER(C.c_uint64)]),
    "sixdof_set_tick": (C.c_int, [_H, C.c_uint64]),
    "sixdof_set_ticks_per_launch": (C.c_int, [_H, C.c_uint32]),
    "sixdof_set_flags": (C.c_int, [_H, C.c_uint32]),
    "sixdof_device_column": (C.c_void_p, [_H, C.c_uint64]),
    "sixdof_stream": (C.c_void_p, [_H]),
    "sixdof_tick_bind": (C.c_int, [_H]),
    "sixdof_tick": (None, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "sixdof_count_nonfinite": (C.c_int, [_H, C.POINTER(C.c_uint64), C.c_void_p]),
    "sixdof_last_timings": (C.c_int, [_H, C.POINTER(Timings)]),
    "sixdof_world_create": (C.c_void_p, []),
    "sixdof_world_destroy": (None, [C.c_void_p]),
    "sixdof_world_last_error": (C.c_char_p, [C.c_void_p]),
    "sixdof_world_spawn": (C.c_uint64, [C.c_void_p]),
    "sixdof_world_entity_len": (C.c_uint64, [C.c_void_p]),
    "sixdof_world_insert": (C.c_int, [C.c_void_p, C.c_uint64, C.c_char_p, C.c_int, C.POINTER(C.c_uint64), C.c_uint32,
                                      C.c_void_p, C.c_size_t]),
    "sixdof_world_column": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(Column)]),
    "sixdof_world_components": (C.c_size_t, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t]),
    "sixdof_world_set_rates": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "sixdof_world_time_step": (C.c_double, [C.c_void_p]),
    "sixdof_world_ticks_per_telemetry": (C.c_uint64, [C.c_void_p]),
    "sixdof_world_tick": (C.c_uint64, [C.c_void_p]),
    "sixdof_world_advance_tick": (None, [C.c_void_p, C.c_uint64]),
    "sixdof_bind_world": (C.c_int, [_H, C.c_void_p]),
    "sixdof_set_custom_pipe": (C.c_int, [_H, C.c_char_p, C.POINTER(C.c_uint64), C.c_size_t]),
    "sixdof_set_custom_pair": (C.c_int, [_H, C.c_char_p]),
    "sixdof_set_fold_edges": (C.c_int, [_H, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_size_t]),
    "sixdof_build_fold_table": (C.c_int, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t, C.c_uint32, C.c_uint32,
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "sixdof_download_async": (C.c_int, [_H, C.c_uint32]),
    "sixdof_download_wait": (C.c_int, [_H]),
    "sixdof_sync": (C.c_int, [_H]),
    "sixdof_set_history": (C.c_int, [_H, C.c_uint32]),
    "sixdof_history_read": (C.c_int, [_H, C.c_uint64, C.c_uint64, C.c_void_p]),
    "sixdof_history_stream": (C.c_int, [_H, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]),
    "sixdof_set_watch": (C.c_int, [_H, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t]),
    "sixdof_watch_read": (C.c_int, [_H, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p), C.c_uint32]),
    "sixdof_history_envelope": (C.c_int, [_H, C.POINTER(C.c_uint64), C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                          C.POINTER(C.c_void_p), C.c_uint32]),
    "sixdof_history_quantiles": (C.c_int, [_H, C.POINTER(C.c_uint64), C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                           C.POINTER(C.c_uint32), C.c_uint32, C.c_size_t, C.POINTER(C.c_void_p), C.c_uint32]),
    "sixdof_history_extremes": (C.c_int, [_H, C.POINTER(C.c_uint64), C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p),
                                          C.c_uint32]),
    "sixdof_history_events": (C.c_int, [_H, C.POINTER(EventTrigger), C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint64,
                                        C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32]),
    "sixdof_history_norms": (C.c_int, [_H, C.POINTER(NormProbe), C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32]),
    "sixdof_history_dwell": (C.c_int, [_H, C.POINTER(DwellCondition), C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32]),
    "sixdof_history_norm_events": (C.c_int, [_H, C.POINTER(NormTrigger), C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint64,
                                             C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32]),
    "sixdof_history_covariance": (C.c_int, [_H, C.POINTER(CovChannel), C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p,
                                            C.c_uint32]),
    "sixdof_set_model_apollo": (C.c_int, [_H, C.c_void_p]),
    "sixdof_download_column": (C.c_int, [_H, C.c_uint64]),
    "sixdof_upload_column": (C.c_int, [_H, C.c_uint64]),
    "sixdof_tick_slots": (C.c_int, [_H, C.POINTER(Slot), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(Slot),
                                    C.c_size_t, C.POINTER(C.c_size_t)]),
    # the commit path's hand-off (csrc/telemetry_sink.cpp)
    "sixdof_pair_id": (C.c_uint64, [C.c_char_p, C.c_char_p]),
    "sixdof_sink_create": (C.c_void_p, []),
    "sixdof_sink_destroy": (None, [C.c_void_p]),
    "sixdof_sink_last_error": (C.c_char_p, [C.c_void_p]),
    "sixdof_sink_register": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_char_p]),
    "sixdof_sink_push": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int64, C.c_void_p, C.c_uint32]),
    "sixdof_sink_sample_count": (C.c_uint64, [C.c_void_p, C.c_uint64]),
    "sixdof_sink_pairs": (C.c_size_t, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t]),
    "sixdof_sink_latest": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_int64), C.c_void_p, C.c_uint32]),
    "sixdof_sink_at": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_uint32]),
    "sixdof_sink_series": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.POINTER(C.c_uint8)),
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "sixdof_sink_truncate": (None, [C.c_void_p]),
    "sixdof_sink_commit_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint32, C.c_uint32, C.c_int64]),
    "sixdof_sink_copy_to_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int)]),
}

_lib = None


class BackendError(RuntimeError):
    """HIP extension missing / no device / HIP runtime failure (Error::CraneliftBackend analogue)."""


def lib() -> C.CDLL:
    """Load libsixdof_hip.so; raise loudly if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise BackendError(f"{LIB_PATH} not built: run `make -C elodin_amd/csrc` "
                               "(no CPU fallback exists for the product path)")
        L = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError here = header/library skew
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def component_id(name: str) -> int:
    return int(lib().sixdof_component_id(name.encode()))
