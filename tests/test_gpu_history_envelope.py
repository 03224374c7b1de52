"""Ring envelopes (sixdof_history_envelope): per sampled tick, group and component element the count of finite elements, their
minimum, maximum, mean and m2 = sum (x - mean)^2, reduced on the device out of the telemetry ring.

The reference of every value test is numpy over the [ticks, n, w] blocks HipExec.history reads from the same ring: upcast to
f64, finite elements selected, mean and m2 two-pass in np.longdouble.  Bounds, with c = count and eps = 2^-52:
  count, min, max   exact
  mean              |mean - ref| <= 2 c eps mean|x|            (any summation order is within (c-1) eps sum|x| / c, Higham §4.2;
                                                                 the factor 2 covers the division and the update form)
  m2                |m2 - ref| <= c eps kappa ref, kappa = sqrt(1 + c mean^2 / ref)   (Chan-Golub-LeVeque, updating algorithms)
Every check prints its worst error as a fraction of the bound before it asserts."""
import ctypes as C
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

import elodin_amd as ea
from elodin_amd import _lib as L
from elodin_amd import dsl, workloads
from tests import golden_util as gu
from tests.test_gpu_history_watch import _exec

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FIELDS = ("world_pos", "world_vel", "world_accel", "force")
STATS = ("count", "min", "max", "mean", "m2", "std")
EPS = float(np.finfo(np.float64).eps)
U64P = C.POINTER(C.c_uint64)


def _reference(blocks, period=1):
    """count, min, max, mean, m2, mean|x| as [ticks, period, w] out of [ticks, n, w] blocks (mean, m2 in long double)."""
    t, n, w = blocks.shape
    x = blocks.astype(np.float64).reshape(t, n // period, period, w)
    fin = np.isfinite(x)
    cnt = fin.sum(axis=1)
    xl = np.where(fin, x, 0.0).astype(np.longdouble)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = xl.sum(axis=1) / cnt
        mean_abs = np.abs(xl).sum(axis=1) / cnt
        dev = np.where(fin, xl - mean[:, None], 0.0)
    return {"count": cnt, "min": np.where(fin, x, np.inf).min(axis=1), "max": np.where(fin, x, -np.inf).max(axis=1), "mean": mean,
            "m2": (dev * dev).sum(axis=1), "mean_abs": mean_abs}


def _check(got, ref, what):
    """One component's statistics against the reference under the module's bounds; returns (mean, m2) errors / bounds."""
    cnt = ref["count"]
    assert got["count"].dtype == np.int64 and got["count"].shape == cnt.shape, what
    assert np.array_equal(got["count"], cnt), (what, "count")
    some = cnt > 0
    for k in ("min", "max", "mean", "m2", "std"):
        assert got[k].dtype == np.float64 and got[k].shape == cnt.shape, (what, k)
        assert np.all(np.isnan(got[k][~some])), (what, k, "a group without a finite element must read NaN")
    assert np.array_equal(got["min"][some], ref["min"][some]) and np.array_equal(got["max"][some], ref["max"][some]), (what, "min / max")
    c = cnt[some].astype(np.longdouble)
    mean, m2 = ref["mean"][some], ref["m2"][some]
    mean_err = np.abs(got["mean"][some].astype(np.longdouble) - mean)
    mean_bound = 2 * c * EPS * ref["mean_abs"][some]
    m2_err = np.abs(got["m2"][some].astype(np.longdouble) - m2)
    m2_bound = c * EPS * np.sqrt(m2 * m2 + c * mean * mean * m2)          # = c eps kappa ref, written without the division
    ratio = lambda err, bound: float(np.max(np.where(err == 0, 0.0, err / np.where(bound == 0, np.finfo(np.float64).tiny, bound)), initial=0.0))
    r_mean, r_m2 = ratio(mean_err, mean_bound), ratio(m2_err, m2_bound)
    print(f"{what}: worst mean error / bound {r_mean:.3g}, worst m2 error / bound {r_m2:.3g}")
    assert np.all(mean_err <= mean_bound), (what, "mean", r_mean)
    assert np.all(m2_err <= m2_bound), (what, "m2", r_m2)
    assert np.array_equal(got["std"][some], np.sqrt(got["m2"][some] / cnt[some])), (what, "std")
    return r_mean, r_m2


def _check_all(hip, names, got, first, last, every, period=1, what=""):
    assert sorted(got) == sorted(names)
    for name in names:
        _check(got[name], _reference(hip.history(name, first, last)[::every], period), f"{what} {name}")


def _same(a, b):
    """Bit-equality of two envelope dicts {name: {statistic: array}} (NaN equals NaN)."""
    assert sorted(a) == sorted(b)
    for name in a:
        for k in STATS:
            assert np.array_equal(a[name][k], b[name][k], equal_nan=True), (name, k)


def _sample(env, j):
    return {name: {k: v[j:j + 1] for k, v in d.items()} for name, d in env.items()}


def _raw(hip, names, first, n_samples, every, period, bufs, flags=0):
    comp = np.array([L.component_id(n) for n in names], dtype=np.uint64)
    ptrs = (C.c_void_p * max(1, len(bufs)))(*[b.ctypes.data for b in bufs])
    return hip._lib.sixdof_history_envelope(hip._h, comp.ctypes.data_as(U64P), len(names), first, n_samples, every, period, ptrs, flags)


# ---- 1. values, range shapes, dtypes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,ring,run,first,every,dtype", [
    (300, 8, 10, 27, 18, 3, np.float64),       # ticks 18 .. 27 sit in slots 7 8 9 0 .. 6: the range wraps the ring
    (4099, 7, 64, 50, 1, 7, np.float64),       # several blocks per sample, a ragged last tile
    (64, 1, 8, 8, 1, 1, np.float32),
    (1, 1, 4, 4, 4, 1, np.float64),            # one sample each: one row, one short of a wavefront, one past it
    (63, 4, 4, 4, 4, 1, np.float64),
    (65, 4, 4, 4, 4, 1, np.float64),
])
def test_envelopes_equal_numpy_over_the_history_blocks(n, k, ring, run, first, every, dtype):
    hip, _ = _exec(n, k, dtype)
    hip.enable_history(ring)
    hip.run(run)
    last = first + (run - first) // every * every
    got = hip.history_envelope(FIELDS, first, run, every)             # the four columns in one call
    samples = (last - first) // every + 1
    assert [got[c]["mean"].shape for c in FIELDS] == [(samples, 1, 7)] + [(samples, 1, 6)] * 3
    _check_all(hip, FIELDS, got, first, last, every, what=f"n {n} {np.dtype(dtype).name}")
    assert np.all(got["world_pos"]["count"] == n)
    if samples > 1:                                                    # the ticks differ: not one block repeated
        assert not np.array_equal(got["world_pos"]["mean"][0], got["world_pos"]["mean"][-1])
    one = hip.history_envelope("world_vel", run, run)                 # one name, one sample
    assert sorted(one) == ["world_vel"] and one["world_vel"]["m2"].shape == (1, 1, 6)
    _check_all(hip, ["world_vel"], one, run, run, 1, what=f"n {n} single sample")
    hip.close()


# ---- 2. non-finite rows ---------------------------------------------------------------------------------------------------
def test_non_finite_elements_are_skipped_and_counted():
    n = 300
    hip, _ = _exec(n, 8)
    hip.world_vel[[0, 63, 64, 299]] = np.nan
    hip.world_vel[150, 4] = np.inf
    hip.upload()
    hip.enable_history(8)
    hip.run(8)
    got = hip.history_envelope(FIELDS, 1, 8, 1)
    _check_all(hip, FIELDS, got, 1, 8, 1, what="diverged rows")
    cnt = got["world_vel"]["count"]
    assert cnt.max() <= n - 4 and cnt.min() >= n - 5 and np.any(cnt == n - 5)      # four NaN rows, and the row with one inf element
    assert np.all(np.isfinite(got["world_vel"]["mean"])) and np.all(got["world_pos"]["count"][-1] < n)
    hip.close()


def _program_exec(n=200, a_nan=False):
    """The f32 program of tests/test_gpu_history_watch.py::test_program_columns_are_watched_with_the_body_columns."""
    np_ = dsl.np

    @dsl.system(a=1, b=2, c=3, buf=dsl.window(4, 2))
    def plant(a, b, c, buf):
        s = a * 0.5 + b[1]
        return {"a": s * 0.25 + 1.0,
                "b": np_.array([b[1] * 0.99 + c[2] * 1e-3, b[0] + 0.125]),
                "c": np_.array([c[1], c[2] * 0.999, c[0] + a * 1e-3]),
                "buf": buf.push(b)}
    rng = np.random.default_rng(3)
    w = workloads.independent_bodies(n)
    a0 = np.full((n, 1), np.nan) if a_nan else rng.uniform(-1, 1, (n, 1))
    hip = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], entity_ids=w["entity_ids"], dtype=np.float32, integrator=L.SEMI_IMPLICIT,
                     effectors=dsl.Program([plant], dsl.Pipe([]), []), ticks_per_launch=12,
                     columns={"a": a0, "b": rng.uniform(-1, 1, (n, 2)), "c": rng.uniform(-1, 1, (n, 3)), "buf": np.zeros((n, 4, 2))})
    return hip


def test_a_column_that_is_nan_in_every_row_reads_count_zero():
    hip = _program_exec(a_nan=True)
    hip.enable_history(16)
    hip.run(12)
    got = hip.history_envelope(["a", "b"], 1, 2)
    assert np.all(got["a"]["count"] == 0) and got["a"]["count"].shape == (2, 1, 1)
    for k in ("min", "max", "mean", "m2", "std"):
        assert np.all(np.isnan(got["a"][k])), k
    # the NaN reaches c[2] in tick 1 and b[0] in tick 2: after tick 1 both elements of b are whole, after tick 2 only b[1]
    assert np.array_equal(got["b"]["count"][:, 0], [[200, 200], [0, 200]])
    _check_all(hip, ["a", "b"], got, 1, 2, 1, what="NaN column")
    hip.close()


# ---- 3. groups -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,period", [(4100, 4), (300, 12), (320, 64)])
def test_groups_reduce_rows_of_equal_index_modulo_period(n, period):
    hip, _ = _exec(n, 4)
    hip.enable_history(8)
    hip.run(8)
    got = hip.history_envelope(FIELDS, 2, 8, 3, period=period)
    assert got["world_pos"]["mean"].shape == (3, period, 7) and np.all(got["force"]["count"] == n // period)
    _check_all(hip, FIELDS, got, 2, 8, 3, period, what=f"n {n} period {period}")
    assert not np.array_equal(got["world_pos"]["mean"][:, 0], got["world_pos"]["mean"][:, 1])       # the groups differ
    hip.close()


def test_refused_periods_copy_nothing():
    hip, _ = _exec(300, 4)
    hip.enable_history(8)
    hip.run(8)
    sentinel = lambda: [np.full((2, 100, 5, 7), 123.0), np.full((2, 100, 5, 6), 123.0)]
    bufs = sentinel()
    assert _raw(hip, ["world_pos", "world_vel"], 7, 2, 1, 7, bufs) == L.ERR_INVALID_ARGUMENT            # 300 % 7 != 0
    assert _raw(hip, ["world_pos", "world_vel"], 7, 2, 1, 0, bufs) == L.ERR_INVALID_ARGUMENT
    # 100 groups of world_vel are 600 (group, element) bins, of world_pos 700: beyond what one block keeps apart
    assert 100 * 6 > L.ENVELOPE_MAX_BINS
    assert _raw(hip, ["world_vel"], 7, 2, 1, 100, bufs[1:]) == L.ERR_INVALID_ARGUMENT
    assert str(L.ENVELOPE_MAX_BINS) in hip._lib.sixdof_last_error(hip._h).decode()
    assert _raw(hip, ["world_vel", "world_pos"], 7, 2, 1, 75, bufs[::-1]) == L.ERR_INVALID_ARGUMENT       # 450 bins fit, 525 do not
    for b, s in zip(bufs, sentinel()):
        assert np.array_equal(b, s)
    for period in (7, 0, 100):
        with pytest.raises(ValueError):
            hip.history_envelope(["world_vel"], 7, 8, 1, period=period)
    got = hip.history_envelope(["world_vel"], 7, 8, 1, period=75)                                        # 450 bins: served
    _check_all(hip, ["world_vel"], got, 7, 8, 1, 75, what="period 75")
    hip.close()


# ---- 4. conditioning ---------------------------------------------------------------------------------------------------
def test_spread_of_positions_metres_apart_at_earth_radius():
    """world_pos' linear part at 6.4e6 m plus a unit normal: the case sum x^2 - (sum x)^2 / n loses entirely."""
    n = 4099
    hip, _ = _exec(n, 4)
    hip.world_pos[:, 4:7] = 6.4e6 + np.random.default_rng(11).normal(size=(n, 3))
    hip.upload()
    hip.enable_history(4)
    hip.run(4)
    got = hip.history_envelope(["world_pos"], 1, 4, 3)["world_pos"]
    ref = _reference(hip.history("world_pos", 1, 4)[::3])
    linear = lambda d: {k: v[..., 4:7] for k, v in d.items()}
    r_mean, r_m2 = _check(linear(got), linear(ref), "positions at 6.4e6 +- 1 m, x y z")
    assert r_m2 <= 1.0 and np.all(got["std"][..., 4:7] > 0.5) and np.all(got["std"][..., 4:7] < 2.0)
    _check(got, ref, "positions at 6.4e6 +- 1 m, all seven")
    hip.close()


# ---- 5. bit-identity ---------------------------------------------------------------------------------------------------
def test_a_tick_reads_the_same_bits_however_it_is_read():
    n = 4099
    hip, _ = _exec(n, 7)
    hip.enable_history(32)
    hip.run(30)
    whole = hip.history_envelope(FIELDS, 3, 30, 3)
    _same(whole, hip.history_envelope(FIELDS, 3, 30, 3))                                  # two identical calls
    for j, tick in enumerate(range(3, 31, 3)):
        _same(_sample(whole, j), hip.history_envelope(FIELDS, tick, tick))                # the one-sample read of that tick
    other = hip.history_envelope(["force", "world_pos"], 6, 30, 6)                        # another every, another component list
    for j, tick in enumerate(range(6, 31, 6)):
        for name in ("force", "world_pos"):
            _same({name: _sample(other, j)[name]}, {name: _sample(whole, (tick - 3) // 3)[name]})
    # synchronous against SIXDOF_ENVELOPE_ASYNC
    bufs = [np.zeros((10, 1, 5, 7 if c == "world_pos" else 6)) for c in FIELDS]
    assert _raw(hip, FIELDS, 3, 10, 3, 1, bufs, L.ENVELOPE_ASYNC) == L.OK
    hip.download_wait()
    _same(whole, hip._envelope_dict(FIELDS, bufs))
    grouped = hip.history_envelope(["world_vel"], 3, 30, 9, period=1)
    _same({"world_vel": _sample(grouped, 1)["world_vel"]}, {"world_vel": _sample(whole, 3)["world_vel"]})
    hip.sync()
    hip.close()


def test_more_components_than_one_launch_covers():
    """34 component ids — the four fields cycled — cross the 32 components of one launch: the second launch reuses the scratch
    offsets of the first.  Every buffer is, byte for byte, the same field's buffer of a four-id read of the same two samples."""
    hip, _ = _exec(65, 4)
    hip.enable_history(4)
    hip.run(4)
    names = [FIELDS[k % 4] for k in range(34)]
    block = lambda c, fill: np.full((2, 5, 5, 7 if c == "world_pos" else 6), fill)
    many, four = [block(c, -7.0) for c in names], [block(c, -9.0) for c in FIELDS]
    assert _raw(hip, names, 3, 2, 1, 5, many) == L.OK and _raw(hip, FIELDS, 3, 2, 1, 5, four) == L.OK
    assert all(np.all(b[:, :, 0] == 13) for b in four)                 # filled: 65 rows in 5 groups
    for k, b in enumerate(many):
        assert b.tobytes() == four[k % 4].tobytes(), (k, names[k])
    hip.close()


# ---- 6. program columns ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("column_soa", ["0", "1"])
def test_program_columns_with_the_body_columns(column_soa, monkeypatch):
    monkeypatch.setenv("SIXDOF_COLUMN_SOA", column_soa)
    hip = _program_exec()
    names = ["a", "world_pos", "b", "c"]
    hip.enable_history(32)
    hip.run(30)
    got = hip.history_envelope(names, 3, 30, 3)
    assert [got[k]["mean"].shape for k in names] == [(10, 1, 1), (10, 1, 7), (10, 1, 2), (10, 1, 3)]
    _check_all(hip, names, got, 3, 30, 3, what=f"program columns, column_soa {column_soa}")
    assert hip._column_soa == (column_soa == "1")
    assert not np.array_equal(got["c"]["mean"][0], got["c"]["mean"][-1])
    grouped = hip.history_envelope(names, 30, 30, period=8)
    _check_all(hip, names, grouped, 30, 30, 1, 8, what="program columns, period 8")
    with pytest.raises(ValueError, match="window component"):
        hip.history_envelope(["buf"], 3, 30)
    with pytest.raises(KeyError):
        hip.history_envelope(["world_pos", "inertia"], 3, 30)
    bufs = [np.full((1, 1, 5, 8), 123.0)]                    # the library refuses the window too, not only the Python surface
    assert _raw(hip, ["buf"], 30, 1, 1, 1, bufs) == L.ERR_COMPONENT_NOT_FOUND
    assert _raw(hip, ["inertia"], 30, 1, 1, 1, bufs) == L.ERR_COMPONENT_NOT_FOUND
    assert np.all(bufs[0] == 123.0)
    hip.close()


# ---- 7. pair path --------------------------------------------------------------------------------------------------------
def test_pair_path_ring_filled_by_per_tick_copies():
    g = gu.load("three_body")
    names = "abc"
    pos = np.stack([g[f"{e}.world_pos"][0] for e in names])
    vel = np.stack([g[f"{e}.world_vel"][0] for e in names])
    inertia = np.stack([g[f"{e}.inertia"][0] for e in names])
    edge_names = ["a_>_b", "b_>_a", "a_>_c", "b_>_c", "c_>_a", "c_>_b"]
    frm = np.array([g[f"{e}.gravity_edge"][0, 0] for e in edge_names], dtype=np.uint64)
    to = np.array([g[f"{e}.gravity_edge"][0, 1] for e in edge_names], dtype=np.uint64)
    hip = ea.HipExec(pos, vel, inertia, entity_ids=[1, 2, 3], simulation_time_step=float(g["globals.simulation_time_step"][0, 0]),
                     effectors=[ea.Effector(L.EFF_EDGE_GRAVITY_NEWTON, (6.6743e-11,))], edges=(frm, to))
    hip.enable_history(8)
    hip.run(13)
    _check_all(hip, FIELDS, hip.history_envelope(FIELDS, 6, 13), 6, 13, 1, what="three bodies")
    _check_all(hip, FIELDS, hip.history_envelope(FIELDS, 7, 13, 3), 7, 13, 3, what="three bodies, every 3")
    per_body = hip.history_envelope(FIELDS, 7, 13, 3, period=3)
    _check_all(hip, FIELDS, per_body, 7, 13, 3, 3, what="three bodies, one per group")
    assert np.all(per_body["world_pos"]["count"] == 1) and np.all(per_body["world_pos"]["m2"] == 0.0)
    assert np.array_equal(per_body["world_pos"]["mean"][-1], hip.world_pos)
    hip.close()


# ---- 8. refusals copy nothing -------------------------------------------------------------------------------------------
def test_refused_reads_copy_nothing():
    hip, _ = _exec(300, 8)
    sentinel = lambda: np.full((4, 1, 5, 6), 123.0)
    buf = sentinel()
    raw_read = lambda first, n_samples, every: _raw(hip, ["world_vel"], first, n_samples, every, 1, [buf])
    assert raw_read(1, 1, 1) == L.ERR_INVALID_ARGUMENT                         # no ring
    hip.run(5)
    hip.enable_history(10)                                                       # recording starts at tick 6
    hip.run(25)                                                                  # the ring keeps 21 .. 30
    assert raw_read(21, 4, 0) == L.ERR_INVALID_ARGUMENT                         # every = 0
    assert raw_read(20, 4, 1) == L.ERR_INVALID_ARGUMENT                         # has fallen out of the ring
    assert raw_read(28, 4, 1) == L.ERR_INVALID_ARGUMENT                         # runs beyond `tick`
    assert raw_read(24, 4, 3) == L.ERR_INVALID_ARGUMENT                         # its last sample does
    assert raw_read(31, 1, 1) == L.ERR_INVALID_ARGUMENT
    assert _raw(hip, ["world_vel"], 21, 4, 1, 1, [buf], 2) == L.ERR_INVALID_ARGUMENT      # unknown flags
    null = (C.c_void_p * 1)(None)
    comp = np.array([L.component_id("world_vel")], dtype=np.uint64)
    assert hip._lib.sixdof_history_envelope(hip._h, comp.ctypes.data_as(U64P), 1, 21, 4, 1, 1, null, 0) == L.ERR_INVALID_ARGUMENT
    assert np.array_equal(buf, sentinel())                                      # nothing was copied
    for bad in ((20, 30, 1), (21, 31, 1), (21, 30, 0), (5, 5, 1)):
        with pytest.raises(ValueError):
            hip.history_envelope(["world_vel"], *bad)
    assert raw_read(21, 0, 1) == L.OK and raw_read(99, 0, 7) == L.OK            # no samples: a no-op
    assert np.array_equal(buf, sentinel())
    assert hip.history_envelope(["world_vel"], 30, 29)["world_vel"]["mean"].shape == (0, 1, 6)
    assert raw_read(21, 4, 3) == L.OK                                           # 21 24 27 30
    _check(hip._envelope_dict(["world_vel"], [buf])["world_vel"], _reference(hip.history("world_vel", 21, 30)[::3]), "after the refusals")
    hip.enable_history(10)                                                       # a ring that starts over
    hip.run(3)                                                                   # 31 .. 33
    buf[...] = 123.0
    assert raw_read(30, 4, 1) == L.ERR_INVALID_ARGUMENT                         # starts before hist_first_tick
    assert np.array_equal(buf, sentinel())
    assert hip.history_envelope(["world_vel"], 31, 33)["world_vel"]["mean"].shape == (3, 1, 6)
    hip.enable_history(0)
    with pytest.raises(ValueError, match="no history ring"):
        hip.history_envelope(["world_vel"], 31, 33)
    hip.close()


# ---- 9. streaming ---------------------------------------------------------------------------------------------------------
def test_streamed_envelopes_equal_a_twin_read_tick_by_tick():
    """stream_envelope: every fourth tick of six 16-tick batches out of a ring one batch deep; each sample is bit-equal to the
    envelope a twin stepped one tick at a time reads at that tick, and streaming leaves the state a plain run leaves."""
    n = 1000
    a, _ = _exec(n, 8)
    b, _ = _exec(n, 1)
    plain, _ = _exec(n, 8)
    got, order = {}, []

    def consume(i, first_tick, env):
        order.append((i, first_tick))
        assert sorted(env) == sorted(FIELDS) and env["world_pos"]["mean"].shape == (4, 1, 7) and env["force"]["count"].dtype == np.int64
        for j in range(4):
            got[first_tick + 4 * j] = {c: {k: v[j:j + 1].copy() for k, v in d.items()} for c, d in env.items()}
    with pytest.raises(ValueError):
        a.stream_envelope(FIELDS, 6, 16, every=5)
    wall = a.stream_envelope(FIELDS, 6, 16, every=4, consume=consume)
    assert wall > 0.0 and a.tick == 96
    assert order == [(i, 16 * i + 4) for i in range(6)] and sorted(got) == list(range(4, 97, 4))
    b.enable_history(4)
    for t in range(1, 97):
        b.run(1)
        if t in got:
            _same(got[t], b.history_envelope(FIELDS, t, t))
    a.download()
    plain.run(96)
    for c in FIELDS:
        assert np.array_equal(getattr(a, c), getattr(plain, c)), c
    for h in (a, b, plain):
        h.close()


def test_async_envelope_alongside_a_history_stream_copy():
    """A sixdof_history_stream copy and, before it is waited for, an asynchronous envelope: one download_wait covers both."""
    n = 500
    hip, _ = _exec(n, 4)
    hip.enable_history(16)
    hip.run(16)
    want_blocks = {c: hip.history(c, 5, 12) for c in FIELDS}
    want = hip.history_envelope(FIELDS, 10, 16, 2, period=5)
    blocks = {c: np.zeros((8, n, 7 if c == "world_pos" else 6)) for c in FIELDS}
    bufs = [np.zeros((4, 5, 5, 7 if c == "world_pos" else 6)) for c in FIELDS]
    rc = hip._lib.sixdof_history_stream(hip._h, 5, 8, (C.c_void_p * 4)(*[blocks[c].ctypes.data for c in FIELDS]))
    assert rc == L.OK
    assert _raw(hip, FIELDS, 10, 4, 2, 5, bufs, L.ENVELOPE_ASYNC) == L.OK
    hip.download_wait()
    for c in FIELDS:
        assert np.array_equal(blocks[c], want_blocks[c]), c
    _same(hip._envelope_dict(FIELDS, bufs), want)
    hip.run(4)                                               # the stepper goes on; the page locks end at sync
    hip.sync()
    assert hip.tick == 20
    hip.close()


def test_two_staged_readers_and_a_stream_copy_pending_on_one_lane():
    """A sixdof_history_stream copy, an asynchronous watch read, an asynchronous envelope read and a second, larger watch read
    — whose staging buffer has to grow while the others are pending — all before ONE download_wait: every buffer holds the bits
    of the blocking read of its range, made beforehand.  (The larger watch read's blocking twin goes through sixdof_history_read,
    so that the watch staging buffer is still the smaller one when the asynchronous reads start.)"""
    n, rows = 300, [0, 63, 64, 299]
    hip, w = _exec(n, 4)
    hip.enable_history(16)
    hip.run(16)
    names = ("world_pos", "world_vel")
    hip.set_watch(names, np.asarray(w["entity_ids"])[rows])
    want_blocks = {c: hip.history(c, 5, 12) for c in FIELDS}
    want_short = hip.history_series(10, 16, 2)
    want_env = [np.zeros((4, 12, 5, 7 if c == "world_pos" else 6)) for c in FIELDS]
    assert _raw(hip, FIELDS, 10, 4, 2, 12, want_env) == L.OK
    want_long = {c: np.ascontiguousarray(hip.history(c, 9, 16)[:, rows].transpose(1, 0, 2)) for c in names}

    blocks = {c: np.zeros((8, n, 7 if c == "world_pos" else 6)) for c in FIELDS}
    got_short, short_ptrs = hip._series_buffers(4)
    got_env = [np.zeros_like(a) for a in want_env]
    got_long, long_ptrs = hip._series_buffers(8)
    assert hip._lib.sixdof_history_stream(hip._h, 5, 8, (C.c_void_p * 4)(*[blocks[c].ctypes.data for c in FIELDS])) == L.OK
    assert hip._lib.sixdof_watch_read(hip._h, 10, 4, 2, short_ptrs, L.WATCH_ASYNC) == L.OK
    assert _raw(hip, FIELDS, 10, 4, 2, 12, got_env, L.ENVELOPE_ASYNC) == L.OK
    assert hip._lib.sixdof_watch_read(hip._h, 9, 8, 1, long_ptrs, L.WATCH_ASYNC) == L.OK
    hip.download_wait()
    for c in FIELDS:
        assert blocks[c].tobytes() == want_blocks[c].tobytes(), c
    for c in names:
        assert got_short[c].tobytes() == want_short[c].tobytes(), c
        assert got_long[c].shape == want_long[c].shape and got_long[c].tobytes() == want_long[c].tobytes(), c
    for c, got, want in zip(FIELDS, got_env, want_env):
        assert got.tobytes() == want.tobytes(), c
    assert want_env[0][:, :, 0].min() == n // 12 and np.any(want_long["world_vel"] != 0)      # the twins read something
    hip.run(4)                                               # the stepper goes on; the page locks end at sync
    hip.sync()
    assert hip.tick == 20
    hip.close()


# ---- 10. front end ---------------------------------------------------------------------------------------------------------
def test_front_end_envelope_of_one_entity_is_its_series():
    spec = importlib.util.spec_from_file_location("ball", ROOT / "examples" / "ball.py")
    ball = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ball)
    ex = ball.world(0).build(ball.system(), simulation_rate=120.0, telemetry_rate=40.0, history=True)
    ex.enable_history(64)
    ex.run(30)
    comps = ["world_pos", "world_vel", "wind", "force"]
    series = ex.history_series(["ball." + c for c in comps], 3, 30, every=3)
    env = ex.history_envelope(comps, 3, 30, every=3)
    assert sorted(env) == sorted(comps + ["time"]) and np.array_equal(env["time"], series["time"])
    for c in comps:
        want = series["ball." + c]
        d = env[c]
        assert d["mean"].shape == (10, 1, want.shape[1])
        assert np.all(d["count"] == 1) and np.all(d["m2"] == 0.0) and np.all(d["std"] == 0.0), c
        for k in ("min", "max", "mean"):
            assert np.array_equal(d[k][:, 0], want), (c, k)
    assert not np.array_equal(env["world_pos"]["mean"][0], env["world_pos"]["mean"][-1])
    with pytest.raises(KeyError):
        ex.history_envelope("nothing", 3, 30)
    with pytest.raises(ValueError):
        ex.history_envelope("world_pos", 0, 30)              # tick 0 is not in the ring
    with pytest.raises(ValueError):
        ex.history_envelope("world_pos", 3, 30, every=0)


def test_campaign_envelope_equals_numpy_over_the_runs_columns(monkeypatch):
    """A 17-run campaign of the Monte-Carlo example: Campaign.envelope per tick against numpy over Campaign.column after each tick."""
    from tests.test_gpu_monte_carlo_example import GOLDEN, example
    from elodin_amd import vectorize
    ex = example(0)
    doc = json.loads((GOLDEN / "monte_carlo_example.json").read_text())
    params = [r["params"] for r in doc["runs"] if r["probe_rows"] == 0]
    c = vectorize.Campaign(ex.build, vectorize.plan_of((params * 17)[:17]), ex.PARAMS, simulation_rate=ex.SIMULATION_RATE_HZ)
    assert c.n_runs == 17 and c.entities_per_run == 1
    comps = ["position", "velocity", "specific_force"]
    c.exec.enable_history(16)
    cols = {name: [] for name in comps}
    for _ in range(12):
        c.exec.run(1)
        for name in comps:
            cols[name].append(np.array(c.column(name), dtype=np.float64).reshape(17, -1))
    env = c.envelope(comps, 2, 12, every=5)                  # ticks 2, 7, 12
    assert np.allclose(env["time"], np.array([2, 7, 12]) / ex.SIMULATION_RATE_HZ)
    for name in comps:
        ref = _reference(np.stack([cols[name][t - 1] for t in (2, 7, 12)]), period=1)
        assert env[name]["mean"].shape == (3, 1, 1)
        _check(env[name], ref, f"campaign {name}")
    assert np.all(env["position"]["count"] == 17) and np.all(env["velocity"]["std"][-1] > 0.0)
