"""Ring covariances (sixdof_history_covariance): per sampled tick and group the count of rows whose k channel values are all
finite (listwise), their mean vector and the co-moment matrix C_ab = sum (x_a - mean_a)(x_b - mean_b), reduced on the device out
of the telemetry ring.

The reference of every value test is numpy over the [ticks, n, w] blocks HipExec.history reads from the same ring: upcast to f64,
the listwise-finite rows selected, means and co-moments two-pass in np.longdouble.  Bounds, with c = count, eps = 2^-52, m2_a the
reference diagonal and S_a = sum x_a^2 over the rows used:
  count       exact
  mean        |mean_a - ref| <= 2 c eps mean|x_a|                                  (the envelope's bound)
  co-moment   |C_ab - ref| <= c eps (sqrt(m2_a S_b) + sqrt(m2_b S_a))              (each term rounds by eps (|d_a||x_b| + |d_b||x_a|);
                                                                                    Cauchy-Schwarz, and c for the accumulation;
                                                                                    at a = b twice the envelope's m2 bound)
Every check prints its worst error as a fraction of the bound before it asserts."""
import ctypes as C
import importlib.util
import math
from pathlib import Path

import numpy as np
import pytest

import elodin_amd as ea
from elodin_amd import _lib as L
from tests import golden_util as gu
from tests.test_gpu_history_envelope import _program_exec
from tests.test_gpu_history_watch import _exec

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FIELDS = ("world_pos", "world_vel", "world_accel", "force")
EPS = float(np.finfo(np.float64).eps)
SIX = [("world_pos", 4), ("world_pos", 5), ("world_pos", 6), ("world_vel", 3), ("world_vel", 4), ("world_vel", 5)]      # position and velocity
TWO = [("world_vel", 0), ("world_vel", 1)]                                                                              # inside one component
FIVE = [("world_pos", 4), ("world_accel", 1), ("force", 4), ("world_vel", 3), ("world_pos", 6)]                         # four components
KEYS = ("count", "mean", "comoment", "cov", "corr")


def _columns(hip, channels, first, last, every):
    """[samples, n, k] f64: the channels' columns out of the blocks HipExec.history reads."""
    blocks = {name: hip.history(name, first, last)[::every] for name in dict.fromkeys(name for name, _ in channels)}
    return np.stack([blocks[name][:, :, element] for name, element in channels], axis=-1).astype(np.float64)


def _reference(x, period=1):
    """Out of [t, n, k] columns: count [t, period], mean and mean|x| and m2 and S [t, period, k], comoment [t, period, k, k]; long double."""
    t, n, k = x.shape
    x = x.reshape(t, n // period, period, k)
    fin = np.isfinite(x).all(axis=-1)                                   # listwise
    cnt = fin.sum(axis=1)
    xl = np.where(fin[..., None], x, 0.0).astype(np.longdouble)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = xl.sum(axis=1) / cnt[..., None]
        mean_abs = np.abs(xl).sum(axis=1) / cnt[..., None]
        dev = np.where(fin[..., None], xl - mean[:, None], 0.0)
    com = (dev[..., :, None] * dev[..., None, :]).sum(axis=1)
    return {"count": cnt, "mean": mean, "mean_abs": mean_abs, "comoment": com, "m2": np.diagonal(com, axis1=-2, axis2=-1), "S": (xl * xl).sum(axis=1)}


def _ratio(err, bound):
    return float(np.max(np.where(err == 0, 0.0, err / np.where(bound == 0, np.finfo(np.float64).tiny, bound)), initial=0.0))


def _check(got, ref, what):
    """One read against the reference under the module's bounds; returns the (mean, co-moment) worst error / bound."""
    cnt = ref["count"]
    k = ref["mean"].shape[-1]
    assert sorted(got) == sorted(KEYS), what
    assert got["count"].dtype == np.int64 and got["count"].shape == cnt.shape, (what, got["count"].shape, cnt.shape)
    assert np.array_equal(got["count"], cnt), (what, "count")
    assert got["mean"].shape == cnt.shape + (k,) and all(got[key].shape == cnt.shape + (k, k) for key in ("comoment", "cov", "corr")), what
    some = cnt > 0
    for key in ("mean", "comoment", "cov", "corr"):
        assert got[key].dtype == np.float64 and np.all(np.isnan(got[key][~some])), (what, key, "a group without a usable row must read NaN")
    c = cnt[some].astype(np.longdouble)
    mean_err = np.abs(got["mean"][some].astype(np.longdouble) - ref["mean"][some])
    mean_bound = 2 * c[:, None] * EPS * ref["mean_abs"][some]
    m2, s = ref["m2"][some], ref["S"][some]
    com_err = np.abs(got["comoment"][some].astype(np.longdouble) - ref["comoment"][some])
    com_bound = c[:, None, None] * EPS * (np.sqrt(m2[:, :, None] * s[:, None, :]) + np.sqrt(m2[:, None, :] * s[:, :, None]))
    r_mean, r_com = _ratio(mean_err, mean_bound), _ratio(com_err, com_bound)
    print(f"{what}: worst mean error / bound {r_mean:.3g}, worst co-moment error / bound {r_com:.3g}")
    assert np.all(mean_err <= mean_bound), (what, "mean", r_mean)
    assert np.all(com_err <= com_bound), (what, "comoment", r_com)
    com = got["comoment"][some]
    assert np.array_equal(com, np.swapaxes(com, -1, -2)), (what, "symmetry")
    assert np.array_equal(got["cov"][some], com / cnt[some][:, None, None]), (what, "cov")
    diag = np.diagonal(com, axis1=-2, axis2=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.sqrt(diag[:, :, None] * diag[:, None, :])
        corr = np.where(scale > 0, com / scale, np.nan)
    assert np.array_equal(got["corr"][some], corr, equal_nan=True), (what, "corr")
    return r_mean, r_com


def _check_read(hip, channels, got, first, last, every, period=1, what=""):
    return _check(got, _reference(_columns(hip, channels, first, last, every), period), what)


def _same(a, b):
    for key in KEYS:
        assert a[key].tobytes() == b[key].tobytes(), key


def _sample(d, j):
    return {k: v[j:j + 1] for k, v in d.items()}


def _channel_array(channels, reserved=0):
    arr = (L.CovChannel * max(1, len(channels)))()
    for i, (name, element) in enumerate(channels):
        arr[i].component_id, arr[i].element, arr[i].reserved = L.component_id(name), element, reserved
    return arr


def _raw(hip, channels, first, n_samples, every, period, buf, flags=0, n_channels=None, arr=None):
    arr = _channel_array(channels) if arr is None else arr
    ptr = buf.ctypes.data if buf is not None else None
    return hip._lib.sixdof_history_covariance(hip._h, arr, len(channels) if n_channels is None else n_channels, first, n_samples, every, period, ptr, flags)


# ---- 1. values, range shapes, dtypes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,ring,run,first,every,dtype", [
    (300, 8, 10, 27, 18, 3, np.float64),       # ticks 18 .. 27 sit in slots 7 8 9 0 .. 6: the range wraps the ring
    (4099, 7, 64, 50, 1, 7, np.float64),       # several blocks per sample, a ragged last tile
    (1, 1, 4, 4, 4, 1, np.float64),            # one sample each: one row, one short of a wavefront, one past it
    (63, 4, 4, 4, 4, 1, np.float64),
    (65, 4, 4, 4, 4, 1, np.float64),
    (64, 1, 8, 8, 1, 1, np.float32),
])
def test_covariances_equal_numpy_over_the_history_blocks(n, k, ring, run, first, every, dtype):
    hip, _ = _exec(n, k, dtype)
    hip.enable_history(ring)
    hip.run(run)
    last = first + (run - first) // every * every
    samples = (last - first) // every + 1
    for channels in (SIX, TWO, FIVE):
        got = hip.history_covariance(channels, first, run, every)
        assert got["mean"].shape == (samples, 1, len(channels))
        _check_read(hip, channels, got, first, last, every, what=f"n {n} {np.dtype(dtype).name} k {len(channels)}")
        assert np.all(got["count"] == n)
    if samples > 1:                                                    # the ticks differ: not one block repeated
        assert not np.array_equal(got["mean"][0], got["mean"][-1])
    if n > 1:                                                          # something varies, and varies together
        six = hip.history_covariance(SIX, run, run)
        assert np.all(np.einsum("spaa->spa", six["comoment"]) > 0) and np.all(np.abs(six["corr"]) <= 1.0 + 1e-12)
    hip.close()


# ---- 2. listwise skipping -----------------------------------------------------------------------------------------------
def test_rows_with_a_non_finite_channel_are_dropped_from_every_entry():
    n = 300
    hip, _ = _exec(n, 8)
    hip.world_vel[[0, 63, 64, 299]] = np.nan
    hip.world_vel[150, 4] = np.inf
    hip.world_vel[5::12, 3] = np.nan                                   # every row of group 5 of 12
    hip.upload()
    hip.enable_history(8)
    hip.run(8)
    for channels in (SIX, TWO, FIVE, [("world_vel", 4), ("world_pos", 4)]):
        got = hip.history_covariance(channels, 1, 8, 1)
        ref = _reference(_columns(hip, channels, 1, 8, 1))
        _check(got, ref, f"diverged rows, k {len(channels)}")
        assert np.all(got["count"] <= n - 4) and np.all(np.isfinite(got["mean"])) and np.all(np.isfinite(got["comoment"]))
    # one channel's inf drops the row from EVERY entry: the mean of the other channel is the mean without row 150
    pair = hip.history_covariance([("world_vel", 4), ("world_vel", 0)], 1, 1)
    vel = hip.history("world_vel", 1, 1)[0].astype(np.float64)
    assert not np.isfinite(vel[150, 4]) and np.isfinite(vel[150, 0])
    used = np.isfinite(vel[:, 4]) & np.isfinite(vel[:, 0])
    assert pair["count"][0, 0] == used.sum() < np.isfinite(vel[:, 0]).sum()
    assert abs(pair["mean"][0, 0, 1] - vel[used, 0].mean()) <= 2 * n * EPS * np.abs(vel[used, 0]).mean()
    # a group whose rows are all dropped: count 0 and NaN, the other groups untouched
    grouped = hip.history_covariance(SIX, 2, 8, 3, period=12)
    _check_read(hip, SIX, grouped, 2, 8, 3, 12, what="diverged rows, period 12")
    assert np.all(grouped["count"][:, 5] == 0) and np.all(np.isnan(grouped["mean"][:, 5])) and np.all(np.isnan(grouped["comoment"][:, 5]))
    assert np.all(grouped["count"][:, [1, 2, 7, 8, 9, 10]] == n // 12)
    hip.close()


def test_a_non_finite_element_that_is_not_listed_drops_nothing():
    """The program of the envelope tests with `a` NaN in every row: the NaN reaches c[2] in tick 1 and b[0] in tick 2."""
    hip = _program_exec(a_nan=True)
    hip.enable_history(16)
    hip.run(12)
    assert np.all(np.isnan(hip.history("a", 1, 2))) and np.all(np.isnan(hip.history("b", 2, 2)[0, :, 0]))
    b = hip.history_covariance([("b", 0), ("b", 1)], 1, 1)                      # `a`, an unlisted component, is NaN
    assert np.all(b["count"] == 200)
    _check_read(hip, [("b", 0), ("b", 1)], b, 1, 1, 1, what="unlisted component NaN")
    bc = hip.history_covariance([("b", 1), ("c", 0), ("world_pos", 4)], 2, 2)    # b[0], an unlisted element of a listed component, is NaN
    assert np.all(bc["count"] == 200)
    _check_read(hip, [("b", 1), ("c", 0), ("world_pos", 4)], bc, 2, 2, 1, what="unlisted element NaN")
    ab = hip.history_covariance([("a", 0), ("b", 1)], 1, 2)                      # listed: every row goes
    assert ab["count"].shape == (2, 1) and np.all(ab["count"] == 0)
    for key in ("mean", "comoment", "cov", "corr"):
        assert np.all(np.isnan(ab[key])), key
    hip.close()


# ---- 3. groups -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,period", [(4100, 4), (300, 12), (320, 64)])
def test_groups_reduce_rows_of_equal_index_modulo_period(n, period):
    hip, _ = _exec(n, 4)
    hip.enable_history(8)
    hip.run(8)
    for channels in (SIX, TWO):
        got = hip.history_covariance(channels, 2, 8, 3, period=period)
        assert got["comoment"].shape == (3, period, len(channels), len(channels)) and np.all(got["count"] == n // period)
        _check_read(hip, channels, got, 2, 8, 3, period, what=f"n {n} period {period} k {len(channels)}")
        assert not np.array_equal(got["mean"][:, 0], got["mean"][:, 1])       # the groups differ
    hip.close()


# ---- 4. conditioning ---------------------------------------------------------------------------------------------------
def test_positions_metres_apart_at_earth_radius():
    """world_pos' linear part at 6.4e6 m plus a unit normal, y tied to x: the case sum x y - c mean_x mean_y loses entirely."""
    n = 4099
    hip, _ = _exec(n, 4)
    z = np.random.default_rng(11).normal(size=(n, 3))
    z[:, 1] = 0.8 * z[:, 0] + 0.6 * z[:, 1]
    hip.world_pos[:, 4:7] = 6.4e6 + z
    hip.upload()
    hip.enable_history(4)
    hip.run(4)
    channels = SIX[:3]
    got = hip.history_covariance(channels, 1, 4, 3)
    x = _columns(hip, channels, 1, 4, 3)
    ref = _reference(x)
    _, r_com = _check(got, ref, "positions at 6.4e6 +- 1 m")
    assert r_com <= 1.0
    std = np.sqrt(np.einsum("spaa->spa", got["cov"]))
    rc = ref["comoment"][:, 0]
    want_corr = (rc[:, 0, 1] / np.sqrt(rc[:, 0, 0] * rc[:, 1, 1])).astype(np.float64)
    assert np.all(std > 0.5) and np.all(std < 2.0) and abs(got["corr"][0, 0, 0, 1] - 0.8) < 0.05      # as planted, before the velocities spread it
    assert np.all(np.abs(got["corr"][:, 0, 0, 1] - want_corr) < 1e-9)
    # the textbook form in f64 over the same rows misses the same bound
    textbook = np.einsum("tna,tnb->tab", x, x) - n * np.einsum("ta,tb->tab", x.mean(axis=1), x.mean(axis=1))
    m2, s = ref["m2"][:, 0], ref["S"][:, 0]
    bound = n * EPS * (np.sqrt(m2[:, :, None] * s[:, None, :]) + np.sqrt(m2[:, None, :] * s[:, :, None]))
    miss = np.abs(textbook.astype(np.longdouble) - ref["comoment"][:, 0]) / bound
    print(f"textbook sum x y - c mean mean: worst error / bound {float(miss.max()):.3g}")
    assert miss.max() > 1.0
    hip.close()


# ---- 5. bit-identity ---------------------------------------------------------------------------------------------------
def test_a_tick_reads_the_same_bits_however_it_is_read():
    n = 4099
    hip, _ = _exec(n, 7)
    hip.enable_history(32)
    hip.run(30)
    whole = hip.history_covariance(SIX, 3, 30, 3)
    _same(whole, hip.history_covariance(SIX, 3, 30, 3))                                   # two identical calls
    for j, tick in enumerate(range(3, 31, 3)):
        _same(_sample(whole, j), hip.history_covariance(SIX, tick, tick))                 # the one-sample read of that tick
    other = hip.history_covariance(SIX, 6, 30, 6)                                         # another every
    for j, tick in enumerate(range(6, 31, 6)):
        _same(_sample(other, j), _sample(whole, (tick - 3) // 3))
    buf = np.zeros((10, 1, 28))                                                           # synchronous against SIXDOF_COVARIANCE_ASYNC
    assert _raw(hip, SIX, 3, 10, 3, 1, buf, L.COVARIANCE_ASYNC) == L.OK
    hip.download_wait()
    _same(whole, hip._covariance_dict(buf, 6))
    grouped = hip.history_covariance(SIX, 3, 30, 3, period=1)
    _same(grouped, whole)
    # no row is non-finite: the count is the envelope's, and the means and diagonals agree with it within both bounds' sum
    env = hip.history_envelope(["world_pos"], 3, 30, 3)["world_pos"]
    assert np.array_equal(whole["count"], env["count"][:, :, 4]) and np.all(whole["count"] == n)
    hip.sync()
    hip.close()


# ---- 6. a duplicated channel ------------------------------------------------------------------------------------------
def test_a_channel_listed_twice_gives_bit_equal_entries():
    hip, _ = _exec(4099, 4)
    hip.enable_history(4)
    hip.run(4)
    twice = hip.history_covariance([("world_pos", 4), ("world_vel", 3), ("world_pos", 4)], 2, 4, period=1)
    com = twice["comoment"]
    assert com[:, :, 0, 0].tobytes() == com[:, :, 0, 2].tobytes() == com[:, :, 2, 2].tobytes()
    assert twice["mean"][:, :, 0].tobytes() == twice["mean"][:, :, 2].tobytes()
    # (C_01 and C_12 are sums of d_0 e_1 and of d_1 e_2 — old mean times new mean, the other way round: equal in value, not in bits)
    assert np.allclose(com[:, :, 0, 1], com[:, :, 1, 2], rtol=1e-9, atol=0.0)
    assert np.all(twice["corr"][:, :, 0, 2] == 1.0)
    once = hip.history_covariance([("world_pos", 4), ("world_vel", 3)], 2, 4)              # the geometry does not depend on the list
    assert once["comoment"].tobytes() == np.ascontiguousarray(com[:, :, :2, :2]).tobytes()
    assert once["mean"].tobytes() == np.ascontiguousarray(twice["mean"][:, :, :2]).tobytes()
    hip.close()


# ---- 7. refusals copy nothing -------------------------------------------------------------------------------------------
def test_refused_reads_copy_nothing():
    hip, _ = _exec(300, 8)
    sentinel = lambda: np.full((4, 100, 28), 123.0)
    buf = sentinel()
    bad = L.ERR_INVALID_ARGUMENT
    assert _raw(hip, SIX, 1, 1, 1, 1, buf) == bad                                 # no ring
    hip.run(5)
    hip.enable_history(10)                                                       # recording starts at tick 6
    hip.run(25)                                                                  # the ring keeps 21 .. 30
    assert _raw(hip, SIX, 21, 4, 0, 1, buf) == bad                                # every = 0
    assert _raw(hip, SIX, 21, 4, 1, 0, buf) == bad                                # period = 0
    assert _raw(hip, SIX, 21, 4, 1, 7, buf) == bad                                # 300 % 7 != 0
    assert _raw(hip, SIX, 21, 4, 1, 300, buf) == bad                              # above the threads of a stage-1 block
    assert str(L.COVARIANCE_MAX_PERIOD) in hip._lib.sixdof_last_error(hip._h).decode()
    assert _raw(hip, SIX, 21, 4, 1, 1, buf, n_channels=0) == bad
    assert _raw(hip, SIX, 21, 4, 1, 1, buf, n_channels=1) == bad                  # one channel: the envelope's job
    assert "envelope" in hip._lib.sixdof_last_error(hip._h).decode()
    assert _raw(hip, SIX + SIX[:1], 21, 4, 1, 1, buf) == bad                      # seven
    assert hip._lib.sixdof_history_covariance(hip._h, None, 6, 21, 4, 1, 1, buf.ctypes.data, 0) == bad
    assert _raw(hip, SIX, 21, 4, 1, 1, None) == bad                               # a null buffer
    assert _raw(hip, [("world_pos", 7), ("world_vel", 0)], 21, 4, 1, 1, buf) == bad          # element >= w
    assert _raw(hip, [("world_pos", 4), ("world_vel", 6)], 21, 4, 1, 1, buf) == bad
    assert _raw(hip, TWO, 21, 4, 1, 1, buf, arr=_channel_array(TWO, reserved=1)) == bad      # reserved != 0
    assert _raw(hip, SIX, 20, 4, 1, 1, buf) == bad                                # has fallen out of the ring
    assert _raw(hip, SIX, 28, 4, 1, 1, buf) == bad                                # runs beyond `tick`
    assert _raw(hip, SIX, 24, 4, 3, 1, buf) == bad                                # its last sample does
    assert _raw(hip, SIX, 31, 1, 1, 1, buf) == bad
    assert _raw(hip, SIX, 21, 4, 1, 1, buf, 2) == bad                             # unknown flags
    assert _raw(hip, [("world_pos", 4), ("inertia", 0)], 21, 4, 1, 1, buf) == L.ERR_COMPONENT_NOT_FOUND
    assert np.array_equal(buf, sentinel())                                      # nothing was copied
    for args in ((20, 30, 1), (21, 31, 1), (21, 30, 0), (5, 5, 1)):
        with pytest.raises(ValueError):
            hip.history_covariance(SIX, *args)
    for period in (7, 0, 300):
        with pytest.raises(ValueError):
            hip.history_covariance(SIX, 21, 30, 1, period=period)
    for channels in (SIX[:1], SIX + SIX[:1], [("world_pos", 7), ("world_vel", 0)]):
        with pytest.raises(ValueError):
            hip.history_covariance(channels, 21, 30)
    with pytest.raises(KeyError):
        hip.history_covariance([("world_pos", 4), ("inertia", 0)], 21, 30)
    assert _raw(hip, SIX, 21, 0, 1, 1, buf) == L.OK and _raw(hip, SIX, 99, 0, 7, 1, buf) == L.OK      # no samples: a no-op
    assert np.array_equal(buf, sentinel())
    assert hip.history_covariance(SIX, 30, 29)["comoment"].shape == (0, 1, 6, 6)
    raw = np.full((4, 100, 28), 123.0)
    assert _raw(hip, SIX, 21, 4, 3, 100, raw) == L.OK                             # 21 24 27 30, three rows per group
    _check_read(hip, SIX, hip._covariance_dict(raw, 6), 21, 30, 3, 100, what="after the refusals")
    hip.enable_history(0)
    with pytest.raises(ValueError, match="no history ring"):
        hip.history_covariance(SIX, 21, 30)
    hip.close()


# ---- 8. streaming ---------------------------------------------------------------------------------------------------------
def test_streamed_covariances_equal_a_twin_read_tick_by_tick():
    """stream_covariance: every fourth tick of six 16-tick batches out of a ring one batch deep; each sample is bit-equal to what a
    twin stepped one tick at a time reads at that tick, and streaming leaves the state a plain run leaves."""
    n = 1000
    a, _ = _exec(n, 8)
    b, _ = _exec(n, 1)
    plain, _ = _exec(n, 8)
    got, order = {}, []

    def consume(i, first_tick, cov):
        order.append((i, first_tick))
        assert sorted(cov) == sorted(KEYS) and cov["comoment"].shape == (4, 5, 6, 6) and cov["count"].dtype == np.int64
        for j in range(4):
            got[first_tick + 4 * j] = {k: v[j:j + 1].copy() for k, v in cov.items()}
    with pytest.raises(ValueError):
        a.stream_covariance(SIX, 6, 16, every=5)
    with pytest.raises(ValueError):
        a.stream_covariance(SIX[:1], 6, 16, every=4)
    wall = a.stream_covariance(SIX, 6, 16, every=4, period=5, consume=consume)
    assert wall > 0.0 and a.tick == 96
    assert order == [(i, 16 * i + 4) for i in range(6)] and sorted(got) == list(range(4, 97, 4))
    b.enable_history(4)
    for t in range(1, 97):
        b.run(1)
        if t in got:
            _same(got[t], b.history_covariance(SIX, t, t, period=5))
    a.download()
    plain.run(96)
    for c in FIELDS:
        assert np.array_equal(getattr(a, c), getattr(plain, c)), c
    for h in (a, b, plain):
        h.close()


def test_async_covariance_alongside_a_history_stream_copy():
    """A sixdof_history_stream copy and, before it is waited for, an asynchronous covariance read: one download_wait covers both."""
    n = 500
    hip, _ = _exec(n, 4)
    hip.enable_history(16)
    hip.run(16)
    want_blocks = {c: hip.history(c, 5, 12) for c in FIELDS}
    want = hip.history_covariance(FIVE, 10, 16, 2, period=5)
    blocks = {c: np.zeros((8, n, 7 if c == "world_pos" else 6)) for c in FIELDS}
    buf = np.zeros((4, 5, 21))
    assert hip._lib.sixdof_history_stream(hip._h, 5, 8, (C.c_void_p * 4)(*[blocks[c].ctypes.data for c in FIELDS])) == L.OK
    assert _raw(hip, FIVE, 10, 4, 2, 5, buf, L.COVARIANCE_ASYNC) == L.OK
    hip.download_wait()
    for c in FIELDS:
        assert np.array_equal(blocks[c], want_blocks[c]), c
    _same(hip._covariance_dict(buf, 5), want)
    _check_read(hip, FIVE, want, 10, 16, 2, 5, what="asynchronous, period 5")
    hip.run(4)                                               # the stepper goes on; the page locks end at sync
    hip.sync()
    assert hip.tick == 20
    hip.close()


# ---- 9. program columns, the pair path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("column_soa", ["0", "1"])
def test_a_program_column_and_a_body_column_in_one_call(column_soa, monkeypatch):
    monkeypatch.setenv("SIXDOF_COLUMN_SOA", column_soa)
    hip = _program_exec()
    channels = [("a", 0), ("world_pos", 4), ("c", 2), ("b", 1)]
    hip.enable_history(32)
    hip.run(30)
    got = hip.history_covariance(channels, 3, 30, 3)
    assert got["comoment"].shape == (10, 1, 4, 4) and np.all(got["count"] == 200)
    _check_read(hip, channels, got, 3, 30, 3, what=f"program columns, column_soa {column_soa}")
    assert hip._column_soa == (column_soa == "1")
    assert not np.array_equal(got["mean"][0], got["mean"][-1])
    grouped = hip.history_covariance(channels, 30, 30, period=8)
    _check_read(hip, channels, grouped, 30, 30, 1, 8, what="program columns, period 8")
    with pytest.raises(ValueError, match="window component"):
        hip.history_covariance([("buf", 0), ("a", 0)], 3, 30)
    buf = np.full((1, 1, 6), 123.0)                          # the library refuses the window too, not only the Python surface
    assert _raw(hip, [("a", 0), ("buf", 0)], 30, 1, 1, 1, buf) == L.ERR_COMPONENT_NOT_FOUND
    assert _raw(hip, [("a", 1), ("b", 0)], 30, 1, 1, 1, buf) == L.ERR_INVALID_ARGUMENT        # `a` is one wide
    assert np.all(buf == 123.0)
    hip.close()


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
    _check_read(hip, SIX, hip.history_covariance(SIX, 6, 13), 6, 13, 1, what="three bodies")
    _check_read(hip, FIVE, hip.history_covariance(FIVE, 7, 13, 3), 7, 13, 3, what="three bodies, every 3")
    per_body = hip.history_covariance(SIX, 7, 13, 3, period=3)
    _check_read(hip, SIX, per_body, 7, 13, 3, 3, what="three bodies, one per group")
    assert np.all(per_body["count"] == 1) and np.all(per_body["comoment"] == 0.0)
    assert np.array_equal(per_body["mean"][-1], np.concatenate([hip.world_pos[:, 4:7], hip.world_vel[:, 3:6]], axis=1))
    hip.close()


# ---- 10. front end ---------------------------------------------------------------------------------------------------------
def test_front_end_covariance_of_one_entity_is_its_series():
    spec = importlib.util.spec_from_file_location("ball", ROOT / "examples" / "ball.py")
    ball = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ball)
    ex = ball.world(0).build(ball.system(), simulation_rate=120.0, telemetry_rate=40.0, history=True)
    ex.enable_history(64)
    ex.run(30)
    channels = [("world_pos", 4), ("world_pos", 6), ("world_vel", 5), ("wind", 0)]
    series = ex.history_series(["ball.world_pos", "ball.world_vel", "ball.wind"], 3, 30, every=3)
    cov = ex.history_covariance(channels, 3, 30, every=3)
    assert sorted(cov) == sorted(KEYS + ("time",)) and np.array_equal(cov["time"], series["time"])
    assert cov["count"].shape == (10, 1) and np.all(cov["count"] == 1)
    assert np.all(cov["comoment"] == 0.0) and np.all(cov["cov"] == 0.0) and np.all(np.isnan(cov["corr"]))
    wind = series["ball.wind"] if series["ball.wind"].ndim == 2 else series["ball.wind"][:, None]
    want = np.stack([series["ball.world_pos"][:, 4], series["ball.world_pos"][:, 6], series["ball.world_vel"][:, 5], wind[:, 0]], axis=1)
    assert np.array_equal(cov["mean"][:, 0], want)
    assert not np.array_equal(cov["mean"][0], cov["mean"][-1])
    with pytest.raises(KeyError):
        ex.history_covariance([("nothing", 0), ("world_pos", 4)], 3, 30)
    with pytest.raises(ValueError):
        ex.history_covariance(channels, 0, 30)               # tick 0 is not in the ring
    with pytest.raises(ValueError):
        ex.history_covariance(channels, 3, 30, every=0)
    ex._hip.close()


def test_campaign_covariance_and_its_dispersion_ellipse():
    """A 400-run campaign of the Monte-Carlo example with the control law on the device: Campaign.covariance per tick against numpy
    over Campaign.column after each tick.  Wind (the initial velocity) and target are drawn normal and independent, and below
    saturation of the command the plant is linear but for a drag of a few per cent, so (position, velocity) is a linear image
    of a bivariate normal: the ellipse dispersion_ellipse makes of their 2 x 2 block at prob p holds Binomial(400, p) of the runs.
    Spread used: 4 standard deviations, 4 sqrt(400 p (1 - p)) — 24 runs at p = 0.9, 40 at p = 0.5."""
    from tests.test_gpu_monte_carlo_example import example
    from elodin_amd import vectorize
    ex = example(0)
    runs = 400
    rng = np.random.default_rng(5)
    params = [{"mass": 1.5, "thrust_gain": 1.0, "wind": float(w), "target_x": float(t)}
              for w, t in zip(np.clip(rng.normal(0.0, 0.5, runs), -4.0, 4.0), np.clip(rng.normal(10.0, 2.0, runs), 5.0, 16.0))]
    c = vectorize.Campaign(ex.build_closed_loop, vectorize.plan_of(params), ex.PARAMS, simulation_rate=ex.SIMULATION_RATE_HZ)
    assert c.n_runs == runs and c.entities_per_run == 1
    channels = [("position", 0), ("velocity", 0), ("specific_force", 0)]
    c.exec.enable_history(16)
    cols = []
    for _ in range(12):
        c.exec.run(1)
        cols.append(np.concatenate([np.array(c.column(name), dtype=np.float64).reshape(runs, 1) for name, _ in channels], axis=1))
    cov = c.covariance(channels, 2, 12, every=5)                  # ticks 2, 7, 12
    assert np.allclose(cov["time"], np.array([2, 7, 12]) / ex.SIMULATION_RATE_HZ)
    ref = _reference(np.stack([cols[t - 1] for t in (2, 7, 12)]))
    _check({k: cov[k] for k in KEYS}, ref, "campaign")
    assert np.all(cov["count"] == runs)
    xy = cols[11][:, :2] - cov["mean"][-1, 0, :2]                 # position and velocity after tick 12, about their mean
    for prob in (0.9, 0.5):
        major, minor, angle = ea.dispersion_ellipse(cov["cov"][-1, 0, :2, :2], prob)
        u = math.cos(angle) * xy[:, 0] + math.sin(angle) * xy[:, 1]
        v = -math.sin(angle) * xy[:, 0] + math.cos(angle) * xy[:, 1]
        inside = int(np.sum((u / major) ** 2 + (v / minor) ** 2 <= 1.0))
        spread = 4.0 * math.sqrt(runs * prob * (1.0 - prob))
        print(f"dispersion ellipse at {prob}: {inside} of {runs} runs inside, expected {runs * prob:.0f} +- {spread:.0f}")
        assert abs(inside - runs * prob) <= spread, (prob, inside)
    c.exec._hip.close()
