"""Ring quantiles (sixdof_history_quantiles): per sampled tick, group and component element the count m of finite elements and,
per rank num / den, the order statistics x(floor(num (m-1) / den)) and x(ceil(num (m-1) / den)), selected on the device out of
the telemetry ring.

The reference of every value test is numpy over the [ticks, n, w] blocks HipExec.history reads from the same ring: upcast to
f64, the finite elements of a group and element selected, np.sort, indexed with the Python integers num * (m - 1) // den and
-(-num * (m - 1) // den).  An order statistic is an element of the ring, not a rounded sum: count, lower and upper are compared
with np.array_equal (NaN equal to NaN) — there is no tolerance anywhere.  Where signed zeros matter the bits are compared too,
against a sort of the order-preserving integer keys."""
import ctypes as C
import importlib.util
import json
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import elodin_amd as ea
from elodin_amd import _lib as L
from elodin_amd import dsl, workloads
from tests import golden_util as gu
from tests.test_gpu_history_envelope import _program_exec
from tests.test_gpu_history_watch import _exec

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FIELDS = ("world_pos", "world_vel", "world_accel", "force")
KEYS = ("count", "lower", "upper", "linear")
U64P = C.POINTER(C.c_uint64)
Q = [(0, 1), (1, 100), (1, 2), (99, 100), (1, 1), (1, 2)]          # the last one a duplicate


def _width(c):
    return 7 if c == "world_pos" else 6


def _reference(blocks, q, period=1):
    """count [t, period, w] and lower, upper [t, period, Q, w] out of [t, n, w] blocks: np.sort and integer indexing."""
    num, den = ea.HipExec.quantile_ranks(q)
    t, n, w = blocks.shape
    x = blocks.astype(np.float64).reshape(t, n // period, period, w)
    count = np.zeros((t, period, w), dtype=np.int64)
    lower = np.full((t, period, len(num), w), np.nan)
    upper = np.full((t, period, len(num), w), np.nan)
    for j in range(t):
        for g in range(period):
            for c in range(w):
                col = x[j, :, g, c]
                v = np.sort(col[np.isfinite(col)])
                m = count[j, g, c] = len(v)
                for i, k in enumerate(num):
                    if m:
                        lower[j, g, i, c] = v[int(k) * (m - 1) // den]
                        upper[j, g, i, c] = v[-(-int(k) * (m - 1) // den)]
    return {"count": count, "lower": lower, "upper": upper}


def _check(got, ref, what):
    assert got["count"].dtype == np.int64 and got["count"].shape == ref["count"].shape, what
    assert np.array_equal(got["count"], ref["count"]), (what, "count")
    for k in ("lower", "upper"):
        assert got[k].dtype == np.float64 and got[k].shape == ref[k].shape, (what, k)
        assert np.array_equal(got[k], ref[k], equal_nan=True), (what, k, int(np.sum(~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k]))))))
    assert got["linear"].shape == ref["lower"].shape, what


def _check_all(hip, names, got, first, last, every, q, period=1, what=""):
    assert sorted(got) == sorted(names)
    for name in names:
        _check(got[name], _reference(hip.history(name, first, last)[::every], q, period), f"{what} {name}")


def _same(a, b):
    """Bit-equality of two quantile dicts {name: {key: array}}."""
    assert sorted(a) == sorted(b)
    for name in a:
        for k in KEYS:
            assert a[name][k].tobytes() == b[name][k].tobytes(), (name, k)


def _sample(d, j):
    return {name: {k: v[j:j + 1] for k, v in e.items()} for name, e in d.items()}


def _ranks(d, idx):
    return {name: {k: (v if k == "count" else v[:, :, idx]) for k, v in e.items()} for name, e in d.items()}


def _raw(hip, names, first, n_samples, every, period, num, den, bufs, flags=0, n_ranks=None):
    comp = np.array([L.component_id(n) for n in names], dtype=np.uint64)
    ptrs = (C.c_void_p * max(1, len(bufs)))(*[b.ctypes.data for b in bufs])
    nums = (C.c_uint32 * max(1, len(num)))(*num)
    return hip._lib.sixdof_history_quantiles(hip._h, comp.ctypes.data_as(U64P), len(names), first, n_samples, every, period, nums, den,
                                             len(num) if n_ranks is None else n_ranks, ptrs, flags)


# ---- 1. values, range shapes, dtypes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,ring,run,first,every,dtype", [
    (300, 8, 10, 27, 18, 3, np.float64),       # ticks 18 .. 27 sit in slots 7 8 9 0 .. 6: the range wraps the ring
    (4099, 7, 64, 50, 1, 7, np.float64),       # several row blocks per sample, a ragged last sweep
    (64, 1, 8, 8, 1, 1, np.float32),
    (1, 1, 4, 4, 4, 1, np.float64),            # one sample each: one row, one short of a wavefront, one past it
    (63, 4, 4, 4, 4, 1, np.float64),
    (65, 4, 4, 4, 4, 1, np.float64),
])
def test_quantiles_equal_numpy_sort_over_the_history_blocks(n, k, ring, run, first, every, dtype):
    hip, _ = _exec(n, k, dtype)
    hip.enable_history(ring)
    hip.run(run)
    last = first + (run - first) // every * every
    got = hip.history_quantiles(FIELDS, first, run, Q, every)             # the four columns in one call
    samples = (last - first) // every + 1
    assert [got[c]["lower"].shape for c in FIELDS] == [(samples, 1, 6, 7)] + [(samples, 1, 6, 6)] * 3
    assert [got[c]["count"].shape for c in FIELDS] == [(samples, 1, 7)] + [(samples, 1, 6)] * 3
    _check_all(hip, FIELDS, got, first, last, every, Q, what=f"n {n} {np.dtype(dtype).name}")
    assert np.all(got["world_pos"]["count"] == n)
    env = hip.history_envelope(FIELDS, first, run, every)                 # rank 0 is the minimum, rank 1 the maximum, bit for bit
    for c in FIELDS:
        for plane in ("lower", "upper"):
            assert got[c][plane][:, :, 0].tobytes() == env[c]["min"].tobytes(), (c, plane, "min")
            assert got[c][plane][:, :, 4].tobytes() == env[c]["max"].tobytes(), (c, plane, "max")
        assert np.array_equal(got[c]["lower"][:, :, 2], got[c]["lower"][:, :, 5]) and np.array_equal(got[c]["upper"][:, :, 2], got[c]["upper"][:, :, 5])
    if samples > 1:                                                        # the ticks differ: not one block repeated
        assert not np.array_equal(got["world_pos"]["lower"][0], got["world_pos"]["lower"][-1])
    one = hip.history_quantiles("world_vel", run, run, [Fraction(1, 3)])   # one name, one sample, one rank
    assert sorted(one) == ["world_vel"] and sorted(one["world_vel"]) == sorted(KEYS)
    assert one["world_vel"]["count"].shape == (1, 1, 6) and all(one["world_vel"][k].shape == (1, 1, 1, 6) for k in KEYS[1:])
    _check_all(hip, ["world_vel"], one, run, run, 1, [Fraction(1, 3)], what=f"n {n} single sample")
    hip.close()


# ---- 2. crafted bit patterns ---------------------------------------------------------------------------------------------
def _crafted(n, dtype):
    """[n, 6]: one pattern per element."""
    f = np.finfo(dtype)
    u = np.uint64 if dtype == np.float64 else np.uint32
    mant = 52 if dtype == np.float64 else 23
    r = np.arange(n)
    x = np.empty((n, 6), dtype=dtype)
    x[:, 0] = -3.25                                                                         # all rows equal
    x[:, 1] = np.where(r < n // 2, 2.5, -1.5)                                               # two values in runs of 150
    x[:, 2] = (np.array(1.0, dtype=dtype).view(u) + ((r * 37) % 251).astype(u)).view(dtype)  # apart in the lowest byte of the mantissa only
    sign = (r % 2).astype(u) << u(dtype().itemsize * 8 - 1)
    x[:, 3] = (sign | ((u(1000 if dtype == np.float64 else 100) + (r % 40).astype(u)) << u(mant))).view(dtype)   # sign and exponent only
    mix = np.array([-1.0, -0.0, 0.0, f.smallest_subnormal, -f.smallest_subnormal, f.max, -f.max, f.tiny, -7.5, 1e-30], dtype=dtype)
    x[:, 4] = mix[(r * 7) % 10]                                                              # negatives, +-0, denormals, +-max
    x[:, 5] = (r % 17 - 8.0).astype(dtype)
    x[[1, 77, 153, 229], 5] = np.nan                                                         # four NaN rows, one +inf, one -inf
    x[5, 5], x[6, 5] = np.inf, -np.inf
    return x


def _keys(x):
    """The order-preserving integer keys of an f32 / f64 array."""
    u = x.view(np.uint64 if x.dtype == np.float64 else np.uint32)
    top = u.dtype.type(1) << u.dtype.type(x.dtype.itemsize * 8 - 1)
    return np.where(u & top, ~u, u | top)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_order_statistic_of_crafted_bit_patterns(dtype):
    n = 300
    np_ = dsl.np

    @dsl.system(c=3, d=3)
    def hold(c, d):
        return {"c": np_.array([c[0], c[1], c[2]]), "d": np_.array([d[0], d[1], d[2]])}
    x = _crafted(n, dtype)
    w = workloads.independent_bodies(n)
    hip = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], entity_ids=w["entity_ids"], dtype=dtype, integrator=L.SEMI_IMPLICIT,
                     effectors=dsl.Program([hold], dsl.Pipe([]), []), ticks_per_launch=2, columns={"c": x[:, :3].copy(), "d": x[:, 3:].copy()})
    hip.enable_history(4)
    hip.run(2)
    held = np.concatenate([hip.history("c", 2, 2)[0], hip.history("d", 2, 2)[0]], axis=1)
    assert held.dtype == dtype and held.tobytes() == x.tobytes()          # the ring holds exactly the uploaded bits: no case has vanished
    order = np.argsort(_keys(x[:, 4]), kind="stable")
    for k0 in range(0, n, 16):
        q = [(k, n - 1) for k in range(k0, min(n, k0 + 16))]
        got = hip.history_quantiles(["c", "d"], 2, 2, q)
        _check_all(hip, ["c", "d"], got, 2, 2, 1, q, what=f"{np.dtype(dtype).name} ranks {k0}..")
        # element 4 (d[1]) has no row skipped: rank k / (n - 1) is the k-th key exactly, signed zeros and denormals in key order
        want = x[order[k0:k0 + 16], 4].astype(np.float64)
        assert got["d"]["lower"][0, 0, :, 1].tobytes() == want.tobytes() and got["d"]["upper"][0, 0, :, 1].tobytes() == want.tobytes()
    assert np.array_equal(got["c"]["count"][0, 0], [n, n, n]) and np.array_equal(got["d"]["count"][0, 0], [n, n, n - 6])     # the skipped rows
    hip.close()


# ---- 3. a column without a finite row ----------------------------------------------------------------------------------
def test_a_column_that_is_nan_in_every_row_reads_count_zero():
    hip = _program_exec(a_nan=True)
    hip.enable_history(16)
    hip.run(12)
    got = hip.history_quantiles(["a", "b"], 1, 2, Q)
    assert np.all(got["a"]["count"] == 0) and got["a"]["count"].shape == (2, 1, 1)
    for k in ("lower", "upper", "linear"):
        assert got["a"][k].shape == (2, 1, 6, 1) and np.all(np.isnan(got["a"][k])), k
    # the NaN reaches c[2] in tick 1 and b[0] in tick 2: after tick 1 both elements of b are whole, after tick 2 only b[1]
    assert np.array_equal(got["b"]["count"][:, 0], [[200, 200], [0, 200]])
    assert np.all(np.isfinite(got["b"]["lower"][:, :, :, 1])) and np.all(np.isnan(got["b"]["upper"][1, :, :, 0]))
    _check_all(hip, ["a", "b"], got, 1, 2, 1, Q, what="NaN column")
    hip.close()


# ---- 4. groups -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,period,names", [(4100, 4, FIELDS), (300, 12, FIELDS), (320, 64, FIELDS), (300, 75, ("world_vel",))])
def test_groups_select_among_rows_of_equal_index_modulo_period(n, period, names):
    hip, _ = _exec(n, 4)
    hip.enable_history(8)
    hip.run(8)
    got = hip.history_quantiles(names, 2, 8, Q, 3, period=period)
    assert got["world_vel"]["lower"].shape == (3, period, 6, 6)
    for c in names:
        assert np.all(got[c]["count"] == n // period), c
    _check_all(hip, names, got, 2, 8, 3, Q, period, what=f"n {n} period {period}")
    assert not np.array_equal(got["world_vel"]["lower"][:, 0], got["world_vel"]["lower"][:, 1])       # the groups differ
    hip.close()


# ---- 5. refusals copy nothing -------------------------------------------------------------------------------------------
def test_refused_reads_copy_nothing():
    hip, _ = _exec(300, 8)
    sentinel = lambda: [np.full((4, 100, 35, 7), 123.0), np.full((4, 100, 35, 6), 123.0)]
    bufs = sentinel()
    num, den = [1, 50, 99], 100
    vel = lambda *a, **kw: _raw(hip, ["world_vel"], *a, bufs[1:], **kw)
    assert vel(1, 1, 1, 1, num, den) == L.ERR_INVALID_ARGUMENT                                  # no ring
    hip.run(5)
    hip.enable_history(10)                                                                       # recording starts at tick 6
    hip.run(25)                                                                                  # the ring keeps 21 .. 30
    assert _raw(hip, ["world_pos", "world_vel"], 27, 2, 1, 7, num, den, bufs) == L.ERR_INVALID_ARGUMENT      # 300 % 7 != 0
    assert _raw(hip, ["world_pos", "world_vel"], 27, 2, 1, 0, num, den, bufs) == L.ERR_INVALID_ARGUMENT      # period 0
    assert 100 * 6 > L.ENVELOPE_MAX_BINS                                                         # 600 (group, element) bins
    assert vel(27, 2, 1, 100, num, den) == L.ERR_INVALID_ARGUMENT
    assert str(L.ENVELOPE_MAX_BINS) in hip._lib.sixdof_last_error(hip._h).decode()
    assert vel(27, 2, 1, 1, [], den) == L.ERR_INVALID_ARGUMENT                                   # no ranks
    assert vel(27, 2, 1, 1, list(range(17)), den) == L.ERR_INVALID_ARGUMENT                      # 17 ranks
    assert vel(27, 2, 1, 1, num, 0) == L.ERR_INVALID_ARGUMENT                                    # denominator 0
    assert vel(27, 2, 1, 1, [1, 101], den) == L.ERR_INVALID_ARGUMENT                             # a numerator above the denominator
    assert vel(20, 4, 1, 1, num, den) == L.ERR_INVALID_ARGUMENT                                  # has fallen out of the ring
    assert vel(28, 4, 1, 1, num, den) == L.ERR_INVALID_ARGUMENT                                  # runs beyond `tick`
    assert vel(21, 4, 0, 1, num, den) == L.ERR_INVALID_ARGUMENT                                  # every = 0
    assert vel(21, 4, 1, 1, num, den, flags=2) == L.ERR_INVALID_ARGUMENT                         # unknown flags
    comp = np.array([L.component_id("world_vel")], dtype=np.uint64)
    nums = (C.c_uint32 * 3)(*num)
    null = (C.c_void_p * 1)(None)
    assert hip._lib.sixdof_history_quantiles(hip._h, comp.ctypes.data_as(U64P), 1, 21, 4, 1, 1, nums, den, 3, null, 0) == L.ERR_INVALID_ARGUMENT
    ptr = (C.c_void_p * 1)(bufs[1].ctypes.data)
    assert hip._lib.sixdof_history_quantiles(hip._h, comp.ctypes.data_as(U64P), 1, 21, 4, 1, 1, None, den, 3, ptr, 0) == L.ERR_INVALID_ARGUMENT
    for b, s in zip(bufs, sentinel()):
        assert np.array_equal(b, s)                                                              # nothing was copied
    for q in ([1.5], [k / 32 for k in range(17)], [(1, 2 ** 32)]):                               # the Python layer's own refusals
        with pytest.raises(ValueError):
            hip.history_quantiles(["world_vel"], 21, 30, q)
    for bad in ((20, 30, 1, 1), (21, 31, 1, 1), (21, 30, 0, 1), (21, 30, 1, 7), (21, 30, 1, 100)):
        with pytest.raises(ValueError):
            hip.history_quantiles(["world_vel"], bad[0], bad[1], [0.5], bad[2], period=bad[3])
    assert vel(99, 0, 7, 1, num, den) == L.OK and np.array_equal(bufs[1], sentinel()[1])          # no samples: a no-op
    got = hip.history_quantiles(["world_vel"], 21, 30, [0.01, 0.5, 0.99], 3)                       # 21 24 27 30
    _check_all(hip, ["world_vel"], got, 21, 30, 3, [0.01, 0.5, 0.99], what="after the refusals")
    hip.close()


# ---- 6. bit-identity ---------------------------------------------------------------------------------------------------
def test_a_tick_reads_the_same_bits_however_it_is_read():
    n = 4099
    hip, _ = _exec(n, 7)
    hip.enable_history(32)
    hip.run(30)
    q = [0.01, 0.25, 0.5, 0.75, 0.99]
    whole = hip.history_quantiles(FIELDS, 3, 30, q, 3)
    _check_all(hip, FIELDS, whole, 3, 30, 3, q, what="whole")
    for j, tick in enumerate(range(3, 31, 3)):
        _same(_sample(whole, j), hip.history_quantiles(FIELDS, tick, tick, q))                # the one-sample read of that tick
    other = hip.history_quantiles(["force", "world_pos"], 6, 30, q, 6)                        # another every, another component list
    for j, tick in enumerate(range(6, 31, 6)):
        for name in ("force", "world_pos"):
            _same({name: _sample(other, j)[name]}, {name: _sample(whole, (tick - 3) // 3)[name]})
    shared = hip.history_quantiles(FIELDS, 3, 30, [Fraction(2, 3), 0.5, 0.0], 3)              # another rank list that shares the median
    _same(_ranks(shared, [1]), _ranks(whole, [2]))
    num, den = hip.quantile_ranks(q)                                                          # synchronous against SIXDOF_QUANTILE_ASYNC
    bufs = [np.zeros((10, 1, 11, _width(c))) for c in FIELDS]
    assert _raw(hip, FIELDS, 3, 10, 3, 1, num, den, bufs, L.QUANTILE_ASYNC) == L.OK
    hip.download_wait()
    _same(whole, hip._quantile_dict(FIELDS, bufs, num, den))
    hip.sync()
    hip.close()


def test_more_components_than_one_launch_covers():
    """34 component ids — the four fields cycled — cross the 32 components of one launch: the second launch reuses the scratch
    offsets of the first.  Every buffer is, byte for byte, the same field's buffer of a four-id read of the same two samples."""
    hip, _ = _exec(65, 4)
    hip.enable_history(4)
    hip.run(4)
    num, den = hip.quantile_ranks([0.01, 0.5, 0.99])
    names = [FIELDS[k % 4] for k in range(34)]
    block = lambda c, fill: np.full((2, 5, 7, _width(c)), fill)
    many, four = [block(c, -7.0) for c in names], [block(c, -9.0) for c in FIELDS]
    assert _raw(hip, names, 3, 2, 1, 5, num, den, many) == L.OK and _raw(hip, FIELDS, 3, 2, 1, 5, num, den, four) == L.OK
    assert all(np.all(b[:, :, 0] == 13) for b in four)                 # filled: 65 rows in 5 groups
    for k, b in enumerate(many):
        assert b.tobytes() == four[k % 4].tobytes(), (k, names[k])
    hip.close()


# ---- 7. linear ---------------------------------------------------------------------------------------------------------
def test_linear_is_the_documented_formula_of_lower_upper_and_count():
    n = 300
    hip, _ = _exec(n, 4)
    hip.enable_history(4)
    hip.run(4)
    q = [Fraction(1, 2), 0.01, Fraction(2, 7), 0.99, 1.0]
    num, den = hip.quantile_ranks(q)
    for period, m_want in ((1, 300), (4, 75)):
        got = hip.history_quantiles(["world_vel", "world_pos"], 3, 4, q, period=period)
        for name, d in got.items():
            assert np.all(d["count"] == m_want)
            m = d["count"][:, :, None, :].astype(np.int64)
            k = np.array(num, dtype=np.int64)[None, None, :, None]
            frac = ((k * (m - 1)) % den).astype(np.float64) / float(den)
            assert np.array_equal(d["linear"], d["lower"] + (d["upper"] - d["lower"]) * frac), name
            assert np.all(d["linear"] >= d["lower"]) and np.all(d["linear"] <= d["upper"]), name
            median = (d["lower"][:, :, 0], d["upper"][:, :, 0])
            if m_want % 2:
                assert np.array_equal(*median), name                      # the median of an odd count is an element
            else:
                assert np.all(median[0] <= median[1]) and np.any(median[0] < median[1]), name
        # numpy's default interpolation evaluates the same formula up to rounding
        x = hip.history("world_vel", 4, 4)[0].astype(np.float64).reshape(n // period, period, 6)
        want = np.quantile(x, [a / den for a in num], axis=0)                 # [Q, period, 6]
        assert np.allclose(got["world_vel"]["linear"][1], want.transpose(1, 0, 2), rtol=1e-12, atol=1e-300)
    hip.close()


# ---- 8. streaming ---------------------------------------------------------------------------------------------------------
def test_streamed_quantiles_equal_a_twin_read_tick_by_tick():
    """stream_quantiles: every second tick of four 8-tick batches out of a ring one batch deep; each sample is bit-equal to the
    quantiles a twin stepped one tick at a time reads at that tick."""
    n = 1000
    q = [0.01, 0.5, 0.99]
    a, _ = _exec(n, 8)
    b, _ = _exec(n, 1)
    got, order = {}, []

    def consume(i, first_tick, d):
        order.append((i, first_tick))
        assert sorted(d) == sorted(FIELDS) and d["world_pos"]["lower"].shape == (4, 1, 3, 7) and d["force"]["count"].dtype == np.int64
        for j in range(4):
            got[first_tick + 2 * j] = {c: {k: v[j:j + 1].copy() for k, v in e.items()} for c, e in d.items()}
    with pytest.raises(ValueError):
        a.stream_quantiles(FIELDS, 4, 8, q, every=3)
    wall = a.stream_quantiles(FIELDS, 4, 8, q, every=2, consume=consume)
    assert wall > 0.0 and a.tick == 32
    assert order == [(i, 8 * i + 2) for i in range(4)] and sorted(got) == list(range(2, 33, 2))
    b.enable_history(4)
    for t in range(1, 33):
        b.run(1)
        if t in got:
            _same(got[t], b.history_quantiles(FIELDS, t, t, q))
    for h in (a, b):
        h.close()


def test_async_quantiles_alongside_a_history_stream_copy_and_an_envelope():
    """A sixdof_history_stream copy, an asynchronous envelope read and an asynchronous quantile read pending on one lane: one
    download_wait covers the three."""
    n = 500
    hip, _ = _exec(n, 4)
    hip.enable_history(16)
    hip.run(16)
    q = [0.25, 0.5]
    num, den = hip.quantile_ranks(q)
    want_blocks = {c: hip.history(c, 5, 12) for c in FIELDS}
    want_env = hip.history_envelope(FIELDS, 10, 16, 2, period=5)
    want = hip.history_quantiles(FIELDS, 10, 16, q, 2, period=5)
    blocks = {c: np.zeros((8, n, _width(c))) for c in FIELDS}
    env = [np.zeros((4, 5, 5, _width(c))) for c in FIELDS]
    bufs = [np.zeros((4, 5, 5, _width(c))) for c in FIELDS]
    assert hip._lib.sixdof_history_stream(hip._h, 5, 8, (C.c_void_p * 4)(*[blocks[c].ctypes.data for c in FIELDS])) == L.OK
    comp = np.array([L.component_id(c) for c in FIELDS], dtype=np.uint64)
    assert hip._lib.sixdof_history_envelope(hip._h, comp.ctypes.data_as(U64P), 4, 10, 4, 2, 5, (C.c_void_p * 4)(*[e.ctypes.data for e in env]),
                                            L.ENVELOPE_ASYNC) == L.OK
    assert _raw(hip, FIELDS, 10, 4, 2, 5, num, den, bufs, L.QUANTILE_ASYNC) == L.OK
    hip.download_wait()
    for c in FIELDS:
        assert np.array_equal(blocks[c], want_blocks[c]), c
    got_env = hip._envelope_dict(FIELDS, env)
    for c in FIELDS:
        for k in ("count", "min", "max", "mean", "m2"):
            assert np.array_equal(got_env[c][k], want_env[c][k], equal_nan=True), (c, k)
    _same(hip._quantile_dict(FIELDS, bufs, num, den), want)
    _check_all(hip, FIELDS, want, 10, 16, 2, q, 5, what="beside a stream copy")
    hip.run(4)                                               # the stepper goes on; the page locks end at sync
    hip.sync()
    assert hip.tick == 20
    hip.close()


# ---- 9. pair path, front end ------------------------------------------------------------------------------------------------
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
    _check_all(hip, FIELDS, hip.history_quantiles(FIELDS, 6, 13, Q), 6, 13, 1, Q, what="three bodies")
    _check_all(hip, FIELDS, hip.history_quantiles(FIELDS, 7, 13, Q, 3), 7, 13, 3, Q, what="three bodies, every 3")
    per_body = hip.history_quantiles(FIELDS, 7, 13, Q, 3, period=3)
    _check_all(hip, FIELDS, per_body, 7, 13, 3, Q, 3, what="three bodies, one per group")
    assert np.all(per_body["world_pos"]["count"] == 1)
    assert np.array_equal(per_body["world_pos"]["lower"][-1, :, 2], hip.world_pos) and np.array_equal(per_body["world_pos"]["upper"][-1, :, 3], hip.world_pos)
    hip.close()


def test_front_end_quantiles_of_one_entity_are_its_series():
    spec = importlib.util.spec_from_file_location("ball", ROOT / "examples" / "ball.py")
    ball = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ball)
    ex = ball.world(0).build(ball.system(), simulation_rate=120.0, telemetry_rate=40.0, history=True)      # three sim steps per world tick
    ex.enable_history(64)
    ex.run(30)
    comps = ["world_pos", "world_vel", "wind", "force"]
    series = ex.history_series(["ball." + c for c in comps], 3, 30, every=3)
    got = ex.history_quantiles(comps, 3, 30, [0.0, 0.5, 1.0], every=3)
    assert sorted(got) == sorted(comps + ["time"]) and np.array_equal(got["time"], series["time"])
    for c in comps:
        want = series["ball." + c]
        d = got[c]
        assert d["lower"].shape == (10, 1, 3, want.shape[1]) and np.all(d["count"] == 1), c
        for k in ("lower", "upper", "linear"):
            for i in range(3):
                assert np.array_equal(d[k][:, 0, i], want), (c, k, i)
    assert not np.array_equal(got["world_pos"]["lower"][0], got["world_pos"]["lower"][-1])
    with pytest.raises(KeyError):
        ex.history_quantiles("nothing", 3, 30, [0.5])
    with pytest.raises(ValueError):
        ex.history_quantiles("world_pos", 0, 30, [0.5])              # tick 0 is not in the ring
    with pytest.raises(ValueError):
        ex.history_quantiles("world_pos", 3, 30, [0.5], every=0)


def test_campaign_quantiles_equal_numpy_over_the_runs_columns(monkeypatch):
    """A 17-run campaign of the Monte-Carlo example: Campaign.quantiles per tick against numpy over Campaign.column after each tick."""
    from tests.test_gpu_monte_carlo_example import GOLDEN, example
    from elodin_amd import vectorize
    ex = example(0)
    doc = json.loads((GOLDEN / "monte_carlo_example.json").read_text())
    params = [r["params"] for r in doc["runs"] if r["probe_rows"] == 0]
    c = vectorize.Campaign(ex.build, vectorize.plan_of((params * 17)[:17]), ex.PARAMS, simulation_rate=ex.SIMULATION_RATE_HZ)
    assert c.n_runs == 17 and c.entities_per_run == 1
    comps = ["position", "velocity", "specific_force"]
    q = (0.01, 0.5, 0.99)
    c.exec.enable_history(16)
    cols = {name: [] for name in comps}
    for _ in range(12):
        c.exec.run(1)
        for name in comps:
            cols[name].append(np.array(c.column(name), dtype=np.float64).reshape(17, -1))
    got = c.quantiles(comps, 2, 12, q, every=5)                 # ticks 2, 7, 12
    assert np.allclose(got["time"], np.array([2, 7, 12]) / ex.SIMULATION_RATE_HZ)
    for name in comps:
        ref = _reference(np.stack([cols[name][t - 1] for t in (2, 7, 12)]), q, period=1)
        assert got[name]["lower"].shape == (3, 1, 3, 1)
        _check(got[name], ref, f"campaign {name}")
    assert np.all(got["position"]["count"] == 17) and np.all(got["velocity"]["upper"][-1, 0, 2] > got["velocity"]["lower"][-1, 0, 0])
