"""Watch lists (sixdof_set_watch / sixdof_watch_read): time series of chosen (entity, component) pairs gathered out of the
telemetry ring on the device.  Every comparison is bit for bit against the [ticks, n, w] blocks HipExec.history reads from
the same ring, sliced on the host — the gather is a copy."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import elodin_amd as ea
from elodin_amd import _lib as L
from elodin_amd import dsl, workloads
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

FIELDS = ("world_pos", "world_vel", "world_accel", "force")
# any order, a duplicate, both sides of a wavefront boundary (a 64-row executor has no row 64: there the list ends at 63)
WATCH_ROWS = lambda n: [r for r in (n - 1, 0, 7, 7, 63, 64) if r < n]


def _exec(n, ticks_per_launch=1, dtype=np.float64, seed=workloads.SEED):
    """The executor of tests/test_gpu_parity.py::_pair, without its oracle twin."""
    w = workloads.independent_bodies(n, seed=seed)
    eff = workloads.gravity_torque_effectors(w["body_torque"])
    hip = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], entity_ids=w["entity_ids"], simulation_time_step=workloads.DT_120HZ,
                     effectors=eff, ticks_per_launch=ticks_per_launch, dtype=dtype)
    return hip, w


def _expected(hip, names, rows, first, last, every):
    """[m, samples, w] per name out of the whole blocks HipExec.history reads."""
    return {name: np.ascontiguousarray(hip.history(name, first, last)[::every][:, rows].transpose(1, 0, 2)) for name in names}


def _assert_series(got, want):
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, name
        assert np.array_equal(got[name], want[name]), name


@pytest.mark.parametrize("n,k,ring,run,first,every,dtype", [
    (300, 8, 10, 27, 18, 1, np.float64),       # ticks 18 .. 27 sit in slots 7 8 9 0 .. 6: the range wraps
    (300, 8, 10, 27, 18, 3, np.float64),
    (4099, 7, 64, 50, 1, 7, np.float64),       # the stride does not divide the ring, n is no multiple of 64
    (64, 1, 8, 8, 1, 1, np.float32),
])
def test_series_equal_slices_of_the_history_blocks(n, k, ring, run, first, every, dtype):
    hip, w = _exec(n, k, dtype)
    hip.enable_history(ring)
    hip.run(run)
    rows = WATCH_ROWS(n)
    hip.set_watch(FIELDS, w["entity_ids"][rows])
    last = first + (run - first) // every * every
    got = hip.history_series(first, run, every)             # the four columns in one call
    assert got["world_pos"].shape == (len(rows), (last - first) // every + 1, 7)
    _assert_series(got, _expected(hip, FIELDS, rows, first, last, every))
    assert not np.array_equal(got["world_pos"][0, 0], got["world_pos"][0, -1])         # the ticks differ: not one block repeated
    # one entity, one sample
    hip.set_watch(["world_vel"], w["entity_ids"][[n // 2]])
    one = hip.history_series(run, run)
    assert one["world_vel"].shape == (1, 1, 6)
    _assert_series(one, _expected(hip, ["world_vel"], [n // 2], run, run, 1))
    hip.close()


def test_watch_by_entity_id_on_a_joined_executor():
    """Every Body column on its own entity set, ids not sequential: a watched id reads the joined row history() shows for it; an
    id outside the join is refused and the previous watch keeps working."""
    rng = np.random.default_rng(5)
    universe = (np.arange(48, dtype=np.uint64) * 3 + 11)
    widths = {"world_pos": 7, "world_vel": 6, "inertia": 7, "world_accel": 6, "force": 6}
    drop = {"world_pos": [], "world_vel": [3, 20], "inertia": [10], "world_accel": [], "force": [41]}
    ids, data = {}, {}
    for name, wd in widths.items():
        keep = np.delete(universe, drop[name])
        if name == "world_vel":
            keep = np.concatenate([keep[5:], keep[:5]])              # rows out of id order
        a = rng.normal(size=(len(keep), wd))
        if name == "world_pos":
            a[:, :4] /= np.linalg.norm(a[:, :4], axis=1, keepdims=True)
        if name == "inertia":
            a = np.concatenate([rng.uniform(0.5, 3.0, (len(keep), 3)), np.zeros((len(keep), 3)), rng.uniform(1.0, 9.0, (len(keep), 1))], axis=1)
        if name in ("world_accel", "force"):
            a[...] = 0.0
        ids[name], data[name] = keep, a
    hip = ea.HipExec(data["world_pos"], data["world_vel"], data["inertia"], world_accel=data["world_accel"], force=data["force"],
                     entity_ids=ids["world_pos"], effectors=[ea.Effector(L.EFF_UNIFORM_GRAVITY, (0.0, 0.3, -9.81))], ticks_per_launch=4,
                     column_entity_ids=ids)
    joined = np.setdiff1d(universe, universe[[3, 20, 10, 41]])           # ascending id = joined row order
    assert hip.n == len(joined) == 44
    hip.enable_history(16)
    hip.run(12)
    watched = joined[[43, 0, 17, 17, 5]]
    hip.set_watch(["world_pos", "force"], watched)
    rows = [int(np.nonzero(joined == e)[0][0]) for e in watched]
    want = _expected(hip, ["world_pos", "force"], rows, 2, 12, 2)
    _assert_series(hip.history_series(2, 12, 2), want)
    for outside in (universe[3], np.uint64(7)):                             # on some columns only / on none
        with pytest.raises(ValueError, match="joined"):
            hip.set_watch(["world_vel"], np.array([joined[0], outside], dtype=np.uint64))
    with pytest.raises(KeyError):
        hip.set_watch(["inertia"], joined[:1])
    _assert_series(hip.history_series(2, 12, 2), want)                      # the previous watch is intact
    hip.close()


@pytest.mark.parametrize("column_soa", ["0", "1"])
def test_program_columns_are_watched_with_the_body_columns(column_soa, monkeypatch):
    """Component columns of widths 1, 2 and 3 of a generated f32 program, 12 ticks per launch, together with world_pos in one
    read; a window component and inertia are refused.  With the program's live columns element-major on the device (what
    executors of 32,768 rows and more get) its rings are in the row layout all the same: the last sample equals the columns."""
    monkeypatch.setenv("SIXDOF_COLUMN_SOA", column_soa)
    np_ = dsl.np

    @dsl.system(a=1, b=2, c=3, buf=dsl.window(4, 2))
    def plant(a, b, c, buf):                                 # a width-1 column arrives as a scalar
        s = a * 0.5 + b[1]
        return {"a": s * 0.25 + 1.0,
                "b": np_.array([b[1] * 0.99 + c[2] * 1e-3, b[0] + 0.125]),
                "c": np_.array([c[1], c[2] * 0.999, c[0] + a * 1e-3]),
                "buf": buf.push(b)}
    n = 200
    rng = np.random.default_rng(3)
    w = workloads.independent_bodies(n)
    hip = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], entity_ids=w["entity_ids"], dtype=np.float32, integrator=L.SEMI_IMPLICIT,
                     effectors=dsl.Program([plant], dsl.Pipe([]), []), ticks_per_launch=12,
                     columns={"a": rng.uniform(-1, 1, (n, 1)), "b": rng.uniform(-1, 1, (n, 2)), "c": rng.uniform(-1, 1, (n, 3)),
                              "buf": np.zeros((n, 4, 2))})
    names = ["a", "world_pos", "b", "c"]
    rows = [n - 1, 0, 7, 7, 63, 64]
    hip.set_watch(names, w["entity_ids"][rows])             # before the ring exists
    hip.enable_history(32)
    hip.run(30)
    got = hip.history_series(3, 30, 3)
    assert [got[k].shape for k in names] == [(6, 10, 1), (6, 10, 7), (6, 10, 2), (6, 10, 3)] and got["a"].dtype == np.float32
    want = _expected(hip, names, rows, 3, 30, 3)
    _assert_series(got, want)
    assert not np.array_equal(got["c"][:, 0], got["c"][:, -1])
    assert hip._column_soa == (column_soa == "1")
    for name in ("a", "b", "c"):                             # tick 30 is the state the run left in the columns
        assert np.array_equal(got[name][:, -1], hip._aux[name][rows]), name
    assert np.array_equal(got["world_pos"][:, -1], hip.world_pos[rows])
    with pytest.raises(ValueError, match="window component"):
        hip.set_watch(["buf"], w["entity_ids"][:1])
    with pytest.raises(KeyError):
        hip.set_watch(["world_pos", "inertia"], w["entity_ids"][:1])
    u64p = C.POINTER(C.c_uint64)                             # the library refuses the window too, not only the Python surface
    comp, one = np.array([L.component_id("buf")], dtype=np.uint64), np.ascontiguousarray(w["entity_ids"][:1], dtype=np.uint64)
    assert hip._lib.sixdof_set_watch(hip._h, comp.ctypes.data_as(u64p), 1, one.ctypes.data_as(u64p), 1) == L.ERR_COMPONENT_NOT_FOUND
    _assert_series(hip.history_series(3, 30, 3), want)
    hip.close()


def test_pair_path_ring_filled_by_per_tick_copies():
    """The three-body world through edges: its ring is filled by device copies after every one-tick launch."""
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
    hip.set_watch(FIELDS, [3, 1, 1, 2])
    _assert_series(hip.history_series(6, 13), _expected(hip, FIELDS, [2, 0, 0, 1], 6, 13, 1))
    _assert_series(hip.history_series(7, 13, 3), _expected(hip, FIELDS, [2, 0, 0, 1], 7, 13, 3))
    hip.close()


def test_refused_reads_copy_nothing():
    hip, w = _exec(300, 8)
    sentinel = lambda: np.full((2, 4, 6), 123.0)
    u64p = C.POINTER(C.c_uint64)

    def raw_read(first, n_samples, every, buf):
        ptrs = (C.c_void_p * 1)(buf.ctypes.data)
        return hip._lib.sixdof_watch_read(hip._h, first, n_samples, every, ptrs, 0)

    buf = sentinel()
    comp = np.array([L.component_id("world_vel")], dtype=np.uint64)
    ids = np.ascontiguousarray(w["entity_ids"][[5, 299]], dtype=np.uint64)
    assert raw_read(1, 1, 1, buf) == L.ERR_INVALID_ARGUMENT                     # neither a watch nor a ring
    hip.run(5)
    hip.enable_history(10)                                                       # recording starts at tick 6
    hip.run(25)                                                                  # the ring keeps 21 .. 30
    assert raw_read(21, 4, 1, buf) == L.ERR_INVALID_ARGUMENT                    # a ring, no watch
    with pytest.raises(ValueError, match="no watch"):
        hip.history_series(21, 30)
    assert hip._lib.sixdof_set_watch(hip._h, comp.ctypes.data_as(u64p), 1, ids.ctypes.data_as(u64p), 2) == L.OK
    hip._watch = (["world_vel"], 2)
    assert raw_read(21, 4, 0, buf) == L.ERR_INVALID_ARGUMENT                    # every = 0
    assert raw_read(20, 4, 1, buf) == L.ERR_INVALID_ARGUMENT                    # has fallen out of the ring
    assert raw_read(28, 4, 1, buf) == L.ERR_INVALID_ARGUMENT                    # runs beyond `tick`
    assert raw_read(24, 4, 3, buf) == L.ERR_INVALID_ARGUMENT                    # its last sample does
    assert raw_read(31, 1, 1, buf) == L.ERR_INVALID_ARGUMENT
    assert np.array_equal(buf, sentinel())                                      # nothing was copied
    for bad in ((20, 30, 1), (21, 31, 1), (21, 30, 0), (5, 5, 1)):
        with pytest.raises(ValueError):
            hip.history_series(*bad)
    assert raw_read(21, 0, 1, buf) == L.OK and raw_read(99, 0, 7, buf) == L.OK  # no samples: a no-op
    assert np.array_equal(buf, sentinel())
    assert hip.history_series(30, 29)["world_vel"].shape == (2, 0, 6)
    assert raw_read(21, 4, 3, buf) == L.OK                                      # 21 24 27 30
    assert np.array_equal(buf, _expected(hip, ["world_vel"], [5, 299], 21, 30, 3)["world_vel"])
    # a ring that starts over: ticks before its first recorded one are gone
    hip.enable_history(10)
    hip.run(3)                                                                   # 31 .. 33
    buf = sentinel()
    assert raw_read(30, 4, 1, buf) == L.ERR_INVALID_ARGUMENT                    # starts before hist_first_tick
    assert np.array_equal(buf, sentinel())
    assert hip.history_series(31, 33)["world_vel"].shape == (2, 3, 6)
    hip.enable_history(0)
    with pytest.raises(ValueError, match="no history ring"):
        hip.history_series(31, 33)
    hip.set_watch([], [])                                                        # 0 / 0 clears
    hip.enable_history(4)
    hip.run(2)
    with pytest.raises(ValueError, match="no watch"):
        hip.history_series(34, 35)
    hip.close()


def test_watch_and_ring_in_either_order_and_after_a_resize():
    hip, w = _exec(1000, 16)
    rows = WATCH_ROWS(1000)
    hip.set_watch(FIELDS, w["entity_ids"][rows])             # the watch first
    hip.enable_history(20)
    hip.run(20)
    _assert_series(hip.history_series(1, 20, 4), _expected(hip, FIELDS, rows, 1, 17, 4))
    hip.enable_history(7)                                    # another size: other ring buffers, other slots
    hip.run(30)
    _assert_series(hip.history_series(44, 50), _expected(hip, FIELDS, rows, 44, 50, 1))
    hip.enable_history(0)
    hip.enable_history(64)
    hip.run(5)
    _assert_series(hip.history_series(51, 55, 2), _expected(hip, FIELDS, rows, 51, 55, 2))
    hip._bind([(c, getattr(hip, c)) for c in FIELDS + ("inertia",)])      # a new join: the rows of the old one mean nothing
    with pytest.raises(ValueError, match="no watch"):
        hip.history_series(51, 55, 2)
    hip.close()


def test_streamed_series_equal_single_tick_runs():
    """stream_series: every fourth tick of six 16-tick batches, the samples of batch i copied while batch i+1 computes out of a ring
    one batch deep; each equals a twin stepped one tick at a time, and streaming leaves the state a plain run leaves."""
    n = 1000
    a, w = _exec(n, 8)
    b, _ = _exec(n, 1)
    plain, _ = _exec(n, 8)
    rows = WATCH_ROWS(n)
    a.set_watch(FIELDS, w["entity_ids"][rows])
    got, order = {}, []

    def consume(i, first_tick, cols):
        order.append((i, first_tick))
        assert sorted(cols) == sorted(FIELDS) and cols["world_pos"].shape == (len(rows), 4, 7)
        for j in range(4):
            got[first_tick + 4 * j] = {c: v[:, j].copy() for c, v in cols.items()}
    with pytest.raises(ValueError):
        a.stream_series(6, 16, every=5)
    wall = a.stream_series(6, 16, every=4, consume=consume)
    assert wall > 0.0 and a.tick == 96
    assert order == [(i, 16 * i + 4) for i in range(6)] and sorted(got) == list(range(4, 97, 4))
    for t in range(1, 97):
        b.run(1)
        if t in got:
            for c in FIELDS:
                assert np.array_equal(got[t][c], getattr(b, c)[rows]), (t, c)
    a.download()
    plain.run(96)
    for c in FIELDS:
        assert np.array_equal(getattr(a, c), getattr(plain, c)), c
    for h in (a, b, plain):
        h.close()


def test_async_watch_read_alongside_a_history_stream_copy():
    """A sixdof_history_stream copy and, before it is waited for, an asynchronous watch read: one download_wait covers both."""
    n = 500
    hip, w = _exec(n, 4)
    hip.enable_history(16)
    hip.run(16)
    rows = WATCH_ROWS(n)
    hip.set_watch(FIELDS, w["entity_ids"][rows])
    want_blocks = {c: hip.history(c, 5, 12) for c in FIELDS}
    want_series = _expected(hip, FIELDS, rows, 10, 16, 2)
    blocks = {c: np.zeros((8, n, 7 if c == "world_pos" else 6)) for c in FIELDS}
    series, ptrs = hip._series_buffers(4)
    for v in series.values():
        v[...] = 0.0
    rc = hip._lib.sixdof_history_stream(hip._h, 5, 8, (C.c_void_p * 4)(*[blocks[c].ctypes.data for c in FIELDS]))
    assert rc == L.OK
    rc = hip._lib.sixdof_watch_read(hip._h, 10, 4, 2, ptrs, L.WATCH_ASYNC)
    assert rc == L.OK
    hip.download_wait()
    for c in FIELDS:
        assert np.array_equal(blocks[c], want_blocks[c]), c
    _assert_series(series, want_series)
    hip.run(4)                                               # the stepper goes on; the page locks end at sync
    hip.sync()
    assert hip.tick == 20
    hip.close()


def test_a_longer_asynchronous_read_into_the_same_buffers_with_no_sync_between():
    """Ticks 9 .. 10 streamed into the buffers, then — nothing waited for — ticks 5 .. 12 into the same buffers, then sync: the
    second read's blocks, complete.  The page lock the first read took covers a quarter of what the second copies."""
    n = 300
    hip, _ = _exec(n, 4)
    hip.enable_history(16)
    hip.run(16)
    want = {c: hip.history(c, 5, 12) for c in FIELDS}
    blocks = {c: np.zeros((8, n, 7 if c == "world_pos" else 6)) for c in FIELDS}
    ptrs = (C.c_void_p * 4)(*[blocks[c].ctypes.data for c in FIELDS])
    assert hip._lib.sixdof_history_stream(hip._h, 9, 2, ptrs) == L.OK
    assert hip._lib.sixdof_history_stream(hip._h, 5, 8, ptrs) == L.OK
    hip.sync()
    for c in FIELDS:
        assert np.array_equal(blocks[c], want[c]), c
    hip.close()


def test_front_end_series_equal_the_history_rows():
    """The ball world with history=True, three ticks per telemetry commit: Exec.history_series at the commit ticks equals the rows
    of exec.history() from the second on — the first is the spawned state, tick 0, which is never in the ring."""
    spec = importlib.util.spec_from_file_location("ball", Path(__file__).resolve().parents[1] / "examples" / "ball.py")
    ball = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ball)
    ex = ball.world(0).build(ball.system(), simulation_rate=120.0, telemetry_rate=40.0, history=True)
    ex.enable_history(64)
    ex.run(30)
    keys = ["ball.world_pos", "ball.world_vel", "ball.wind", "ball.force"]
    whole = ex.history(keys)
    series = ex.history_series(keys, 3, 30, every=3)
    assert len(whole["time"]) == 11 and whole["time"][0] == 0.0
    assert sorted(series) == sorted(whole)
    for k in ["time"] + keys:
        assert series[k].shape == whole[k][1:].shape and np.array_equal(series[k], whole[k][1:]), k
    assert not np.array_equal(series["ball.world_pos"][0], series["ball.world_pos"][-1])
    one = ex.history_series("ball.world_pos", 29, 30)
    assert np.array_equal(one["ball.world_pos"][1], whole["ball.world_pos"][-1]) and len(one["time"]) == 2
    with pytest.raises(KeyError):
        ex.history_series("nobody.world_pos", 3, 30)
    with pytest.raises(ValueError):
        ex.history_series("ball.world_pos", 0, 30)           # tick 0 is not in the ring
