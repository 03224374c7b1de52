"""Fold stages that read their edges from device memory (HipExec(graph_tables="device"), sixdof_set_fold_edges) on the GPU: the same
bits as the baked flavour on the same graph, graphs beyond the 65,536-edge cap, sources binned by out-degree (one wave per long
source of a plain sum, one lane per other source), edges replaced between batches, one cached object for every graph.

Tolerances: BIT-IDENTICAL wherever a source is folded sequentially (the reference's association), the 1e-9 contract of
tests/parity.py where a wave folds a source (another association of the same sum)."""
import ctypes as C

import numpy as np
import pytest

import elodin_amd as ea
from elodin_amd import _lib as L, codegen, dsl
from elodin_amd import stablehlo as sh
from elodin_amd import workloads
from oracle import oracle as orc
from tests import fold_tables_common as ft
from tests.golden import hlo_world_builder as hb
from tests.test_program_folds_host import EDGES, add_one, double, fold_test

pytestmark = pytest.mark.gpu


def _exec(prog, comps, edges, n, **kw):
    """A systems-only executor of n rows; edges: {component: (src rows, dst rows)}."""
    ids = np.arange(1, n + 1, dtype=np.uint64)
    ge = {k: (v if isinstance(v[0], str) else (ids[np.asarray(v[0], dtype=np.int64)], ids[np.asarray(v[1], dtype=np.int64)])) for k, v in edges.items()}
    return ea.HipExec(np.tile([0, 0, 0, 1.0, 0, 0, 0], (n, 1)), np.zeros((n, 6)), np.ones((n, 7)), entity_ids=ids, integrator=L.INTEGRATOR_NONE,
                      effectors=prog, columns={k: v.copy() for k, v in comps.items()}, graph_edges=ge, **kw)


def _xyz(n, seed, extra=()):
    x0 = np.random.default_rng(seed).uniform(-1.0, 1.0, n)
    return x0, {"x": x0[:, None].copy(), **{c: np.zeros((n, 1)) for c in ("y", "z") + tuple(extra)}}


def _both_flavours(make_prog, comps, edges, n, ticks, names, **kw):
    out = {}
    for flavour in ("baked", "device"):
        hip = _exec(make_prog(), comps, edges, n, graph_tables=flavour, **kw)
        assert (flavour == "device") == any(c is not None for c in hip._device_folds)
        hip.run(ticks)
        out[flavour] = {c: hip.component(c).copy() for c in names}
        hip.close()
    for c in names:
        assert np.array_equal(out["baked"][c], out["device"][c]), c
    return out["device"]


def test_the_same_graph_gives_the_same_bits_baked_and_from_device_memory():
    # the three-row program of the host test
    got = _both_flavours(lambda: dsl.Program([double, fold_test, add_one], dsl.pipe(), []), {"x": np.array([[1.0], [2.0], [2.0]]), "n": np.zeros((3, 1))},
                         EDGES, 3, 50, ("x", "n"))
    assert np.all(got["n"] == 50) and got["x"][0, 0] > 2.0 ** 50
    # a plain sum that asked for waves, every source listing 64 targets: a wave per source in both flavours (the same partition and tree)
    n = 128
    src, dst = ft.regular_graph(n, 64, stride=1)
    _, comps = _xyz(n, 11)
    got = _both_flavours(lambda: ft.sum_program(True), comps, {"e": (src, dst)}, n, 50, ("x", "y", "z"))
    assert np.abs(got["z"]).max() > 0.1


def test_a_replicated_world_folds_over_one_table_in_device_memory():
    """7 rows x 300 replicas (tests/test_gpu_program_folds.py's satellites and sensors, three folds around six_dof): one template
    table, row = base + src_rows[i], baked and from device memory bit for bit."""
    import tests.test_gpu_program_folds as g
    n_sats = 300
    w, comps, edges, ids = g._world(n_sats)
    first = {name: (f_[:6], t_[:6]) for name, (f_, t_) in edges.items()}
    out = {}
    for flavour in ("baked", "device"):
        prog = dsl.Program([g.sun_direction, g.sensor_reading, g.sun_estimate, g.point_at_sun], g.apply_torque | dsl.pipe(),
                           [g.log_alignment, g.echo_to_sensors, g.count_seen])
        hip = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], entity_ids=ids, simulation_time_step=workloads.DT_120HZ, integrator=L.RK4,
                         effectors=prog, columns=comps, graph_edges=first, graph_replicas=(n_sats, 7), ticks_per_launch=5, graph_tables=flavour)
        hip.run(50)
        out[flavour] = {"world_pos": hip.world_pos.copy(), "world_vel": hip.world_vel.copy(),
                        **{c: hip.component(c).copy() for c in ("reading", "estimate", "torque_cmd", "log", "echo", "seen")}}
        hip.close()
    for c in out["baked"]:
        assert np.array_equal(out["baked"][c], out["device"][c]), c
    assert np.all(np.abs(out["device"]["estimate"][np.arange(0, 7 * n_sats, 7)]).sum(axis=1) > 0.1)


def test_forcing_device_tables_on_complete_graphs_builds_and_runs():
    nb = 128
    text, slots = hb.nbody_world(nb, 2.9591220828e-4, 1e-6)
    rng = np.random.default_rng(nb)
    pos = np.concatenate([np.tile([0, 0, 0, 1.0], (nb, 1)), rng.normal(size=(nb, 3)) * 3], axis=1)
    vel = np.concatenate([np.zeros((nb, 3)), rng.normal(size=(nb, 3)) * 1e-3], axis=1)
    m = rng.uniform(1e-6, 1e-3, nb)
    inertia = np.concatenate([np.tile(m[:, None], (1, 3)), np.zeros((nb, 3)), m[:, None]], axis=1)
    ids = np.arange(1, nb + 1, dtype=np.uint64)
    out = {}
    for flavour in ("auto", "device"):
        prog, manifest, edges = sh.world_program(text, slots)
        cols = {c["column"]: np.zeros((nb, c["width"])) for c in manifest["columns"]}
        cols["hlo_simulation_time_step"][:] = 0.5
        cols["hlo_world_pos"], cols["hlo_world_vel"], cols["hlo_inertia"] = pos.copy(), vel.copy(), inertia.copy()
        hip = ea.HipExec(np.tile([0, 0, 0, 1.0, 0, 0, 0], (nb, 1)), np.zeros((nb, 6)), np.ones((nb, 7)), entity_ids=ids, integrator=L.INTEGRATOR_NONE,
                         effectors=prog, columns=cols, graph_edges=sh.edges_as_entity_ids(edges, ids), graph_tables=flavour)
        assert hip._device_folds == [None] * 4                                         # a complete graph never has a table
        hip.run(5)
        out[flavour] = {c: hip._aux[c].copy() for c in ("hlo_world_pos", "hlo_world_vel", "hlo_world_accel", "hlo_force", "hlo_tick")}
        hip.close()
    for c in out["auto"]:
        assert np.array_equal(out["auto"][c], out["device"][c]), c


def test_an_order_sensitive_fold_beyond_the_cap_equals_its_numpy_twin():
    """8,192 rows x 16 targets = 131,072 edges, acc * 0.5 + a * b between two systems: refused before this flavour existed.  The twin
    (tests/fold_tables_common.damped_twin, pinned on the walker in tests/test_fold_tables_host.py) does per source the same operations in
    the same order."""
    n, k = 8192, 16
    src, dst = ft.regular_graph(n, k)
    x0, comps = _xyz(n, 8)
    with pytest.raises(ValueError, match="bake their edges"):
        _exec(ft.damped_program(), comps, {"e": (src, dst)}, n, graph_tables="baked")
    hip = _exec(ft.damped_program(), comps, {"e": (src, dst)}, n)                     # "auto": device beyond the cap
    assert hip._device_folds == ["e"]
    hip.run(20)
    x, y, z = ft.damped_twin(x0, src, dst, k, 20)
    for name, ref in (("x", x), ("y", y), ("z", z)):
        assert np.array_equal(hip.component(name)[:, 0], ref), name
    assert np.abs(z).max() > 0.1
    hip.close()


@pytest.mark.parametrize("wave_fold", [True, False])
def test_a_hub_is_folded_by_a_wave_and_its_spokes_by_lanes(wave_fold):
    """Row 0 lists all 4,095 other rows and its ring successor, every other row its ring successor: with wave_fold the hub gets a wave
    (another association: the 1e-9 contract, scaled by the sum of |terms| so that cancellation does not decide the figure) and every
    ring row stays sequential (bit-identical); without it every row is sequential."""
    n, ticks = 4096, 10
    src, dst = ft.hub_and_ring(n)
    x0, comps = _xyz(n, 9, extra=("w",))
    hip = _exec(ft.sum_program(wave_fold, feedback=False), comps, {"e": (src, dst)}, n, graph_tables="device")
    tp = ft.sum_program(wave_fold, feedback=False).trace({"x": 1, "y": 1, "z": 1, "w": 1}, fold_edges={"e": (src, dst)}, fold_tables="device")
    want = {k: v.copy() for k, v in comps.items()}
    worst = 0.0
    for t in range(1, ticks + 1):
        hip.run(1)
        ft.walker_run(tp, want, 1, first_tick=t)
        y = want["y"][:, 0]
        scale = np.abs(y[0] * y[dst[src == 0]]).sum()
        worst = max(worst, abs(hip.component("z")[0, 0] - want["z"][0, 0]) / scale)
        for name in ("x", "y"):
            assert np.array_equal(hip.component(name), want[name]), (t, name)
        assert np.array_equal(hip.component("z")[1:], want["z"][1:]) and np.array_equal(hip.component("w")[1:], want["w"][1:]), t
    print(f"hub of 4,096 out-edges, wave_fold={wave_fold}: worst |z - walker| / sum|terms| over {ticks} ticks = {worst:.3e}")
    if wave_fold:
        assert worst <= 1e-9
    else:
        assert worst == 0.0 and np.array_equal(hip.component("w"), want["w"])
    assert abs(want["z"][0, 0]) > 1.0
    hip.close()


@pytest.fixture(scope="module")
def big_newton_world():
    """The 8,192-body, nine-target Newton module (73,728 edges per scan): half a minute of ingest, built once."""
    nb = 8192
    targets = {s_: [(s_ + k) % nb for k in (1, 5, 11, 17, 23, 29, 31, 37, 41)] for s_ in range(nb)}
    G = 6.6743e-11
    text, slots = hb.edge_fold_world(nb, targets, "newton", (G,))
    prog, manifest, edges = sh.world_program(text, slots)
    return nb, targets, G, prog, manifest, edges


def test_a_stablehlo_world_past_the_cap_runs_against_the_oracle(big_newton_world):
    nb, targets, G, prog, manifest, edges = big_newton_world
    assert manifest["edges_per_fold"] == [9 * nb] * 4
    rng = np.random.default_rng(3)
    pos = np.concatenate([np.tile([0, 0, 0, 1.0], (nb, 1)), rng.normal(size=(nb, 3)) * 10], axis=1)
    vel = np.concatenate([np.zeros((nb, 3)), rng.normal(size=(nb, 3))], axis=1)
    m = rng.uniform(1e9, 1e10, nb)
    inertia = np.concatenate([np.tile(m[:, None], (1, 3)), np.zeros((nb, 3)), m[:, None]], axis=1)
    cols = {c["column"]: np.zeros((nb, c["width"])) for c in manifest["columns"]}
    cols["hlo_simulation_time_step"][:] = 0.01
    cols["hlo_world_pos"], cols["hlo_world_vel"], cols["hlo_inertia"] = pos.copy(), vel.copy(), inertia.copy()
    ids = np.arange(1, nb + 1, dtype=np.uint64)
    hip = ea.HipExec(np.tile([0, 0, 0, 1.0, 0, 0, 0], (nb, 1)), np.zeros((nb, 6)), np.ones((nb, 7)), entity_ids=ids, integrator=L.INTEGRATOR_NONE,
                     effectors=prog, columns=cols, graph_edges=sh.edges_as_entity_ids(edges, ids), graph_tables="auto")
    assert len(hip._device_folds) == 4 and all(c is not None for c in hip._device_folds)
    hip.run(10)
    src = np.array([s_ for s_ in range(nb) for _ in targets[s_]], dtype=np.uint32)
    dst = np.array([t for s_ in range(nb) for t in targets[s_]], dtype=np.uint32)
    ref = orc.OracleWorld(pos, vel, inertia, simulation_time_step=0.01, ops=[(orc.EFF_EDGE_GRAVITY_NEWTON, (G,), None)], edges=(src, dst)).step(10)
    worst = 0.0
    for c, r in (("world_pos", ref.world_pos), ("world_vel", ref.world_vel), ("world_accel", ref.world_accel), ("force", ref.force)):
        g = hip._aux["hlo_" + c]
        for sl in ((slice(0, 4), slice(4, 7)) if c == "world_pos" else (slice(0, 3), slice(3, 6))):
            scale = np.maximum(np.max(np.abs(r[:, sl]), axis=1, keepdims=True), 1e-300)
            worst = max(worst, float(np.max(np.abs(g[:, sl] - r[:, sl]) / scale)))
    print(f"8,192-body Newton world, 73,728 edges per scan, 10 ticks vs the oracle: {worst:.3e}; hlo_force bit-identical: {np.array_equal(hip._aux['hlo_force'], ref.force)}")
    assert worst <= 1e-9 and np.all(hip._aux["hlo_tick"] == 10)
    # nine edges per source: every fold is sequential, one lane per source in slot order — the oracle's association, and measured on the
    # MI355X the result IS the oracle's bit for bit (worst = 0), so that is asserted as well
    for c, r in (("world_pos", ref.world_pos), ("world_vel", ref.world_vel), ("world_accel", ref.world_accel), ("force", ref.force)):
        assert np.array_equal(hip._aux["hlo_" + c], r), c
    hip.close()


def _sparse(n, keep_every, k, stride):
    s = np.repeat(np.arange(0, n, keep_every, dtype=np.int64), k)
    j = np.tile(np.arange(k, dtype=np.int64), len(s) // k)
    return s, (s + j * stride + 2) % n


def test_edges_are_replaced_between_batches():
    n = 64
    a = ft.regular_graph(n, 8, stride=5)
    b = _sparse(n, 2, 5, 7)                                                            # another size, another source set (even rows only)
    x0, comps = _xyz(n, 10)
    tp_a = ft.damped_program().trace({"x": 1, "y": 1, "z": 1}, fold_edges={"e": a}, fold_tables="device")
    tp_b = ft.damped_program().trace({"x": 1, "y": 1, "z": 1}, fold_edges={"e": b}, fold_tables="device")
    want = {k: v.copy() for k, v in comps.items()}
    ft.walker_run(tp_a, want, 10)
    z_mid = want["z"].copy()
    ft.walker_run(tp_b, want, 10, first_tick=11)
    assert np.array_equal(want["z"][1::2], z_mid[1::2]) and not np.array_equal(want["z"][0::2], z_mid[0::2])      # rows that stopped being sources keep their value
    ids = np.arange(1, n + 1, dtype=np.uint64)
    hip = _exec(ft.damped_program(), comps, {"e": a}, n, graph_tables="device")
    hip.run(10)
    hip.set_graph_edges({"e": (ids[b[0]], ids[b[1]])})
    hip.run(10)
    for name in ("x", "y", "z"):
        assert np.array_equal(hip.component(name), want[name]), name
    with pytest.raises(KeyError, match="nobody"):
        hip.set_graph_edges({"nobody": (ids[:1], ids[:1])})
    with pytest.raises(KeyError, match="not an entity"):
        hip.set_graph_edges({"e": (ids[:1], np.array([n + 5], dtype=np.uint64))})
    hip.run(1)                                                                         # a refused table leaves the installed one in place
    ft.walker_run(tp_b, want, 1, first_tick=21)
    assert np.array_equal(hip.component("z"), want["z"])
    hip.close()
    # replayed batches: the captured chain holds pointers and grid sizes, so new edges rebuild it — same bits as the eager run
    out = {}
    for graph in (False, True):
        hip = _exec(ft.damped_program(body_free=True), comps, {"e": a}, n, graph_tables="device", use_graph=graph)
        if graph:
            hip.prepare(48)
        t1 = hip.run(48)
        hip.set_graph_edges({"e": (ids[b[0]], ids[b[1]])})
        if graph:
            hip.prepare(48)
        t2 = hip.run(48)
        assert (t1.graph_launches == 48) == graph and (t2.graph_launches == 48) == graph, (graph, t1.graph_launches, t2.graph_launches)
        out[graph] = {c: hip.component(c).copy() for c in ("x", "y", "z")}
        hip.close()
    for c in out[False]:
        assert np.array_equal(out[False][c], out[True][c]), c
    baked = _exec(ft.damped_program(), comps, {"e": a}, n)                             # "auto" below the cap: baked, its graph is its code
    assert baked._device_folds == [None]
    with pytest.raises(ValueError, match="bakes"):
        baked.set_graph_edges({"e": (ids[b[0]], ids[b[1]])})
    baked.close()


def test_two_graphs_share_one_cached_object():
    n = 64
    x0, comps = _xyz(n, 12)
    paths = []
    for edges in (ft.regular_graph(n, 8, stride=5), _sparse(n, 2, 5, 7)):
        tp = ft.damped_program().trace({"x": 1, "y": 1, "z": 1}, fold_edges={"e": edges}, fold_tables="device")
        paths.append(codegen.build(tp, "float64", 2, policy=codegen.policy_for(n, 32 + 4, 8)))
    assert paths[0] == paths[1]
    # ... and two executors of one process over that one object keep their own tables
    a, b = ft.regular_graph(n, 8, stride=5), _sparse(n, 2, 5, 7)
    ha = _exec(ft.damped_program(), comps, {"e": a}, n, graph_tables="device")
    hb_ = _exec(ft.damped_program(), comps, {"e": b}, n, graph_tables="device")
    for _ in range(3):
        ha.run(2)
        hb_.run(2)
    for hip, edges in ((ha, a), (hb_, b)):
        want = {k: v.copy() for k, v in comps.items()}
        ft.walker_run(ft.damped_program().trace({"x": 1, "y": 1, "z": 1}, fold_edges={"e": edges}, fold_tables="device"), want, 6)
        assert np.array_equal(hip.component("z"), want["z"]) and np.array_equal(hip.component("x"), want["x"])
        hip.close()


def test_an_empty_graph_and_a_self_loop_do_not_fault():
    n = 16
    x0, comps = _xyz(n, 13)
    none = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    hip = _exec(ft.damped_program(), comps, {"e": none}, n, graph_tables="device")
    hip.run(3)
    x = x0.copy()
    for _ in range(3):
        y = x * 0.75 + 0.25
        x = x * 0.5 + 0.0 * 0.0625
    assert np.array_equal(hip.component("z"), np.zeros((n, 1))) and np.array_equal(hip.component("x")[:, 0], x) and np.array_equal(hip.component("y")[:, 0], y)
    hip.close()
    loop = (np.array([5]), np.array([5]))
    for prog in (ft.damped_program, lambda: ft.sum_program(True)):
        hip = _exec(prog(), comps, {"e": loop}, n, graph_tables="device")
        hip.run(3)
        want = ft.walker_run(prog().trace({"x": 1, "y": 1, "z": 1}, fold_edges={"e": loop}, fold_tables="device"), {k: v.copy() for k, v in comps.items()}, 3)
        for name in ("x", "y", "z"):
            assert np.array_equal(hip.component(name), want[name]), name
        assert want["z"][5, 0] != 0.0 and np.count_nonzero(want["z"]) == 1
        hip.close()


def test_the_library_refuses_what_it_cannot_install():
    """Statuses with a message, nothing half-installed: no program, a baked object, a bad fold index, a row outside replica 0, and a
    step before every fold has its table."""
    lib = L.lib()
    u64p = C.POINTER(C.c_uint64)
    n = 6
    ids = np.arange(1, n + 1, dtype=np.uint64)
    two = (C.c_uint64 * 2)(1, 2)
    x0, comps = _xyz(n, 14)
    plain = ea.HipExec(np.tile([0, 0, 0, 1.0, 0, 0, 0], (n, 1)), np.zeros((n, 6)), np.ones((n, 7)), entity_ids=ids)
    assert lib.sixdof_set_fold_edges(plain._h, 0, two, two, 2) == L.ERR_UNSUPPORTED and b"no generated program" in lib.sixdof_last_error(plain._h)
    plain.close()
    baked = _exec(ft.damped_program(), comps, {"e": EDGES["e"]}, n, graph_tables="baked")
    assert lib.sixdof_set_fold_edges(baked._h, 0, two, two, 2) == L.ERR_UNSUPPORTED and b"bakes" in lib.sixdof_last_error(baked._h)
    baked.close()
    hip = _exec(ft.damped_program(), comps, {"e": EDGES["e"]}, n, graph_tables="device", graph_replicas=(2, 3))
    assert lib.sixdof_set_fold_edges(hip._h, 1, two, two, 2) == L.ERR_INVALID_ARGUMENT and b"out of range" in lib.sixdof_last_error(hip._h)
    far = (C.c_uint64 * 2)(1, 5)                                                       # entity 5 is row 4: not in replica 0 (rows 0..2)
    assert lib.sixdof_set_fold_edges(hip._h, 0, two, far, 2) == L.ERR_INVALID_ARGUMENT and b"replica 0" in lib.sixdof_last_error(hip._h)
    hip.run(2)                                                                         # the table installed at build time is still the one in use
    want = {k: v.copy() for k, v in comps.items()}
    tp = ft.damped_program().trace({"x": 1, "y": 1, "z": 1}, fold_edges=EDGES, fold_replicas=(2, 3), fold_tables="device")
    ft.walker_run(tp, want, 2)
    assert np.array_equal(hip.component("z"), want["z"]) and np.count_nonzero(want["z"]) == 4
    # the same object on a fresh handle, no table yet: the step is a status, not a launch
    so = codegen.build(tp, "float64", 2, policy=codegen.policy_for(n, 32 + 4, 8))
    cols = [("x", comps["x"]), ("y", comps["y"]), ("z", comps["z"]), ("z#fold0", np.zeros((n, 1)))]
    assert [c for c, _ in tp.columns] == [c for c, _ in cols]
    cid = (C.c_uint64 * 4)(*[L.component_id(c) for c, _ in cols])
    assert lib.sixdof_set_custom_pipe(hip._h, str(so).encode(), cid, 4) == L.OK      # re-installing drops the tables
    t = L.Timings()
    assert lib.sixdof_step(hip._h, 1, C.byref(t)) == L.ERR_UNSUPPORTED and b"sixdof_set_fold_edges" in lib.sixdof_last_error(hip._h)
    e = EDGES["e"]
    assert lib.sixdof_set_fold_edges(hip._h, 0, ids[np.array(e[0])].ctypes.data_as(u64p), ids[np.array(e[1])].ctypes.data_as(u64p), 3) == L.OK
    assert lib.sixdof_step(hip._h, 1, C.byref(t)) == L.OK
    hip.close()


def test_world_build_keeps_a_folds_edges_in_device_memory_when_asked():
    """World.build(graph_tables="device") on the three-entity world of test_fold_between_systems_through_world_build_without_six_dof:
    the same values, the executor holds a table it can replace; the default build of the same world stays baked."""
    import elodin_amd as el

    def world():
        w = el.World()
        a = w.spawn([el.C("x", [1.0]), el.C("n", [0.0])], "e1")
        b = w.spawn([el.C("x", [2.0]), el.C("n", [0.0])], "e2")
        c = w.spawn([el.C("x", [2.0]), el.C("n", [0.0])], "e3")
        for f_, t_ in ((a, b), (a, c), (b, c)):
            w.spawn(el.Edge(f_, t_, component="e"))
        return w
    ex = world().build(double | fold_test | add_one, graph_tables="device")
    assert ex._hip._device_folds == ["e"]
    x = np.array([1.0, 2.0, 2.0])
    for _ in range(3):
        ex.run()
        x = x * 2.0
        x = np.array([5.0 + (x[0] + x[1]) + (x[0] + x[2]), 5.0 + (x[1] + x[2]), x[2]]) + 1.0
        assert np.array_equal(ex.column_array("x")[:, 0], x)
    assert world().build(double | fold_test | add_one)._hip._device_folds == [None]
    with pytest.raises(ValueError, match="graph_tables"):
        world().build(double | fold_test | add_one, graph_tables="hbm")


def test_a_loaded_object_installs_the_edges_of_its_sidecar(tmp_path):
    """compile_world(fold_tables="device") on the 70-body sparse Newton world, then load_world + HipExec: nothing traced or compiled, the
    sidecar's edges installed — against the oracle inside the 1e-9 gate of test_a_sparse_newton_fold_world_on_the_gpu."""
    nb = 70
    targets = {s_: [(s_ + k) % nb for k in (1, 5, 11)] for s_ in range(nb)}
    G = 6.6743e-11
    text, slots = hb.edge_fold_world(nb, targets, "newton", (G,))
    meta = {"arg_ids": [L.component_id(c) for c, _, _ in slots], "ret_ids": [L.component_id(c) for c, _, _ in slots], "names": {str(L.component_id(c)): c for c, _, _ in slots},
            "rows": nb, "arg_slots": [{"component_id": L.component_id(c), "shape": s_, "entity_axis_elided": e_} for c, s_, e_ in slots]}
    so, manifest = sh.compile_world(text, meta, out=str(tmp_path / "pipe.so"), fold_tables="device")
    assert manifest["fold_tables"] == "device" and (tmp_path / "pipe.so.edges").exists()
    prog, manifest = sh.load_world(str(so))
    rng = np.random.default_rng(3)
    pos = np.concatenate([np.tile([0, 0, 0, 1.0], (nb, 1)), rng.normal(size=(nb, 3)) * 10], axis=1)
    vel = np.concatenate([np.zeros((nb, 3)), rng.normal(size=(nb, 3))], axis=1)
    m = rng.uniform(1e9, 1e10, nb)
    inertia = np.concatenate([np.tile(m[:, None], (1, 3)), np.zeros((nb, 3)), m[:, None]], axis=1)
    cols = {c["column"]: np.zeros((nb, c["width"])) for c in manifest["columns"]}
    cols["hlo_simulation_time_step"][:] = 0.01
    cols["hlo_world_pos"], cols["hlo_world_vel"], cols["hlo_inertia"] = pos.copy(), vel.copy(), inertia.copy()
    hip = ea.HipExec(np.tile([0, 0, 0, 1.0, 0, 0, 0], (nb, 1)), np.zeros((nb, 6)), np.ones((nb, 7)), integrator=L.INTEGRATOR_NONE, effectors=prog, columns=cols)
    assert len(hip._device_folds) == 4 and all(c is not None for c in hip._device_folds)
    hip.run(50)
    src = np.array([s_ for s_ in range(nb) for _ in targets[s_]], dtype=np.uint32)
    dst = np.array([t for s_ in range(nb) for t in targets[s_]], dtype=np.uint32)
    ref = orc.OracleWorld(pos, vel, inertia, simulation_time_step=0.01, ops=[(orc.EFF_EDGE_GRAVITY_NEWTON, (G,), None)], edges=(src, dst)).step(50)
    worst = 0.0
    for c, r in (("world_pos", ref.world_pos), ("world_vel", ref.world_vel), ("world_accel", ref.world_accel), ("force", ref.force)):
        g = hip._aux["hlo_" + c]
        for sl in ((slice(0, 4), slice(4, 7)) if c == "world_pos" else (slice(0, 3), slice(3, 6))):
            scale = np.maximum(np.max(np.abs(r[:, sl]), axis=1, keepdims=True), 1e-300)
            worst = max(worst, float(np.max(np.abs(g[:, sl] - r[:, sl]) / scale)))
    print(f"70-body sparse Newton world from a loaded object and its sidecar, 50 ticks vs the oracle: {worst:.3e}")
    assert worst <= 1e-9
    hip.close()
