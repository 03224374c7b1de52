"""Step batches as AQL chains (csrc/aql_chain.cpp): the benchmark's handle takes that path, and what it computes and counts is
what eager launches and the hipGraph path (SIXDOF_AQL=0) compute and count, bit for bit."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
from tests.test_gpu_graph_replay import COLUMNS, K1_LADDER, K4_LADDER  # noqa: E402

pytestmark = pytest.mark.gpu


def _exec(monkeypatch, k, use_graph, aql=True, dtype=np.float64, integrator=None, n=65536):
    import elodin_amd as ea
    from elodin_amd import _lib as L
    from elodin_amd import workloads
    if aql:
        monkeypatch.delenv("SIXDOF_AQL", raising=False)
    else:
        monkeypatch.setenv("SIXDOF_AQL", "0")        # read when the handle is created
    w = workloads.independent_bodies(n)
    eff = workloads.gravity_torque_effectors(w["body_torque"])
    ex = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], entity_ids=w["entity_ids"],
                    simulation_time_step=workloads.DT_120HZ, effectors=eff, device=0, ticks_per_launch=k,
                    use_graph=use_graph, dtype=dtype, integrator=L.RK4 if integrator is None else integrator)
    monkeypatch.delenv("SIXDOF_AQL", raising=False)
    return ex


def test_bench_handle_takes_the_aql_path():
    ex = bench.make_exec(65536, 0, 0, 1, True)[0]
    try:
        assert ex.step_path == "aql"
        ex.prepare(20)
        t = ex.invoke_batch(20)
        assert (t.launches, t.graph_launches) == (20, 19)   # the accel-check launch, then a 19-launch chain
        assert t.kernel_device_ms > 0
        assert ex.step_path == "aql"
    finally:
        ex.close()
    ex = bench.make_exec(65536, 0, 0, 1, False)[0]
    try:
        assert ex.step_path.startswith("eager")
    finally:
        ex.close()


@pytest.mark.parametrize("k, ladder", [(1, K1_LADDER), (4, K4_LADDER)], ids=["k1", "k4"])
@pytest.mark.parametrize("kind", ["f64_rk4", "f32_rk4", "f64_semi_implicit"])
def test_aql_bits_and_counts_match_eager_and_hipgraph(monkeypatch, k, ladder, kind):
    from elodin_amd import _lib as L
    kw = {"f64_rk4": {}, "f32_rk4": {"dtype": np.float32}, "f64_semi_implicit": {"integrator": L.SEMI_IMPLICIT}}[kind]
    if kind != "f64_rk4":
        ladder = ladder[:4]
    aql = _exec(monkeypatch, k, True, **kw)
    graph = _exec(monkeypatch, k, True, aql=False, **kw)
    eager = _exec(monkeypatch, k, False, **kw)
    try:
        assert aql.step_path == "aql"
        assert graph.step_path == "hipgraph: SIXDOF_AQL=0"
        ticks = 0
        for n, launches, graph_launches in ladder:
            counts = []
            for ex in (aql, graph, eager):
                ex.prepare(n)
                t = ex.invoke_batch(n)
                counts.append((t.launches, t.graph_launches))
            ticks += n
            if kind != "f64_semi_implicit":   # no accel-check launch without RK4: the ladders are RK4's
                assert counts[0] == counts[1] == (launches, graph_launches), (n, counts)
                assert counts[2] == (launches, 0), (n, counts)
            else:
                assert counts[0] == counts[1] and counts[0][0] == counts[2][0], (n, counts)
            assert aql.tick == graph.tick == eager.tick == ticks
            for ex in (aql, graph, eager):
                ex.download()
            for f in COLUMNS:
                a, b, c = (getattr(ex, f) for ex in (aql, graph, eager))
                assert a.tobytes() == b.tobytes() == c.tobytes(), (kind, n, f, float(np.max(np.abs(a - c))))
    finally:
        for ex in (aql, graph, eager):
            ex.close()


# K = 8: remainders 1 .. 7 and batches shorter than K need argument blocks of their own, more than the blocks the handle
# keeps at once; every batch is bit-compared with eager launches.  Odd entries are prepared first, even ones are not.
K8_TICKS = [20, 17, 18, 19, 21, 22, 23, 5, 3, 100, 7, 23, 61, 8, 30, 1, 4099]


def test_k8_remainders_match_eager_and_hipgraph(monkeypatch):
    aql = _exec(monkeypatch, 8, True)
    graph = _exec(monkeypatch, 8, True, aql=False)
    eager = _exec(monkeypatch, 8, False)
    try:
        assert aql.step_path == "aql"
        ticks = 0
        for i, n in enumerate(K8_TICKS):
            if i == 9:      # a new upload: the next batch opens with the accel-check launch again
                for ex in (aql, graph, eager):
                    ex.upload()
            counts = []
            for ex in (aql, graph, eager):
                if i % 2:
                    ex.prepare(n)
                t = ex.invoke_batch(n)
                counts.append((t.launches, t.graph_launches))
            ticks += n
            assert counts[0] == counts[1] and counts[0][0] == counts[2][0] == -(-n // 8), (n, counts)
            assert aql.tick == graph.tick == eager.tick == ticks
            for ex in (aql, graph, eager):
                ex.download()
            for f in COLUMNS:
                a, b, c = (getattr(ex, f) for ex in (aql, graph, eager))
                assert a.tobytes() == b.tobytes() == c.tobytes(), (n, f, float(np.max(np.abs(a - c))))
    finally:
        for ex in (aql, graph, eager):
            ex.close()


def test_a_handle_after_the_last_one_closed_still_works(monkeypatch):
    a = _exec(monkeypatch, 1, True, n=4096)
    assert a.step_path == "aql"
    a.invoke_batch(40)
    a.download()
    first = {f: getattr(a, f).copy() for f in COLUMNS}
    a.close()                                    # the last handle: the queue and its code objects go
    b = _exec(monkeypatch, 1, True, n=4096)
    try:
        assert b.step_path == "aql"
        t = b.invoke_batch(40)
        assert (t.launches, t.graph_launches) == (40, 39) and b.tick == 40
        b.download()
        for f in COLUMNS:
            assert getattr(b, f).tobytes() == first[f].tobytes(), f
    finally:
        b.close()
