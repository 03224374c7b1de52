"""The replay-chain plan of sixdof_step (csrc/step_plan.hpp plan_chains): how many launches of a batch replay from a
captured graph at the benchmark's size, and that the replayed launches give the bits of eager ones."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402

pytestmark = pytest.mark.gpu

COLUMNS = ("world_pos", "world_vel", "world_accel", "force")

# (ticks, launches, graph_launches), in order on one handle, each batch prepared first.  The first batch after the upload
# opens with the eager accel-check launch; 35 and 547 leave a 3-launch tail, 4099 three launches, which run eagerly.
K1_LADDER = [(40, 40, 39), (3, 3, 0), (4, 4, 4), (20, 20, 20), (35, 35, 32), (36, 36, 36), (543, 543, 543),
             (547, 547, 544), (600, 600, 600), (4099, 4099, 4096)]
# K = 4: a first batch takes the accel-check launch; then 25 four-tick launches replay and the 3-tick remainder is eager
K4_LADDER = [(8, 2, 0), (103, 26, 25)]


@pytest.mark.parametrize("k, ladder", [(1, K1_LADDER), (4, K4_LADDER)], ids=["k1", "k4"])
def test_replayed_launch_counts_and_bits(k, ladder):
    graph = bench.make_exec(65536, 0, 0, k, True)[0]
    eager = bench.make_exec(65536, 0, 0, k, False)[0]
    try:
        ticks = 0
        for n, launches, graph_launches in ladder:
            graph.prepare(n)
            eager.prepare(n)
            t = graph.invoke_batch(n)
            e = eager.invoke_batch(n)
            ticks += n
            assert (t.launches, t.graph_launches) == (launches, graph_launches), n
            assert (e.launches, e.graph_launches) == (launches, 0), n
            assert graph.tick == eager.tick == ticks
            graph.download()
            eager.download()
            for f in COLUMNS:
                a, b = getattr(graph, f), getattr(eager, f)
                assert a.tobytes() == b.tobytes(), (n, f, float(np.max(np.abs(a - b))))
    finally:
        graph.close()
        eager.close()
