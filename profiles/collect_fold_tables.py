"""Per-tick device time of fold stages with baked tables and with tables in device memory (profiles/fold_device_tables.md).

    python profiles/collect_fold_tables.py [--ticks 2000] [--repeats 3]

One process, the cases alternating inside every repeat (so drift of the machine hits all of them alike): Timings.kernel_device_ms of
one batch of `ticks` one-tick chains after a warm-up batch, divided by `ticks`.  Eager launches (no replay): every case issues the
same four launches per tick (five with out-degree bins), so the launch floor is common to the cases compared."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import elodin_amd as ea                                     # noqa: E402
from elodin_amd import _lib as L                            # noqa: E402
from tests import fold_tables_common as ft                  # noqa: E402


def _exec(prog, n, edges, flavour, extra=()):
    ids = np.arange(1, n + 1, dtype=np.uint64)
    x0 = np.random.default_rng(1).uniform(-1.0, 1.0, n)
    comps = {"x": x0[:, None].copy(), **{c: np.zeros((n, 1)) for c in ("y", "z") + tuple(extra)}}
    ge = {"e": (ids[edges[0]], ids[edges[1]])}
    return ea.HipExec(np.tile([0, 0, 0, 1.0, 0, 0, 0], (n, 1)), np.zeros((n, 6)), np.ones((n, 7)), entity_ids=ids, integrator=L.INTEGRATOR_NONE,
                      effectors=prog, columns=comps, graph_edges=ge, graph_tables=flavour)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    hub = ft.hub_and_ring(4096)
    cases = [
        ("4,096 rows x 16 targets (65,536 edges), sequential fold, baked", _exec(ft.damped_program(), 4096, ft.regular_graph(4096, 16), "baked")),
        ("4,096 rows x 16 targets (65,536 edges), sequential fold, device", _exec(ft.damped_program(), 4096, ft.regular_graph(4096, 16), "device")),
        ("65,536 rows x 16 targets (1,048,576 edges), sequential fold, device", _exec(ft.damped_program(), 65536, ft.regular_graph(65536, 16), "device")),
        ("hub of 4,096 out-edges + ring of 4,096, plain sum, device, bins (wave_fold)", _exec(ft.sum_program(True, feedback=False), 4096, hub, "device", ("w",))),
        ("hub of 4,096 out-edges + ring of 4,096, plain sum, device, one list", _exec(ft.sum_program(False, feedback=False), 4096, hub, "device", ("w",))),
    ]
    for _, hip in cases:
        hip.invoke_batch(200)
    rows = {name: [] for name, _ in cases}
    for _ in range(a.repeats):
        for name, hip in cases:
            t = hip.invoke_batch(a.ticks)
            rows[name].append(1e3 * t.kernel_device_ms / a.ticks)
    for name, hip in cases:
        hip.close()
    print(f"| case | us per tick, {a.repeats} repeats of {a.ticks} ticks | median | spread (max - min) |")
    print("|---|---|---|---|")
    for name, v in rows.items():
        print(f"| {name} | {', '.join(f'{x:.2f}' for x in v)} | {float(np.median(v)):.2f} | {max(v) - min(v):.2f} |")
    print(json.dumps({"ticks": a.ticks, "us_per_tick": rows}))


if __name__ == "__main__":
    main()
