#!/usr/bin/env python3
"""Ring envelopes against whole-block telemetry reads, on one GPU at 65,536 bodies f64 (profiles/history_envelope.md).

Three questions:
  read-back   time of one HipExec.history_envelope over 1,024 ticks of the four recorded columns, against HipExec.history (one
              [n, w] block per tick and column) plus numpy for the same five numbers — the only way to them without the feature.
  bandwidth   ring bytes the reduction reads per second: the bytes of the sampled blocks (the floor: each is read once)
              over the time of the blocking call, host clock, so the two launches and the 1 MB copy of the result are inside.
  streaming   entity-steps/s of the stepper while envelopes leave the device: stream_envelope in 64-tick batches against
              recording only on the same handle.

Every leg runs in a child process of its own, under its own time limit, several windows per child after a warm-up; the legs
alternate over `--rounds` rounds and a failed child ends the run.

    python tools/history_envelope_ab.py [--out profiles/history_envelope.md]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

N = 65536
FIELDS = ("world_pos", "world_vel", "world_accel", "force")
READ_TICKS = 1024
BATCH = 64
ROW_BYTES = (7 + 6 + 6 + 6) * 8          # the four recorded columns of one body, f64
COPY_KERNEL_TBS = 6.29                   # float4 copy on one MI355X, the figure the kernel guide quotes


def _exec(ticks_per_launch):
    import elodin_amd as ea
    from elodin_amd import workloads
    w = workloads.independent_bodies(N)
    eff = workloads.gravity_torque_effectors(w["body_torque"])
    return ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], entity_ids=w["entity_ids"], simulation_time_step=workloads.DT_120HZ,
                      effectors=eff, ticks_per_launch=ticks_per_launch)


def leg_read_envelope(windows, period):
    ex = _exec(BATCH)
    ex.enable_history(READ_TICKS)
    ex.invoke_batch(READ_TICKS)
    for _ in range(2):
        ex.history_envelope(FIELDS, 1, READ_TICKS, period=period)
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        got = ex.history_envelope(FIELDS, 1, READ_TICKS, period=period)      # returns after a stream synchronise
        out.append(time.perf_counter() - t0)
    assert got["world_pos"]["mean"].shape == (READ_TICKS, period, 7)
    return {"seconds": out, "bytes": READ_TICKS * period * 5 * 25 * 8, "ring_bytes": N * READ_TICKS * ROW_BYTES}


def leg_read_blocks(windows):
    import numpy as np
    ex = _exec(BATCH)
    ex.enable_history(READ_TICKS)
    ex.invoke_batch(READ_TICKS)
    ex.history("force", 1, 64)
    out, reduce_s = [], []
    for _ in range(windows):
        t0 = time.perf_counter()
        spent = 0.0
        for name in FIELDS:                              # a synchronise per tick inside
            for first in range(1, READ_TICKS + 1, BATCH):        # 64 ticks at a time: the host holds one slab, not 13 GB
                block = ex.history(name, first, first + BATCH - 1)
                t1 = time.perf_counter()
                fin = np.isfinite(block)
                cnt = fin.sum(axis=1)
                x = np.where(fin, block, 0.0)
                mean = x.sum(axis=1) / cnt
                m2 = (np.where(fin, block - mean[:, None], 0.0) ** 2).sum(axis=1)
                lo, hi = np.where(fin, block, np.inf).min(axis=1), np.where(fin, block, -np.inf).max(axis=1)
                spent += time.perf_counter() - t1
                del block, fin, x, m2, lo, hi
        out.append(time.perf_counter() - t0)
        reduce_s.append(spent)
    return {"seconds": out, "reduce_seconds": reduce_s, "bytes": N * READ_TICKS * ROW_BYTES}


def _rate(wall, batches):
    return N * BATCH * batches / wall


def leg_stream_envelope(windows, batches, every):
    ex = _exec(BATCH)
    ex.stream_envelope(FIELDS, 4, BATCH, every=every)
    return {"entity_steps_per_s": [_rate(ex.stream_envelope(FIELDS, batches, BATCH, every=every), batches) for _ in range(windows)],
            "bytes_per_batch": (BATCH // every) * 5 * 25 * 8}


def leg_record_only(windows, batches):
    from elodin_amd import _lib as L
    ex = _exec(BATCH)
    ex.enable_history(BATCH)
    ex.invoke_batch(4 * BATCH)
    out = []
    for _ in range(windows):
        ex.sync()
        ex.set_flags(L.FLAG_ASYNC_STEP)
        t0 = time.perf_counter()
        for _ in range(batches):
            ex.invoke_batch(BATCH)
        ex.sync()
        out.append(_rate(time.perf_counter() - t0, batches))
        ex.set_flags(0)
    return {"entity_steps_per_s": out, "bytes_per_batch": 0}


LEGS = {
    # name: (function, extra arguments, time limit of one child in seconds)
    "read: history_envelope": (leg_read_envelope, (1,), 240),
    "read: history_envelope period=64": (leg_read_envelope, (64,), 240),
    "read: history + numpy": (leg_read_blocks, (), 900),
    "stream: stream_envelope every=1": (leg_stream_envelope, (1,), 240),
    "stream: stream_envelope every=8": (leg_stream_envelope, (8,), 240),
    "stream: record only": (leg_record_only, (), 240),
}


def run_leg(name, windows, batches):
    fn, extra, _ = LEGS[name]
    res = fn(windows, *extra) if name.startswith("read") else fn(windows, batches, *extra)
    print("LEG_RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", help="(internal) run one leg in this process")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5, help="timed windows per child")
    ap.add_argument("--block-windows", type=int, default=1, help="timed windows per child of the whole-block read (13.4 GB each)")
    ap.add_argument("--batches", type=int, default=1024, help="64-tick batches per streaming window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "history_envelope.md"))
    a = ap.parse_args()
    if a.leg:
        run_leg(a.leg, a.windows, a.batches)
        return
    pooled = {name: [] for name in LEGS}
    meta = {}
    for rnd in range(a.rounds):
        for name, (_, _, limit) in LEGS.items():
            windows = a.block_windows if "numpy" in name else a.windows
            cmd = [sys.executable, str(Path(__file__).resolve()), "--leg", name, "--windows", str(windows), "--batches", str(a.batches)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"{name}: no result within {limit} s; nothing more is started")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG_RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit(f"{name}: child failed (status {p.returncode}); nothing more is started\n{p.stdout[-1500:]}\n{p.stderr[-3000:]}")
            res = json.loads(line[-1][len("LEG_RESULT "):])
            pooled[name] += res.get("seconds") or res["entity_steps_per_s"]
            meta.setdefault(name, {}).update({k: v for k, v in res.items() if k != "reduce_seconds"})
            meta[name].setdefault("reduce_seconds", []).extend(res.get("reduce_seconds", []))
            print(f"round {rnd} {name}: {pooled[name][-windows:]}", flush=True)
    med = {name: statistics.median(v) for name, v in pooled.items()}
    rows = ["# Ring envelopes against whole-block telemetry reads",
            "",
            f"One MI355X, {N:,} bodies, f64, RK4, {BATCH} ticks per launch.  tools/history_envelope_ab.py: every leg in a child process of its own,",
            f"{a.rounds} rounds of alternating legs, a warm-up and then {a.windows} timed windows per child ({a.block_windows} for the whole-block read);",
            "median, and [min .. max], over all windows.  The whole-block leg uses nothing this feature added: it is the only way to these",
            "numbers without it.",
            "",
            f"## Read-back: the envelopes of {READ_TICKS:,} ticks of the four recorded columns",
            "",
            "| path | bytes to the host | time (host clock around a call that ends in a stream synchronise) |",
            "|---|---|---|"]
    for name in LEGS:
        if name.startswith("read"):
            v = pooled[name]
            rows.append(f"| {name[6:]} | {meta[name]['bytes'] / 1e6:,.1f} MB | {med[name] * 1e3:,.3f} ms [{min(v) * 1e3:,.3f} .. {max(v) * 1e3:,.3f}] |")
    blocks = "read: history + numpy"
    reduce_med = statistics.median(meta[blocks]["reduce_seconds"])
    rows += ["",
             f"Of the whole-block time, {reduce_med:,.1f} s is numpy reducing the blocks and {med[blocks] - reduce_med:,.1f} s is reading them.",
             f"history_envelope is {med[blocks] / med['read: history_envelope']:,.0f} times faster than the whole path, "
             f"{(med[blocks] - reduce_med) / med['read: history_envelope']:,.0f} times faster than its read alone.",
             "",
             "## Bandwidth of the reduction",
             "",
             "| read | ring bytes read (the floor: each sampled block once) | ring bytes per second | of the float4 copy kernel's 6.29 TB/s |",
             "|---|---|---|---|"]
    for name in ("read: history_envelope", "read: history_envelope period=64"):
        tbs = meta[name]["ring_bytes"] / med[name] / 1e12
        rows.append(f"| {name[6:]} | {meta[name]['ring_bytes'] / 1e9:,.2f} GB | {tbs:.2f} TB/s | {100 * tbs / COPY_KERNEL_TBS:.0f} % |")
    rows += ["",
             f"## Streaming: {a.batches:,} batches of {BATCH} ticks per window, the envelopes of the four columns",
             "",
             "| path | bytes to the host per batch | entity-steps/s (wall time of the window) |",
             "|---|---|---|"]
    for name in LEGS:
        if name.startswith("stream"):
            v = pooled[name]
            rows.append(f"| {name[8:]} | {meta[name]['bytes_per_batch'] / 1e6:,.3f} MB | {med[name]:.3e} [{min(v):.3e} .. {max(v):.3e}] |")
    rec = med["stream: record only"]
    rows += ["",
             f"Relative to recording with nothing read back: stream_envelope every=1 {med['stream: stream_envelope every=1'] / rec:.2f}, "
             f"every=8 {med['stream: stream_envelope every=8'] / rec:.2f}.",
             ""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(rows))
    print("\n".join(rows))


if __name__ == "__main__":
    main()
