#!/usr/bin/env python3
"""Watch lists against whole-block telemetry reads, on one GPU at 65,536 bodies f64 (profiles/history_watch.md).

Two questions:
  read-back   time to read 16 entities x 1,024 ticks of the four recorded columns: HipExec.history_series (one gather, four
              copies of m rows per tick) against HipExec.history (one [n, w] block per tick and column).
  streaming   entity-steps/s of the stepper while telemetry leaves the device: stream_series (16 watched entities, 64-tick
              batches) against stream_history (every row of every tick) and against recording with nothing read back.

Every leg runs in a child process of its own, under its own time limit, several windows per child after a warm-up; the legs
alternate over `--rounds` rounds and a failed child ends the run.  The baseline legs (history, stream_history, record only)
do not touch anything this feature added; with --baseline-root they import elodin_amd from that built checkout instead, e.g.
one of the commit before the feature.

    python tools/history_watch_ab.py [--baseline-root DIR] [--out profiles/history_watch.md]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, os.environ.get("HISTORY_WATCH_IMPORT_ROOT") or str(ROOT))      # a child of a baseline leg imports the baseline tree

N = 65536
FIELDS = ("world_pos", "world_vel", "world_accel", "force")
WATCHED = 16
READ_TICKS = 1024
BATCH = 64
ROW_BYTES = (7 + 6 + 6 + 6) * 8          # the four recorded columns of one body, f64


def _exec(ticks_per_launch):
    import elodin_amd as ea
    from elodin_amd import workloads
    w = workloads.independent_bodies(N)
    eff = workloads.gravity_torque_effectors(w["body_torque"])
    ex = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], entity_ids=w["entity_ids"], simulation_time_step=workloads.DT_120HZ,
                    effectors=eff, ticks_per_launch=ticks_per_launch)
    watched = w["entity_ids"][:: N // WATCHED][:WATCHED]
    return ex, watched


def leg_read_series(windows):
    ex, watched = _exec(BATCH)
    ex.enable_history(READ_TICKS)
    ex.invoke_batch(READ_TICKS)
    ex.set_watch(FIELDS, watched)
    for _ in range(2):
        ex.history_series(1, READ_TICKS)
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        got = ex.history_series(1, READ_TICKS)           # returns after a stream synchronise
        out.append(time.perf_counter() - t0)
    assert got["world_pos"].shape == (WATCHED, READ_TICKS, 7)
    return {"seconds": out, "bytes": WATCHED * READ_TICKS * ROW_BYTES}


def leg_read_blocks(windows):
    ex, _ = _exec(BATCH)
    ex.enable_history(READ_TICKS)
    ex.invoke_batch(READ_TICKS)
    ex.history("force", 1, 64)
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for name in FIELDS:                              # a synchronise per tick inside
            block = ex.history(name, 1, READ_TICKS)
            assert block.shape[0] == READ_TICKS
            del block
        out.append(time.perf_counter() - t0)
    return {"seconds": out, "bytes": N * READ_TICKS * ROW_BYTES}


def _rate(wall, batches):
    return N * BATCH * batches / wall


def leg_stream_series(windows, batches, every):
    ex, watched = _exec(BATCH)
    ex.set_watch(FIELDS, watched)
    ex.stream_series(4, BATCH, every=every)
    return {"entity_steps_per_s": [_rate(ex.stream_series(batches, BATCH, every=every), batches) for _ in range(windows)],
            "bytes_per_batch": WATCHED * (BATCH // every) * ROW_BYTES}


def leg_stream_history(windows, batches):
    ex, _ = _exec(BATCH)
    ex.stream_history(4, BATCH)
    return {"entity_steps_per_s": [_rate(ex.stream_history(batches, BATCH), batches) for _ in range(windows)],
            "bytes_per_batch": N * BATCH * ROW_BYTES}


def leg_record_only(windows, batches):
    from elodin_amd import _lib as L
    ex, _ = _exec(BATCH)
    ex.enable_history(2 * BATCH)
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
    # name: (function, extra arguments, runs on the baseline library, time limit of one child in seconds)
    "read: history_series": (leg_read_series, (), False, 240),
    "read: history, whole blocks": (leg_read_blocks, (), True, 600),
    "stream: stream_series every=1": (leg_stream_series, (1,), False, 240),
    "stream: stream_series every=8": (leg_stream_series, (8,), False, 240),
    "stream: stream_history": (leg_stream_history, (), True, 420),
    "stream: record only": (leg_record_only, (), True, 240),
}


def run_leg(name, windows, batches):
    fn, extra, _, _ = LEGS[name]
    res = fn(windows) if name.startswith("read") else fn(windows, batches, *extra)
    print("LEG_RESULT " + json.dumps(res), flush=True)


def _fmt_rate(v):
    return f"{v:.3e}"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", help="(internal) run one leg in this process")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5, help="timed windows per child")
    ap.add_argument("--block-windows", type=int, default=2, help="timed windows per child of the whole-block read (13.4 GB each)")
    ap.add_argument("--batches", type=int, default=4096, help="64-tick batches per streaming window (most of a second of stepping)")
    ap.add_argument("--history-batches", type=int, default=64, help="64-tick batches per stream_history window (0.84 GB each)")
    ap.add_argument("--baseline-root", default=None, help="built checkout the baseline legs import elodin_amd from (default: this one)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "history_watch.md"))
    a = ap.parse_args()
    if a.leg:
        run_leg(a.leg, a.windows, a.batches)
        return
    pooled = {name: [] for name in LEGS}
    meta = {}
    for rnd in range(a.rounds):
        for name, (_, _, baseline, limit) in LEGS.items():
            env = dict(os.environ)
            if baseline and a.baseline_root:
                env["HISTORY_WATCH_IMPORT_ROOT"] = str(Path(a.baseline_root).resolve())
            windows = a.block_windows if "whole blocks" in name else a.windows
            batches = a.history_batches if "stream_history" in name else a.batches
            cmd = [sys.executable, str(Path(__file__).resolve()), "--leg", name, "--windows", str(windows), "--batches", str(batches)]
            try:
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"{name}: no result within {limit} s; nothing more is started")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG_RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit(f"{name}: child failed (status {p.returncode}); nothing more is started\n{p.stdout[-1500:]}\n{p.stderr[-3000:]}")
            res = json.loads(line[-1][len("LEG_RESULT "):])
            pooled[name] += res.get("seconds") or res["entity_steps_per_s"]
            meta[name] = res
            print(f"round {rnd} {name}: {pooled[name][-windows:]}", flush=True)
    med = {name: statistics.median(v) for name, v in pooled.items()}
    base = "the tree under test (the baseline legs use nothing the feature added)" if not a.baseline_root else \
        "a built checkout of the commit before the feature"
    rows = [f"# Watch lists against whole-block telemetry reads",
            "",
            f"One MI355X, {N:,} bodies, f64, RK4, {BATCH} ticks per launch.  tools/history_watch_ab.py: every leg in a child process of its own,",
            f"{a.rounds} rounds of alternating legs, a warm-up and then {a.windows} timed windows per child ({a.block_windows} for the whole-block read);",
            f"median, and [min .. max], over all windows.  Baseline legs ran on {base}.",
            "",
            f"## Read-back: {WATCHED} entities x {READ_TICKS:,} ticks of the four recorded columns",
            "",
            "| path | bytes to the host | time (host clock around a call that ends in a stream synchronise) |",
            "|---|---|---|"]
    for name in LEGS:
        if name.startswith("read"):
            v = pooled[name]
            rows.append(f"| {name[6:]} | {meta[name]['bytes'] / 1e6:,.1f} MB | {med[name] * 1e3:,.3f} ms [{min(v) * 1e3:,.3f} .. {max(v) * 1e3:,.3f}] |")
    rows += ["",
             f"history_series is {med['read: history, whole blocks'] / med['read: history_series']:,.0f} times faster than reading the whole blocks and keeping {WATCHED} rows.",
             "",
             f"## Streaming: {a.batches:,} batches of {BATCH} ticks per window ({a.history_batches} for stream_history), {WATCHED} watched entities",
             "",
             "| path | bytes to the host per batch | entity-steps/s (wall time of the window) |",
             "|---|---|---|"]
    for name in LEGS:
        if name.startswith("stream"):
            v = pooled[name]
            rows.append(f"| {name[8:]} | {meta[name]['bytes_per_batch'] / 1e6:,.3f} MB | {_fmt_rate(med[name])} [{_fmt_rate(min(v))} .. {_fmt_rate(max(v))}] |")
    rec = med["stream: record only"]
    rows += ["",
             f"Relative to recording with nothing read back: stream_series every=1 {med['stream: stream_series every=1'] / rec:.2f}, "
             f"every=8 {med['stream: stream_series every=8'] / rec:.2f}, stream_history {med['stream: stream_history'] / rec:.3f}.",
             ""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(rows))
    print("\n".join(rows))


if __name__ == "__main__":
    main()
