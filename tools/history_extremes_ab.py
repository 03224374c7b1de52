#!/usr/bin/env python3
"""Ring extremes against ring envelopes and against whole-block reads plus numpy, on one GPU, f64, at 65,536 bodies and at 1,024
(profiles/history_extremes.md).  The four recorded Body columns, ring of 1,024 ticks.

  read-back   one HipExec.history_extremes over the 1,024 ticks — delivered, and reduced only (SIXDOF_EXTREMES_HOLD, then a
              synchronise) — beside one HipExec.history_envelope over the same range, which reads the same bytes of the ring once
              and is the yardstick for ring-read bandwidth on the box at hand, and beside the host route: HipExec.history + numpy
              min / max / argmin / argmax, timed on 32 ticks and scaled to 1,024.
  segments    the reduce-only read under the plan's own time segments and under 1, 2, 4, 8, 16, 32 forced ones (SIXDOF_EXTREMES_SEGMENTS,
              read at every call: the settings alternate inside one child).  What extremes_plan.hpp's extremes_segments is chosen from.
  streaming   entity-steps/s of the stepper at 65,536 bodies while extremes accumulate on the device: stream_extremes in 64-tick
              batches at every 1 and 8, against stream_envelope at the same rates and against recording only.

Every leg runs in a child process of its own, under its own time limit, several windows per child after a warm-up; a window is
`reps` calls behind one another, each ending in a stream synchronise.  The legs alternate over `--rounds` rounds and a failed
child ends the run.

    python tools/history_extremes_ab.py [--out profiles/history_extremes.md]
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
sys.path.insert(0, str(ROOT))

SIZES = (65536, 1024)
FIELDS = ("world_pos", "world_vel", "world_accel", "force")
READ_TICKS = 1024
HOST_TICKS = 32                          # the host route is timed on this many ticks and scaled
BATCH = 64
ROW_BYTES = (7 + 6 + 6 + 6) * 8          # the four recorded columns of one body, f64
SEGMENTS = ("0", "1", "2", "4", "8", "16", "32")     # 0: the plan's choice
REPS = {65536: 10, 1024: 100}            # calls per window


def _exec(n, ticks_per_launch):
    import elodin_amd as ea
    from elodin_amd import workloads
    w = workloads.independent_bodies(n)
    eff = workloads.gravity_torque_effectors(w["body_torque"])
    return ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], entity_ids=w["entity_ids"], simulation_time_step=workloads.DT_120HZ,
                      effectors=eff, ticks_per_launch=ticks_per_launch)


def _recorded(n):
    ex = _exec(n, BATCH)
    ex.enable_history(READ_TICKS)
    ex.invoke_batch(READ_TICKS)
    return ex


def _windows(windows, reps, call):
    for _ in range(2):
        call()
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        out.append((time.perf_counter() - t0) / reps)
    return out


def _held(ex):
    """One reduce-only read of the whole ring: nothing is delivered, the call is waited for."""
    import numpy as np
    from elodin_amd import _lib as L
    comp = np.array([L.component_id(c) for c in FIELDS], dtype=np.uint64)

    def call():
        ex._extremes_read(comp, 1, READ_TICKS, 1, None, L.EXTREMES_HOLD)
        ex.sync()
    return call


def leg_read_extremes(windows, n):
    ex = _recorded(n)
    got = ex.history_extremes(FIELDS, 1, READ_TICKS)
    assert got["world_pos"]["min"].shape == (n, 7) and int(got["force"]["count"].min()) == READ_TICKS
    return {"seconds": _windows(windows, REPS[n], lambda: ex.history_extremes(FIELDS, 1, READ_TICKS)),
            "held_seconds": _windows(windows, REPS[n], _held(ex)), "bytes": 6 * n * 25 * 8}


def leg_read_envelope(windows, n):
    ex = _recorded(n)
    return {"seconds": _windows(windows, REPS[n], lambda: ex.history_envelope(FIELDS, 1, READ_TICKS)), "bytes": READ_TICKS * 5 * 25 * 8}


def leg_read_blocks(windows, n):
    import numpy as np
    ex = _exec(n, BATCH)
    ex.enable_history(BATCH)
    ex.invoke_batch(BATCH)
    ex.history("force", 1, 8)
    out, numpy_s = [], []
    for _ in range(windows):
        t0 = time.perf_counter()
        spent = 0.0
        for name in FIELDS:                              # a synchronise per tick inside
            block = ex.history(name, 1, HOST_TICKS)
            t1 = time.perf_counter()
            res = (np.isfinite(block).sum(axis=0), block.min(axis=0), block.argmin(axis=0), block.max(axis=0), block.argmax(axis=0))   # every element is finite here
            spent += time.perf_counter() - t1
            del block, res
        scale = READ_TICKS / HOST_TICKS
        out.append((time.perf_counter() - t0) * scale)
        numpy_s.append(spent * scale)
    return {"seconds": out, "numpy_seconds": numpy_s, "bytes": n * READ_TICKS * ROW_BYTES}


def leg_segments(windows, n):
    ex = _recorded(n)
    call = _held(ex)
    out = {s: [] for s in SEGMENTS}
    for s in SEGMENTS:                                   # every setting once before anything is timed
        os.environ["SIXDOF_EXTREMES_SEGMENTS"] = s
        call()
    for _ in range(windows):
        for s in SEGMENTS:
            os.environ["SIXDOF_EXTREMES_SEGMENTS"] = s
            out[s] += _windows(1, REPS[n], call)
    return {"by_segments": out}


def _rate(n, wall, batches):
    return n * BATCH * batches / wall


def leg_stream_extremes(windows, batches, every):
    n = SIZES[0]
    ex = _exec(n, BATCH)
    ex.stream_extremes(FIELDS, 4, BATCH, every=every)
    return {"entity_steps_per_s": [_rate(n, ex.stream_extremes(FIELDS, batches, BATCH, every=every)[0], batches) for _ in range(windows)],
            "bytes_per_batch": 0, "bytes_at_the_end": 6 * n * 25 * 8}


def leg_stream_envelope(windows, batches, every):
    n = SIZES[0]
    ex = _exec(n, BATCH)
    ex.stream_envelope(FIELDS, 4, BATCH, every=every)
    return {"entity_steps_per_s": [_rate(n, ex.stream_envelope(FIELDS, batches, BATCH, every=every), batches) for _ in range(windows)],
            "bytes_per_batch": (BATCH // every) * 5 * 25 * 8, "bytes_at_the_end": 0}


def leg_record_only(windows, batches):
    from elodin_amd import _lib as L
    n = SIZES[0]
    ex = _exec(n, BATCH)
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
        out.append(_rate(n, time.perf_counter() - t0, batches))
        ex.set_flags(0)
    return {"entity_steps_per_s": out, "bytes_per_batch": 0, "bytes_at_the_end": 0}


LEGS = {}       # name: (function, extra arguments, time limit of one child in seconds)
for _n in SIZES:
    LEGS[f"read n={_n}: history_extremes"] = (leg_read_extremes, (_n,), 300)
    LEGS[f"read n={_n}: history_envelope"] = (leg_read_envelope, (_n,), 300)
    LEGS[f"read n={_n}: history + numpy"] = (leg_read_blocks, (_n,), 600)
    LEGS[f"read n={_n}: segments"] = (leg_segments, (_n,), 300)
LEGS.update({
    "stream: stream_extremes every=1": (leg_stream_extremes, (1,), 300),
    "stream: stream_extremes every=8": (leg_stream_extremes, (8,), 300),
    "stream: stream_envelope every=1": (leg_stream_envelope, (1,), 300),
    "stream: stream_envelope every=8": (leg_stream_envelope, (8,), 300),
    "stream: record only": (leg_record_only, (), 240),
})


def run_leg(name, windows, batches):
    fn, extra, _ = LEGS[name]
    res = fn(windows, *extra) if name.startswith("read") else fn(windows, batches, *extra)
    print("LEG_RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", help="(internal) run one leg in this process")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--windows", type=int, default=3, help="timed windows per child")
    ap.add_argument("--batches", type=int, default=64, help="64-tick batches per streaming window")
    ap.add_argument("--box", default="one MI355X", help="how the note names the machine")
    ap.add_argument("--registers", default="", help="the kernels' register counts, as the compiler reports them, for the note")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "history_extremes.md"))
    a = ap.parse_args()
    if a.leg:
        run_leg(a.leg, a.windows, a.batches)
        return
    pooled = {name: {} for name in LEGS}       # name -> series -> values
    meta = {}
    for rnd in range(a.rounds):
        for name, (_, _, limit) in LEGS.items():
            windows = 1 if "numpy" in name else a.windows
            cmd = [sys.executable, str(Path(__file__).resolve()), "--leg", name, "--windows", str(windows), "--batches", str(a.batches)]
            env = dict(os.environ)
            env.pop("SIXDOF_EXTREMES_SEGMENTS", None)
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=env)
            except subprocess.TimeoutExpired:
                sys.exit(f"{name}: no result within {limit} s; nothing more is started")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG_RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit(f"{name}: child failed (status {p.returncode}); nothing more is started\n{p.stdout[-1500:]}\n{p.stderr[-3000:]}")
            res = json.loads(line[-1][len("LEG_RESULT "):])
            series = dict(res.get("by_segments", {}))
            for key in ("seconds", "held_seconds", "numpy_seconds", "entity_steps_per_s"):
                if key in res:
                    series[key] = res[key]
            for key, v in series.items():
                pooled[name].setdefault(key, []).extend(v)
            meta[name] = {k: v for k, v in res.items() if k.startswith("bytes")}
            print(f"round {rnd} {name}: " + json.dumps(series), flush=True)
    med = lambda name, key: statistics.median(pooled[name][key])

    def ms(name, key="seconds"):
        v = pooled[name][key]
        return f"{statistics.median(v) * 1e3:,.3f} ms [{min(v) * 1e3:,.3f} .. {max(v) * 1e3:,.3f}]"
    rows = ["# Ring extremes against ring envelopes and whole-block reads",
            "",
            f"{a.box[0].upper() + a.box[1:]}, f64, RK4, {BATCH} ticks per launch, ring of {READ_TICKS:,} ticks, the four recorded Body columns.",
            f"tools/history_extremes_ab.py: every leg in a child process of its own, {a.rounds} rounds of alternating legs, a warm-up and then",
            f"{a.windows} timed windows per child, a window being {REPS[SIZES[0]]} calls behind one another at 65,536 bodies and {REPS[SIZES[1]]} at 1,024, each ending in a",
            "stream synchronise; per call: median, and [min .. max], over all windows.  Nothing here is a gate.",
            ""]
    if a.registers:
        rows += [f"Registers, as the compiler reports them for gfx950 (no spills, no scratch): {a.registers}.", ""]
    for n in SIZES:
        ring_bytes = n * READ_TICKS * ROW_BYTES
        ext, env, blocks = f"read n={n}: history_extremes", f"read n={n}: history_envelope", f"read n={n}: history + numpy"
        gbs = lambda seconds: f"{ring_bytes / seconds / 1e9:,.0f} GB/s"
        rows += [f"## Read-back at {n:,} bodies: {READ_TICKS:,} ticks, {ring_bytes / 1e6:,.0f} MB of ring",
                 "",
                 "| path | bytes to the host | time per call | ring bytes / time |",
                 "|---|---|---|---|",
                 f"| history_extremes, delivered | {meta[ext]['bytes'] / 1e6:,.2f} MB | {ms(ext)} | {gbs(med(ext, 'seconds'))} |",
                 f"| history_extremes, reduced only (HOLD, synchronise) | 0 | {ms(ext, 'held_seconds')} | {gbs(med(ext, 'held_seconds'))} |",
                 f"| history_envelope | {meta[env]['bytes'] / 1e6:,.2f} MB | {ms(env)} | {gbs(med(env, 'seconds'))} |",
                 f"| history + numpy (timed on {HOST_TICKS} ticks, scaled by {READ_TICKS // HOST_TICKS}) | {meta[blocks]['bytes'] / 1e6:,.0f} MB | {ms(blocks)} | {gbs(med(blocks, 'seconds'))} |",
                 "",
                 f"Of the host route {med(blocks, 'numpy_seconds'):,.2f} s is numpy, the rest is reading the blocks.  history_extremes delivered is "
                 f"{med(blocks, 'seconds') / med(ext, 'seconds'):,.0f} times faster than the host route; reduced only it takes "
                 f"{med(ext, 'held_seconds') / med(env, 'seconds'):,.2f} of the envelope's time over the same bytes of the ring.",
                 "",
                 f"### Time segments at {n:,} bodies (reduced only)",
                 "",
                 "| SIXDOF_EXTREMES_SEGMENTS | time per call |",
                 "|---|---|"]
        seg = f"read n={n}: segments"
        for s in SEGMENTS:
            rows.append(f"| {'0 (the plan)' if s == '0' else s} | {ms(seg, s)} |")
        rows.append("")
    rows += [f"## Streaming at {SIZES[0]:,} bodies: {a.batches:,} batches of {BATCH} ticks per window",
             "",
             "| path | bytes to the host per batch | at the end | entity-steps/s (wall time of the window) |",
             "|---|---|---|---|"]
    for name in LEGS:
        if name.startswith("stream"):
            v = pooled[name]["entity_steps_per_s"]
            rows.append(f"| {name[8:]} | {meta[name]['bytes_per_batch'] / 1e6:,.3f} MB | {meta[name]['bytes_at_the_end'] / 1e6:,.2f} MB | "
                        f"{statistics.median(v):.3e} [{min(v):.3e} .. {max(v):.3e}] |")
    rec = med("stream: record only", "entity_steps_per_s")
    rel = lambda name: med(name, "entity_steps_per_s") / rec
    rows += ["",
             f"Relative to recording with nothing read back: stream_extremes every=1 {rel('stream: stream_extremes every=1'):.2f}, every=8 "
             f"{rel('stream: stream_extremes every=8'):.2f}; stream_envelope every=1 {rel('stream: stream_envelope every=1'):.2f}, every=8 "
             f"{rel('stream: stream_envelope every=8'):.2f}.",
             ""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(rows))
    print("\n".join(rows))


if __name__ == "__main__":
    main()
