#!/usr/bin/env python3
"""Ring events against ring extremes and against whole-block reads plus numpy, on one GPU, f64, at 65,536 bodies and at 1,024
(profiles/history_events.md).  Ring of 1,024 ticks; one trigger — world_pos z falls through 0, as a crossing — that captures
world_pos and world_vel.  The bodies start between -1,000 m and 1,000 m and fall under gravity: some runs fire early, some late,
some never, and the share that fires is in the note, because a run that has had its event stops loading.

  read-back   one HipExec.history_events over the 1,024 ticks — delivered, and reduced only (SIXDOF_EVENTS_HOLD, then a
              synchronise) — beside HipExec.history_extremes over world_pos alone IN THE SAME CHILD, windows alternating: it reads
              the same cache lines of the ring once and is the yardstick; and beside the host route, HipExec.history of the three
              blocks + a numpy first-crossing search, timed on 32 ticks and scaled to 1,024.
  segments    the reduce-only read under the plan's own time segments and under 1 .. 64 forced ones (SIXDOF_EVENTS_SEGMENTS, read at
              every call: the settings alternate inside one child).  What events_plan.hpp's events_segments is chosen from.
  streaming   entity-steps/s of the stepper at 65,536 bodies while events accumulate on the device: stream_events in 64-tick batches
              at every 1 and 8, against stream_extremes of world_pos at the same rates and against recording only.

Every leg runs in a child process of its own, under its own time limit, several windows per child after a warm-up; a window is
`reps` calls behind one another, each ending in a stream synchronise.  The legs alternate over `--rounds` rounds and a failed
child ends the run.

    python tools/history_events_ab.py [--out profiles/history_events.md]
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
CAPTURE = ("world_pos", "world_vel")
READ_TICKS = 1024
HOST_TICKS = 32                          # the host route is timed on this many ticks and scaled
BATCH = 64
SEGMENTS = ("0", "1", "2", "4", "8", "16", "32", "64")     # 0: the plan's choice
REPS = {65536: 10, 1024: 100}            # calls per window


def _event():
    import elodin_amd as ea
    return ea.Event("world_pos", 6, "<=", 0.0)


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


def _held_events(ex):
    """One reduce-only read of the whole ring: nothing is delivered, the call is waited for."""
    import numpy as np
    from elodin_amd import _lib as L
    trig = ex._event_triggers(_event())
    comp = np.array([L.component_id(c) for c in CAPTURE], dtype=np.uint64)

    def call():
        ex._scan_read(ex._EVENTS_SCAN, trig, comp, 1, 1, READ_TICKS, 1, None, None, L.EVENTS_HOLD)
        ex.sync()
    return call


def _held_extremes(ex):
    import numpy as np
    from elodin_amd import _lib as L
    comp = np.array([L.component_id("world_pos")], dtype=np.uint64)

    def call():
        ex._extremes_read(comp, 1, READ_TICKS, 1, None, L.EXTREMES_HOLD)
        ex.sync()
    return call


def leg_read(windows, n):
    ex = _recorded(n)
    got = ex.history_events(_event(), CAPTURE, 1, READ_TICKS)
    fired = got["tick"][0] > 0
    assert got["capture"]["world_vel"].shape == (1, n, 6) and fired.any()
    calls = {"events": lambda: ex.history_events(_event(), CAPTURE, 1, READ_TICKS), "events_held": _held_events(ex),
             "extremes": lambda: ex.history_extremes(["world_pos"], 1, READ_TICKS), "extremes_held": _held_extremes(ex)}
    out = {k: [] for k in calls}
    for k, call in calls.items():                        # every path once before anything is timed
        call()
    for _ in range(windows):                             # the paths alternate inside the child
        for k, call in calls.items():
            out[k] += _windows(1, REPS[n], call)
    return {"series": out, "fired": float(fired.mean()), "median_tick": float(statistics.median(got["tick"][0][fired].tolist())),
            "bytes_events": (4 + 13) * n * 8, "bytes_extremes": 6 * n * 7 * 8}


def leg_read_blocks(windows, n):
    import numpy as np
    ex = _exec(n, BATCH)
    ex.enable_history(BATCH)
    ex.invoke_batch(BATCH)
    ex.history("world_pos", 1, 8)
    out, numpy_s = [], []
    for _ in range(windows):
        t0 = time.perf_counter()
        pos, vel = ex.history("world_pos", 1, HOST_TICKS), ex.history("world_vel", 1, HOST_TICKS)       # a synchronise per tick inside
        t1 = time.perf_counter()
        holds = pos[:, :, 6] <= 0.0                      # every element is finite here
        cross = holds[1:] & ~holds[:-1]
        at = np.where(cross.any(axis=0), cross.argmax(axis=0) + 1, 0)
        rows = np.arange(n)
        res = (at, pos[at, rows], vel[at, rows], pos[np.maximum(at - 1, 0), rows, 6])
        spent = time.perf_counter() - t1
        del pos, vel, res
        scale = READ_TICKS / HOST_TICKS
        out.append((time.perf_counter() - t0) * scale)
        numpy_s.append(spent * scale)
    return {"series": {"seconds": out, "numpy_seconds": numpy_s}, "bytes": n * READ_TICKS * 13 * 8}


def leg_segments(windows, n):
    ex = _recorded(n)
    call = _held_events(ex)
    out = {s: [] for s in SEGMENTS}
    for s in SEGMENTS:                                   # every setting once before anything is timed
        os.environ["SIXDOF_EVENTS_SEGMENTS"] = s
        call()
    for _ in range(windows):
        for s in SEGMENTS:
            os.environ["SIXDOF_EVENTS_SEGMENTS"] = s
            out[s] += _windows(1, REPS[n], call)
    return {"series": out}


def _rate(n, wall, batches):
    return n * BATCH * batches / wall


def leg_stream_events(windows, batches, every):
    n = SIZES[0]
    ex = _exec(n, BATCH)
    ex.stream_events(_event(), CAPTURE, 4, BATCH, every=every)
    return {"series": {"entity_steps_per_s": [_rate(n, ex.stream_events(_event(), CAPTURE, batches, BATCH, every=every)[0], batches) for _ in range(windows)]},
            "bytes_at_the_end": (4 + 13) * n * 8}


def leg_stream_extremes(windows, batches, every):
    n = SIZES[0]
    ex = _exec(n, BATCH)
    ex.stream_extremes(["world_pos"], 4, BATCH, every=every)
    return {"series": {"entity_steps_per_s": [_rate(n, ex.stream_extremes(["world_pos"], batches, BATCH, every=every)[0], batches) for _ in range(windows)]},
            "bytes_at_the_end": 6 * n * 7 * 8}


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
    return {"series": {"entity_steps_per_s": out}, "bytes_at_the_end": 0}


LEGS = {}       # name: (function, extra arguments, time limit of one child in seconds)
for _n in SIZES:
    LEGS[f"read n={_n}: events and extremes"] = (leg_read, (_n,), 300)
    LEGS[f"read n={_n}: history + numpy"] = (leg_read_blocks, (_n,), 300)
    LEGS[f"read n={_n}: segments"] = (leg_segments, (_n,), 300)
LEGS.update({
    "stream: stream_events every=1": (leg_stream_events, (1,), 240),
    "stream: stream_events every=8": (leg_stream_events, (8,), 240),
    "stream: stream_extremes every=1": (leg_stream_extremes, (1,), 240),
    "stream: stream_extremes every=8": (leg_stream_extremes, (8,), 240),
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "history_events.md"))
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
            env.pop("SIXDOF_EVENTS_SEGMENTS", None)
            env.pop("SIXDOF_EXTREMES_SEGMENTS", None)
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=env)
            except subprocess.TimeoutExpired:
                sys.exit(f"{name}: no result within {limit} s; nothing more is started")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG_RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit(f"{name}: child failed (status {p.returncode}); nothing more is started\n{p.stdout[-1500:]}\n{p.stderr[-3000:]}")
            res = json.loads(line[-1][len("LEG_RESULT "):])
            for key, v in res["series"].items():
                pooled[name].setdefault(key, []).extend(v)
            meta[name] = {k: v for k, v in res.items() if k != "series"}
            print(f"round {rnd} {name}: " + json.dumps(res["series"]), flush=True)
    med = lambda name, key: statistics.median(pooled[name][key])

    def ms(name, key="seconds"):
        v = pooled[name][key]
        return f"{statistics.median(v) * 1e3:,.3f} ms [{min(v) * 1e3:,.3f} .. {max(v) * 1e3:,.3f}]"
    rows = ["# Ring events against ring extremes and whole-block reads",
            "",
            f"{a.box[0].upper() + a.box[1:]}, f64, RK4, {BATCH} ticks per launch, ring of {READ_TICKS:,} ticks.  One trigger, world_pos z <= 0 as a crossing,",
            "capturing world_pos and world_vel; the yardstick is history_extremes over world_pos alone, which reads the same cache lines once.",
            f"tools/history_events_ab.py: every leg in a child process of its own, {a.rounds} rounds of alternating legs, a warm-up and then",
            f"{a.windows} timed windows per child, a window being {REPS[SIZES[0]]} calls behind one another at 65,536 bodies and {REPS[SIZES[1]]} at 1,024, each ending in a",
            "stream synchronise; events and extremes alternate inside one child.  Per call: median, and [min .. max], over all windows.",
            "Nothing here is a gate.",
            ""]
    if a.registers:
        rows += [f"Registers, as the compiler reports them for gfx950 (no spills, no scratch): {a.registers}.", ""]
    for n in SIZES:
        both, blocks, seg = f"read n={n}: events and extremes", f"read n={n}: history + numpy", f"read n={n}: segments"
        m = meta[both]
        rows += [f"## Read-back at {n:,} bodies: {READ_TICKS:,} ticks",
                 "",
                 f"{m['fired'] * 100:.1f} % of the runs have an event in the range, at tick {m['median_tick']:,.0f} in the median; the others are walked to the end.",
                 "",
                 "| path | bytes to the host | time per call |",
                 "|---|---|---|",
                 f"| history_events, delivered | {m['bytes_events'] / 1e6:,.2f} MB | {ms(both, 'events')} |",
                 f"| history_events, reduced only (HOLD, synchronise) | 0 | {ms(both, 'events_held')} |",
                 f"| history_extremes of world_pos, delivered | {m['bytes_extremes'] / 1e6:,.2f} MB | {ms(both, 'extremes')} |",
                 f"| history_extremes of world_pos, reduced only | 0 | {ms(both, 'extremes_held')} |",
                 f"| history + numpy (timed on {HOST_TICKS} ticks, scaled by {READ_TICKS // HOST_TICKS}) | {meta[blocks]['bytes'] / 1e6:,.0f} MB | {ms(blocks)} |",
                 "",
                 f"Of the host route {med(blocks, 'numpy_seconds'):,.2f} s is numpy, the rest is reading the blocks.  history_events delivered is "
                 f"{med(blocks, 'seconds') / med(both, 'events'):,.0f} times faster than the host route; reduced only it takes "
                 f"{med(both, 'events_held') / med(both, 'extremes_held'):,.2f} of the time of the extremes of world_pos.",
                 "",
                 f"### Time segments at {n:,} bodies (reduced only)",
                 "",
                 "| SIXDOF_EVENTS_SEGMENTS | time per call |",
                 "|---|---|"]
        for s in SEGMENTS:
            rows.append(f"| {'0 (the plan)' if s == '0' else s} | {ms(seg, s)} |")
        rows.append("")
    rows += [f"## Streaming at {SIZES[0]:,} bodies: {a.batches:,} batches of {BATCH} ticks per window",
             "",
             "| path | bytes to the host at the end | entity-steps/s (wall time of the window) |",
             "|---|---|---|"]
    for name in LEGS:
        if name.startswith("stream"):
            v = pooled[name]["entity_steps_per_s"]
            rows.append(f"| {name[8:]} | {meta[name]['bytes_at_the_end'] / 1e6:,.2f} MB | {statistics.median(v):.3e} [{min(v):.3e} .. {max(v):.3e}] |")
    rec = med("stream: record only", "entity_steps_per_s")
    rel = lambda name: med(name, "entity_steps_per_s") / rec
    rows += ["",
             f"Relative to recording with nothing read back: stream_events every=1 {rel('stream: stream_events every=1'):.2f}, every=8 "
             f"{rel('stream: stream_events every=8'):.2f}; stream_extremes of world_pos every=1 {rel('stream: stream_extremes every=1'):.2f}, every=8 "
             f"{rel('stream: stream_extremes every=8'):.2f}.",
             ""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(rows))
    print("\n".join(rows))


if __name__ == "__main__":
    main()
