#!/usr/bin/env python3
"""Ring dwell against ring norms and against whole-block reads plus numpy, on one GPU, f64, at 65,536 runs and at 1,024
(profiles/history_dwell.md).  A run is two rows (period 2); ring of 1,024 ticks.  Two conditions, each read alone: the speed |v| of
a run's row 0 at or above a level (3 loads per sample) and the separation |r_0 - r_1| of its two rows at or above one (6 loads per
sample); each level is the median over the runs of the middle between the smallest and the largest norm of the range, so that
runs hold for a part of it.

  read-back   one HipExec.history_dwell over the 1,024 ticks — delivered, and reduced only (SIXDOF_DWELL_HOLD, then a synchronise)
              — beside HipExec.history_norms of the same probe IN THE SAME CHILD, windows alternating: that walk makes the same
              loads and carries a 6-field record against the 12 fields here, and is the yardstick (the reduce-only dwell read
              appears twice: two rows of identical code, whose spread is the margin of the ratio); and beside the host route,
              HipExec.history of the blocks + numpy, timed on 32 ticks and scaled to 1,024.
  segments    the reduce-only |v| read under the plan's own time segments and under 1 .. 32 forced ones (SIXDOF_DWELL_SEGMENTS, read
              at every call: the settings alternate inside one child).  What dwell_plan.hpp's kDwellFillThreads is chosen from.
  streaming   entity-steps/s of the stepper at 65,536 runs while both conditions accumulate on the device: stream_dwell in 64-tick
              batches at every 1 and 8, against recording only.

Every leg runs in a child process of its own, under its own time limit, several windows per child after a warm-up; a window is
`reps` calls behind one another, each ending in a stream synchronise.  The legs alternate over `--rounds` rounds and a failed
child ends the run.

    python tools/history_dwell_ab.py [--out profiles/history_dwell.md]
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

RUNS = (65536, 1024)
PERIOD = 2
READ_TICKS = 1024
HOST_TICKS = 32                          # the host route is timed on this many ticks and scaled
BATCH = 64
SEGMENTS = ("0", "1", "2", "4", "8", "16", "32")     # 0: the plan's choice
REPS = {65536: 10, 1024: 100}            # calls per window
PROBES = ("speed", "separation")


def _norm(which):
    import elodin_amd as ea
    return ea.Norm("world_vel", 3, 3) if which == "speed" else ea.Norm("world_pos", 4, 3, group=0, minus="world_pos", minus_group=1)


def _level(ex, which, last=READ_TICKS):
    """The median over the runs of the middle between the smallest and the largest norm of ticks 1 .. last."""
    import numpy as np
    got = ex.history_norms(_norm(which), 1, last, period=PERIOD)
    return float(np.median(0.5 * (got["min"] + got["max"])))


def _dwell(which, level):
    import elodin_amd as ea
    return ea.Dwell(_norm(which), ">=", level)


def _exec(runs, ticks_per_launch):
    import elodin_amd as ea
    from elodin_amd import workloads
    w = workloads.independent_bodies(runs * PERIOD)
    eff = workloads.gravity_torque_effectors(w["body_torque"])
    return ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], entity_ids=w["entity_ids"], simulation_time_step=workloads.DT_120HZ,
                      effectors=eff, ticks_per_launch=ticks_per_launch)


def _recorded(runs):
    ex = _exec(runs, BATCH)
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


def _held(ex, scan, items, hold_flag):
    """One reduce-only read of the whole ring: nothing is delivered, the call is waited for."""
    def call():
        ex._scan_read(scan, items, None, PERIOD, 1, READ_TICKS, 1, None, None, hold_flag)
        ex.sync()
    return call


def leg_read(windows, runs):
    from elodin_amd import _lib as L
    ex = _recorded(runs)
    calls, shares = {}, {}
    for which in PROBES:
        level = _level(ex, which)
        got = ex.history_dwell(_dwell(which, level), 1, READ_TICKS, period=PERIOD)
        assert got["held"].shape == (1, runs) and (got["count"] == READ_TICKS).all()
        shares[which] = {"fraction": float(got["fraction"].mean()), "runs_that_toggle": float(((got["held"] > 0) & (got["held"] < READ_TICKS)).mean())}
        calls[which] = lambda which=which, level=level: ex.history_dwell(_dwell(which, level), 1, READ_TICKS, period=PERIOD)
        calls[which + "_held"] = _held(ex, ex._DWELL_SCAN, ex._dwell_conditions(_dwell(which, level)), L.DWELL_HOLD)
        calls[which + "_held_again"] = _held(ex, ex._DWELL_SCAN, ex._dwell_conditions(_dwell(which, level)), L.DWELL_HOLD)
        calls[which + "_norms_held"] = _held(ex, ex._NORMS_SCAN, ex._norm_probes(_norm(which)), L.NORMS_HOLD)
    out = {k: [] for k in calls}
    for k, call in calls.items():                        # every path once before anything is timed
        call()
    for _ in range(windows):                             # the paths alternate inside the child
        for k, call in calls.items():
            out[k] += _windows(1, REPS[runs], call)
    return {"series": out, "bytes_dwell": 12 * runs * 8, "shares": shares}


def leg_read_blocks(windows, runs):
    import numpy as np
    ex = _exec(runs, BATCH)
    ex.enable_history(BATCH)
    ex.invoke_batch(BATCH)
    ex.history("world_pos", 1, 8)
    levels = {which: _level(ex, which, HOST_TICKS) for which in PROBES}
    out = {"speed": [], "separation": [], "speed_numpy": [], "separation_numpy": []}
    scale = READ_TICKS / HOST_TICKS
    for _ in range(windows):
        for which in PROBES:
            t0 = time.perf_counter()
            if which == "speed":
                d = ex.history("world_vel", 1, HOST_TICKS)[:, 0::PERIOD, 3:6]      # a synchronise per tick inside
            else:
                pos = ex.history("world_pos", 1, HOST_TICKS)
                d = pos[:, 0::PERIOD, 4:7] - pos[:, 1::PERIOD, 4:7]
            t1 = time.perf_counter()
            s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            h = s >= levels[which] * levels[which]                                # every element is finite here
            opens = np.concatenate([h[:1], h[1:] & ~h[:-1]])
            run_length = np.zeros(h.shape[1], dtype=np.int64)
            longest = np.zeros(h.shape[1], dtype=np.int64)
            for row in h:                                                         # the stretches: one pass over the ticks
                run_length = np.where(row, run_length + 1, 0)
                longest = np.maximum(longest, run_length)
            res = (h.sum(axis=0), opens.sum(axis=0), h.argmax(axis=0) + 1, longest, h[0], h[-1])
            spent = time.perf_counter() - t1
            del d, s, h, res
            out[which].append((time.perf_counter() - t0) * scale)
            out[which + "_numpy"].append(spent * scale)
    return {"series": out, "bytes_speed": runs * PERIOD * READ_TICKS * 6 * 8, "bytes_separation": runs * PERIOD * READ_TICKS * 7 * 8}


def leg_segments(windows, runs):
    from elodin_amd import _lib as L
    ex = _recorded(runs)
    call = _held(ex, ex._DWELL_SCAN, ex._dwell_conditions(_dwell("speed", _level(ex, "speed"))), L.DWELL_HOLD)
    out = {s: [] for s in SEGMENTS}
    for s in SEGMENTS:                                   # every setting once before anything is timed
        os.environ["SIXDOF_DWELL_SEGMENTS"] = s
        call()
    for _ in range(windows):
        for s in SEGMENTS:
            os.environ["SIXDOF_DWELL_SEGMENTS"] = s
            out[s] += _windows(1, REPS[runs], call)
    return {"series": out}


def _rate(n, wall, batches):
    return n * BATCH * batches / wall


def leg_stream_dwell(windows, batches, every):
    runs = RUNS[0]
    ex = _exec(runs, BATCH)
    conditions = [_dwell("speed", 5.0), _dwell("separation", 100.0)]         # the levels do not change what a thread does per sample
    ex.stream_dwell(conditions, 4, BATCH, every=every, period=PERIOD)
    return {"series": {"entity_steps_per_s": [_rate(runs * PERIOD, ex.stream_dwell(conditions, batches, BATCH, every=every, period=PERIOD)[0], batches)
                                              for _ in range(windows)]},
            "bytes_at_the_end": 2 * 12 * runs * 8}


def leg_record_only(windows, batches):
    from elodin_amd import _lib as L
    runs = RUNS[0]
    ex = _exec(runs, BATCH)
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
        out.append(_rate(runs * PERIOD, time.perf_counter() - t0, batches))
        ex.set_flags(0)
    return {"series": {"entity_steps_per_s": out}, "bytes_at_the_end": 0}


LEGS = {}       # name: (function, extra arguments, time limit of one child in seconds)
for _runs in RUNS:
    LEGS[f"read runs={_runs}: dwell and norms"] = (leg_read, (_runs,), 300)
    LEGS[f"read runs={_runs}: history + numpy"] = (leg_read_blocks, (_runs,), 300)
    LEGS[f"read runs={_runs}: segments"] = (leg_segments, (_runs,), 300)
LEGS.update({
    "stream: stream_dwell every=1": (leg_stream_dwell, (1,), 240),
    "stream: stream_dwell every=8": (leg_stream_dwell, (8,), 240),
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "history_dwell.md"))
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
            env.pop("SIXDOF_DWELL_SEGMENTS", None)
            env.pop("SIXDOF_NORMS_SEGMENTS", None)
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

    def ms(name, key):
        v = pooled[name][key]
        return f"{statistics.median(v) * 1e3:,.3f} ms [{min(v) * 1e3:,.3f} .. {max(v) * 1e3:,.3f}]"
    rows = ["# Ring dwell against ring norms and whole-block reads",
            "",
            f"{a.box[0].upper() + a.box[1:]}, f64, RK4, {BATCH} ticks per launch, ring of {READ_TICKS:,} ticks, runs of {PERIOD} rows.  Two conditions, each read alone: the speed |v| of",
            "a run's row 0 at or above a level (3 loads per sample) and the separation |r_0 - r_1| of its two rows at or above one (6 loads per",
            "sample), each level the median over the runs of the middle between the smallest and the largest norm of the range.  The yardstick is",
            "history_norms of the same probe: the same loads, a 6-field record against the 12 fields here.",
            f"tools/history_dwell_ab.py: every leg in a child process of its own, {a.rounds} rounds of alternating legs, a warm-up and then",
            f"{a.windows} timed windows per child, a window being {REPS[RUNS[0]]} calls behind one another at 65,536 runs and {REPS[RUNS[1]]} at 1,024, each ending in a",
            "stream synchronise; the paths alternate inside one child.  Per call: median, and [min .. max], over all windows.  The",
            "reduce-only dwell read appears twice: two rows of identical code, whose spread is the margin of every ratio below.",
            "Nothing here is a gate.",
            ""]
    if a.registers:
        rows += [f"Registers, as the compiler reports them for gfx950 (no spills, no scratch): {a.registers}.", ""]
    for runs in RUNS:
        both, blocks, seg = f"read runs={runs}: dwell and norms", f"read runs={runs}: history + numpy", f"read runs={runs}: segments"
        rows += [f"## Read-back at {runs:,} runs ({runs * PERIOD:,} rows): {READ_TICKS:,} ticks",
                 "",
                 "| path | bytes to the host | time per call |",
                 "|---|---|---|"]
        for which in PROBES:
            share = meta[both]["shares"][which]
            rows += [f"| history_dwell {which}, delivered | {meta[both]['bytes_dwell'] / 1e6:,.2f} MB | {ms(both, which)} |",
                     f"| history_dwell {which}, reduced only (HOLD, synchronise); held {share['fraction']:.0%} of the samples, {share['runs_that_toggle']:.0%} of the runs toggle | 0 | {ms(both, which + '_held')} |",
                     f"| the same again (identical code) | 0 | {ms(both, which + '_held_again')} |",
                     f"| history_norms {which}, reduced only | 0 | {ms(both, which + '_norms_held')} |",
                     f"| history + numpy {which} (timed on {HOST_TICKS} ticks, scaled by {READ_TICKS // HOST_TICKS}) | {meta[blocks]['bytes_' + which] / 1e6:,.0f} MB | {ms(blocks, which)} |"]
        rows += [""]
        for which in PROBES:
            twin = abs(med(both, which + "_held_again") / med(both, which + "_held") - 1.0)
            rows += [f"{which}: reduced only {med(both, which + '_held') / med(both, which + '_norms_held'):,.3f} of the time of the norms walk (identical rows differ by {twin:.1%}); "
                     f"delivered {med(blocks, which) / med(both, which):,.0f} times faster than the host route, of which {med(blocks, which + '_numpy'):,.2f} s is numpy."]
        rows += ["",
                 f"### Time segments at {runs:,} runs (|v|, reduced only)",
                 "",
                 "| SIXDOF_DWELL_SEGMENTS | time per call |",
                 "|---|---|"]
        for s in SEGMENTS:
            rows.append(f"| {'0 (the plan)' if s == '0' else s} | {ms(seg, s)} |")
        rows.append("")
    rows += [f"## Streaming at {RUNS[0]:,} runs ({RUNS[0] * PERIOD:,} rows), both conditions: {a.batches:,} batches of {BATCH} ticks per window",
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
             f"Relative to recording with nothing read back: stream_dwell every=1 {rel('stream: stream_dwell every=1'):.2f}, every=8 "
             f"{rel('stream: stream_dwell every=8'):.2f}.",
             ""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(rows))
    print("\n".join(rows))


if __name__ == "__main__":
    main()
