#!/usr/bin/env python3
"""Ring covariances against ring envelopes and against whole-block reads plus numpy, on one GPU, f64, at 65,536 bodies and at
1,024 (profiles/history_covariance.md).  Ring of 1,024 ticks; the channel lists are the six of world_pos[4:7] + world_vel[3:6] and
the two of world_pos[4:6].

  read-back   one HipExec.history_covariance over the 1,024 ticks for each list, beside HipExec.history_envelope over the same
              components IN THE SAME CHILD, windows alternating.  The envelope touches every line of the two components' tick
              blocks once — the covariance's floor — and is in the rotation TWICE: the gap between its two rows is the spread two
              rows of identical code show in this job.  Every call is blocking: it ends with its (small) output on the host.  Beside
              them the host route, HipExec.history of the blocks + numpy for the same matrices, timed on 32 ticks and scaled.
  geometry    the six-channel read under other threads-per-block x block-cap choices: libraries built by
              `make -C elodin_amd/csrc cov_variant COV_THREADS=.. COV_BLOCKS=..`, each loaded by a child through SIXDOF_LIBRARY, the
              cells alternating over the rounds.  What covariance_plan.hpp's kCovarianceThreads and kCovarianceMaxBlocks are chosen
              from.  Cells whose library has not been built are left out.
  streaming   entity-steps/s of the stepper at 65,536 bodies while the six-channel covariance of every tick, or of every eighth, is
              read back: stream_covariance in 64-tick batches, against recording only.

Every leg runs in a child process of its own, under its own time limit, several windows per child after a warm-up; a window is
`reps` calls behind one another.  The legs alternate over `--rounds` rounds and a failed child ends the run.

    python tools/history_covariance_ab.py [--out profiles/history_covariance.md]
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
SIX = [("world_pos", 4), ("world_pos", 5), ("world_pos", 6), ("world_vel", 3), ("world_vel", 4), ("world_vel", 5)]
TWO = [("world_pos", 4), ("world_pos", 5)]
COMPONENTS = ("world_pos", "world_vel")
READ_TICKS = 1024
HOST_TICKS = 32                          # the host route is timed on this many ticks and scaled
BATCH = 64
REPS = {65536: 10, 1024: 100}            # calls per window
GEOMETRY = [(128, 32), (128, 128), (256, 4), (256, 8), (256, 16), (256, 32), (256, 128), (512, 32), (512, 128)]      # threads of a stage-1 block x cap on blocks per sample
DEFAULT_GEOMETRY = (256, 8)              # covariance_plan.hpp: kCovarianceThreads, kCovarianceMaxBlocks


def _variant(threads, blocks):
    return ROOT / "elodin_amd" / f"libsixdof_hip_cov_{threads}_{blocks}.so"


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


def leg_read(windows, n):
    ex = _recorded(n)
    got = ex.history_covariance(SIX, 1, READ_TICKS)
    assert got["comoment"].shape == (READ_TICKS, 1, 6, 6) and (got["count"] == n).all()
    calls = {"envelope_a": lambda: ex.history_envelope(COMPONENTS, 1, READ_TICKS), "covariance_6": lambda: ex.history_covariance(SIX, 1, READ_TICKS),
             "covariance_2": lambda: ex.history_covariance(TWO, 1, READ_TICKS), "envelope_b": lambda: ex.history_envelope(COMPONENTS, 1, READ_TICKS),
             "envelope_pos": lambda: ex.history_envelope(COMPONENTS[:1], 1, READ_TICKS)}
    out = {k: [] for k in calls}
    for call in calls.values():                          # every path once before anything is timed
        call()
    for _ in range(windows):                             # the paths alternate inside the child
        for k, call in calls.items():
            out[k] += _windows(1, REPS[n], call)
    return {"series": out, "bytes_6": READ_TICKS * 28 * 8, "bytes_2": READ_TICKS * 6 * 8, "bytes_envelope": READ_TICKS * 5 * 13 * 8,
            "ring_bytes": READ_TICKS * n * 13 * 8}


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
        x = np.concatenate([pos[:, :, 4:7], vel[:, :, 3:6]], axis=2)          # every element is finite here
        res = [np.cov(x[t], rowvar=False, bias=True) for t in range(HOST_TICKS)]
        mean = x.mean(axis=1)
        spent = time.perf_counter() - t1
        del pos, vel, x, res, mean
        scale = READ_TICKS / HOST_TICKS
        out.append((time.perf_counter() - t0) * scale)
        numpy_s.append(spent * scale)
    return {"series": {"seconds": out, "numpy_seconds": numpy_s}, "bytes": n * READ_TICKS * 13 * 8}


def leg_geometry(windows, n):
    """The six-channel read with whatever library SIXDOF_LIBRARY names (the parent sets it per cell)."""
    ex = _recorded(n)
    return {"series": {"seconds": _windows(windows, REPS[n], lambda: ex.history_covariance(SIX, 1, READ_TICKS))}}


def _rate(n, wall, batches):
    return n * BATCH * batches / wall


def leg_stream_covariance(windows, batches, every):
    n = SIZES[0]
    ex = _exec(n, BATCH)
    ex.stream_covariance(SIX, 4, BATCH, every=every)
    return {"series": {"entity_steps_per_s": [_rate(n, ex.stream_covariance(SIX, batches, BATCH, every=every), batches) for _ in range(windows)]},
            "bytes_per_batch": BATCH // every * 28 * 8}


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
    return {"series": {"entity_steps_per_s": out}, "bytes_per_batch": 0}


LEGS = {}       # name: (function, extra arguments, time limit of one child in seconds, SIXDOF_LIBRARY or None)
for _n in SIZES:
    LEGS[f"read n={_n}: covariance and envelope"] = (leg_read, (_n,), 300, None)
    LEGS[f"read n={_n}: history + numpy"] = (leg_read_blocks, (_n,), 300, None)
    for _t, _b in GEOMETRY:
        if (_t, _b) == DEFAULT_GEOMETRY or _variant(_t, _b).exists():
            LEGS[f"read n={_n}: geometry {_t} x {_b}"] = (leg_geometry, (_n,), 300, None if (_t, _b) == DEFAULT_GEOMETRY else str(_variant(_t, _b)))
LEGS.update({
    "stream: stream_covariance every=1": (leg_stream_covariance, (1,), 240, None),
    "stream: stream_covariance every=8": (leg_stream_covariance, (8,), 240, None),
    "stream: record only": (leg_record_only, (), 240, None),
})


def run_leg(name, windows, batches):
    fn, extra, _, _ = LEGS[name]
    res = fn(windows, *extra) if name.startswith("read") else fn(windows, batches, *extra)
    print("LEG_RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", help="(internal) run one leg in this process")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--windows", type=int, default=3, help="timed windows per child")
    ap.add_argument("--batches", type=int, default=64, help="64-tick batches per streaming window")
    ap.add_argument("--box", default="one MI355X", help="how the note names the machine")
    ap.add_argument("--registers", default="", help="the kernels' resource usage, as the compiler reports it, for the note")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "history_covariance.md"))
    a = ap.parse_args()
    if a.leg:
        run_leg(a.leg, a.windows, a.batches)
        return
    pooled = {name: {} for name in LEGS}       # name -> series -> values
    meta = {}
    for rnd in range(a.rounds):
        for name, (_, _, limit, library) in LEGS.items():
            windows = 1 if "numpy" in name else a.windows
            cmd = [sys.executable, str(Path(__file__).resolve()), "--leg", name, "--windows", str(windows), "--batches", str(a.batches)]
            env = dict(os.environ)
            env.pop("SIXDOF_COVARIANCE_CHUNK", None)
            env.pop("SIXDOF_LIBRARY", None)
            if library:
                env["SIXDOF_LIBRARY"] = library
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
    rows = ["# Ring covariances against ring envelopes and whole-block reads",
            "",
            f"{a.box[0].upper() + a.box[1:]}, f64, RK4, {BATCH} ticks per launch, ring of {READ_TICKS:,} ticks.  Six channels: world_pos[4:7] + world_vel[3:6]; two:",
            "world_pos[4:6].  The yardstick is history_envelope over world_pos and world_vel, which reads every line of the two components' tick",
            "blocks once; it is in the rotation twice (a, b), and the gap between its two rows is the spread of identical code in this job.",
            f"tools/history_covariance_ab.py: every leg in a child process of its own, {a.rounds} rounds of alternating legs, a warm-up and then",
            f"{a.windows} timed windows per child, a window being {REPS[SIZES[0]]} blocking calls behind one another at 65,536 bodies and {REPS[SIZES[1]]} at 1,024;",
            "covariances and envelopes alternate inside one child.  Per call: median, and [min .. max], over all windows.  Nothing here is a gate.",
            ""]
    if a.registers:
        rows += [f"Resources, as the compiler reports them for gfx950 (no spills, no scratch): {a.registers}.", ""]
    for n in SIZES:
        both, blocks = f"read n={n}: covariance and envelope", f"read n={n}: history + numpy"
        m = meta[both]
        env = statistics.median(pooled[both]["envelope_a"] + pooled[both]["envelope_b"])
        spread = abs(med(both, "envelope_a") - med(both, "envelope_b")) / env
        rows += [f"## Read-back at {n:,} bodies: {READ_TICKS:,} ticks",
                 "",
                 f"The two components' tick blocks are {m['ring_bytes'] / 1e6:,.0f} MB of the ring.",
                 "",
                 "| path | bytes to the host | time per call |",
                 "|---|---|---|",
                 f"| history_covariance, 6 channels | {m['bytes_6'] / 1e6:,.2f} MB | {ms(both, 'covariance_6')} |",
                 f"| history_covariance, 2 channels | {m['bytes_2'] / 1e6:,.2f} MB | {ms(both, 'covariance_2')} |",
                 f"| history_envelope of world_pos + world_vel (a) | {m['bytes_envelope'] / 1e6:,.2f} MB | {ms(both, 'envelope_a')} |",
                 f"| history_envelope of world_pos + world_vel (b) | {m['bytes_envelope'] / 1e6:,.2f} MB | {ms(both, 'envelope_b')} |",
                 f"| history_envelope of world_pos alone | {m['bytes_envelope'] * 7 / 13 / 1e6:,.2f} MB | {ms(both, 'envelope_pos')} |",
                 f"| history + numpy (timed on {HOST_TICKS} ticks, scaled by {READ_TICKS // HOST_TICKS}) | {meta[blocks]['bytes'] / 1e6:,.0f} MB | {ms(blocks)} |",
                 "",
                 f"The two envelope rows differ by {spread * 100:.1f} % of their median.  The six-channel covariance takes {med(both, 'covariance_6') / env:,.2f} of the envelope's",
                 f"time over the same two components, the two-channel one {med(both, 'covariance_2') / med(both, 'envelope_pos'):,.2f} of the envelope's over world_pos alone.  Of the host",
                 f"route {med(blocks, 'numpy_seconds'):,.2f} s is numpy, the rest is reading the blocks; history_covariance delivers the same matrices",
                 f"{med(blocks, 'seconds') / med(both, 'covariance_6'):,.0f} times faster.",
                 "",
                 f"### Threads of a stage-1 block x cap on blocks per sample at {n:,} bodies (six channels)",
                 "",
                 "| threads x cap | time per call |",
                 "|---|---|"]
        for t, b in GEOMETRY:
            name = f"read n={n}: geometry {t} x {b}"
            if name in LEGS:
                rows.append(f"| {t} x {b}{' (the plan)' if (t, b) == DEFAULT_GEOMETRY else ''} | {ms(name)} |")
        rows.append("")
    rows += [f"## Streaming at {SIZES[0]:,} bodies: {a.batches:,} batches of {BATCH} ticks per window",
             "",
             "| path | bytes to the host per batch | entity-steps/s (wall time of the window) |",
             "|---|---|---|"]
    for name in LEGS:
        if name.startswith("stream"):
            v = pooled[name]["entity_steps_per_s"]
            rows.append(f"| {name[8:]} | {meta[name]['bytes_per_batch'] / 1e3:,.1f} KB | {statistics.median(v):.3e} [{min(v):.3e} .. {max(v):.3e}] |")
    rec = med("stream: record only", "entity_steps_per_s")
    rel = lambda name: med(name, "entity_steps_per_s") / rec
    rows += ["",
             f"Relative to recording with nothing read back: stream_covariance every=1 {rel('stream: stream_covariance every=1'):.2f}, every=8 "
             f"{rel('stream: stream_covariance every=8'):.2f}.",
             ""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(rows))
    print("\n".join(rows))


if __name__ == "__main__":
    main()
