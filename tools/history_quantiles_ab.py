#!/usr/bin/env python3
"""Ring quantiles against ring envelopes and against whole-block reads plus numpy.sort, on one GPU at 65,536 bodies f64
(profiles/history_quantiles.md).  Ranks 1/100, 25/100, 50/100, 75/100, 99/100 of the four recorded columns, ring of 1,024 ticks.

  read-back   one HipExec.history_quantiles over the 1,024 ticks (period 1 and 64), beside one HipExec.history_envelope over the
              same range — the radix select reads a tick's block passes + 1 = 9 times, the envelope once — and beside the host
              route: HipExec.history + numpy.sort + integer indexing, timed on 32 ticks and scaled to 1,024.
  contention  the same read with the wave's equal (histogram, digit) addresses combined before the LDS atomic in up to 8 rounds
              (the default), in up to 64, and not at all (SIXDOF_QUANTILE_ROUNDS).
  streaming   entity-steps/s of the stepper while quantiles leave the device: stream_quantiles in 64-tick batches at every 1
              and 8 against recording only on the same handle.

Every leg runs in a child process of its own, under its own time limit, several windows per child after a warm-up; the legs
alternate over `--rounds` rounds and a failed child ends the run.

    python tools/history_quantiles_ab.py [--out profiles/history_quantiles.md]
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

N = 65536
FIELDS = ("world_pos", "world_vel", "world_accel", "force")
Q = [(1, 100), (25, 100), (50, 100), (75, 100), (99, 100)]
READ_TICKS = 1024
HOST_TICKS = 32                          # the host route is timed on this many ticks and scaled
BATCH = 64
ROW_BYTES = (7 + 6 + 6 + 6) * 8          # the four recorded columns of one body, f64
READS = 9                                # of a tick's block: 8 digit passes and the closing one for x(hi)


def _exec(ticks_per_launch):
    import elodin_amd as ea
    from elodin_amd import workloads
    w = workloads.independent_bodies(N)
    eff = workloads.gravity_torque_effectors(w["body_torque"])
    return ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], entity_ids=w["entity_ids"], simulation_time_step=workloads.DT_120HZ,
                      effectors=eff, ticks_per_launch=ticks_per_launch)


def _recorded():
    ex = _exec(BATCH)
    ex.enable_history(READ_TICKS)
    ex.invoke_batch(READ_TICKS)
    return ex


def leg_read_quantiles(windows, period):
    ex = _recorded()
    for _ in range(2):
        ex.history_quantiles(FIELDS, 1, READ_TICKS, Q, period=period)
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        got = ex.history_quantiles(FIELDS, 1, READ_TICKS, Q, period=period)      # returns after a stream synchronise
        out.append(time.perf_counter() - t0)
    assert got["world_pos"]["lower"].shape == (READ_TICKS, period, len(Q), 7) and int(got["force"]["count"].min()) == N // period
    return {"seconds": out, "bytes": READ_TICKS * period * (1 + 2 * len(Q)) * 25 * 8}


def leg_read_envelope(windows, period):
    ex = _recorded()
    for _ in range(2):
        ex.history_envelope(FIELDS, 1, READ_TICKS, period=period)
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        ex.history_envelope(FIELDS, 1, READ_TICKS, period=period)
        out.append(time.perf_counter() - t0)
    return {"seconds": out, "bytes": READ_TICKS * period * 5 * 25 * 8}


def leg_read_blocks(windows):
    import numpy as np
    ex = _exec(BATCH)
    ex.enable_history(BATCH)
    ex.invoke_batch(BATCH)
    ex.history("force", 1, 8)
    out, sort_s = [], []
    for _ in range(windows):
        t0 = time.perf_counter()
        spent = 0.0
        for name in FIELDS:                              # a synchronise per tick inside
            block = ex.history(name, 1, HOST_TICKS)
            t1 = time.perf_counter()
            v = np.sort(block, axis=1)                   # every row is finite here: NaN would sort last and count would cut it off
            m = v.shape[1]
            lower = np.stack([v[:, num * (m - 1) // den] for num, den in Q], axis=1)
            upper = np.stack([v[:, -(-num * (m - 1) // den)] for num, den in Q], axis=1)
            spent += time.perf_counter() - t1
            del block, v, lower, upper
        scale = READ_TICKS / HOST_TICKS
        out.append((time.perf_counter() - t0) * scale)
        sort_s.append(spent * scale)
    return {"seconds": out, "sort_seconds": sort_s, "bytes": N * READ_TICKS * ROW_BYTES}


def _rate(wall, batches):
    return N * BATCH * batches / wall


def leg_stream_quantiles(windows, batches, every):
    ex = _exec(BATCH)
    ex.stream_quantiles(FIELDS, 4, BATCH, Q, every=every)
    return {"entity_steps_per_s": [_rate(ex.stream_quantiles(FIELDS, batches, BATCH, Q, every=every), batches) for _ in range(windows)],
            "bytes_per_batch": (BATCH // every) * (1 + 2 * len(Q)) * 25 * 8}


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
    # name: (function, extra arguments, time limit of one child in seconds, SIXDOF_QUANTILE_ROUNDS of the child)
    "read: history_quantiles": (leg_read_quantiles, (1,), 300, None),
    "read: history_quantiles period=64": (leg_read_quantiles, (64,), 300, None),
    "read: history_envelope": (leg_read_envelope, (1,), 240, None),
    "read: history_envelope period=64": (leg_read_envelope, (64,), 240, None),
    "read: history + numpy.sort": (leg_read_blocks, (), 600, None),
    "read: history_quantiles, every lane its own atomic": (leg_read_quantiles, (1,), 300, "0"),
    "read: history_quantiles period=64, every lane its own atomic": (leg_read_quantiles, (64,), 300, "0"),
    "read: history_quantiles, every address once": (leg_read_quantiles, (1,), 300, "64"),
    "read: history_quantiles period=64, every address once": (leg_read_quantiles, (64,), 300, "64"),
    "stream: stream_quantiles every=1": (leg_stream_quantiles, (1,), 300, None),
    "stream: stream_quantiles every=8": (leg_stream_quantiles, (8,), 300, None),
    "stream: record only": (leg_record_only, (), 240, None),
}


def run_leg(name, windows, batches):
    fn, extra, _, _ = LEGS[name]
    res = fn(windows, *extra) if name.startswith("read") else fn(windows, batches, *extra)
    print("LEG_RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", help="(internal) run one leg in this process")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--windows", type=int, default=3, help="timed windows per child")
    ap.add_argument("--batches", type=int, default=64, help="64-tick batches per streaming window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "history_quantiles.md"))
    a = ap.parse_args()
    if a.leg:
        run_leg(a.leg, a.windows, a.batches)
        return
    pooled = {name: [] for name in LEGS}
    meta = {}
    for rnd in range(a.rounds):
        for name, (_, _, limit, rounds_env) in LEGS.items():
            windows = 1 if "numpy" in name else a.windows
            cmd = [sys.executable, str(Path(__file__).resolve()), "--leg", name, "--windows", str(windows), "--batches", str(a.batches)]
            env = dict(os.environ)
            env.pop("SIXDOF_QUANTILE_ROUNDS", None)
            if rounds_env is not None:
                env["SIXDOF_QUANTILE_ROUNDS"] = rounds_env
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=env)
            except subprocess.TimeoutExpired:
                sys.exit(f"{name}: no result within {limit} s; nothing more is started")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG_RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit(f"{name}: child failed (status {p.returncode}); nothing more is started\n{p.stdout[-1500:]}\n{p.stderr[-3000:]}")
            res = json.loads(line[-1][len("LEG_RESULT "):])
            pooled[name] += res.get("seconds") or res["entity_steps_per_s"]
            meta.setdefault(name, {}).update({k: v for k, v in res.items() if k != "sort_seconds"})
            meta[name].setdefault("sort_seconds", []).extend(res.get("sort_seconds", []))
            print(f"round {rnd} {name}: {pooled[name][-windows:]}", flush=True)
    med = {name: statistics.median(v) for name, v in pooled.items()}
    ms = lambda name: f"{med[name] * 1e3:,.1f} ms [{min(pooled[name]) * 1e3:,.1f} .. {max(pooled[name]) * 1e3:,.1f}]"
    rows = ["# Ring quantiles against ring envelopes and whole-block reads",
            "",
            f"One MI355X, {N:,} bodies, f64, RK4, {BATCH} ticks per launch, ring of {READ_TICKS:,} ticks, ranks 1/100 25/100 50/100 75/100 99/100 of the",
            f"four recorded columns.  tools/history_quantiles_ab.py: every leg in a child process of its own, {a.rounds} rounds of alternating legs, a",
            f"warm-up and then {a.windows} timed windows per child; median, and [min .. max], over all windows.",
            "",
            f"## Read-back: {READ_TICKS:,} ticks of the four recorded columns",
            "",
            "| path | bytes to the host | time (host clock around a call that ends in a stream synchronise) |",
            "|---|---|---|"]
    for name in list(LEGS)[:5]:
        rows.append(f"| {name[6:]} | {meta[name]['bytes'] / 1e6:,.1f} MB | {ms(name)} |")
    blocks = "read: history + numpy.sort"
    sort_med = statistics.median(meta[blocks]["sort_seconds"])
    rows += ["",
             f"The host route was timed on {HOST_TICKS} ticks and scaled by {READ_TICKS // HOST_TICKS} to the {READ_TICKS:,}: {sort_med:,.1f} s of it is numpy.sort and the",
             f"indexing, {med[blocks] - sort_med:,.1f} s is reading the blocks.  history_quantiles is {med[blocks] / med['read: history_quantiles']:,.0f} times faster than the",
             f"host route at period 1 and {med[blocks] / med['read: history_quantiles period=64']:,.0f} times at period 64 (the host figure is that of period 1: its sort does not care).",
             "",
             f"The select reads a tick's block {READS} times (8 digit passes and the closing one for x(hi)), the envelope once:",
             "",
             "| period | history_quantiles / history_envelope | per read of the ring |",
             "|---|---|---|"]
    for suffix in ("", " period=64"):
        ratio = med["read: history_quantiles" + suffix] / med["read: history_envelope" + suffix]
        rows.append(f"| {64 if suffix else 1} | {ratio:,.1f} | {ratio / READS:,.2f} |")
    rows += ["",
             "## Contention: equal (histogram, digit) addresses of a wave combined before the LDS atomic",
             "",
             "| form | period 1 | period 64 |",
             "|---|---|---|",
             f"| up to 8 distinct addresses combined, the rest lane by lane (kept) | {ms('read: history_quantiles')} | {ms('read: history_quantiles period=64')} |",
             f"| every lane its own atomic | {ms('read: history_quantiles, every lane its own atomic')} | {ms('read: history_quantiles period=64, every lane its own atomic')} |",
             f"| every distinct address combined (up to 64 rounds) | {ms('read: history_quantiles, every address once')} | {ms('read: history_quantiles period=64, every address once')} |",
             "",
             f"## Streaming: {a.batches:,} batches of {BATCH} ticks per window, the quantiles of the four columns",
             "",
             "| path | bytes to the host per batch | entity-steps/s (wall time of the window) |",
             "|---|---|---|"]
    for name in LEGS:
        if name.startswith("stream"):
            v = pooled[name]
            rows.append(f"| {name[8:]} | {meta[name]['bytes_per_batch'] / 1e6:,.3f} MB | {med[name]:.3e} [{min(v):.3e} .. {max(v):.3e}] |")
    rec = med["stream: record only"]
    rows += ["",
             f"Relative to recording with nothing read back: stream_quantiles every=1 {med['stream: stream_quantiles every=1'] / rec:.2f}, "
             f"every=8 {med['stream: stream_quantiles every=8'] / rec:.2f}.",
             ""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(rows))
    print("\n".join(rows))


if __name__ == "__main__":
    main()
