"""Side legs of the benchmark: everything that is NOT the headline line bench.py prints.

`python bench.py --extras` runs them after the headline's timed region (rank 0, N = 1) and writes one JSON document to the
sidecar file (`--extras-out`, default gpurun_out/bench_extras.json); nothing here is printed on bench.py's final stdout line,
which stays the compact object the driver parses.  A leg that raises is recorded in the sidecar AND makes bench.py exit
non-zero: a broken leg is a failure, not a string in a JSON field.

Legs: `roofline_hbm` (the step kernel at 4,194,304 bodies, where the working set leaves the Infinity Cache), `fused` /
`recording` (ticks_per_launch > 1, the telemetry ring), `generated_pipe`, `f32`, `nbody` (BASELINE configs[2]), `sparse_edges`,
`telemetry_commit`, `history_stream`, `monte_carlo_example`, `apollo_mc` / `falcon9_mc` (configs[3] / [4] on one GPU),
`world_module` (whole-world StableHLO ticks), `build` (cold / cached build times), `campaigns` (whole campaigns over the ranks).
"""
from __future__ import annotations

import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from bench import (BYTES_PER_ENTITY_STEP_F64, ENTITIES, HBM_PEAK_GBPS, make_exec, roofline_from)  # noqa: E402

PMC_VALU_FILE = ROOT / "profiles" / "pmc_valu.json"   # profiles/collect_compute.sh + summarize_compute.py --json: VALU per wave and tick
WORLD_VALU_FILE = ROOT / "profiles" / "pmc_valu_world.json"   # profiles/collect_world.sh: the same count for the whole-world StableHLO ticks
VALU_PEAK_WAVE_INSTR_PER_S = 1024 * 2.4e9 / 4      # 1,024 SIMDs x 2.4 GHz / 4 clocks per 64-wide VALU instruction (MI355X_MICROARCH.md)
CAMPAIGN_TOTALS = {"apollo": 8192, "falcon9": 32768}      # BASELINE configs[3] / configs[4]: rollouts of the WHOLE campaign

_stream_cache = {}


def measured_stream_GBps(device=0):
    """What this box's HBM actually streams: a 1 GiB device-to-device copy (read + write = 2 GiB of traffic), best of 5, HIP events.
    MI355X_MICROARCH.md measures 6.29 TB/s for a float4 copy against the 8 TB/s spec the headline `frac` is priced on."""
    if device not in _stream_cache:
        import torch
        a = torch.empty(1 << 28, dtype=torch.float32, device=f"cuda:{device}")
        b = torch.empty_like(a)
        b.copy_(a)
        best = 1e30
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b.copy_(a)
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1))
        _stream_cache[device] = 2 * a.numel() * 4 / (best * 1e-3) / 1e9
        del a, b
    return _stream_cache[device]


def valu_roofline(key, rollouts, ticks, seconds, file=None):
    """The roofline that bounds a campaign kernel (BASELINE configs[3] / [4]): VALU ISSUE.  One lane flies one rollout with its
    state in registers, so a tick is `valu_per_wave_per_tick` vector instructions per wave (measured: SQ_INSTS_VALU / SQ_WAVES /
    ticks in its own rocprofv3 --pmc pass, committed as profiles/pmc_valu.json + profiles/r05_compute_kernels_pmc.md) and the chip
    issues at most one per SIMD every 4 clocks.  achieved = that count x waves x ticks / the seconds measured HERE."""
    waves = (int(rollouts) + 63) // 64
    out = {"bound": "valu issue", "unit": "wave-instructions/s", "peak": VALU_PEAK_WAVE_INSTR_PER_S, "waves": waves, "simds": 1024,
           "simds_occupied": min(waves, 1024), "achieved": None, "frac": None}
    try:
        src = Path(file) if file else PMC_VALU_FILE
        k = json.loads(src.read_text())["kernels"][key]
        per_tick = float(k["valu_per_wave_per_tick"])
        out.update({"valu_per_wave_per_tick": per_tick, "achieved": round(per_tick * waves * ticks / seconds, 1),
                    "frac": round(per_tick * waves * ticks / seconds / VALU_PEAK_WAVE_INSTR_PER_S, 4),
                    "frac_of_occupied_simds": round(per_tick * waves * ticks / seconds / (VALU_PEAK_WAVE_INSTR_PER_S * min(waves, 1024) / 1024), 4),
                    "counted_at": {"grid": k["grid"], "waves": k["waves"], "file": "profiles/" + src.name}})
    except Exception as e:  # noqa: BLE001
        out["note"] = f"no VALU count on file for {key!r} ({type(e).__name__}): run profiles/collect_compute.sh / collect_world.sh"
    return out


def kernel_roofline(ex, n, steps, warmup):
    """Average duration of one launch of the step kernel at ticks_per_launch = 1: `steps` launches enqueued back
    to back on the handle's stream between ONE HIP event pair (so inter-kernel gaps count against us)."""
    ex.set_ticks_per_launch(1)
    ex.invoke_batch(warmup)
    t = ex.invoke_batch(steps)
    return roofline_from(t.kernel_device_ms / max(1, t.launches), n, t.launches,
                         "HIP events around the batch on the launch stream / launches")


def generated_leg(device, n):
    """The same workload with its effectors written as user code (elodin_amd.dsl) and compiled into the step kernel
    at build time — the effector front-end must not cost throughput against the hand-written pipe."""
    import elodin_amd as ea
    from elodin_amd import dsl, workloads
    np_ = dsl.np

    @dsl.effector
    def gravity(force, inertia):
        return force + dsl.SpatialForce(linear=np_.array([0.0, 0.0, -9.81]) * inertia.mass())

    @dsl.effector(body_torque=3)
    def rcs(force, pos, body_torque):
        return force + dsl.SpatialForce(torque=pos.angular() @ body_torque)

    w = workloads.independent_bodies(n)
    t0 = time.perf_counter()
    ex = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], simulation_time_step=workloads.DT_120HZ,
                    effectors=gravity | rcs, columns={"body_torque": w["body_torque"]}, device=device, use_graph=True)
    build_s = time.perf_counter() - t0
    out = {"build_seconds_incl_hipcc_or_cache": round(build_s, 3)}
    for K in (1, 64):
        ex.set_ticks_per_launch(K)
        ex.invoke_batch(256)
        t = ex.invoke_batch(2048)
        out[f"entity_steps_per_s_k{K}"] = round(n * 2048 / (t.kernel_device_ms * 1e-3), 1)
    ex.close()
    return out


def f32_leg(device):
    """The f32 instantiation (BASELINE configs[4] asks for f32 state): same kernel, 192 B per entity-step."""
    import elodin_amd as ea
    from elodin_amd import workloads
    out = {}
    for n, reps in ((65536, 2048), (1 << 22, 64)):
        w = workloads.independent_bodies(n, dtype=np.float32)
        eff = workloads.gravity_torque_effectors(w["body_torque"])
        ex = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], dtype=np.float32, simulation_time_step=0.008333333,
                        effectors=eff, device=device, use_graph=True)
        ex.invoke_batch(reps // 8)
        t = ex.invoke_batch(reps)
        us = t.kernel_device_ms / reps * 1e3
        out[str(n)] = {"us_per_tick": round(us, 3), "entity_steps_per_s": round(n / us * 1e6, 1),
                       "algorithmic_GBps": round(192.0 * n / us / 1e3, 1)}
        ex.close()
    return out


def nbody_leg(device):
    """BASELINE configs[2]: all-pairs softened gravity, 16,384 bodies, RK4 f64 (parity case; timing for reference)."""
    import elodin_amd as ea
    from elodin_amd import _lib as L
    n = 16384
    rng = np.random.default_rng(7)
    u = rng.uniform(0.05, 0.95, n)
    d = rng.normal(size=(n, 3))
    p = d / np.linalg.norm(d, axis=1, keepdims=True) * (1.0 / np.sqrt(u ** (-2.0 / 3.0) - 1.0))[:, None]  # Plummer, a = 1 AU
    m = rng.uniform(1e-9, 1e-3, n)
    pos = np.concatenate([np.tile([0, 0, 0, 1.0], (n, 1)), p], axis=1)
    vel = np.concatenate([np.zeros((n, 3)), rng.normal(scale=1e-7, size=(n, 3))], axis=1)
    inertia = np.concatenate([np.tile(m[:, None], (1, 3)), np.zeros((n, 3)), m[:, None]], axis=1)
    ex = ea.HipExec(pos, vel, inertia, simulation_time_step=3600.0, device=device,
                    effectors=[ea.Effector(L.EFF_ALLPAIRS_GRAVITY_SOFTENED, (2.9591220828e-4 / 86400.0 ** 2, 1.0e-10))])
    ex.invoke_batch(3)
    t = ex.invoke_batch(20)
    ex.close()
    ms = t.kernel_device_ms / 20
    evals = 3.0 * n * (n - 1)   # every pair is visited once per tick and accumulates the 3 distinct stage forces
    return {"bodies": n, "ms_per_tick": round(ms, 4), "body_steps_per_s": round(n / ms * 1e3, 1),
            "pair_evals_per_s": round(evals / ms * 1e3, 1), "bound": "f64 vector ALU",
            "f64_instr_per_eval": "17 VALU + 1 v_rsq_f64",
            # ALGORITHMIC flops of config 3 = 4 N (N - 1) 20 per tick, against the 78.6 TF f64 vector peak
            "roofline": {"bound": "f64 vector ALU", "achieved": round(4.0 * n * (n - 1) * 20 / (ms * 1e-3) / 1e12, 2), "peak": 78.6,
                         "unit": "TFLOP/s", "frac": round(4.0 * n * (n - 1) * 20 / (ms * 1e-3) / 78.6e12, 4),
                         # what the kernel really executes: THREE sweeps (stages 1 and 2 see the same positions), 20 flop each
                         "achieved_executed": round(3.0 * n * (n - 1) * 20 / (ms * 1e-3) / 1e12, 2),
                         "frac_executed": round(3.0 * n * (n - 1) * 20 / (ms * 1e-3) / 78.6e12, 4),
                         "note": "`frac` prices SURVEY 8(d)'s algorithmic 4 sweeps; three are executed (`frac_executed`) for the reference's four"},
            # spec: 39.3e12 lane-FMA/s at 2.4 GHz; measured sustained issue (profiles/r01_ubench_f64_rates.txt):
            # 2.42 ns per f64 wave-op per SIMD, v_rsq_f64 7.0 ns -> 48.1 ns per wave-eval -> 1.36e12 evals/s
            "frac_of_spec_f64_fma_peak": round(evals * 17 / (ms * 1e-3) / 39.3e12, 4),
            "frac_of_measured_issue_bound": round(evals / (ms * 1e-3) / (1024 * 64 / 48.1e-9), 4)}


def sparse_edges_leg(device, hubs: int = 0):
    """A sparse GraphQuery.edge_fold: 65,536 bodies on a ring lattice, 16 out-edges each (1,048,576
    directed edges in spawn order), Newton gravity, RK4 — the CSR edge kernel (one lane per source, sequential fold over
    its out-edges, 80-byte gathers of the packed targets).  `hubs` > 0 adds that many sources with an edge to EVERY other
    body (65,535 out-edges each): folded by whole waves in 256-edge chunks (pair_kernel.hpp 2c)."""
    import elodin_amd as ea
    from elodin_amd import _lib as L
    n, deg = 65536, 16
    rng = np.random.default_rng(11)
    pos = np.concatenate([np.tile([0, 0, 0, 1.0], (n, 1)), rng.normal(size=(n, 3)) * 1e3], axis=1)
    vel = np.concatenate([np.zeros((n, 3)), rng.normal(size=(n, 3))], axis=1)
    m = rng.uniform(1.0, 10.0, n)
    inertia = np.concatenate([np.tile(m[:, None], (1, 3)), np.zeros((n, 3)), m[:, None]], axis=1)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    offs = np.array([k for k in range(-deg // 2, deg // 2 + 1) if k != 0][:deg])
    frm = np.repeat(ids, deg)
    to = ((np.repeat(np.arange(n), deg) + np.tile(offs, n)) % n + 1).astype(np.uint64)
    for hub in range(hubs):
        row = (hub * 7919 + 13) % n
        frm = np.concatenate([frm, np.full(n - 1, row + 1, dtype=np.uint64)])
        to = np.concatenate([to, np.delete(ids, row)])
    ex = ea.HipExec(pos, vel, inertia, entity_ids=ids, simulation_time_step=0.01, device=device, edges=(frm, to),
                    effectors=[ea.Effector(L.EFF_EDGE_GRAVITY_NEWTON, (6.6743e-11,))])
    ex.invoke_batch(5)
    t = ex.invoke_batch(50)
    ex.close()
    ms = t.kernel_device_ms / 50
    ne = int(len(frm))
    return {"bodies": n, "edges": ne, "hubs": hubs, "ms_per_tick": round(ms, 4), "edge_evals_per_s": round(3.0 * ne / ms * 1e3, 1),
            "body_steps_per_s": round(n / ms * 1e3, 1), "launches_per_tick": int(t.launches // 50),
            "gather_GBps": round(ne * 80 / (ms * 1e-3) / 1e9, 1)}


def apollo_leg(device):
    """BASELINE configs[3]: Apollo-lander Monte-Carlo, 8,192 rollouts x 10,000 steps (one GPU's worth here)."""
    from elodin_amd import monte_carlo as mc
    from elodin_amd.models import apollo
    spec = mc.load_spec(ROOT / "tests" / "golden" / "plans" / "apollo.toml")
    spec["monte_carlo"]["n_samples"] = 8192
    P = mc.materialize(spec).table()
    ex = apollo.ApolloExec(P, ticks_per_launch=1000, device=device)
    ex.invoke_batch(1000)
    t0 = time.perf_counter()
    tm = ex.invoke_batch(10000)
    dt = time.perf_counter() - t0
    ex.close()
    out = {"rollouts": 8192, "steps": 10000, "seconds": round(dt, 5), "rollout_steps_per_s": round(8192 * 10000 / dt, 1),
           "roofline": valu_roofline("apollo", 8192, 10000, dt),
           "parity": "plant pinned on the reference's Python (sim.py under refshim); guidance law a restatement of the Rust sidecar: unpinned",
           "launches": tm.launches, "integrator": "semi-implicit", "guidance": "in-kernel, on the reference cadence: post_step once per 3-tick telemetry batch, exchange when end_tick % 5 == 0 (every 15 ticks)"}
    # time per tick against the number of rollouts on ONE GPU: each rollout is a serial chain of ticks (one lane), so below
    # one wave per SIMD (65,536 rollouts) the tick time is the latency of one wave's tick whatever the count — this curve IS
    # the strong-scaling prediction for BASELINE's total split over G GPUs: speed-up(G) = t(total) / t(total / G)
    spec["monte_carlo"]["n_samples"] = 65536
    big = mc.materialize(spec).table()
    curve = {}
    for n in (1024, 2048, 4096, 8192, 16384, 32768, 65536):
        cx = apollo.ApolloExec(big[:n], ticks_per_launch=1000, device=device)
        cx.invoke_batch(1000)
        ct = cx.invoke_batch(2000)
        cx.close()
        curve[str(n)] = round(ct.kernel_device_ms / 2000 * 1e3, 4)
    out["rollouts_vs_time"] = {"unit": "us per tick (device time, 1000 ticks per launch)", "by_rollouts": curve,
                               "predicted_strong_speedup_8gpu": round(curve["8192"] / curve["1024"], 3),
                               "prediction": "t(8192 rollouts) / t(1024 rollouts): what sharding BASELINE's 8,192 rollouts over 8 GPUs can gain at best"}
    if True:    # the CPU restatement of the same rollout model (oracle/apollo_oracle.c, one thread) on a bounded sample
        from oracle.apollo import ApolloOracle
        ref = apollo.load_reference()
        o = ApolloOracle(apollo.initial_columns(P[:64], ref), ref, max_ticks=apollo.max_ticks(ref))
        t0 = time.perf_counter()
        o.step(10000)
        cs = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(64 * 10000 / cs, 1), "unit": "rollout-steps/s", "cores": 1, "kind": "port",
                               "sample": "64 rollouts x 10000 steps, oracle/apollo_oracle.c"}
    return out


def telemetry_leg(device, n):
    """The commit step either side of the path: every batch of ticks is followed by a copy of the four output columns
    into the host columns (exec.rs:110-172 + commit_world_head).  `sync` = step, then a blocking download (what JaxExec
    does, jax_exec.rs:150-178); `streaming` = sixdof_download_async, the copy overlapping the next batch.  Two batch
    shapes: 8 ticks fused in one launch (compute << copy: PCIe-bound either way) and 48 single-tick launches (compute ~
    copy: the overlap shows)."""
    from elodin_amd import _lib as L
    mask = L.COL_ALL & ~L.COL_INERTIA
    mb = n * 8 * (7 + 6 + 6 + 6) / 1e6
    out = {"entities": n, "column_MB_per_batch": round(mb, 2)}
    for label, tpl, k, batches in (("fused8", 8, 8, 200), ("k1x48", 1, 48, 100)):
        ex, w, eff = make_exec(n, 0, device, tpl, tpl == 1)      # single-tick batches replay a captured chain, like the headline
        if tpl == 1:
            ex.prepare(k)
        ex.invoke_batch(k)
        ex.download(mask)
        t0 = time.perf_counter()
        for _ in range(batches):
            ex.invoke_batch(k)
            ex.download(mask)
        sync_s = time.perf_counter() - t0
        gflag = L.FLAG_USE_GRAPH if tpl == 1 else 0            # run_streaming sets the handle's flags: keep the replay on
        ex.run_streaming(8, k, flags=gflag)
        stream_s = ex.run_streaming(batches, k, flags=gflag)
        ex.close()
        out[label] = {"ticks_per_batch": k, "ticks_per_launch": tpl, "batches": batches,
                      "sync_ms_per_batch": round(sync_s / batches * 1e3, 4),
                      "streaming_ms_per_batch": round(stream_s / batches * 1e3, 4),
                      "streaming_host_GBps": round(mb * batches / stream_s / 1e3, 2),
                      "entity_steps_per_s_sync": round(n * k * batches / sync_s, 1),
                      "entity_steps_per_s_streaming": round(n * k * batches / stream_s, 1)}
    return out


def history_stream_leg(device, n):
    """EVERY tick's output columns to the host (what a full-rate telemetry consumer needs), overlapped with the stepper:
    in-kernel recording into a two-batch device ring + sixdof_history_stream into page-locked host buffers."""
    ex, w, eff = make_exec(n, 0, device, 16, False)
    k, batches = 16, 40
    ex.stream_history(4, k)
    secs = ex.stream_history(batches, k)
    ex.close()
    mb = n * 8 * (7 + 6 + 6 + 6) / 1e6
    return {"entities": n, "ticks_per_batch": k, "batches": batches, "MB_per_tick": round(mb, 2),
            "ms_per_tick": round(secs / (k * batches) * 1e3, 4), "host_GBps": round(mb * k * batches / secs / 1e3, 2),
            "entity_steps_per_s": round(n * k * batches / secs, 1), "bound": "PCIe (device to host)"}


def falcon9_leg(device):
    """BASELINE configs[4]: Falcon 9 ascent Monte-Carlo, 32,768 rollouts, f32, the whole ascent to past MECO (one GPU's
    worth here; the closed loop is a generated program: models/falcon9.py)."""
    from elodin_amd.models import falcon9 as f9
    n = 32768
    ex = f9.AscentExec(f9.sample_params(n), dtype=np.float32, ticks_per_launch=1000, device=device, fast_math=True)
    ex.hip.invoke_batch(1000)
    t0 = time.perf_counter()
    tm = ex.hip.invoke_batch(f9.ASCENT_TICKS - 1000)
    dt = time.perf_counter() - t0
    ex.hip.download()
    res = ex.result
    widths = dict(ex.program.trace().columns)
    state_bytes = 4 * (sum(widths.values()) + 7 + 6 + 6 + 6 + 7)
    ex.close()
    # the same program with every tick round-tripping every column through HBM (the reference's per-tick column
    # semantics), at a rollout count that fills the chip: the HBM-roofline statement BASELINE asks for on this config
    hbm = {}
    for n1 in (262144, 32768):      # a count that fills the chip, and the config's own
        k1 = f9.AscentExec(np.tile(f9.default_param_row(), (n1, 1)), dtype=np.float32, ticks_per_launch=1, device=device, fast_math=True)
        tr = k1.program.trace()
        written = {t.split("_")[0] for s_ in tr.pre + tr.post for t in s_.written if t[0] == "c"}
        read_b = 4 * (sum(w for _, w in tr.columns) + 7 + 6 + 7)
        write_b = 4 * (sum(w for k, (_, w) in enumerate(tr.columns) if f"c{k}" in written) + 7 + 6 + 6 + 6 + 7)
        k1.hip.invoke_batch(20)
        t1 = k1.hip.invoke_batch(200)
        us1 = t1.kernel_device_ms / 200 * 1e3
        k1.close()
        rec = {"rollouts": n1, "ticks_per_launch": 1, "us_per_tick": round(us1, 2), "bytes_per_rollout_tick": read_b + write_b,
               "algorithmic_GBps": round((read_b + write_b) * n1 / us1 / 1e3, 1),
               "frac_of_hbm_peak": round((read_b + write_b) * n1 / us1 / 1e3 / HBM_PEAK_GBPS, 4)}
        if n1 == 262144:
            hbm = rec
        else:
            hbm["at_config_size"] = rec      # 32,768 rollouts = 512 waves: half the SIMDs, a launch-latency chain rather than a stream
    steps = f9.ASCENT_TICKS - 1000
    curve = {}
    for m in (4096, 8192, 16384, 32768, 65536, 131072, 262144):
        cx = f9.AscentExec(np.tile(f9.default_param_row(), (m, 1)), dtype=np.float32, ticks_per_launch=1000, device=device, fast_math=True)
        cx.hip.invoke_batch(1000)
        ct = cx.hip.invoke_batch(2000)
        cx.close()
        curve[str(m)] = round(ct.kernel_device_ms / 2000 * 1e3, 4)
    vs = {"unit": "us per tick (device time, 1000 ticks per launch)", "by_rollouts": curve,
          "predicted_strong_speedup_8gpu": round(curve["32768"] / curve["4096"], 3),
          "prediction": "t(32768 rollouts) / t(4096 rollouts): what sharding BASELINE's 32,768 rollouts over 8 GPUs can gain at best — "
                        "one lane flies one rollout, 32,768 rollouts are 512 waves on 1,024 SIMDs, so the tick time is one wave's "
                        "latency from 64 rollouts up to 65,536; weak scaling (32,768 per GPU) is what this path scales as"}
    return {"rollouts": n, "steps": steps, "roofline": valu_roofline("falcon9", n, steps, dt),
            "parity": "plant + helpers pinned on the reference's Python modules; flight software a restatement of the Rust sidecar (oracle/falcon9_fsw.c): "
                      "unpinned; this f32 fast-math build is compared with the f64 flight of the same plan rows (campaign metrics <= 1 %), pinned on nothing bit-wise",
            "roofline_hbm_k1": hbm, "rollouts_vs_time": vs, "seconds": round(dt, 4), "rollout_steps_per_s": round(n * steps / dt, 1),
            "dtype": "f32", "math": "hardware transcendentals in the generated user code (codegen fast_math)",
            "launches": tm.launches, "integrator": "semi-implicit @ 1 kHz", "guidance": "in-kernel, 100 Hz",
            "bound": "valu (state stays in registers for 1000 ticks per launch)",
            "state_bytes_per_rollout": state_bytes,
            "hbm_GBps_if_every_tick_round_tripped": round(2 * state_bytes * n * steps / dt / 1e9, 1),
            "reached_meco": int(np.sum(res[:, 3] > 0.0)), "meco_t_s": [round(float(res[:, 3].min()), 2), round(float(res[:, 3].max()), 2)],
            "meco_alt_km": [round(float(res[:, 4].min()) / 1e3, 2), round(float(res[:, 4].max()) / 1e3, 2)]}


def build_times_leg(device):
    """`build_time_ms` (the reference gates it in CI: scripts/ci/baseline/three-body-csv/profile-metrics.json 249 ms,
    tolerances.json; libs/nox-py/src/profile.rs:14-59): per generated program the COLD build on this host — trace + generate + every
    hipcc run, into an empty cache directory — and the cached one (what every later executor of the same program pays)."""
    import shutil
    import tempfile
    from elodin_amd import codegen, dsl
    from elodin_amd import stablehlo as sh
    saved = codegen.JIT_DIR
    out = {"unit": "ms", "compiler": "hipcc --offload-arch=gfx950, one cache-policy instantiation per object, flag sets of a large program compiled concurrently, "
                           "the kernel headers precompiled once per flag set (device + host PCH, codegen._Hipcc) and hipcc's own plan replayed with -include-pch"}

    def timed(name, make):
        """make() -> a callable that builds (trace + generate + compile) and returns the object's path."""
        tmp = Path(tempfile.mkdtemp(prefix="jit_cold_"))
        try:
            codegen.JIT_DIR = tmp
            first = None
            for attempt in range(2):
                n0, p0 = codegen.build_stats["hipcc_invocations"], codegen.build_stats.get("pch_builds", 0)
                build = make()                # (constructing the world / importing the example is not part of a build)
                t0 = time.perf_counter()
                build()
                cold = time.perf_counter() - t0
                inv = codegen.build_stats["hipcc_invocations"] - n0
                if codegen.build_stats.get("pch_builds", 0) == p0:
                    break
                # this build also compiled the precompiled preamble of its flag set (once per install and header state, shared by
                # every later program): reported on its own, and the program is built cold again with the preamble in place
                first = cold
                shutil.rmtree(tmp, ignore_errors=True)
                tmp.mkdir()
            build = make()
            t0 = time.perf_counter()
            build()
            cached = time.perf_counter() - t0
            out[name] = {"cold_ms": round(cold * 1e3, 1), "cached_ms": round(cached * 1e3, 1), "hipcc_invocations": int(inv),
                         "resources": {k: codegen.last_resources.get(k) for k in ("vgprs", "agprs", "scratch_bytes_per_lane", "flags")}}
            if first is not None:
                out[name]["first_build_incl_precompiled_preamble_ms"] = round(first * 1e3, 1)
        finally:
            codegen.JIT_DIR = saved
            shutil.rmtree(tmp, ignore_errors=True)

    def example(mod_name):
        def make():
            import importlib
            mod = importlib.import_module("examples." + mod_name)
            w, sys_ = (mod.world(), mod.system()) if mod_name == "ball" else mod.world_and_system()
            def build():
                dsl.Expr.fresh()
                srcs = w.generated_sources(sys_, simulation_rate=120.0, policy=1)      # as exec.HipExec builds it: the one cache policy its row count selects
                return [codegen._compile(src, kind) for kind, src in srcs.items()]
            return build
        return make
    timed("three_body_fold", example("three_body"))
    timed("ball_program", example("ball"))

    def falcon9():
        from elodin_amd.models import falcon9 as f9
        cols = f9.initial_columns(f9.default_param_row()[None, :])
        widths = {k: v.shape[1] for k, v in cols.items()}
        def build():
            dsl.Expr.fresh()
            tp = f9.build_program(origin=f9.pad_ecef(), algebraic_geodesy=True).trace(widths)
            return codegen.build(tp, "float32", 1, fast_math=True, column_soa=True, guard_selects=True, policy=1)
        return build
    timed("falcon9_f32_campaign", falcon9)

    def world_module():
        sys.path.insert(0, str(ROOT))
        from tests.golden import hlo_world_builder as hb
        text, slots = hb.three_body_world()
        doc = {"inputs": [{"component": c, "shape": s_, "entity_axis_elided": e} for c, s_, e in slots], "rows": 4096}
        return lambda: sh.compile_world(text, doc)[0]
    timed("three_body_world_module", world_module)
    out["apollo"] = {"cold_ms": 0.0, "cached_ms": 0.0, "hipcc_invocations": 0,
                     "note": "the Apollo rollout kernel is hand-written and compiled ahead of time into libsixdof_hip.so (csrc/apollo_kernels.hip): nothing is built per program"}
    return out


def world_module_leg(device):
    """f1 in its literal form: the reference's WHOLE-WORLD StableHLO tick (what cranelift_compile.rs:47-68 hands a backend) through
    the generated kernel.  (a) the three-body world module (edge_fold while + gathers), one lane per WORLD: a Monte-Carlo of
    worlds; (b) BASELINE configs[1] spelled as an entity-batched module ([65536, 7] tensors), one lane per ENTITY, next to the
    hand-written step kernel on the same world."""
    import elodin_amd as ea
    from elodin_amd import _lib as L
    from elodin_amd import dsl, workloads
    from elodin_amd import stablehlo as sh
    sys.path.insert(0, str(ROOT))
    from tests.golden import hlo_world_builder as hb
    out = {}
    text, slots = hb.three_body_world()
    system, manifest = sh.world_system(text, slots, mode="world")
    widths = {c["column"]: c["width"] for c in manifest["columns"]}
    g_pos = np.array([0, 0, 0, 1, 0.8920281421, 0, 0, 0, 0, 0, 1, -0.6628498947, 0, 0, 0, 0, 0, 1, -0.2291782474, 0, 0.0])
    g_vel = np.array([0, 0, 0, 0, 0.9957939373, 0, 0, 0, 0, 0, -1.6191613336, 0, 0, 0, 0, 0, 0.6233673964, 0.0])
    m = 1.0 / 6.6743e-11
    g_in = np.tile([m, m, m, 0, 0, 0, m], 3)
    for worlds in (4096, 65536):
        w = workloads.independent_bodies(worlds)
        cols = {"hlo_tick": np.zeros((worlds, 1)), "hlo_simulation_time_step": np.full((worlds, 1), 0.008333333),
                "hlo_world_pos": np.tile(g_pos, (worlds, 1)), "hlo_world_vel": np.tile(g_vel, (worlds, 1)),
                "hlo_world_accel": np.zeros((worlds, 18)), "hlo_force": np.zeros((worlds, 18)), "hlo_inertia": np.tile(g_in, (worlds, 1))}
        ex = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], integrator=L.INTEGRATOR_NONE, effectors=dsl.Program([system], dsl.Pipe([]), []),
                        columns=cols, ticks_per_launch=100, device=device)
        ex.invoke_batch(100)
        tm = ex.invoke_batch(1000)
        ex.close()
        rsys, _ = sh.world_system(text, slots, mode="world", arith="relaxed")      # opt-in: finite values, shared reciprocals, contraction (<= 1e-9 of G1, not its bits)
        ex = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], integrator=L.INTEGRATOR_NONE, effectors=dsl.Program([rsys], dsl.Pipe([]), []),
                        columns={k: v.copy() for k, v in cols.items()}, ticks_per_launch=100, device=device)
        ex.invoke_batch(100)
        tr = ex.invoke_batch(1000)
        ex.close()
        out[f"three_body_worlds_{worlds}"] = {"mode": manifest["mode"], "worlds": worlds, "ticks": 1000, "us_per_tick": round(tm.kernel_device_ms, 3),
                                             "us_per_tick_relaxed_arithmetic": round(tr.kernel_device_ms, 3),
                                             "world_steps_per_s": round(worlds * 1000 / (tm.kernel_device_ms * 1e-3), 1),
                                             "body_steps_per_s": round(3 * worlds * 1000 / (tm.kernel_device_ms * 1e-3), 1),
                                             "roofline": valu_roofline("three_body_world_mode", worlds, 1000, tm.kernel_device_ms * 1e-3, WORLD_VALU_FILE)}
    # the same module with one lane per ENTITY (mode "auto"): a world = 4 consecutive rows, the fold's targets read from the other
    # lanes of the world (lane_read = ds_bpermute) — the layout IS the ECS column layout, [worlds * 4, 7] rows of world_pos
    lsys, lman = sh.world_system(text, slots, mode="auto")
    S = lman.get("rows_per_world", 3)
    for worlds in (16384, 262144):
        rows = S * worlds
        w = workloads.independent_bodies(rows)
        def lay(vals, width, fill):
            a = np.tile(np.asarray(fill, dtype=np.float64), (rows, 1))
            for i in range(3):
                a[i::S] = vals[i * width:(i + 1) * width]
            return a
        cols = {"hlo_tick": np.zeros((rows, 1)), "hlo_simulation_time_step": np.full((rows, 1), 0.008333333),
                "hlo_world_pos": lay(g_pos, 7, [0, 0, 0, 1.0, 0, 0, 0]), "hlo_world_vel": lay(g_vel, 6, np.zeros(6)), "hlo_inertia": lay(g_in, 7, np.ones(7)),
                "hlo_world_accel": np.zeros((rows, 6)), "hlo_force": np.zeros((rows, 6))}
        ex = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], integrator=L.INTEGRATOR_NONE, effectors=dsl.Program([lsys], dsl.Pipe([]), []),
                        columns=cols, ticks_per_launch=100, device=device)
        ex.invoke_batch(100)
        tm = ex.invoke_batch(1000)
        ex.close()
        rsys, _ = sh.world_system(text, slots, mode="auto", arith="relaxed")
        ex = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], integrator=L.INTEGRATOR_NONE, effectors=dsl.Program([rsys], dsl.Pipe([]), []),
                        columns={k: v.copy() for k, v in cols.items()}, ticks_per_launch=100, device=device)
        ex.invoke_batch(100)
        tr = ex.invoke_batch(1000)
        ex.close()
        out[f"three_body_worlds_{worlds}_lane_mode"] = {"mode": lman["mode"], "rows_per_world": S, "worlds": worlds, "rows": rows, "ticks": 1000,
                                                       "us_per_tick": round(tm.kernel_device_ms, 3), "us_per_tick_relaxed_arithmetic": round(tr.kernel_device_ms, 3),
                                                       "world_steps_per_s": round(worlds * 1000 / (tm.kernel_device_ms * 1e-3), 1),
                                                       "body_steps_per_s": round(3 * worlds * 1000 / (tm.kernel_device_ms * 1e-3), 1),
                                                       "roofline": valu_roofline("three_body_lane_mode", rows, 1000, tm.kernel_device_ms * 1e-3, WORLD_VALU_FILE)}
    if True:      # examples/n-body's 10-body solar system (90 edges, softened fold): too wide for one lane per world; lane mode, a world = 16 rows
        from tests import solar_util as su
        _, spos, svel, sin_ = su.load()
        nb = spos.shape[0]
        ntext, nslots = hb.nbody_world(nb, su.K_SQUARED, su.SOFTENING_AU2)
        nsys, nman = sh.world_system(ntext, nslots, mode="auto")
        S = nman["rows_per_world"]
        worlds = 4096
        rows = S * worlds
        w = workloads.independent_bodies(rows)
        def nlay(a, fill):
            o = np.tile(np.asarray(fill, dtype=np.float64), (rows, 1))
            for i in range(nb):
                o[i::S] = a[i]
            return o
        cols = {"hlo_tick": np.zeros((rows, 1)), "hlo_simulation_time_step": np.full((rows, 1), su.DT), "hlo_world_pos": nlay(spos, [0, 0, 0, 1.0, 0, 0, 0]),
                "hlo_world_vel": nlay(svel, np.zeros(6)), "hlo_inertia": nlay(sin_, np.ones(7)), "hlo_world_accel": np.zeros((rows, 6)), "hlo_force": np.zeros((rows, 6))}
        ex = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], integrator=L.INTEGRATOR_NONE, effectors=dsl.Program([nsys], dsl.Pipe([]), []),
                        columns=cols, ticks_per_launch=100, device=device)
        ex.invoke_batch(100)
        tm = ex.invoke_batch(1000)
        ex.close()
        out["solar_system_10_bodies_lane_mode"] = {"mode": nman["mode"], "rows_per_world": S, "entities_per_world": nb, "worlds": worlds, "rows": rows, "ticks": 1000,
                                                   "us_per_tick": round(tm.kernel_device_ms, 3), "world_steps_per_s": round(worlds * 1000 / (tm.kernel_device_ms * 1e-3), 1),
                                                   "pair_evals_per_s": round(4.0 * nb * (nb - 1) * worlds * 1000 / (tm.kernel_device_ms * 1e-3), 1),
                                                   "exchange_reads_per_tick_in_the_program": nman.get("exchange_reads"),
                                                   "roofline": valu_roofline("solar_system_10_bodies_lane_mode", rows, 1000, tm.kernel_device_ms * 1e-3, WORLD_VALU_FILE)}
    if True:      # a 35-body cluster (1,190 edges): a world = one whole wavefront (64 rows); its four 34-trip scans stay counted loops
        nb = 35
        rng = np.random.default_rng(nb)
        cpos = np.concatenate([np.tile([0, 0, 0, 1.0], (nb, 1)), rng.normal(size=(nb, 3)) * 3], axis=1)
        cvel = np.concatenate([np.zeros((nb, 3)), rng.normal(size=(nb, 3)) * 1e-3], axis=1)
        cm = rng.uniform(1e-6, 1e-3, nb)
        cin = np.concatenate([np.tile(cm[:, None], (1, 3)), np.zeros((nb, 3)), cm[:, None]], axis=1)
        ctext, cslots = hb.nbody_world(nb, 2.9591220828e-4, 1e-6)
        csys, cman = sh.world_system(ctext, cslots, mode="auto")
        S = cman["rows_per_world"]

        def cluster(worlds):
            rows = S * worlds
            w = workloads.independent_bodies(rows)
            def clay(a, fill):
                o = np.tile(np.asarray(fill, dtype=np.float64), (rows, 1))
                for i in range(nb):
                    o[i::S] = a[i]
                return o
            cols = {"hlo_tick": np.zeros((rows, 1)), "hlo_simulation_time_step": np.full((rows, 1), 0.5), "hlo_world_pos": clay(cpos, [0, 0, 0, 1.0, 0, 0, 0]),
                    "hlo_world_vel": clay(cvel, np.zeros(6)), "hlo_inertia": clay(cin, np.ones(7)), "hlo_world_accel": np.zeros((rows, 6)), "hlo_force": np.zeros((rows, 6))}
            ex = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], integrator=L.INTEGRATOR_NONE, effectors=dsl.Program([csys], dsl.Pipe([]), []),
                            columns=cols, ticks_per_launch=50, device=device)
            ex.invoke_batch(50)
            tm = ex.invoke_batch(500)
            ex.close()
            return {"mode": cman["mode"], "rows_per_world": S, "entities_per_world": nb, "worlds": worlds, "rows": rows, "ticks": 500,
                    "us_per_tick": round(tm.kernel_device_ms * 2, 3), "world_steps_per_s": round(worlds * 500 / (tm.kernel_device_ms * 1e-3), 1),
                    "pair_evals_per_s": round(4.0 * nb * (nb - 1) * worlds * 500 / (tm.kernel_device_ms * 1e-3), 1),
                    "exchange_reads_per_tick_in_the_program": cman.get("exchange_reads"),
                    "loops": "four 34-trip counted loops (lane_read_dyn), not unrolled",
                    "roofline": valu_roofline("cluster_35_bodies_lane_mode", rows, 500, tm.kernel_device_ms * 1e-3, WORLD_VALU_FILE)}
        out["cluster_35_bodies_lane_mode"] = cluster(1024)              # one wave per SIMD
        out["cluster_35_bodies_lane_mode_4096_worlds"] = cluster(4096)  # four (254 registers: two resident at a time hide each other's trip-opening latency)
    n = 65536
    text, slots = hb.independent_bodies_world(n)
    w = workloads.independent_bodies(n)

    def module_leg(arith, one_world):
        system, manifest = sh.world_system(text, slots, mode="lane", arith=arith, one_world=one_world)
        cols = {"hlo_tick": np.zeros((n, 1)), "hlo_simulation_time_step": np.full((n, 1), workloads.DT_120HZ), "hlo_world_pos": w["world_pos"].copy(),
                "hlo_world_vel": w["world_vel"].copy(), "hlo_world_accel": np.zeros((n, 6)), "hlo_force": np.zeros((n, 6)), "hlo_inertia": w["inertia"].copy(),
                "hlo_torque": w["body_torque"].copy()}
        ex = ea.HipExec(w["world_pos"], w["world_vel"], w["inertia"], integrator=L.INTEGRATOR_NONE, effectors=dsl.Program([system], dsl.Pipe([]), []),
                        columns=cols, device=device, use_graph=True)       # replayed like the headline: the program never looks at the absolute tick
        ex.prepare(1024)
        ex.invoke_batch(64)
        tm = ex.invoke_batch(1024)
        us = tm.kernel_device_ms / 1024 * 1e3
        ex.set_ticks_per_launch(64)
        ex.invoke_batch(64)
        tf = ex.invoke_batch(64 * 32)
        ex.close()
        wtp = dsl.Program([system], dsl.Pipe([]), []).trace({c["column"]: c["width"] for c in manifest["columns"]})
        written = {t.split("_")[0] for s_ in wtp.pre + wtp.post for t in s_.written if t[0] == "c"}
        read = {f"c{k}" for s_ in wtp.pre + wtp.post for k in codegen_slots(s_)}
        uni = {f"c{k}" for k in wtp.uniform_slots}
        # slots the traced tick reads (a wave-uniform one costs a line per wavefront, counted as 1 B per row) + the ones it changes
        bytes_per = sum(8 * w_ if f"c{k}" not in uni else 1 for k, (_, w_) in enumerate(wtp.columns) if f"c{k}" in read) \
            + 8 * sum(w_ for k, (_, w_) in enumerate(wtp.columns) if f"c{k}" in written)
        return {"mode": manifest["mode"], "arith": arith, "one_world": one_world, "entities": n, "us_per_tick_k1": round(us, 3),
                "entity_steps_per_s_k1": round(n / us * 1e6, 1), "bytes_per_entity_tick": bytes_per,
                "algorithmic_GBps": round(bytes_per * n / us / 1e3, 1), "frac_of_hbm_peak": round(bytes_per * n / us / 1e3 / HBM_PEAK_GBPS, 4),
                "graph_launches_k1": int(tm.graph_launches), "entity_steps_per_s_k64": round(n * 64 * 32 / (tf.kernel_device_ms * 1e-3), 1)}

    def codegen_slots(traced_system):      # column slots whose values the traced tick READS (leaves of its expressions)
        names = dsl._leaves_of([e for _, e in traced_system.assign])
        return sorted({int(n_[1:].split("_")[0]) for n_ in names if n_[0] == "c" and "_" in n_ and n_[1:].split("_")[0].isdigit()})
    out["independent_bodies_65536_lane_mode"] = {
        **module_leg("reference", False),
        "what": "the whole tick is the module's (integrator NONE, the executor's Body slabs untouched), the reference's arithmetic operation for "
                "operation: bit for bit the oracle's.  `bytes_per_entity_tick`: the slots the traced tick reads + the ones it changes (by PMC 460 B: "
                "profiles/r06_world_module_bytes_pmc.md); its time is instruction issue (1,744 VALU per wave and tick)"}
    out["independent_bodies_65536_lane_mode_relaxed"] = {
        **module_leg("relaxed", True),
        "what": "the same module under world_system(arith='relaxed', one_world=True): finite values assumed (the 0 * world_accel read is gone), one "
                "division per denominator, a * b + c contracted, Globals read once per wavefront — inside 1e-9 of the oracle (measured 3e-15), not its "
                "last bits; the hand-written kernel: 384 B, 4.8 us"}
    return out


def monte_carlo_example_leg(device):
    """The reference's own Monte-Carlo example (examples/monte-carlo: sim.py's point-mass plant gathering its drag coefficient
    from a lookup table, main.py's post_step control law, spec.toml's 100-run LHS plan = its plan.csv; grid size 4,096 as
    monte_carlo_scaling_sweep.py sweeps it) as ONE executor (elodin_amd/vectorize.py; examples/monte_carlo_sitl.py generates byte
    for byte the program of the unmodified script).  (a) the script's post_step called per run and tick on the host, the way
    main.py runs; (b) the same law as a system on the device, at the plan's size and at a count that fills the chip."""
    os.environ["ELODIN_MONTE_CARLO_GRID_SIZE"], os.environ["ELODIN_MONTE_CARLO_PROBE_ROWS"] = "4096", "0"
    from examples import monte_carlo_sitl as ex
    from elodin_amd import monte_carlo as mc
    from elodin_amd import vectorize
    plan = mc.materialize(ex.SPEC)
    t0 = time.perf_counter()
    c = vectorize.Campaign(ex.build, plan, ex.PARAMS, simulation_rate=ex.SIMULATION_RATE_HZ, device=device)
    build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    c.run(ex.DEFAULT_MAX_TICKS, post_step=ex.post_step)
    host_s = time.perf_counter() - t0
    res = c.result_table(["final_position", "target", "error"])
    out = {"plan": "spec.toml: 100 runs, LHS seed 42 (parameter values = the example's plan.csv)", "grid_size": 4096, "ticks": ex.DEFAULT_MAX_TICKS,
           "build_seconds": round(build_s, 3),
           "host_post_step": {"runs": len(plan), "seconds": round(host_s, 4), "rollout_steps_per_s": round(len(plan) * ex.DEFAULT_MAX_TICKS / host_s, 1),
                              "what": "main.py's post_step per run and tick through StepContext (read x3, write x1), columns committed every tick",
                              "captured_fraction": round(float(np.mean(res[:, 2] < 8.5)), 3), "mean_error_m": round(float(res[:, 2].mean()), 4)}}
    c.exec._hip.close()
    for runs in (100, 65536):
        spec = {"monte_carlo": dict(ex.SPEC["monte_carlo"], n_samples=runs)}
        t0 = time.perf_counter()
        d = vectorize.Campaign(ex.build_closed_loop, mc.materialize(spec), ex.PARAMS, simulation_rate=ex.SIMULATION_RATE_HZ, device=device)
        b = time.perf_counter() - t0
        d.exec._hip.set_ticks_per_launch(ex.DEFAULT_MAX_TICKS)
        d.exec._hip.invoke_batch(ex.DEFAULT_MAX_TICKS)                      # untimed: code-object load
        tm = d.exec._hip.invoke_batch(ex.DEFAULT_MAX_TICKS)
        d.exec._hip.download()
        err = np.abs(d.column("target")[:, 0] - d.column("position")[:, 0]) if "target" in d.exec._hip._aux else None
        out[f"device_controller_{runs}"] = {"runs": runs, "build_seconds_incl_host_spawn": round(b, 3), "device_ms_per_360_ticks": round(tm.kernel_device_ms, 4),
                                            "rollout_steps_per_s": round(runs * ex.DEFAULT_MAX_TICKS / (tm.kernel_device_ms * 1e-3), 1)}
        d.exec._hip.close()
    return out


def campaign_bench(which, rank, world, local_rank, comm_device, barrier, capi_comm=None, scaling="strong"):
    """One whole campaign over the ranks.  `strong` = BASELINE's rollout count as it is stated (8,192 Apollo descents /
    32,768 Falcon 9 ascents IN TOTAL) split over the ranks in run-id order; `weak` = that count PER GPU.  Rank 0 samples the
    plan, the table is broadcast and the result rows are gathered over the process group (RCCL on `nccl`); no exchange while
    the rollouts fly.  Timed region = broadcast + flight + gather, max over ranks."""
    from elodin_amd import monte_carlo as mc
    from elodin_amd import shard
    total = CAMPAIGN_TOTALS[which] * (world if scaling == "weak" else 1)
    lo, hi = shard.shard_range(total, world, rank)
    how = (f"{CAMPAIGN_TOTALS[which]} rollouts per GPU (weak)" if scaling == "weak" else
           f"{total} rollouts in total, split over {world} GPU(s) (strong, as BASELINE states it; predicted 8-GPU speed-up 1.0x: a tick is ONE wave's "
           "latency whatever the rollout count below one wave per SIMD — what scales is the number of rollouts, see the weak line)")
    if which == "apollo":
        from elodin_amd.models import apollo as model
        dtype = "f64"
        spec = mc.load_spec(ROOT / "tests" / "golden" / "plans" / "apollo.toml")
        spec["monte_carlo"]["n_samples"] = total
        table = mc.materialize(spec).table() if rank == 0 else None
        ticks = model.max_ticks(model.load_reference())
        run = lambda: model.run_campaign(table, total, ticks, device=local_rank, comm_device=comm_device, comm=capi_comm)
        ok = lambda res: float(res[:, 8].mean())           # landed
        desc = f"Apollo-lander Monte-Carlo, {how} x {ticks} ticks max, semi-implicit f64 (BASELINE configs[3])"
    else:
        from elodin_amd.models import falcon9 as model
        ticks, dtype = model.ASCENT_TICKS, "f32"
        table = model.sample_params(total) if rank == 0 else None
        run = lambda: model.run_campaign(table, total, ticks, device=local_rank, comm_device=comm_device, comm=capi_comm)
        ok = lambda res: float((res[:, 3] > 0.0).mean())   # reached MECO
        desc = f"Falcon 9 ascent Monte-Carlo, {how} x {ticks} ticks, semi-implicit f32 (BASELINE configs[4])"
    warmup = 0
    if which == "falcon9":
        # one untimed launch of the executor the campaign will build (same row count -> same generated object and device
        # layout): hipcc / the cached object, the code-object load and, on a freshly booted box, ~6 s of paging the toolchain
        # and libraries in happen here once per process — a second process measured 0.15 s for the same construction
        w = model.AscentExec(np.tile(model.default_param_row(), (hi - lo, 1)), dtype=np.float32, device=local_rank, fast_math=True)
        w.hip.invoke_batch(1000)
        w.close()
        warmup = 1
    barrier()
    t0 = time.perf_counter()
    res = run()
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        elapsed = shard.max_over_ranks(elapsed, device=comm_device)
    return {"metric": "rollout-steps/s (whole campaign)", "value": round(total * ticks / elapsed, 1), "unit": "rollout-steps/s",
            "n_gpus": world, "steps": ticks, "warmup": warmup, "ms_per_step": round(elapsed / ticks * 1e3, 6),
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None, "dtype": dtype, "data": "synthetic (sampled plan)",
            "config": {"workload": desc, "rollouts": total, "rollouts_per_gpu": hi - lo,
                       "parallelism": f"run-id shards x{world}; broadcast plan + gather results",
                       "collectives": "C ABI (sixdof_campaign_broadcast / _gather over RCCL)" if capi_comm is not None else "torch.distributed"},
            "campaign_seconds": round(elapsed, 4), "success_fraction": round(ok(res), 4) if rank == 0 else None,
            "roofline": valu_roofline(which, hi - lo, ticks, max(getattr(model, "last_campaign_phases", {}).get("flight_and_download_s", elapsed), 1e-9)),
            "parity": ("plant pinned on the reference's Python; guidance restatement unpinned" if which == "apollo" else
                       "plant pinned on the reference's Python; flight-software restatement unpinned; f32 fast-math build bounded against the f64 flight, not pinned bit-wise"),
            "phases": {k: round(v, 4) for k, v in getattr(model, "last_campaign_phases", {}).items()}}


def step_variants(device, n):
    """The headline handle's other shapes: a long K = 1 batch, K = 16 / 64 / 256 ticks per launch (state in registers), and the
    in-kernel telemetry ring (every tick's rows written to HBM)."""
    import torch
    ex, _, _ = make_exec(n, 0, device, 1, True)
    out = {}
    ex.prepare(4096)
    ex.invoke_batch(256)
    st = ex.invoke_batch(4096)
    out["k1_long_batch"] = roofline_from(st.kernel_device_ms / max(1, st.launches), n, st.launches,
                                         "HIP events around a 4,096-launch batch on the launch stream / launches")
    bw = measured_stream_GBps(device)
    out["measured_stream_GBps"] = round(bw, 1)
    out["measured_stream_how"] = "1 GiB device-to-device copy (2 GiB of traffic), best of 5, on this GPU in this run"
    # fused batch: the reference's ticks_per_telemetry semantics, state held in VGPRs
    ex.set_ticks_per_launch(64)
    ex.invoke_batch(64 * 4)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ft = ex.invoke_batch(64 * 64)
    fe = time.perf_counter() - t1
    out["fused"] = {"ticks_per_launch": 64, "value": round(n * 64 * 64 / fe, 1), "unit": "entity-steps/s",
                    "device_ms_per_tick": round(ft.kernel_device_ms / (64 * 64), 6)}
    for kk in (16, 256):  # K in {1, 16, 256} ticks per launch reported separately (K = 1 is the headline `value`)
        ex.set_ticks_per_launch(kk)
        ex.invoke_batch(kk * 4)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ex.invoke_batch(kk * 32)
        out["fused"][f"value_k{kk}"] = round(n * kk * 32 / (time.perf_counter() - t1), 1)
    # fused + telemetry ring: EVERY tick's pos/vel/accel/force rows are written to HBM (200 B per entity-step, write-once)
    ex.set_ticks_per_launch(64)
    ex.enable_history(256)
    ex.invoke_batch(256)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    rt = ex.invoke_batch(64 * 64)
    re_ = time.perf_counter() - t2
    wr = 200.0 * n / (rt.kernel_device_ms / (64 * 64) * 1e-3) / 1e9
    out["recording"] = {"ticks_per_launch": 64, "ring_ticks": 256, "value": round(n * 64 * 64 / re_, 1),
                        "unit": "entity-steps/s", "device_ms_per_tick": round(rt.kernel_device_ms / (64 * 64), 6),
                        "write_GBps": round(wr, 1), "frac_of_hbm_peak": round(wr / HBM_PEAK_GBPS, 4)}
    ex.enable_history(0)
    ex.close()
    return out


def roofline_hbm_leg(device):
    big = 1 << 22
    bex, _, _ = make_exec(big, 0, device, 1, False)
    r = kernel_roofline(bex, big, 64, 8)
    bex.close()
    return r


def single_gpu_legs(device, n):
    """(name, callable) of every informational single-GPU leg, in the order they run."""
    return [("step_variants", lambda: step_variants(device, n)),
            ("roofline_hbm", lambda: roofline_hbm_leg(device)),
            ("generated_pipe", lambda: generated_leg(device, n)),
            ("f32", lambda: f32_leg(device)),
            ("nbody", lambda: nbody_leg(device)),
            ("sparse_edges", lambda: sparse_edges_leg(device)),
            ("sparse_edges_hubs", lambda: sparse_edges_leg(device, 8)),
            ("telemetry_commit", lambda: telemetry_leg(device, n)),
            ("history_stream", lambda: history_stream_leg(device, n)),
            ("monte_carlo_example", lambda: monte_carlo_example_leg(device)),
            ("apollo_mc", lambda: apollo_leg(device)),
            ("falcon9_mc", lambda: falcon9_leg(device)),
            ("world_module", lambda: world_module_leg(device)),
            ("build", lambda: build_times_leg(device))]


def run_legs(legs, only=(), skip=()):
    """Runs the legs; returns (document, errors).  An exception is recorded under the leg's name and in `errors`."""
    doc, errors = {}, {}
    for name, fn in legs:
        if (only and name not in only) or name in skip:
            continue
        t0 = time.perf_counter()
        try:
            doc[name] = fn()
        except Exception as e:  # noqa: BLE001 - recorded, then bench.py exits non-zero
            import traceback
            errors[name] = f"{type(e).__name__}: {e}"
            doc[name] = {"error": errors[name], "traceback": traceback.format_exc()[-1500:]}
        if isinstance(doc[name], dict):
            doc[name]["leg_seconds"] = round(time.perf_counter() - t0, 2)
    tc = doc.get("telemetry_commit", {}).get("k1x48", {}) if isinstance(doc.get("telemetry_commit"), dict) else {}
    if tc.get("entity_steps_per_s_streaming"):
        # SURVEY 8(d)'s metric as it is defined (commit of the output columns included), both ways a host can write
        # invoke_batch; the headline `value` is the step alone, columns resident in HBM
        doc["incl_commit"] = {"unit": "entity-steps/s", "streaming": tc["entity_steps_per_s_streaming"], "blocking": tc.get("entity_steps_per_s_sync"),
                              "streaming_is": "sixdof_step + sixdof_download_async: the D2H of batch k overlaps batch k + 1",
                              "blocking_is": "sixdof_step, then a blocking sixdof_download per batch (jax_exec.rs:150-178's shape)",
                              "batch": "48 single-tick launches, 13.1 MB of output columns per commit: PCIe-bound"}
    return doc, errors
