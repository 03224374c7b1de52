#!/usr/bin/env python3
"""Where a one-tick launch of BASELINE configs[1] (65,536 bodies) spends its time.

  python tools/k1_floor.py

Per entity count: the driver's 20-step window (host clock and HIP events) and a 4,096-launch batch, three interleaved passes."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def measure(n):
    import torch
    import bench
    ex, w, eff = bench.make_exec(n, 0, 0, 1, True)
    ex.prepare(20)
    ex.invoke_batch(5)
    out = {"n": n}
    host, dev = [], []
    for _ in range(30):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tm = ex.invoke_batch(20)
        host.append((time.perf_counter() - t0) / 20 * 1e6)
        dev.append(tm.kernel_device_ms / 20 * 1e3)
        time.sleep(0.002)              # the idle gap a barrier leaves in front of the timed region
    out["steps20_host_us"] = [round(min(host), 3), round(sorted(host)[len(host) // 2], 3)]
    out["steps20_device_us"] = [round(min(dev), 3), round(sorted(dev)[len(dev) // 2], 3)]
    ex.prepare(4096)
    ex.invoke_batch(256)
    long_ = []
    for _ in range(5):
        tm = ex.invoke_batch(4096)
        long_.append(tm.kernel_device_ms / 4096 * 1e3)
    out["long_batch_us"] = [round(min(long_), 3), round(sorted(long_)[2], 3)]
    ex.close()
    return out


def main():
    for rep in range(3):
        for n in (65536, 262144):
            print(json.dumps(measure(n)), flush=True)


if __name__ == "__main__":
    main()
