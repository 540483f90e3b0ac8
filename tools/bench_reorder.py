#!/usr/bin/env python3
"""Time the native BPP-k reorder search (online-3d-bpp-drl_amd/reorder.py) with the int64-exact stand-in policy of the
fixtures (bpp_amd.reorder.int_policy: a few torch ops and one feasibility-mask launch) between the levels, which isolates
tree + env (the CNN is not timed here): n real bins (+ n scratch bins) of 10x10x10 cut-2 sequences, one decision at a time.
Writes profiles/reorder_bench.json.

    python tools/bench_reorder.py [--ns 2100 16384] [--ks 3 5] [--reps 3] [--out profiles/reorder_bench.json]

Per (n, k): wall time of a decision (enqueue + device, synchronised), its levels (k (1 + times)) and launches, us per level
and decisions per second.  Kernel times: run the same command under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bpp_amd  # noqa: E402
from bpp_amd.reorder import int_policy  # noqa: E402


def run(n, k, reps, size=(10, 10, 10)):
    pool = bpp_amd.sequences.cut2_pool(size, n, seed=5)
    env = bpp_amd.BppVecEnv(2 * n, size, pool=pool, device="cuda")
    env.reset()
    rs = bpp_amd.ReorderSearch(env, k)
    policy = int_policy(size)
    ids = torch.arange(n, device=env.device)
    rs.decide(policy, ids, ids + n)
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        act, _, _ = rs.decide(policy, ids, ids + n, check=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    levels = k * (1 + rs.times)
    return dict(n=n, k=k, times=rs.times, levels=levels, launches_per_level=3, copies=1 + rs.times,
                decision_s=best, us_per_level=best / levels * 1e6, decisions_per_s=n / best,
                overflow=int(rs.overflow.item()), policy="fake")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, nargs="+", default=[2100, 16384])
    ap.add_argument("--ks", type=int, nargs="+", default=[3, 5])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reorder_bench.json"))
    a = ap.parse_args()
    rows = []
    for n in a.ns:
        for k in a.ks:
            r = run(n, k, a.reps)
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
