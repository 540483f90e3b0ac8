#!/usr/bin/env python3
"""Times what recording packing plans costs (include/bpp_placements.h).

    python tools/bench_placements.py [--out profiles/placements.json]

65 536 bins, 10x10x10, rotation on, static CUT-2 pool, uniform-feasible actions drawn inside the step kernel.  Two envs in the same
process -- one recording, one not -- play the same lock-steps, ALTERNATING batch by batch; every sample is a batch of back-to-back
step_tensors calls between two device events, so a figure is device time per lock-step with the launches' enqueue cost in it (what a
loop pays).  Then, on the recording env: placements() of all bins (bpp_placements_gather, running plans) and replay_plans of the
65 536 plans at the depth the lock-steps reached.  Reported: median and 10th / 90th percentiles over the batches, the difference of
the on / off medians, and the bytes note + commit and replay move (counted from the shapes, not measured).  No threshold: the off
figure of the same run is the yardstick.  Needs a HIP device; there is no CPU mode.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bpp_amd

HBM_PEAK = 8.0e12      # bytes/s, MI355X


def summary(us):
    return {"median_us": float(np.median(us)), "p10_us": float(np.percentile(us, 10)), "p90_us": float(np.percentile(us, 90)), "batches": len(us)}


def batch_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=20, help="lock-steps per batch")
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "placements.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_placements needs a HIP device")
    dev, size, E = "cuda:0", (10, 10, 10), args.bins
    pool = bpp_amd.sequences.cut2_pool(size, 1024, seed=0)
    envs, acts, tick = {}, {}, {}
    for name in ("off", "on"):
        env = bpp_amd.BppVecEnv(E, size, enable_rotation=True, pool=pool, device=dev)
        env.reset()
        if name == "on":
            env.record_placements()
        envs[name], acts[name], tick[name] = env, env.sample_feasible(seed=1, step=0), [1]

    def lockstep(name):
        def fn():
            env, a, t = envs[name], acts[name], tick[name]
            env.step_tensors(a, sample=(1, t[0], a))       # the next action is drawn inside the step kernel
            t[0] += 1
        return fn

    steps = {k: lockstep(k) for k in envs}
    for _ in range(args.warmup):
        for k in steps:
            steps[k]()
    torch.cuda.synchronize()
    samples = {"off": [], "on": []}
    for _ in range(args.batches):
        for k in ("off", "on"):
            samples[k].append(batch_us(steps[k], args.calls))
    on = envs["on"]
    same = bool(torch.equal(envs["off"].hmap, on.hmap)) and bool(torch.equal(envs["off"].state, on.state))      # recording changes no result
    plans = on.placements()
    depth = plans.count.to(torch.float64)
    consistent = bool(torch.equal(plans.count, on.state[:, 2]))
    hmap, status, volume = bpp_amd.replay_plans(plans)
    sound = bool((status == -1).all()) and bool(torch.equal(hmap.reshape(E, -1), on.hmap)) and bool(torch.equal(volume, on.state[:, 3]))
    g_us = [batch_us(lambda: on.placements(), 5) for _ in range(args.batches)]
    r_us = [batch_us(lambda: bpp_amd.replay_plans(plans), 5) for _ in range(args.batches)]
    cap, A = plans.capacity, size[0] * size[1]
    off_s, on_s = summary(samples["off"]), summary(samples["on"])
    # note: 4 B item + 8 B action + 8 B note read and written; commit: 8 B note, 16 B counts read and written, 1 B done, 4 B episode,
    # 1 B height, 8 B record -- per bin
    note_commit_bytes = E * ((4 + 8 + 8 + 8) + (8 + 8 + 16 + 16 + 1 + 4 + 1 + 8))
    gather_bytes = E * (cap * 8 + 8 * float(depth.mean()) + 16 + 8 + 8)
    replay_bytes = E * (8 * float(depth.mean()) + 4 + A + 8)
    out = {
        "what": "cost of recording packing plans beside step_tensors; gather and replay of all plans (tools/bench_placements.py)",
        "bins": E, "size": list(size), "rotation": True, "capacity": cap, "calls_per_batch": args.calls,
        "lock_steps_played": tick["on"][0] - 1, "results_identical_with_and_without_recording": same,
        "count_equals_n_boxes": consistent, "replay_sound_and_equal_to_heightmaps": sound,
        "plan_depth": {"mean": float(depth.mean()), "max": int(depth.max())},
        "step_tensors_recording_off": off_s, "step_tensors_recording_on": on_s,
        "recording_costs_us_per_lock_step": on_s["median_us"] - off_s["median_us"],
        "recording_costs_percent": 100.0 * (on_s["median_us"] / off_s["median_us"] - 1.0),
        "note_commit_bytes_per_lock_step": note_commit_bytes,
        "note_commit_time_at_hbm_peak_us": note_commit_bytes / HBM_PEAK * 1e6,
        "gather_all_bins": dict(summary(g_us), bytes=gather_bytes, share_of_hbm_peak=gather_bytes / HBM_PEAK / (np.median(g_us) * 1e-6),
                                note="includes the allocation of the result tensors and the copy of the overflow counter"),
        "replay_all_plans": dict(summary(r_us), bytes=replay_bytes, plans_per_s=E / (np.median(r_us) * 1e-6),
                                 boxes_per_s=float(depth.sum()) / (np.median(r_us) * 1e-6)),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
