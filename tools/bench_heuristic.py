#!/usr/bin/env python3
"""Timing of bpp_heuristic_act (include/bpp_heuristic.h) -> profiles/heuristic_act.json.

Per geometry (65 536 bins at 10x10 and 10x10 + rotation, 32 768 bins at 20x20) three kinds of state -- just reset (every in-range
entry ties: the worst case of the tie-break), after 12 and after 30 lock-steps under the heuristic itself -- and both rules.  A
figure is the time of LAUNCHES launches back to back through the C ABI between one pair of HIP events, divided by LAUNCHES; the
configurations of a geometry, bpp_mask_from_obs and bpp_masked_act among them, alternate within a round, and the median over the
rounds is reported with the 10th and 90th percentile.  Beside them: env steps/s of the step_tensors + heuristic_act loop (host
clock around 30 lock-steps that end in a synchronise) and the host oracle's time per row on this machine's CPU, whose actions the
device's are compared with on the same rows.

    python tools/bench_heuristic.py [--out profiles/heuristic_act.json] [--scale 1.0]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bpp_amd
from bpp_amd import _lib
from oracle import policies

LAUNCHES, ROUNDS, ORACLE_ROWS, LOOP_STEPS = 200, 7, 256, 30
GEOMS = [((10, 10, 10), False, 65536), ((10, 10, 10), True, 65536), ((20, 20, 20), False, 32768)]
STATES = (("reset", 0), ("after_12", 12), ("after_30", 30))


def percentiles(ts):
    return {"median_us": round(float(np.median(ts)), 2), "p10_us": round(float(np.percentile(ts, 10)), 2),
            "p90_us": round(float(np.percentile(ts, 90)), 2)}


def geometry(size, rotation, n):
    dev = torch.device("cuda:0")
    L = _lib.lib()
    W, Ln, H = size
    A, M = W * Ln, W * Ln * (1 + int(rotation))
    env = bpp_amd.BppVecEnv(n, size, enable_rotation=rotation, pool=bpp_amd.sequences.cut2_pool(size, 128, seed=1), device=dev)
    act = torch.empty(n, dtype=torch.int64, device=dev)

    def loop(steps, keep=None):
        env.reset()
        for t in range(steps + 1):
            if keep is not None and t in keep:
                keep[t] = (env._res.obs.clone(), env.location_masks.clone())
            if t < steps:
                env.heuristic_act(out=act)
                env.step_tensors(act)

    loop(3)                                     # warm-up of both kernels
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop(LOOP_STEPS)
    torch.cuda.synchronize()
    loop_seconds = time.perf_counter() - t0
    keep = {k: None for _, k in STATES}
    loop(LOOP_STEPS, keep)
    torch.cuda.synchronize()

    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    top = torch.empty(n, dtype=torch.int32, device=dev)
    logp = torch.empty(n, dtype=torch.float32, device=dev)
    mask_out = torch.empty((n, M), dtype=torch.float32, device=dev)
    logits = torch.randn((n, M), device=dev)
    configs = {}
    for name, k in STATES:
        o, m = keep[k]
        for rule, rid in _lib.HEURISTIC_RULES.items():
            configs["%s/%s" % (name, rule)] = (lambda o=o, m=m, rid=rid: L.bpp_heuristic_act(o.data_ptr(), 4 * A, m.data_ptr(), n, W, Ln, int(rotation), rid,
                                                                                             act.data_ptr(), top.data_ptr(), sp))
    o12, m12 = keep[12]
    configs["bpp_mask_from_obs/after_12"] = lambda: L.bpp_mask_from_obs(o12.data_ptr(), mask_out.data_ptr(), n, W, Ln, H, int(rotation), _lib.RULE_UTILS, sp)
    configs["bpp_masked_act/after_12"] = lambda: L.bpp_masked_act(logits.data_ptr(), m12.data_ptr(), act.data_ptr(), logp.data_ptr(), n, M, 0, 1, 0, 1, sp)
    times = {c: [] for c in configs}
    for c, call in configs.items():             # every shape warmed up
        for _ in range(5):
            assert call() == 0, L.bpp_last_error()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for c, call in configs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                call()
            e1.record()
            torch.cuda.synchronize()
            times[c].append(e0.elapsed_time(e1) / LAUNCHES * 1e3)
    res = {"bins": n, "launch": _lib.heuristic_info(size, rotation, n), "bytes_read_per_bin": 4 * (A + 3 + M),
           "loop_env_steps_per_s": round(n * LOOP_STEPS / loop_seconds), "loop_lock_steps": LOOP_STEPS,
           "kernels": {c: percentiles(ts) for c, ts in times.items()}}
    # the host oracle on the first rows of every state, timed on this machine's CPU; the device's actions are compared with its
    states = {}
    for name, k in STATES:
        o, m = (t[:ORACLE_ROWS].cpu().numpy() for t in keep[k])
        K = np.where(m > 0.5, policies.window_tops(o, size, rotation)[0], policies._BIG + 1)
        ties = (K == K.min(axis=1, keepdims=True)).sum(axis=1)
        entry = {"mean_tied_entries": round(float(ties.mean()), 1), "most_tied_entries": int(ties.max())}
        for rule in _lib.HEURISTIC_RULES:
            t0 = time.perf_counter()
            want = policies.lowest_top_actions(o, m, size, rotation, smooth=(rule == "lowest_top"))
            entry["host_oracle_us_per_row_" + rule] = round((time.perf_counter() - t0) / ORACLE_ROWS * 1e6, 1)
            got = bpp_amd.heuristic_act(keep[k][0][:ORACLE_ROWS], keep[k][1][:ORACLE_ROWS], size, rotation, rule).cpu().numpy()
            entry["actions_equal_oracle_" + rule] = bool(np.array_equal(got, want))
        states[name] = entry
    res["states"] = states
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heuristic_act.json"))
    ap.add_argument("--scale", type=float, default=1.0, help="multiply the bin counts (a rehearsal at a small size measures overheads only)")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "launches_per_event_pair": LAUNCHES, "rounds": ROUNDS,
           "method": "HIP events around %d back-to-back launches through the C ABI; the configurations of a geometry alternate within each of %d "
                     "rounds; median, 10th and 90th percentile over the rounds, microseconds per launch" % (LAUNCHES, ROUNDS),
           "geometries": {}}
    for size, rotation, n in GEOMS:
        key = "%dx%dx%d%s" % (size + ("+rot" if rotation else "",))
        out["geometries"][key] = geometry(size, rotation, max(1, int(n * args.scale)))
        print(key, json.dumps(out["geometries"][key]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
