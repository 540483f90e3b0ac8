#!/usr/bin/env python3
"""Cost of one lookahead expansion: n branches are cloned from n source bins, stepped once and their
masks read -- what a BPP-k reorder or MCTS search does per expansion (acktr/reorder.py:245-262, MCTS/node.py:92-137).

  today:  clone_into(src, dst) + step_subset(dst, a) + mask[dst]    (full-batch launches: cost grows with E)
  native: clone_bins(src, dst) + step_bins(dst, a) + the compact mask (include/bpp_branch.h: cost grows with n)

Every expansion re-clones the same sources, so each rep does the same work.  Time = HIP events around `--reps` back-to-back
expansions after a warm-up, per expansion (host overhead included: it is what a search loop pays).  Static CUT-2 pool.

    python tools/bench_lookahead.py [--reps 50] [--out profiles/lookahead_bench.json]
    python tools/bench_lookahead.py --stats-csv <rocprofv3 kernel_stats.csv>     (kernel times of a traced run as JSON)
"""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [("10x10x10", (10, 10, 10), False), ("10x10x10_rot", (10, 10, 10), True), ("20x20x20", (20, 20, 20), False)]
ENVS = (4096, 65536)
BRANCHES = (64, 1024, 16384)


def time_expansions(fn, reps, warmup=5):
    import torch
    for t in range(warmup):
        fn(t)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(reps):
        fn(t)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per expansion


def bench_one(size, rot, E, n, reps):
    import torch
    import bpp_amd
    env = bpp_amd.BppVecEnv(E, size, enable_rotation=rot, pool=bpp_amd.sequences.cut2_pool(size, 4096, seed=1))
    env.reset()
    env.rollout_uniform(seed=1, step0=0, nsteps=6)      # bins with some boxes in them
    g = torch.Generator().manual_seed(n)
    perm = torch.randperm(E, generator=g).to(env.device)
    src, dst = perm[:n].contiguous(), perm[n:2 * n].contiguous()
    a = env.sample_feasible(seed=2, step=0)[src].contiguous()   # feasible for the fresh clones of src

    def today(t):
        env.clone_into(src, dst)
        r = env.step_subset(dst, a)
        return r.mask[dst]

    def native(t):
        env.clone_bins(src, dst, check=False)
        return env.step_bins(dst, a, check=False).mask

    # same results first: both paths leave the branches in the same state and show the same masks
    m_today = today(0).clone()
    h_today, s_today = env.hmap[dst].clone(), env.state[dst].clone()
    m_native = native(0)
    same = bool(torch.equal(m_today, m_native) and torch.equal(h_today, env.hmap[dst]) and torch.equal(s_today, env.state[dst]))
    res = {"E": E, "n": n, "same_results": same}
    for name, fn in (("today", today), ("native", native)):
        us = time_expansions(fn, reps)
        res[name + "_us_per_expansion"] = round(us, 1)
        res[name + "_branches_per_s"] = round(n / (us * 1e-6))
    res["speedup"] = round(res["today_us_per_expansion"] / res["native_us_per_expansion"], 2)
    del env
    torch.cuda.empty_cache()
    return res


def stats_json(path):
    """rocprofv3 --kernel-trace --stats: the kernel_stats CSV as a list of {kernel, calls, total_ms, avg_us} rows."""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append({"kernel": r["Name"], "calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3),
                         "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                         "max_us": round(float(r["MaxNs"]) / 1e3, 2)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--envs", type=int, nargs="*", default=list(ENVS))
    ap.add_argument("--branches", type=int, nargs="*", default=list(BRANCHES))
    ap.add_argument("--configs", nargs="*", default=[c[0] for c in CONFIGS])
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats-csv", default=None)
    args = ap.parse_args()
    if args.stats_csv:
        print(json.dumps({"kernel_stats": stats_json(args.stats_csv)}, indent=1))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lookahead needs a HIP device")
    results = []
    for name, size, rot in CONFIGS:
        if name not in args.configs:
            continue
        for E in args.envs:
            for n in args.branches:
                if 2 * n > E:           # src and dst are disjoint sets of bins
                    results.append({"config": name, "E": E, "n": n, "skipped": "2 n > E"})
                    continue
                r = bench_one(size, rot, E, n, args.reps)
                r["config"] = name
                results.append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
    # the targets of the issue this tool was written for: native cost independent of E at n = 1024 (within 15 %), >= 5x
    # today's at n <= 1024 in a 65 536-bin env
    summary = {}
    for name, _, _ in CONFIGS:
        by = {(r["E"], r["n"]): r for r in results if r.get("config") == name and "skipped" not in r}
        if (4096, 1024) in by and (65536, 1024) in by:
            summary[name + "_native_E65536_over_E4096_n1024"] = round(by[(65536, 1024)]["native_us_per_expansion"] /
                                                                       by[(4096, 1024)]["native_us_per_expansion"], 3)
        sp = [by[(65536, n)]["speedup"] for n in (64, 1024) if (65536, n) in by]
        if sp:
            summary[name + "_min_speedup_E65536_n_le_1024"] = min(sp)
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "results": results, "summary": summary}
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
