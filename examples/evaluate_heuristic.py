#!/usr/bin/env python3
"""Evaluate the lowest-top packing heuristic on a whole test set IN ONE BATCH on the HIP environment.

examples/evaluate_checkpoint.py with the heuristic in place of the network: every trajectory of the dataset is one bin of ONE
BppVecEnv (2 100 bins for cut_2.pt); a lock-step is one bpp_heuristic_act (include/bpp_heuristic.h: lowest resulting top, then
smoothest surface, then lowest index) and one fused environment step; a bin that has finished its trajectory is left alone
(BPP_ACTION_NOOP).  The two averages it prints are what a checkpoint's are compared with on the same trajectories.

    python examples/evaluate_heuristic.py [--dataset tests/golden/cut2_dataset_10.npz | <reference>/dataset/cut_2.pt]
        [--rotation] [--rule lowest_top | lowest_top_plain] [--plans OUT.npz]

--plans OUT.npz: also record where every box was placed and write every trajectory's finished packing plan to OUT.npz; the plans
are then checked by bpp_amd.replay_plans, which rebuilds every bin from its plan.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bpp_amd

DATASET = os.path.join(ROOT, "tests", "golden", "cut2_dataset_10.npz")


def evaluate(dataset=DATASET, rotation=False, rule="lowest_top", device="cuda:0", size=(10, 10, 10), limit=None, plans=False):
    """-> dict(ratio float64 [n], counter int32 [n], steps int32 [n], lock_steps, seconds): trajectory i of `dataset` (a .pt of
    the reference's or an .npz pool) packed by the heuristic, all of them at once.  limit: only the first `limit` trajectories.
    plans: also record the packing plans; the dict then has `plans`, the PackingPlans of every trajectory's finished episode."""
    dev = torch.device(device)
    pool = bpp_amd.sequences.from_dataset(dataset, size, first_index=0)          # row r = trajectory r
    n = pool.shape[0] if limit is None else min(int(limit), pool.shape[0])
    env = bpp_amd.BppVecEnv(n, size, enable_rotation=rotation, pool=pool, device=dev)    # episode 0 of bin g plays row g
    env.reset()
    if plans:
        env.record_placements()
    live = torch.ones(n, dtype=torch.bool, device=dev)
    ratio = torch.zeros(n, dtype=torch.float64, device=dev)
    counter = torch.zeros(n, dtype=torch.int32, device=dev)
    steps = torch.zeros(n, dtype=torch.int32, device=dev)
    noop = torch.full((n,), env.NOOP, dtype=torch.int64, device=dev)
    action = torch.empty(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    t = 0
    while bool(live.any()):
        env.heuristic_act(rule, out=action)
        res = env.step_tensors(torch.where(live, action, noop))
        fin = live & res.done.reshape(-1).bool()
        ratio = torch.where(fin, res.ratio.reshape(-1), ratio)
        counter = torch.where(fin, res.counter.reshape(-1), counter)
        steps += live.to(torch.int32)
        live = live & ~fin
        t += 1
    torch.cuda.synchronize(dev)
    out = dict(ratio=ratio.cpu().numpy(), counter=counter.cpu().numpy(), steps=steps.cpu().numpy(), lock_steps=t,
               seconds=time.perf_counter() - t0)
    if plans:
        out["plans"] = env.placements(finished=True)
    return out


def check_plans(plans, path, ratio):
    """Write `plans` to `path`, read them back, replay them box by box -> (plans sound, plans whose volume reproduces `ratio`)."""
    plans.save(path)
    W, L, H = plans.size
    _, status, volume = bpp_amd.replay_plans(bpp_amd.PackingPlans.load(path), device=plans.records.device)
    return int((status == -1).sum()), int((volume.cpu().numpy() / float(W * L * H) == ratio).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default=DATASET)
    ap.add_argument("--rotation", action="store_true")
    ap.add_argument("--rule", default="lowest_top", choices=bpp_amd.heuristic.RULES)
    ap.add_argument("--plans", default=None, metavar="OUT.npz", help="record the packing plans and write every trajectory's finished plan there")
    args = ap.parse_args()
    r = evaluate(args.dataset, args.rotation, args.rule, plans=bool(args.plans))
    print("%d trajectories in one batch, %d lock-steps, %.2f s: average space utilization %.4f, average put item number %.4f, "
          "completely packed bins %d" % (len(r["ratio"]), r["lock_steps"], r["seconds"], r["ratio"].mean(), r["counter"].mean(),
                                         int((r["ratio"] == 1.0).sum())))
    if args.plans:
        sound, same = check_plans(r["plans"], args.plans, r["ratio"])
        print("%d packing plans written to %s: %d sound when replayed box by box, %d reproduce their trajectory's utilization as "
              "volume / (W L H), %d records dropped" % (len(r["plans"]), args.plans, sound, same, int(r["plans"].numpy()["overflow"][0])))


if __name__ == "__main__":
    main()
