#!/usr/bin/env python3
"""Evaluate one of the reference's pretrained checkpoints on a whole test set IN ONE BATCH on the HIP environment.

What the reference's test mode does one trajectory at a time (main.py:26-29 -> unified_test.py:29-67, model_loader.py:9-35
with --preview 1): play every trajectory of dataset/cut_2.pt greedily -- the actor's argmax under the true feasibility
mask -- and report the mean space utilisation and the mean number of packed items.  Here every trajectory is one bin of
ONE BppVecEnv (2 100 bins for cut_2.pt); a lock-step is one policy forward on the device, one bpp_masked_act
(softmax(x - 14 (1 - mask)) + 1e-5, mode; acktr/distributions.py:71-84) and one fused environment step; a bin that has
finished its trajectory is left alone (BPP_ACTION_NOOP).

    python examples/evaluate_checkpoint.py --checkpoint <reference>/pretrained_models/default_cut_2.pt \
        --dataset <reference>/dataset/cut_2.pt [--rotation] [--plans OUT.npz]

--plans OUT.npz: also record where every box was placed (BppVecEnv.record_placements; the reference's space.boxes) and write every
trajectory's finished packing plan to OUT.npz (bpp_amd.PackingPlans.load reads it back; .boxes(i) is trajectory i's list of
(x, y, z, lx, ly, lz), .write_txt(path, i) the line format of user_study/user_study.py); the plans are then checked by
bpp_amd.replay_plans, which rebuilds every bin from its plan.

Only this package and torch are needed: the actor below is the reference's CNNPro actor path (acktr/model.py:265-323)
rebuilt from plain torch layers; the checkpoint's keys are mapped onto it (`base.share.N.module.weight` -> share.N.weight,
`add_bias._bias` [C, 1] -> bias [C], as main.py:66-76 does for the reference's own modules).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import bpp_amd
from rollout_with_policy import Actor


def load_actor(path, side, n_actions, device, hidden=256):
    """The reference checkpoint (a (state_dict, ob_rms) pair saved by main.py:186-191) -> Actor on `device`."""
    state, ob_rms = torch.load(path, map_location="cpu", weights_only=False)
    if ob_rms is not None:
        raise ValueError("checkpoint carries observation statistics (VecNormalize ob=True); the BPP checkpoints do not")
    sd = {}
    for k, v in state.items():
        k = k.replace("module.", "").replace("add_bias.", "").replace("_bias", "bias")
        if v.dim() <= 3:
            v = v.squeeze(-1)
        if k.startswith("base.share.") or k.startswith("base.actor."):
            sd[k[len("base."):]] = v
        elif k.startswith("dist.linear."):
            sd["linear." + k[len("dist.linear."):]] = v
    actor = Actor(side, n_actions, hidden)
    actor.load_state_dict(sd)
    return actor.to(device).eval()


def evaluate(checkpoint, dataset, rotation=False, device="cuda:0", size=(10, 10, 10), policy_device=None, limit=None, native=False, plans=False):
    """-> dict(ratio float64 [n], counter int32 [n], steps int32 [n], seconds): trajectory i of `dataset` played greedily
    by the checkpoint, all of them at once.  policy_device: where the network runs (default: the env's device).
    native: the network is bpp_amd.NativePolicy (one fused call per lock-step, logits only) instead of torch layers.
    plans: also record the packing plans; the dict then has `plans`, the PackingPlans of every trajectory's finished episode."""
    dev = torch.device(device)
    pdev = torch.device(policy_device) if policy_device else dev
    pool = bpp_amd.sequences.from_dataset(dataset, size, first_index=0)          # row r = trajectory r
    n = pool.shape[0] if limit is None else min(int(limit), pool.shape[0])
    env = bpp_amd.BppVecEnv(n, size, enable_rotation=rotation, pool=pool, device=dev)    # episode 0 of bin g plays row g
    if native:
        policy = bpp_amd.NativePolicy.from_checkpoint(checkpoint, size[0], env.action_space.n).to(pdev)

        def actor(x):
            return policy(x, want=("logits",))[1]
    else:
        actor = load_actor(checkpoint, size[0], env.action_space.n, pdev)
    obs = env.reset()
    if plans:
        env.record_placements()
    mask = env.location_masks
    live = torch.ones(n, dtype=torch.bool, device=dev)
    ratio = torch.zeros(n, dtype=torch.float64, device=dev)
    counter = torch.zeros(n, dtype=torch.int32, device=dev)
    steps = torch.zeros(n, dtype=torch.int32, device=dev)
    noop = torch.full((n,), env.NOOP, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    t = 0
    while bool(live.any()):
        with torch.no_grad():
            logits = actor(obs.to(pdev)).float().to(dev)
        action, _ = bpp_amd.masked_act(logits, mask, deterministic=True)
        res = env.step_tensors(torch.where(live, action.reshape(-1), noop))
        fin = live & res.done.reshape(-1).bool()
        ratio = torch.where(fin, res.ratio.reshape(-1), ratio)
        counter = torch.where(fin, res.counter.reshape(-1), counter)
        steps += live.to(torch.int32)
        live = live & ~fin
        obs, mask = res.obs, res.mask
        t += 1
    torch.cuda.synchronize(dev)
    out = dict(ratio=ratio.cpu().numpy(), counter=counter.cpu().numpy(), steps=steps.cpu().numpy(), lock_steps=t,
               seconds=time.perf_counter() - t0)
    if plans:
        out["plans"] = env.placements(finished=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--rotation", action="store_true")
    ap.add_argument("--policy-device", default=None)
    ap.add_argument("--native", action="store_true", help="run the network as bpp_amd.NativePolicy (one fused call per lock-step)")
    ap.add_argument("--plans", default=None, metavar="OUT.npz", help="record the packing plans and write every trajectory's finished plan there")
    args = ap.parse_args()
    r = evaluate(args.checkpoint, args.dataset, args.rotation, policy_device=args.policy_device, native=args.native, plans=bool(args.plans))
    print("%d trajectories in one batch, %d lock-steps, %.2f s: average space utilization %.4f, average put item number %.4f, "
          "completely packed bins %d" % (len(r["ratio"]), r["lock_steps"], r["seconds"], r["ratio"].mean(), r["counter"].mean(),
                                         int((r["ratio"] == 1.0).sum())))
    if args.plans:
        plans = r["plans"]
        plans.save(args.plans)
        W, L, H = plans.size
        _, status, volume = bpp_amd.replay_plans(bpp_amd.PackingPlans.load(args.plans), device=plans.records.device)
        sound = int((status == -1).sum())
        same = int((volume.cpu().numpy() / float(W * L * H) == r["ratio"]).sum())
        print("%d packing plans written to %s: %d sound when replayed box by box, %d reproduce their trajectory's utilization as "
              "volume / (W L H), %d records dropped" % (len(plans), args.plans, sound, same, int(plans.numpy()["overflow"][0])))


if __name__ == "__main__":
    main()
