#!/usr/bin/env python3
"""Times the native half of a PPO update (include/bpp_ppo.h) against the torch expressions it replaces.

    python tools/bench_ppo.py [--out profiles/ppo.json]

Cells: T * N = 320 rows in 4 mini-batches and 327 680 rows in 32, at M = 100 and M = 200.  Three things per cell, native and torch
alternated batch by batch in one process on the same tensors, every sample a batch of back-to-back calls between two device events:
  loss      one mini-batch loss with its backward to the network's outputs (leaf tensors stand for them):
            native = ppo_loss(...).backward() through the rollout's slabs and the mini-batch's indices;
            torch  = seven index_selects of the rollout (mask rows included), bpp_masked_evaluate for the head, the expressions of
                     ppo_loss_torch (ppo.py:60-80) around it, autograd
  gather    the observation rows of a mini-batch: native = bpp_gather_rows on obs (400 floats a row); torch = index_select on obs.
            `masks` adds what the torch side must also gather and the native loss reads in place: index_select on the mask rows
  update    one PPO.update (1 epoch) of the stand-in network of tests/golden/make_ppo_golden.py's shape at the cell's sizes:
            native = bpp_amd.PPO on a device storage; torch = the same loop with the torch loss
Reported: median and 10th / 90th percentile, and torch / native of the medians -- wherever it falls.  Needs a HIP device.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bpp_amd
from bpp_amd import ppo as ppo_mod

COEFS = dict(clip_param=0.1, value_loss_coef=0.5, entropy_coef=0.01)
OBS = 400


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def summary(us):
    return {"median_us": float(np.median(us)), "p10_us": float(np.percentile(us, 10)), "p90_us": float(np.percentile(us, 90)), "batches": len(us)}


def alternate(runs, batches, calls):
    samples = {k: [] for k in runs}
    for _ in range(batches):
        for k, fn in runs.items():
            samples[k].append(timed(fn, calls, 2))
    return {k: summary(v) for k, v in samples.items()}


class Net(torch.nn.Module):
    def __init__(self, M, hidden=256):
        super().__init__()
        self.M = M
        self.body = torch.nn.Sequential(torch.nn.Linear(OBS, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, M + 1))

    def forward(self, obs):
        out = self.body(obs)
        return out[:, :self.M], out[:, self.M:], None


def torch_loss(logits, values, m, a, vp, r, old, adv):
    """The torch side's mini-batch loss on gathered tensors: bpp_masked_evaluate for the head, ppo.py:60-80 in torch."""
    logp, ent, _ = bpp_amd.masked_evaluate(logits, m, a)
    ratio = torch.exp(logp - old)
    surr1 = ratio * adv
    surr2 = torch.clamp(ratio, 1.0 - COEFS["clip_param"], 1.0 + COEFS["clip_param"]) * adv
    action_loss = -torch.min(surr1, surr2).mean()
    vpc = vp + (values - vp).clamp(-COEFS["clip_param"], COEFS["clip_param"])
    value_loss = 0.5 * torch.max((values - r).pow(2), (vpc - r).pow(2)).mean()
    return value_loss * COEFS["value_loss_coef"] + action_loss - ent * COEFS["entropy_coef"], value_loss, action_loss, ent


def fill(st, M, g):
    T, N = st.num_steps, st.num_envs
    st.obs.copy_(torch.randn(T + 1, N, OBS, generator=g))
    st.location_masks.copy_((torch.rand(T + 1, N, M, generator=g) < 0.3).float())
    st.value_preds.copy_(torch.randn(T + 1, N, 1, generator=g))
    st.returns.copy_(st.value_preds + torch.randn(T + 1, N, 1, generator=g))
    st.actions.copy_(torch.randint(0, M, (T, N, 1), generator=g))
    st.action_log_probs.copy_(-torch.rand(T, N, 1, generator=g) * 4)


def torch_update(net, opt, st, mini):
    """bpp_amd.PPO.update's loop with the torch side's gathers and loss (one epoch)."""
    adv = st.returns[:-1] - st.value_preds[:-1]
    adv = (adv - adv.mean()) / (adv.std() + 1e-5)
    acc = None
    for b in st.feed_forward_generator(adv, mini):
        i = b.indices
        E = st.num_steps * st.num_envs
        sel = lambda t: t.reshape(E, -1).index_select(0, i)                             # noqa: E731
        logits, values, _ = net(sel(st.obs[:-1]))
        loss, vl, al, ent = torch_loss(logits.contiguous(), values, sel(st.location_masks[:-1]), sel(st.actions), sel(st.value_preds[:-1]),
                                       sel(st.returns[:-1]), sel(st.action_log_probs), sel(adv))
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 0.5)
        opt.step()
        t = torch.stack([vl, al, ent]).detach()
        acc = t if acc is None else acc + t
    return acc


def bench(T, N, M, mini, batches, calls, dev):
    g = torch.Generator(device="cpu").manual_seed(T * N + M)
    cpu = bpp_amd.RolloutStorage(T, N, (OBS,), bpp_amd.Discrete(M))
    fill(cpu, M, g)
    st = bpp_amd.RolloutStorage(T, N, (OBS,), bpp_amd.Discrete(M), device=dev)
    for k, v in cpu._slabs.items():
        st._slabs[k].copy_(v)
    E, B = T * N, T * N // mini
    adv = st.normalized_advantages()
    idx = torch.randperm(E, generator=g)[:B].to(dev)
    logits = (torch.randn(B, M, generator=g) * 3).to(dev).requires_grad_(True)
    values = torch.randn(B, 1, generator=g).to(dev).requires_grad_(True)
    leaves = (logits, values)
    flat = lambda t: t.reshape(E, -1)                                                   # noqa: E731
    masks, obs = flat(st.location_masks[:-1]), flat(st.obs[:-1])
    batch = ppo_mod.MiniBatch(st, idx, adv)

    def native_loss():
        for t in leaves:
            t.grad = None
        out = st.ppo_loss(logits, values, None, batch, adv, **COEFS)
        out.backward()
        return out.terms

    def torch_side_loss():
        for t in leaves:
            t.grad = None
        sel = lambda t: flat(t).index_select(0, idx)                                    # noqa: E731
        out = torch_loss(logits, values, sel(st.location_masks[:-1]), sel(st.actions), sel(st.value_preds[:-1]), sel(st.returns[:-1]),
                         sel(st.action_log_probs), sel(adv))
        out[0].backward()
        return torch.stack(out).detach()

    cell = {"T": T, "N": N, "E": E, "M": M, "mini_batches": mini, "B": B}
    tn, gn = native_loss().cpu().numpy(), [t.grad.clone() for t in leaves]
    tt = torch_side_loss().cpu().numpy()
    cell["terms_native"], cell["terms_torch"] = tn[:3].tolist(), tt[1:].tolist()
    cell["max_abs_gradient_difference"] = [float((t.grad - g0).abs().max()) for t, g0 in zip(leaves, gn)]
    cell["loss"] = alternate({"native": native_loss, "torch": torch_side_loss}, batches, calls)
    cell["gather"] = alternate({"native": lambda: bpp_amd.gather_rows(obs, idx), "torch": lambda: obs.index_select(0, idx),
                                "torch_masks": lambda: masks.index_select(0, idx)}, batches, calls)
    nets = [Net(M).to(dev) for _ in range(2)]
    nets[1].load_state_dict(nets[0].state_dict())
    agent = bpp_amd.PPO(nets[0], COEFS["clip_param"], 1, mini, COEFS["value_loss_coef"], COEFS["entropy_coef"], lr=1e-4, eps=1e-5, max_grad_norm=0.5)
    opt = torch.optim.Adam(nets[1].parameters(), lr=1e-4, eps=1e-5)
    cell["update"] = alternate({"native": lambda: agent.update(st), "torch": lambda: torch_update(nets[1], opt, st, mini).tolist()},
                               max(3, batches // 2), 1)
    for k in ("loss", "gather", "update"):
        cell[k]["torch_over_native"] = cell[k]["torch"]["median_us"] / cell[k]["native"]["median_us"]
    cell["gather"]["torch_with_masks_over_native"] = (cell["gather"]["torch"]["median_us"] + cell["gather"]["torch_masks"]["median_us"]) / \
        cell["gather"]["native"]["median_us"]
    return cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ppo.json"))
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ppo.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev),
           "method": "device events around batches of %d back-to-back calls (update: 1), native and torch alternated batch by batch; median and "
                     "10th / 90th percentile of the per-call time over %d batches; leaf tensors stand for the network's outputs in `loss`"
                     % (args.calls, args.batches), "cells": []}
    for T, N, mini in ((5, 64, 4), (5, 65536, 32)):
        for M in (100, 200):
            cell = bench(T, N, M, mini, args.batches, args.calls, dev)
            res["cells"].append(cell)
            print(json.dumps(cell), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
