#!/usr/bin/env python3
"""Times the fused loss of the A2C update (bpp_a2c_loss through bpp_amd.a2c_loss) against the expression it replaces:
bpp_masked_evaluate + the torch terms + loss.backward() (examples/train_with_storage.py without --fused-loss).

    python tools/bench_a2c_loss.py [--out profiles/a2c_loss.json]

Cells: E = 5 x 65 536 and 5 x 4 096 rows, M = 100 and 200.  The network is left out: logits, values and predicted mask are leaf
tensors, both sides end with their gradients in `.grad`.  Three things are timed in the same process on the same tensors,
alternating batch by batch:
  parent          masked_evaluate, the torch terms, loss.backward()
  fused           a2c_loss(...).backward() -- for LEAF tensors autograd copies each incoming gradient into `.grad` (it does not
                  adopt a buffer somebody else holds), two passes over [E, M] a network's backward does not make
  fused_call      a2c_loss(...) alone: terms and all three gradients are complete when it returns
Every sample is a batch of back-to-back calls between two device events: device time per call with the enqueue cost in it.
Reported: median and 10th / 90th percentile over the batches, the ratios of the medians, and for fused_call the bytes the
algorithm moves (from the shapes) per second against the rate a copy kernel reaches from HBM.  Needs a HIP
device; there is no CPU mode.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bpp_amd

COPY_KERNEL_RATE = 6.29e12      # bytes/s a copy kernel reaches from HBM on the MI355X
COEFS = dict(value_loss_coef=0.5, entropy_coef=0.01, invalid_coef=2.0, mask_coef=5.0)


def a2c_bytes(E, M):
    """Bytes one bpp_a2c_loss call must read and write: three [E, M] inputs, two [E, M] gradients, the per-row vectors."""
    return E * M * 4 * 5 + E * (8 + 4 + 4 + 4)


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


def bench(E, M, batches, calls, dev):
    g = torch.Generator(device="cpu").manual_seed(E + M)
    logits = (torch.randn(E, M, generator=g) * 3).to(dev).requires_grad_(True)
    values = (torch.randn(E, 1, generator=g) * 2).to(dev).requires_grad_(True)
    pred = torch.rand(E, M, generator=g).to(dev).requires_grad_(True)
    truth = (torch.rand(E, M, generator=g) < 0.3).float().to(dev)
    action = torch.randint(0, M, (E, 1), generator=g).to(dev)
    returns = (torch.randn(E, 1, generator=g) * 2).to(dev)
    leaves = (logits, values, pred)

    def parent():
        for t in leaves:
            t.grad = None
        logp, ent, prob = bpp_amd.masked_evaluate(logits, truth, action)
        adv = returns - values
        value_loss = adv.pow(2).mean()
        action_loss = -(adv.detach() * logp).mean()
        graph_loss = torch.nn.functional.mse_loss(pred, truth)
        loss = value_loss * COEFS["value_loss_coef"] + action_loss + prob * COEFS["invalid_coef"] - ent * COEFS["entropy_coef"] + \
            COEFS["mask_coef"] * graph_loss
        loss.backward()
        return torch.stack([value_loss, action_loss, ent, prob, graph_loss, loss]).detach()

    def fused():
        for t in leaves:
            t.grad = None
        out = bpp_amd.a2c_loss(logits, values, pred, truth, action, returns, **COEFS)
        out.backward()
        return out.terms

    def fused_call():
        return bpp_amd.a2c_loss(logits, values, pred, truth, action, returns, **COEFS).terms

    cell = {"E": E, "M": M}
    # the same numbers first
    tp = parent().cpu().numpy()
    gp = [t.grad.clone() for t in leaves]
    tf = fused().cpu().numpy()
    cell["terms_parent"], cell["terms_fused"] = tp.tolist(), tf.tolist()
    cell["max_abs_gradient_difference"] = [float((t.grad - g0).abs().max()) for t, g0 in zip(leaves, gp)]
    cell["max_abs_gradient"] = [float(g0.abs().max()) for g0 in gp]
    cell["fused_terms_repeat_bit_for_bit"] = bool(np.array_equal(fused().cpu().numpy().view(np.uint32), tf.view(np.uint32)))
    runs = {"parent": parent, "fused": fused, "fused_call": fused_call}
    samples = {k: [] for k in runs}
    for _ in range(batches):
        for k, fn in runs.items():
            samples[k].append(timed(fn, calls, 3))
    for k, v in samples.items():
        cell[k] = summary(v)
    for k in ("fused", "fused_call"):
        cell[k]["speedup_over_parent"] = cell["parent"]["median_us"] / cell[k]["median_us"]
    nbytes = a2c_bytes(E, M)
    cell["fused_call"]["bytes"] = nbytes
    cell["fused_call"]["bytes_per_s"] = nbytes / (cell["fused_call"]["median_us"] * 1e-6)
    cell["fused_call"]["fraction_of_copy_kernel_rate"] = cell["fused_call"]["bytes_per_s"] / COPY_KERNEL_RATE
    return cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "a2c_loss.json"))
    ap.add_argument("--batches", type=int, default=11)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_a2c_loss.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "copy_kernel_bytes_per_s": COPY_KERNEL_RATE,
           "method": "device events around batches of %d back-to-back calls, the three sides alternated batch by batch; median and 10th / "
                     "90th percentile of the per-call time over %d batches; leaf tensors stand for the network's outputs" % (args.calls, args.batches),
           "cells": []}
    for E in (5 * 65536, 5 * 4096):
        for M in (100, 200):
            cell = bench(E, M, args.batches, args.calls, dev)
            res["cells"].append(cell)
            print(json.dumps(cell), flush=True)
    res["fused_faster_than_parent_in_every_cell"] = all(c["fused"]["median_us"] < c["parent"]["median_us"] for c in res["cells"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
