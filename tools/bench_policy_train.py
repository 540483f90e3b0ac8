#!/usr/bin/env python3
"""The native trunk's training pass (bpp_policy_trunk_forward_train + bpp_policy_trunk_backward) against torch
autograd over the same layers (torch_forward's convolutions) on the device: forward + backward from a given gradient at the head
features to the gradient of every trunk parameter, float32, batch sizes 320 (the reference's 5 x 64), 2 100, 16 384 and 65 536.

Method, as tools/bench_policy.py: device events around batches of back-to-back calls, the two forms alternated round by round,
medians and p10-p90 over the rounds.  TF/s is counted on 3 x the trunk's forward 2 * MAC (forward, input gradient, weight
gradient; share.0 has no input gradient, which is ignored).  No ratio is promised: rows where native loses are written as they are.

    python tools/bench_policy_train.py --out profiles/policy_train.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.nn.functional as F

import bpp_amd  # noqa: F401
from bpp_amd import policy as pol

PEAK_TF = 155.0


def trunk_macs(S):
    return S * S * (36 * 64 + 4 * 576 * 64 + 64 * 20)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # microseconds per call


def summary(xs):
    xs = np.asarray(xs)
    return {"median_us": float(np.median(xs)), "p10_us": float(np.percentile(xs, 10)), "p90_us": float(np.percentile(xs, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="320,2100,16384,65536")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_train.json"))
    args = ap.parse_args()
    import policy_cases as pc
    dev = torch.device("cuda:0")
    S, geom = 10, (10, 256, 100)
    A = S * S
    plain = {k: v.to(dev) for k, v in pc.real_weights(*geom, 11).items() if k in pol.TRUNK_PARAMETERS}
    params = {k: v.clone().requires_grad_(True) for k, v in plain.items()}
    order = [params[k] for k in pol.TRUNK_PARAMETERS]
    blob, blob_bwd = pol.pack_trunk(plain), pol.pack_trunk_backward(plain)
    states = torch.from_numpy(pc.deep_states(False, 64)).to(dev)
    rows = []
    for n in (int(v) for v in args.sizes.split(",")):
        obs = states[torch.arange(n, device=dev) % states.shape[0]].contiguous()
        grad_feat = torch.randn(n, 20 * A, device=dev)
        feat, acts = pol.trunk_forward_train(obs, blob, geom)
        grads, gw = pol.trunk_backward(obs, geom, blob_bwd, feat, acts, grad_feat)
        ws = torch.empty(pol._lib.lib().bpp_policy_trunk_backward_workspace(pol._lib.kfac_geom(geom), n) // 4, dtype=torch.float32, device=dev)

        def native():
            pol.trunk_forward_train(obs, blob, geom, feat=feat, acts=acts)
            pol.trunk_backward(obs, geom, blob_bwd, feat, acts, grad_feat, grads=grads, grad_weights=gw, workspace=ws)

        def native_forward():
            pol.trunk_forward_train(obs, blob, geom, feat=feat, acts=acts)

        def autograd():
            x = obs.reshape(-1, 4, S, S)
            for name in pol.TRUNK:
                x = F.relu(F.conv2d(x, params[name + ".weight"], params[name + ".bias"], padding=1))
            out = torch.cat([F.relu(F.conv2d(x, params[nm + ".weight"], params[nm + ".bias"])) for nm in pol.HEAD_CONVS], 1).flatten(1)
            torch.autograd.grad(out, order, grad_feat)

        calls = max(1, min(20, 4000 // n))
        for fn in (native, autograd, native_forward):                       # warm-up
            timed(fn, 2)
        t_native, t_torch, t_fwd = [], [], []
        for r in range(args.rounds):
            pairs = ((native, t_native), (autograd, t_torch), (native_forward, t_fwd))
            for fn, acc in pairs if r % 2 == 0 else pairs[::-1]:
                acc.append(timed(fn, calls))
        flop = 3 * 2.0 * trunk_macs(S) * n
        a, b, c = summary(t_native), summary(t_torch), summary(t_fwd)
        row = {"n": n, "calls_per_round": calls, "rounds": args.rounds, "native": a, "torch_autograd": b, "native_forward_only": c,
               "native_over_torch": a["median_us"] / b["median_us"], "native_tflops": flop / a["median_us"] * 1e-6,
               "native_fraction_of_155tf": flop / a["median_us"] * 1e-6 / PEAK_TF, "torch_tflops": flop / b["median_us"] * 1e-6,
               "info": pol.trunk_backward_info(geom, n), "workspace_bytes": ws.numel() * 4, "acts_bytes": acts.numel() * 4}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del obs, grad_feat, feat, acts, grads, gw, ws
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "mflop_per_bin_forward": 2e-6 * trunk_macs(S),
           "method": "device events around `calls_per_round` back-to-back calls, forms alternated, `rounds` rounds; float32; forward + "
                     "backward of the five 3x3 layers and the head convolutions, 10 x 10", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
