#!/usr/bin/env python3
"""The native heads' training pass (bpp_policy_heads_forward_train + bpp_policy_heads_backward) on the device,
float32, 10 x 10, H = 256, M = 100, batch sizes 320 (the reference's 5 x 64), 2 100, 16 384 and 65 536:

  (a) heads    forward + backward of the six Linear layers from given gradients at value, logits and pred to grad_feat and the
               twelve parameter gradients: the two native calls against torch autograd over the same layers on the same feat;
  (b) module   forward + backward of the whole TrainablePolicy from the same output gradients to all 28 parameter gradients:
               heads="native" against heads="torch", the same weights, in the same run.

Method, as tools/bench_policy_train.py: device events around batches of back-to-back calls, the two sides alternated round by
round, medians and p10-p90 over the rounds.  No ratio is promised: rows where native loses are written as they are.

    python tools/bench_policy_heads_train.py --out profiles/policy_heads_train.json
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

import bpp_amd
from bpp_amd import policy as pol


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


def alternated(sides, calls, rounds):
    """{name: summary} of the callables in `sides`, warmed up, then timed in an order that flips every round."""
    for fn in sides.values():
        timed(fn, 2)
    times = {k: [] for k in sides}
    for r in range(rounds):
        for k in list(sides) if r % 2 == 0 else list(sides)[::-1]:
            times[k].append(timed(sides[k], calls))
    return {k: summary(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="320,2100,16384,65536")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_heads_train.json"))
    args = ap.parse_args()
    import policy_cases as pc
    dev = torch.device("cuda:0")
    S, H, M = geom = (10, 256, 100)
    A = S * S
    plain = {k: v.to(dev) for k, v in pc.real_weights(*geom, 11).items()}
    params = {k: plain[k].clone().requires_grad_(True) for k in pol.HEAD_PARAMETERS}
    order = [params[k] for k in pol.HEAD_PARAMETERS]
    blob, blob_bwd = pol.pack_weights(plain, *geom), pol.pack_heads_backward(plain)
    nets = {}
    for mode in pol.HEADS_MODES:
        nets[mode] = bpp_amd.TrainablePolicy(S, M, H, heads=mode).to(dev)
        nets[mode].load_state_dict(plain)
    states = torch.from_numpy(pc.deep_states(False, 64)).to(dev)
    macs = 2 * (8 * A * H + H * M) + 4 * A * H + H           # per bin, forward
    rows = []
    for n in (int(v) for v in args.sizes.split(",")):
        obs = states[torch.arange(n, device=dev) % states.shape[0]].contiguous()
        feat = pol.trunk_forward_train(obs, blob, geom)[0]
        gv, gl, gp = torch.randn(n, device=dev), torch.randn(n, M, device=dev), torch.randn(n, M, device=dev)
        value, logits, pred, hidden = pol.heads_forward_train(feat, blob, geom)
        grad_feat, grad_hidden, grad_out_mask, gw = pol.heads_backward(feat, hidden, pred, gv, gl, gp, geom, blob_bwd)
        ws = torch.empty(pol._lib.lib().bpp_policy_heads_backward_workspace(pol._lib.kfac_geom(geom), n) // 4, dtype=torch.float32, device=dev)

        def native():
            pol.heads_forward_train(feat, blob, geom, value=value, logits=logits, pred=pred, hidden=hidden)
            pol.heads_backward(feat, hidden, pred, gv, gl, gp, geom, blob_bwd, grad_feat=grad_feat, grad_hidden=grad_hidden,
                               grad_out_mask=grad_out_mask, grad_weights=gw, workspace=ws)

        def autograd():
            f = feat.detach().requires_grad_(True)

            def head(name, lo, hi):
                return F.relu(F.linear(f[:, lo * A:hi * A], params[name + ".3.weight"], params[name + ".3.bias"]))

            v = F.linear(head("base.critic", 16, 20), params["base.critic_linear.weight"], params["base.critic_linear.bias"]).reshape(-1)
            lg = F.linear(head("base.actor", 0, 8), params["dist.linear.weight"], params["dist.linear.bias"])
            pr = F.relu(F.linear(head("base.mask", 8, 16), params["base.mask.5.weight"], params["base.mask.5.bias"]))
            torch.autograd.grad([v, lg, pr], [f] + order, [gv, gl, gp])

        def module(mode):
            net = nets[mode]
            weights = list(net.parameters())

            def run():
                torch.autograd.grad(list(net(obs)), weights, [gv, gl, gp])
            return run

        calls = max(1, min(20, 4000 // n))
        heads = alternated({"native": native, "torch_autograd": autograd}, calls, args.rounds)
        whole = alternated({"heads_native": module("native"), "heads_torch": module("torch")}, calls, args.rounds)
        flop = 3 * 2.0 * macs * n
        row = {"n": n, "calls_per_round": calls, "rounds": args.rounds, "heads": heads, "module": whole,
               "heads_native_over_torch": heads["native"]["median_us"] / heads["torch_autograd"]["median_us"],
               "module_native_over_torch": whole["heads_native"]["median_us"] / whole["heads_torch"]["median_us"],
               "heads_native_tflops": flop / heads["native"]["median_us"] * 1e-6, "heads_torch_tflops": flop / heads["torch_autograd"]["median_us"] * 1e-6,
               "info": pol.heads_backward_info(geom, n), "workspace_bytes": ws.numel() * 4, "kept_bytes": (hidden.numel() + grad_hidden.numel() + grad_out_mask.numel()) * 4}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del obs, feat, gv, gl, gp, value, logits, pred, hidden, grad_feat, grad_hidden, grad_out_mask, gw, ws
        for net in nets.values():
            net.release_buffers()
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "mflop_per_bin_forward": 2e-6 * macs,
           "method": "device events around `calls_per_round` back-to-back calls, sides alternated, `rounds` rounds; float32; heads: forward + "
                     "backward of the six Linear layers on the same feat; module: forward + backward of the whole TrainablePolicy, 10 x 10, "
                     "H = 256, M = 100", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
