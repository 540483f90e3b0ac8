#!/usr/bin/env python3
"""Multi-bin packing with one of the reference's pretrained 10x10x10 checkpoints on a whole test set IN ONE BATCH.

What multi_bin/multi_bin.py does one trajectory at a time -- cut the 20x20x10 pallet into 10x10 windows, ask the network
for a value and a position in every window, pick a window by the advantage rule, step -- here runs for every trajectory
of the 4-bin set (dataset/4bins_cut_2.pt, tests/golden/cut2_dataset_4bins_20x20x10.npz: 2 100 trajectories) at once: one
pallet per trajectory of ONE BppVecEnv, one MultiBinPacker decision (emit, the network's forward over 4 window rows per
pallet, choose) and one step of the live pallets per lock-step.  The pool is what the reference's LoadBoxCreator plays:
its pre-incremented index (pallet r plays trajectory r + 1) and the [20, 20, 10] that ends every stored trajectory (the
[10, 10, 10] the creator appends after it is never reached: nothing fits after [20, 20, 10]).

    python examples/multibin_checkpoint.py --checkpoint <reference>/pretrained_models/default_cut_2.pt [--limit N] [--native]

The network is the reference's CNNPro (acktr/model.py:265-323) rebuilt from plain torch layers: the actor path of
examples/evaluate_checkpoint.py plus the critic (base.critic.*, base.critic_linear.*), which gives the value.  --native runs it
as bpp_amd.NativePolicy of the window's side instead: one fused call over the 4 window rows of every pallet.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from torch import nn  # noqa: E402

import bpp_amd  # noqa: E402

DATASET = os.path.join(ROOT, "tests", "golden", "cut2_dataset_4bins_20x20x10.npz")


class ActorCritic(nn.Module):
    """CNNPro's shared trunk, actor head with the distribution's linear layer, and critic head (no mask head: the
    reference's multi_bin evaluates with use_mask=False)."""

    def __init__(self, side, n_actions, hidden=256):
        super().__init__()
        layers, c = [], 4
        for _ in range(5):
            layers += [nn.Conv2d(c, 64, 3, padding=1), nn.ReLU()]
            c = 64
        self.share = nn.Sequential(*layers)
        self.actor = nn.Sequential(nn.Conv2d(64, 8, 1), nn.ReLU(), nn.Flatten(), nn.Linear(8 * side * side, hidden), nn.ReLU())
        self.critic = nn.Sequential(nn.Conv2d(64, 4, 1), nn.ReLU(), nn.Flatten(), nn.Linear(4 * side * side, hidden), nn.ReLU())
        self.critic_linear = nn.Linear(hidden, 1)
        self.linear = nn.Linear(hidden, n_actions)
        self.side = side

    def forward(self, obs):
        s = self.share(obs.reshape(-1, 4, self.side, self.side))
        return self.critic_linear(self.critic(s)), self.linear(self.actor(s))


def load_actor_critic(path, side, n_actions, device, hidden=256):
    """The reference checkpoint (a (state_dict, ob_rms) pair saved by main.py:186-191) -> ActorCritic on `device`."""
    state, ob_rms = torch.load(path, map_location="cpu", weights_only=False)
    if ob_rms is not None:
        raise ValueError("checkpoint carries observation statistics (VecNormalize ob=True); the BPP checkpoints do not")
    sd = {}
    for k, v in state.items():
        k = k.replace("module.", "").replace("add_bias.", "").replace("_bias", "bias")
        if v.dim() <= 3:
            v = v.squeeze(-1)
        if k.startswith(("base.share.", "base.actor.", "base.critic.", "base.critic_linear.")):
            sd[k[len("base."):]] = v
        elif k.startswith("dist.linear."):
            sd["linear." + k[len("dist.linear."):]] = v
    net = ActorCritic(side, n_actions, hidden)
    net.load_state_dict(sd)
    return net.to(device).eval()


def evaluate(checkpoint, device="cuda:0", limit=None, window=10, stride=10, native=False):
    """-> dict(ratio float64 [n], counter int32 [n], steps int32 [n], lock_steps, seconds).
    native: the network is bpp_amd.NativePolicy of side `window` (one fused call per decision) instead of torch layers."""
    dev = torch.device(device)
    size = (20, 20, 10)
    pool = bpp_amd.sequences.from_dataset(DATASET, size, terminator=(20, 20, 10))       # row r = trajectory r + 1
    n = pool.shape[0] if limit is None else min(int(limit), pool.shape[0])
    env = bpp_amd.BppVecEnv(n, size, pool=pool, device=dev)
    env.reset()
    mb = bpp_amd.MultiBinPacker(env, window, stride)
    if native:
        net = bpp_amd.NativePolicy.from_checkpoint(checkpoint, window, window * window).to(dev)

        def policy(obs):
            value, logits, _ = net(obs, want=("value", "logits"))
            return value, logits, None
    else:
        net = load_actor_critic(checkpoint, window, window * window, dev)

        def policy(obs):
            with torch.no_grad():
                value, logits = net(obs)
            return value, logits, None

    live = torch.arange(n, device=dev)
    ratio = torch.zeros(n, dtype=torch.float64, device=dev)
    counter = torch.zeros(n, dtype=torch.int32, device=dev)
    steps = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    t = 0
    while live.numel():
        action, _, _ = mb.decide(policy, live, check=False)
        res = env.step_bins(live, action, check=False)
        mb.commit(res.done)
        fin = res.done.bool()
        ratio[live[fin]] = res.ratio[fin]
        counter[live[fin]] = res.counter[fin]
        steps[live] += 1
        live = live[~fin]
        t += 1
    torch.cuda.synchronize(dev)
    return dict(ratio=ratio.cpu().numpy(), counter=counter.cpu().numpy(), steps=steps.cpu().numpy(), lock_steps=t,
                seconds=time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--limit", type=int)
    ap.add_argument("--native", action="store_true", help="run the network as bpp_amd.NativePolicy (one fused call per decision)")
    args = ap.parse_args()
    r = evaluate(args.checkpoint, limit=args.limit, native=args.native)
    print("%d trajectories of 20x20x10 in one batch, %d lock-steps, %.2f s: average ratio %.4f, average item number %.4f" % (
        len(r["ratio"]), r["lock_steps"], r["seconds"], r["ratio"].mean(), r["counter"].mean()))


if __name__ == "__main__":
    main()
