#!/usr/bin/env python3
"""MCTS with one of the reference's pretrained 10x10x10 checkpoints on a whole test set IN ONE BATCH.

What MCTS/mcts_test.py does one trajectory at a time -- an MCTree over the k known items, sim_times simulations with the
network's evaluate(obs, False) at every expansion and rollout step, sample_action, the real step, succeed -- here runs for
every trajectory of cut_2.pt (tests/golden/cut2_dataset_10.npz: 2 100 trajectories) at once: real bin r plays trajectory
r, scratch bins [n, 2n) hold the simulations' copies, and one MCTSearch decision (every forward batched over the slots)
plus one step of the live bins is a lock-step.  The greedy evaluation of the same checkpoint (examples/evaluate_checkpoint.py)
gives mean ratio 0.6631 and 17.593 items.

    python examples/mcts_checkpoint.py --checkpoint <reference>/pretrained_models/default_cut_2.pt [--limit N] [--sims 100] [--native]

The network is the reference's CNNPro (acktr/model.py:265-323) rebuilt from plain torch layers: the actor path and the
critic head of examples/multibin_checkpoint.py, which gives the value.  --native runs it as bpp_amd.NativePolicy instead: one
fused call per forward (value and logits; MCTS reads no mask prediction).
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import torch  # noqa: E402

import bpp_amd  # noqa: E402
from multibin_checkpoint import load_actor_critic  # noqa: E402

DATASET = os.path.join(ROOT, "tests", "golden", "cut2_dataset_10.npz")


def evaluate(checkpoint, device="cuda:0", limit=None, k=4, sims=100, seed=0, native=False):
    """-> dict(ratio float64 [n], counter int32 [n], lock_steps, seconds, overflow).
    native: the network is bpp_amd.NativePolicy (one fused call per forward) instead of torch layers."""
    dev = torch.device(device)
    size = (10, 10, 10)
    pool = bpp_amd.sequences.from_dataset(DATASET, size, first_index=0)                 # row r = trajectory r
    n = pool.shape[0] if limit is None else min(int(limit), pool.shape[0])
    pool = pool[:n]
    env = bpp_amd.BppVecEnv(2 * n, size, pool=pool, device=dev, compute_mask=False)
    env.reset()
    ms = bpp_amd.MCTSearch(env, k, sim_times=sims)
    ids = torch.arange(n, device=dev)
    ms.seed(ids, ids + seed)
    if native:
        net = bpp_amd.NativePolicy.from_checkpoint(checkpoint, size[0], size[0] * size[1]).to(dev)

        def policy(obs):
            value, logits, _ = net(obs, want=("value", "logits"))
            return value, logits, None
    else:
        net = load_actor_critic(checkpoint, size[0], size[0] * size[1], dev)

        def policy(obs):
            with torch.no_grad():
                value, logits = net(obs)
            return value, logits, None

    live = ids.clone()
    ratio = torch.zeros(n, dtype=torch.float64, device=dev)
    counter = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    t = 0
    while live.numel():
        action, _ = ms.decide(policy, live, live + n, check=False)
        res = env.step_bins(live, action, check=False)
        ms.advance(res.done)
        fin = res.done.bool()
        ratio[live[fin]] = res.ratio[fin]
        counter[live[fin]] = res.counter[fin]
        live = live[~fin]
        t += 1
    torch.cuda.synchronize(dev)
    return dict(ratio=ratio.cpu().numpy(), counter=counter.cpu().numpy(), lock_steps=t, seconds=time.perf_counter() - t0,
                overflow=int(ms.overflow.item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--limit", type=int)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--native", action="store_true", help="run the network as bpp_amd.NativePolicy (one fused call per forward)")
    args = ap.parse_args()
    r = evaluate(args.checkpoint, limit=args.limit, k=args.k, sims=args.sims, native=args.native)
    print("%d trajectories of 10x10x10 in one batch, k = %d, %d simulations, %d lock-steps, %.1f s: average ratio %.4f, "
          "average item number %.4f (greedy evaluate_checkpoint.py: 0.6631 / 17.593), overflow %d" % (
              len(r["ratio"]), args.k, args.sims, r["lock_steps"], r["seconds"], r["ratio"].mean(), r["counter"].mean(),
              r["overflow"]))


if __name__ == "__main__":
    main()
