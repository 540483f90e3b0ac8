#!/usr/bin/env python3
"""PPO (the reference's `--algorithm ppo`, acktr/algo/ppo.py) on a device-resident rollout storage.

    python examples/train_ppo.py --envs 4096 --updates 4
    python examples/train_ppo.py --envs 64 --updates 4 --native-trunk

Per update: `--steps` lock-steps collected as examples/train_with_storage.py collects them (the step kernel writes observation,
mask, reward and done straight into the storage), the returns with GAE from one native call (`storage.compute_returns`), then
`bpp_amd.PPO.update`: `--epochs` passes over the rollout in `--mini-batches` mini-batches, each of them one bpp_gather_rows for
the observation rows and one bpp_ppo_loss around the network (include/bpp_ppo.h) -- feasibility masks, actions, old values,
returns, old log-probabilities and advantages are read in place in the storage.

The network is the stand-in of train_with_storage.py, or with --native-trunk bpp_amd.TrainablePolicy (the rollouts then act on
bpp_amd.NativePolicy refreshed after every update).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import bpp_amd
from train_with_storage import ActorCritic, NativeTrunkNet


def collect(net, actor, env, storage, counter, gamma, gae_lambda):
    """`storage.num_steps` lock-steps into the storage and the GAE returns (main.py:150-181 with use_gae)."""
    for t in range(storage.num_steps):
        with torch.no_grad():
            if actor is not None:
                value, logits, _ = actor(storage.obs[t], want=("value", "logits"))
                value = value.reshape(-1, 1)
            else:
                logits, value, _ = net(storage.obs[t])
        action, logp = bpp_amd.masked_act(logits, storage.location_masks[t], counter=counter)
        counter[1:].add_(1)
        storage.step(env, action, value, logp)
    with torch.no_grad():
        next_value = actor(storage.obs[-1], want=("value",))[0].reshape(-1, 1) if actor is not None else net(storage.obs[-1])[1]
    storage.compute_returns(next_value, True, gamma, gae_lambda, False)


def train(envs=4096, steps=5, updates=4, rotation=False, gamma=0.99, gae_lambda=0.95, lr=7e-4, clip_param=0.1, epochs=4, mini_batches=32,
          seed=0, device="cuda:0", verbose=True, native_trunk=False, invalid_coef=0.0, mask_coef=0.0):
    """Runs `updates` PPO updates; returns one (value_loss, action_loss, dist_entropy) tuple of floats per update: the means over
    the update's mini-batches, as the reference's PPO.update returns them."""
    dev = torch.device(device)
    size = (10, 10, 10)
    torch.manual_seed(seed)
    env = bpp_amd.BppVecEnv(envs, size, enable_rotation=rotation, pool=bpp_amd.sequences.cut2_pool(size, 1024, seed=seed), device=dev)
    net = (NativeTrunkNet if native_trunk else ActorCritic)(size[0], env.action_space.n).to(dev)
    actor = bpp_amd.NativePolicy(size[0], env.action_space.n, device=dev).refresh(net.policy) if native_trunk else None
    mini_batches = min(mini_batches, steps * envs)
    agent = bpp_amd.PPO(net, clip_param, epochs, mini_batches, 0.5, 0.01, lr=lr, eps=1e-5, max_grad_norm=0.5, invalid_coef=invalid_coef,
                        mask_coef=mask_coef)
    storage = bpp_amd.RolloutStorage(steps, env, env.observation_space.shape, env.action_space)
    storage.reset(env)
    counter = torch.tensor([seed, 0], dtype=torch.int64, device=dev)
    history = []
    for j in range(updates):
        collect(net, actor, env, storage, counter, gamma, gae_lambda)
        history.append(agent.update(storage))
        if native_trunk:
            actor.refresh(net.policy)
        storage.after_update()
        if verbose:
            finished = storage.done.bool()
            n_done = int(finished.sum())
            print("update %d: value %.4f  action %.4f  entropy %.4f | %d episodes finished, mean space utilisation %.3f"
                  % ((j + 1,) + history[-1] + (n_done, float(storage.ratio[finished].mean()) if n_done else float("nan"))))
    env.close()
    return history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=4)
    ap.add_argument("--rotation", action="store_true")
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--gae-lambda", type=float, default=0.95)
    ap.add_argument("--clip-param", type=float, default=0.1)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--mini-batches", type=int, default=32)
    ap.add_argument("--native-trunk", action="store_true", help="train bpp_amd.TrainablePolicy: the trunk forward and backward in native kernels")
    args = ap.parse_args()
    train(args.envs, args.steps, args.updates, args.rotation, args.gamma, args.gae_lambda, clip_param=args.clip_param, epochs=args.epochs,
          mini_batches=args.mini_batches, native_trunk=args.native_trunk)


if __name__ == "__main__":
    main()
