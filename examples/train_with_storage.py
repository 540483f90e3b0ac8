#!/usr/bin/env python3
"""The training loop of the reference's main.py:148-185, tensor-native, on a device-resident rollout storage.

    python examples/train_with_storage.py --envs 4096 --updates 4
    python examples/train_with_storage.py --envs 4096 --updates 4 --acktr
    python examples/train_with_storage.py --envs 64 --updates 4 --native-trunk [--fused-loss]
    python examples/train_with_storage.py --envs 64 --updates 4 --native-heads [--fused-loss]

Per update: `--steps` lock-steps in which the policy's logits go through bpp_masked_act and `storage.step` lets the step kernel
write observation, mask, reward and done straight into the storage (no insert, no copy of an environment output); then ONE
native call for the returns (`storage.compute_returns`, the reference's main.py variant: no GAE, no time limits), the
reference's five loss terms (acktr/algo/acktr_pipeline.py:45-92: value, action, entropy, invalid-probability and mask-prediction
loss) with the log-probabilities, entropy and invalid probability from bpp_masked_evaluate, and RMSprop with gradient clipping:
the reference's own optimiser path with acktr=False.  With --acktr the optimiser is bpp_amd.KFACOptimizer and the update adds the
sampled-Fisher pass of acktr_pipeline.py:68-84, as main.py does by default (`--algorithm acktr`): the Kronecker factors come from
bpp_kfac_factor, which never writes an im2col patch.

The network is a plain-torch stand-in shaped like the reference's CNNPro (acktr/model.py:265-323) with random weights.  With
--native-trunk it is bpp_amd.TrainablePolicy instead: CNNPro under the reference's names, whose five 3x3 layers and 1x1 head
convolutions run forward and backward through the native trunk kernels (include/bpp_policy_train.h), and the rollouts act on
bpp_amd.NativePolicy refreshed from it after every update.  K-FAC finds its layers by module hooks, which the native trunk does
not have yet: --native-trunk with --acktr is refused.  --native-heads (which implies --native-trunk) also runs the six Linear
layers of the heads forward and backward in native kernels (include/bpp_policy_heads_train.h): nothing of the network is torch's
then, and --acktr is refused in the same way.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

import bpp_amd


class ActorCritic(nn.Module):
    """5 x conv3x3(64) trunk; actor, critic and mask-prediction heads of 1x1 conv + linear layers."""

    def __init__(self, side, n_actions, hidden=256):
        super().__init__()
        layers, c = [], 4
        for _ in range(5):
            layers += [nn.Conv2d(c, 64, 3, padding=1), nn.ReLU()]
            c = 64
        self.share = nn.Sequential(*layers)

        def head(channels, out):
            return nn.Sequential(nn.Conv2d(64, channels, 1), nn.ReLU(), nn.Flatten(), nn.Linear(channels * side * side, hidden), nn.ReLU(),
                                 nn.Linear(hidden, out))

        self.actor, self.critic, self.mask = head(8, n_actions), head(4, 1), head(8, n_actions)
        self.side = side

    def forward(self, obs):
        x = self.share(obs.reshape(-1, 4, self.side, self.side))
        return self.actor(x), self.critic(x), torch.sigmoid(self.mask(x))


class NativeTrunkNet(nn.Module):
    """bpp_amd.TrainablePolicy behind the stand-in's interface: forward -> (logits, values, pred_mask)."""

    def __init__(self, side, n_actions, heads="torch"):
        super().__init__()
        self.policy = bpp_amd.TrainablePolicy(side, n_actions, heads=heads)

    def forward(self, obs):
        value, logits, pred = self.policy(obs)
        return logits, value.reshape(-1, 1), pred


def collect(net, actor, env, storage, counter, gamma):
    """`storage.num_steps` lock-steps into the storage and the returns (main.py:150-181).  actor: the bpp_amd.NativePolicy the
    rollout acts on when `net` is a NativeTrunkNet, else None."""
    for t in range(storage.num_steps):                   # main.py:150-174
        with torch.no_grad():
            if actor is not None:                        # the inference forward of the weights being trained
                value, logits, _ = actor(storage.obs[t], want=("value", "logits"))
                value = value.reshape(-1, 1)
            else:
                logits, value, _ = net(storage.obs[t])
        action, logp = bpp_amd.masked_act(logits, storage.location_masks[t], counter=counter)
        counter[1:].add_(1)
        storage.step(env, action, value, logp)           # ONE lock-step; its outputs are row t of the storage
    with torch.no_grad():
        next_value = actor(storage.obs[-1], want=("value",))[0].reshape(-1, 1) if actor is not None else net(storage.obs[-1])[1]
    storage.compute_returns(next_value, False, gamma, 0.95, False)             # main.py:181


def loss_terms(logits, values, pred_mask, storage):
    """(value_loss, action_loss, dist_entropy, prob_loss, graph_loss, action_log_probs) of acktr/algo/acktr_pipeline.py:45-66 from
    the network's outputs on storage.obs[:-1], in torch expressions around bpp_masked_evaluate."""
    T, N = storage.num_steps, storage.num_envs
    truth = storage.location_masks[:-1].view(T * N, -1)
    action_log_probs, dist_entropy, prob_loss = bpp_amd.masked_evaluate(logits, truth, storage.actions.view(T * N, 1))
    advantages = storage.returns[:-1] - values.view(T, N, 1)
    value_loss = advantages.pow(2).mean()
    action_loss = -(advantages.detach() * action_log_probs.view(T, N, 1)).mean()
    graph_loss = nn.functional.mse_loss(pred_mask, truth)
    return value_loss, action_loss, dist_entropy, prob_loss, graph_loss, action_log_probs


def total_loss(terms, coefs):
    """acktr_pipeline.py:86-92; coefs = (value, entropy, invalid, mask)."""
    value_loss, action_loss, dist_entropy, prob_loss, graph_loss = terms[:5]
    return value_loss * coefs[0] + action_loss + prob_loss * coefs[2] - dist_entropy * coefs[1] + coefs[3] * graph_loss


COEFS, MAX_GRAD_NORM = (0.5, 0.01, 2.0, 0.5 * 10), 0.5      # value, entropy, invalid, mask (`force`): the reference's defaults


def train(envs=4096, steps=5, updates=4, rotation=False, gamma=1.0, lr=7e-4, seed=0, device="cuda:0", verbose=True, fused_loss=False,
          acktr=False, native_trunk=False, native_heads=False):
    """Runs `updates` updates; returns one (value_loss, action_loss, dist_entropy, prob_loss, graph_loss) tuple of floats per update.
    fused_loss: the five terms and the gradients at the network's outputs from ONE native call (storage.a2c_loss) instead of
    bpp_masked_evaluate + torch expressions + their autograd backward.  acktr: K-FAC (bpp_amd.KFACOptimizer) with the Fisher pass
    of acktr_pipeline.py:68-84 instead of RMSprop with gradient clipping.  native_trunk: train bpp_amd.TrainablePolicy and roll
    out on bpp_amd.NativePolicy.  native_heads: the same with TrainablePolicy(heads="native"), the Linear layers native as well."""
    if acktr and native_heads:
        raise ValueError("K-FAC hooks into torch modules, which the native network does not have yet: --native-heads goes with RMSprop, "
                         "not with --acktr")
    native_trunk = native_trunk or native_heads
    if acktr and native_trunk:
        raise ValueError("K-FAC hooks into torch modules, which the native trunk does not have yet: --native-trunk goes with RMSprop, "
                         "not with --acktr")
    if acktr and fused_loss:
        raise ValueError("the Fisher pass needs the log-probabilities in the autograd graph: --acktr goes without --fused-loss")
    dev = torch.device(device)
    size = (10, 10, 10)
    torch.manual_seed(seed)
    env = bpp_amd.BppVecEnv(envs, size, enable_rotation=rotation, pool=bpp_amd.sequences.cut2_pool(size, 1024, seed=seed), device=dev)
    if native_trunk:
        net = NativeTrunkNet(size[0], env.action_space.n, heads="native" if native_heads else "torch").to(dev)
    else:
        net = ActorCritic(size[0], env.action_space.n).to(dev)
    actor = bpp_amd.NativePolicy(size[0], env.action_space.n, device=dev).refresh(net.policy) if native_trunk else None
    # acktr/algo/acktr_pipeline.py:33 with acktr=False; coefficients of the reference's defaults
    optimizer = bpp_amd.KFACOptimizer(net) if acktr else torch.optim.RMSprop(net.parameters(), lr, eps=1e-5, alpha=0.99)
    storage = bpp_amd.RolloutStorage(steps, env, env.observation_space.shape, env.action_space)
    storage.reset(env)                                   # observation and mask of the reset land in slot 0
    counter = torch.tensor([seed, 0], dtype=torch.int64, device=dev)     # (seed, step) of the sampler, read by the kernel
    T, N = steps, envs
    history = []
    for j in range(updates):
        collect(net, actor, env, storage, counter, gamma)
        if fused_loss:
            history.append(fused_update(net, optimizer, storage, COEFS, MAX_GRAD_NORM))
            if native_trunk:
                actor.refresh(net.policy)
            report(j, history, storage, verbose)
            continue
        # acktr/algo/acktr_pipeline.py:45-101
        logits, values, pred_mask = net(storage.obs[:-1].view(T * N, -1))
        terms = loss_terms(logits, values, pred_mask, storage)
        if acktr and optimizer.steps % optimizer.Ts == 0:                      # sampled Fisher, acktr_pipeline.py:68-84
            net.zero_grad()
            pg_fisher_loss = -terms[5].mean()
            sample_values = values + torch.randn(values.size(), device=dev)
            vf_fisher_loss = -(values - sample_values.detach()).pow(2).mean()
            fisher_loss = pg_fisher_loss + vf_fisher_loss + terms[4] * 1e-8
            optimizer.acc_stats = True
            fisher_loss.backward(retain_graph=True)
            optimizer.acc_stats = False
        optimizer.zero_grad()
        total_loss(terms, COEFS).backward()
        if not acktr:
            nn.utils.clip_grad_norm_(net.parameters(), MAX_GRAD_NORM)
        optimizer.step()
        if native_trunk:
            actor.refresh(net.policy)
        storage.after_update()
        history.append(tuple(float(v.detach()) for v in terms[:5]))
        report(j, history, storage, verbose)            # the infos scan of main.py:159-162, once per update over the [T][N] slabs
    env.close()
    return history


def fused_gradients(net, optimizer, storage, coefs):
    """Forward, storage.a2c_loss and backward: the parameters' gradients are there afterwards; returns the A2CLoss."""
    T, N = storage.num_steps, storage.num_envs
    logits, values, pred_mask = net(storage.obs[:-1].view(T * N, -1))
    out = storage.a2c_loss(logits, values, pred_mask, value_loss_coef=coefs[0], entropy_coef=coefs[1], invalid_coef=coefs[2], mask_coef=coefs[3])
    optimizer.zero_grad()
    out.backward()
    return out


def fused_update(net, optimizer, storage, coefs, max_grad_norm):
    """One update through storage.a2c_loss; returns the five terms as floats."""
    out = fused_gradients(net, optimizer, storage, coefs)
    nn.utils.clip_grad_norm_(net.parameters(), max_grad_norm)
    optimizer.step()
    storage.after_update()
    return tuple(out.terms[:5].tolist())


def report(j, history, storage, verbose):
    if verbose:
        finished = storage.done.bool()
        n_done = int(finished.sum())
        mean_ratio = float(storage.ratio[finished].mean()) if n_done else float("nan")
        print("update %d: value %.4f  action %.4f  entropy %.4f  invalid-prob %.5f  mask %.4f | %d episodes finished, "
              "mean space utilisation %.3f" % ((j + 1,) + history[-1] + (n_done, mean_ratio)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=4)
    ap.add_argument("--rotation", action="store_true")
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--fused-loss", action="store_true", help="loss terms and output gradients from one native call (bpp_amd.a2c_loss)")
    ap.add_argument("--acktr", action="store_true", help="K-FAC with the sampled-Fisher pass (bpp_amd.KFACOptimizer) instead of RMSprop")
    ap.add_argument("--native-trunk", action="store_true", help="train bpp_amd.TrainablePolicy: the trunk forward and backward in native kernels")
    ap.add_argument("--native-heads", action="store_true", help="--native-trunk, and the heads' Linear layers in native kernels as well")
    args = ap.parse_args()
    train(args.envs, args.steps, args.updates, args.rotation, args.gamma, fused_loss=args.fused_loss, acktr=args.acktr,
          native_trunk=args.native_trunk, native_heads=args.native_heads)


if __name__ == "__main__":
    main()
