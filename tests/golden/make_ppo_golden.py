#!/usr/bin/env python3
"""BUILD CONTAINER ONLY -- records tests/golden/ppo_update_reference.npz: the unmodified reference's PPO.update
(acktr/algo/ppo.py) on its unmodified RolloutStorage (acktr/storage.py), on a small fixed rollout in float64.

    python tests/golden/make_ppo_golden.py

T = 5, N = 8, M = 25, 2 epochs x 4 mini-batches.  The reference's ppo.py calls evaluate_actions without feasibility masks, so the
network is a stub of this project's own writing whose observation carries them: obs = [mask (M) | features (F)], a two-layer
module, evaluate_actions applies the masked head of acktr/distributions.py:71-101 through the reference's own FixedCategorical.
Recorded: the rollout, the initial parameters, the three returned means, every parameter after the update and the index sequence
the reference's sampler drew under torch.manual_seed(SEED).  Data only."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_shims  # noqa: E402

T, N, M, F, HIDDEN = 5, 8, 25, 15, 32
EPOCHS, MINI_BATCHES, SEED = 2, 4, 11
HYPER = dict(clip_param=0.1, value_loss_coef=0.5, entropy_coef=0.01, lr=3e-3, eps=1e-5, max_grad_norm=0.5)


class Stub(nn.Module):
    """net(obs) -> (logits, values, None); the first M entries of an observation row are its feasibility mask."""
    is_recurrent = False

    def __init__(self):
        super().__init__()
        self.body = nn.Sequential(nn.Linear(M + F, HIDDEN), nn.Tanh(), nn.Linear(HIDDEN, M + 1))

    def forward(self, obs):
        out = self.body(obs)
        return out[:, :M], out[:, M:], None

    def evaluate_actions(self, obs, rnn_hxs, masks, action):
        from acktr.distributions import FixedCategorical
        logits, values, _ = self(obs)
        mask = obs[:, :M]
        lx = torch.softmax(logits - (1.0 - mask) * 14.0, dim=-1) + 1e-5           # distributions.py:76-80
        dist = FixedCategorical(probs=lx)
        return values, dist.log_probs(action), dist.entropy().mean(), rnn_hxs


def main():
    ref_shims.install()
    from acktr.algo.ppo import PPO
    from acktr.storage import RolloutStorage
    from bpp_amd.spaces import Discrete
    torch.set_default_dtype(torch.float64)
    rng = np.random.RandomState(5)
    torch.manual_seed(3)
    net = Stub()
    init = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    st = RolloutStorage(T, N, (M + F,), Discrete(M), 1, False, False, 5)
    mask = np.zeros((T + 1, N, M))
    for t in range(T + 1):
        for n in range(N):
            mask[t, n, rng.permutation(M)[:rng.randint(1, M + 1)]] = 1.0
    obs = np.concatenate([mask, rng.randn(T + 1, N, F)], axis=2)
    st.obs.copy_(torch.from_numpy(obs))
    st.location_masks.copy_(torch.from_numpy(mask))
    st.value_preds.copy_(torch.from_numpy(rng.randn(T + 1, N, 1)))
    st.returns.copy_(st.value_preds + torch.from_numpy(rng.randn(T + 1, N, 1)))
    actions = rng.randint(0, M, size=(T, N, 1))
    for t in range(T):                                  # three actions in four on feasible cells
        for n in range(N):
            cells = np.nonzero(mask[t, n])[0]
            if (t + n) % 4:
                actions[t, n, 0] = rng.choice(cells)
    st.actions.copy_(torch.from_numpy(actions))
    with torch.no_grad():                               # the old policy: the initial network, moved a little
        _, logp, _, _ = net.evaluate_actions(st.obs[:-1].view(T * N, -1), None, None, st.actions.view(T * N, 1))
    st.action_log_probs.copy_((logp + 0.05 * torch.from_numpy(rng.randn(T * N, 1))).view(T, N, 1))
    rollout = {k: getattr(st, k).numpy().copy() for k in ("obs", "location_masks", "value_preds", "returns", "actions", "action_log_probs")}

    agent = PPO(net, HYPER["clip_param"], EPOCHS, MINI_BATCHES, HYPER["value_loss_coef"], HYPER["entropy_coef"], lr=HYPER["lr"],
                eps=HYPER["eps"], max_grad_norm=HYPER["max_grad_norm"])
    torch.manual_seed(SEED)
    means = agent.update(st)
    # the index sequence of the same seed, from the reference's own generator
    torch.manual_seed(SEED)
    seen = []
    flat = torch.arange(T * N, dtype=torch.float64).view(T, N, 1)
    for _ in range(EPOCHS):
        for sample in st.feed_forward_generator(flat, MINI_BATCHES):
            seen.append(sample[7].view(-1).long().numpy())
    out = dict(rollout)
    out.update({"init." + k: v for k, v in init.items()})
    out.update({"final." + k: v.detach().numpy().copy() for k, v in net.state_dict().items()})
    out.update(means=np.array(means), indices=np.stack(seen), shape=np.array([T, N, M, F, HIDDEN, EPOCHS, MINI_BATCHES, SEED]),
               hyper=np.array([HYPER[k] for k in ("clip_param", "value_loss_coef", "entropy_coef", "lr", "eps", "max_grad_norm")]))
    path = os.path.join(ROOT, "tests", "golden", "ppo_update_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; means", means)


if __name__ == "__main__":
    main()
