#!/usr/bin/env python3
"""Records tests/golden/policy_forward_cut2_10{,_rot}.npz from the live reference's Policy (acktr/model.py) on the CPU under its
pretrained checkpoints pretrained_models/default_cut_2.pt and rotation_cut_2.pt: for the 32 observations
policy_cases.deep_states(rot, 32) (states of tests/golden/rollout_deep_cut2_10{,_rot}.npz) its float32

    value [32]         critic_linear(critic(share))
    logits [32, M]     dist.linear(actor features)
    pred_mask [32, M]  the mask head

Outputs only: the observations are rebuilt from the rollout fixture, the weights come from the checkpoint files at test time.

    python tests/golden/make_policy_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import policy_cases as pc  # noqa: E402
from oracle import ref_shims  # noqa: E402


def main():
    import bpp_amd
    ref_shims.install()
    from acktr.model import Policy
    for rot, ckpt, name in ((False, "default_cut_2.pt", "policy_forward_cut2_10"), (True, "rotation_cut_2.pt", "policy_forward_cut2_10_rot")):
        M = 100 * (1 + rot)
        args = types.SimpleNamespace(channel=4, container_size=(10, 10, 10), pallet_size=10, enable_rotation=rot, hidden_size=256, device="cpu")
        state, ob_rms = torch.load(os.path.join(ref_shims.REFERENCE_ROOT, "pretrained_models", ckpt), map_location="cpu", weights_only=False)
        assert ob_rms is None
        net = Policy((400,), bpp_amd.Discrete(M), base_kwargs={"recurrent": False, "hidden_size": 256, "args": args})
        sd = {k.replace("module.", "").replace("add_bias.", "").replace("_bias", "bias"): v for k, v in state.items()}     # main.py:66-76
        net.load_state_dict({k: (v.squeeze(-1) if v.dim() <= 3 else v) for k, v in sd.items()})
        net.eval()
        obs = torch.from_numpy(pc.deep_states(rot, 32))
        with torch.no_grad():
            value, features, _, pred = net.base(obs, None, None)
            logits = net.dist.linear(features)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, value=value.reshape(-1).numpy(), logits=logits.numpy(), pred_mask=pred.numpy(), states=np.int32(32),
                            checkpoint=ckpt)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
