#!/usr/bin/env python3
"""Golden vectors for the native returns (include/bpp_rollout.h), recorded by RUNNING THE UNMODIFIED REFERENCE
acktr/storage.py RolloutStorage.compute_returns (build container only):   python tests/golden/make_returns_golden.py

tests/golden/returns_golden.npz holds, per input set s (`shapes` int64 [S, 2] = (T, N)):
  rewards_s f32 [T, N], value_preds_s f32 [T+1, N] (row T is what next_value overwrites under GAE), next_value_s f32 [N],
  masks_s f32 [T+1, N] (about 20 % zeros), bad_masks_s f32 [T+1, N] (about 10 % zeros), returns0_s f32 [T+1, N] (what `returns`
  held before the call: rows the reference does not write must keep it)
and per case `cases` int64 [C, 4] = (s, index into `gl`, use_gae, use_proper_time_limits), `gl` float64 [G, 2] = (gamma,
gae_lambda):  returns_<c> f32 [T+1, N] and vlast_<c> f32 [N] (value_preds[T]) AFTER the reference's call.
The last input set has bad_masks of ones and -0.0 scattered over rewards, values and next_value.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_shims  # noqa: E402

ref_shims.install()

from acktr.storage import RolloutStorage  # noqa: E402

import bpp_amd  # noqa: E402

SHAPES = [(5, 256), (1, 257), (32, 67), (5, 256)]       # the last one: bad_masks of ones, signed zeros
GL = [(1.0, 0.95), (0.99, 0.95), (0.9, 0.5)]


def inputs(s, T, N, signed_zeros):
    rng = np.random.RandomState(1000 + s)
    d = {"rewards": rng.uniform(0.0, 2.0, (T, N)), "value_preds": rng.normal(0.0, 3.0, (T + 1, N)),
         "next_value": rng.normal(0.0, 3.0, (N,)), "masks": (rng.uniform(size=(T + 1, N)) >= 0.2) * 1.0,
         "bad_masks": (rng.uniform(size=(T + 1, N)) >= 0.1) * 1.0, "returns0": rng.normal(0.0, 100.0, (T + 1, N))}
    d = {k: v.astype(np.float32) for k, v in d.items()}
    if signed_zeros:
        d["bad_masks"][:] = 1.0
        for k in ("rewards", "value_preds", "next_value"):
            z = rng.uniform(size=d[k].shape)
            d[k][z < 0.15] = -0.0
            d[k][(z >= 0.15) & (z < 0.25)] = 0.0
    return d


def reference(d, T, N, use_gae, gamma, lam, proper):
    st = RolloutStorage(T, N, (1,), bpp_amd.Discrete(1), 1, can_give_up=False, enable_rotation=False, pallet_size=1)
    st.rewards.copy_(torch.from_numpy(d["rewards"]).unsqueeze(-1))
    st.value_preds.copy_(torch.from_numpy(d["value_preds"]).unsqueeze(-1))
    st.masks.copy_(torch.from_numpy(d["masks"]).unsqueeze(-1))
    st.bad_masks.copy_(torch.from_numpy(d["bad_masks"]).unsqueeze(-1))
    st.returns.copy_(torch.from_numpy(d["returns0"]).unsqueeze(-1))
    st.compute_returns(torch.from_numpy(d["next_value"]).unsqueeze(-1), use_gae, gamma, lam, proper)
    assert np.array_equal(st.masks.numpy()[:, :, 0], d["masks"])
    return st.returns.numpy()[:, :, 0].copy(), st.value_preds.numpy()[-1, :, 0].copy()


def main():
    out = {"shapes": np.array(SHAPES, dtype=np.int64), "gl": np.array(GL, dtype=np.float64)}
    cases = []
    for s, (T, N) in enumerate(SHAPES):
        last = s == len(SHAPES) - 1
        d = inputs(s, T, N, last)
        out.update({"%s_%d" % (k, s): v for k, v in d.items()})
        for g, (gamma, lam) in enumerate(GL):
            if last and g != 1:
                continue
            for use_gae in (0, 1):
                for proper in (0, 1):
                    c = len(cases)
                    out["returns_%d" % c], out["vlast_%d" % c] = reference(d, T, N, bool(use_gae), gamma, lam, bool(proper))
                    cases.append((s, g, use_gae, proper))
    out["cases"] = np.array(cases, dtype=np.int64)
    path = os.path.join(HERE, "returns_golden.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
