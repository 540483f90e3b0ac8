#!/usr/bin/env python3
"""The reference's rollout buffer across updates, recorded by RUNNING THE UNMODIFIED REFERENCE acktr/storage.py RolloutStorage
(insert, compute_returns, after_update) on what the reference's environment produced (build container only):
    python tests/golden/make_storage_golden.py

For rollout_cut2_10.npz and rollout_cut2_10_rot.npz (make_golden.py: the reference env's observations, masks, rewards, dones and
actions of 320 lock-steps on 8 bins) the first U * T lock-steps are cut into U = 4 updates of T = 5.  Every lock-step is insert()ed
as main.py does (masks = 0 where the episode ended, bad_masks of ones, recurrent state of zeros) with seeded random values and
log-probabilities; after T of them compute_returns runs twice -- main.py's variant (no GAE, no proper time limits), then GAE with
proper time limits -- with a seeded next_value, then after_update.

tests/golden/storage_updates_<case>.npz: T, U; the seeded inputs values f32 [U,T,N], log_probs f32 [U,T,N], next_value f32 [U,N];
`main` / `gae` float64 [4] = (use_gae, gamma, gae_lambda, use_proper_time_limits) of the two calls; and the reference's storage per
update: returns_main f32 [U,T+1,N] (after the first call), returns f32 [U,T+1,N], value_preds f32 [U,T+1,N], masks f32 [U,T+1,N],
bad_masks f32 [U,T+1,N] (after the second call).  Observations, masks of positions, rewards and actions are not stored again: slot
s of update u holds lock-step u * T + s - 1 of the rollout recording (slot 0: what after_update carried over; obs0 at the start),
which this script asserts of the reference's storage before it writes the file.
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

T, U = 5, 4
MAIN = (False, 1.0, 0.95, False)
GAE = (True, 0.99, 0.95, True)


def record(case, seed):
    g = np.load(os.path.join(HERE, case + ".npz"))
    rot, N, M = int(g["rotation"]), g["actions"].shape[1], g["mask"].shape[2]
    assert U >= 3 and g["actions"].shape[0] >= U * T
    for u in range(U):
        assert g["done"][u * T:(u + 1) * T].any(), "episodes must end inside every update"
    rng = np.random.RandomState(seed)
    values = rng.normal(0.0, 3.0, (U, T, N)).astype(np.float32)
    log_probs = (-rng.uniform(0.0, 5.0, (U, T, N))).astype(np.float32)
    next_value = rng.normal(0.0, 3.0, (U, N)).astype(np.float32)
    st = RolloutStorage(T, N, (g["obs"].shape[2],), bpp_amd.Discrete(M), 1, can_give_up=False, enable_rotation=bool(rot),
                        pallet_size=int(g["size"][0]))
    st.obs[0].copy_(torch.from_numpy(g["obs0"].astype(np.float32)))
    st.location_masks[0].copy_(torch.from_numpy(g["mask0"].astype(np.float32)))
    out = {k: [] for k in ("returns_main", "returns", "value_preds", "masks", "bad_masks")}
    col = lambda a: torch.from_numpy(np.ascontiguousarray(a)).unsqueeze(-1)     # noqa: E731
    for u in range(U):
        for t in range(T):
            k = u * T + t
            assert st.step == t
            done = g["done"][k]
            st.insert(torch.from_numpy(g["obs"][k].astype(np.float32)), torch.zeros(N, 1), col(g["actions"][k]), col(log_probs[u, t]),
                      col(values[u, t]), col(g["reward"][k]), col(np.where(done != 0, 0.0, 1.0).astype(np.float32)), torch.ones(N, 1),
                      torch.from_numpy(g["mask"][k].astype(np.float32)))
        assert st.step == 0
        st.compute_returns(col(next_value[u]), *MAIN)
        out["returns_main"].append(st.returns.numpy()[:, :, 0].copy())
        st.compute_returns(col(next_value[u]), *GAE)
        for k in ("returns", "value_preds", "masks", "bad_masks"):
            out[k].append(getattr(st, k).numpy()[:, :, 0].copy())
        # slot s = lock-step u * T + s - 1 of the recording
        first = (g["obs0"], g["mask0"]) if u == 0 else (g["obs"][u * T - 1], g["mask"][u * T - 1])
        assert np.array_equal(st.obs[0].numpy(), first[0]) and np.array_equal(st.location_masks[0].numpy(), first[1])
        assert np.array_equal(st.obs[1:].numpy(), g["obs"][u * T:(u + 1) * T])
        assert np.array_equal(st.location_masks[1:].numpy(), g["mask"][u * T:(u + 1) * T])
        assert np.array_equal(st.rewards.numpy()[:, :, 0], g["reward"][u * T:(u + 1) * T])
        assert np.array_equal(st.actions.numpy()[:, :, 0], g["actions"][u * T:(u + 1) * T])
        assert (out["masks"][-1][1:] == 0.0).any()
        st.after_update()
    res = {k: np.stack(v) for k, v in out.items()}
    assert np.isfinite(res["returns"]).all() and not np.array_equal(res["returns"], res["returns_main"])
    res.update(T=np.int64(T), U=np.int64(U), values=values, log_probs=log_probs, next_value=next_value,
               main=np.array(MAIN, dtype=np.float64), gae=np.array(GAE, dtype=np.float64))
    path = os.path.join(HERE, "storage_updates_%s.npz" % case[len("rollout_"):])
    np.savez_compressed(path, **res)
    print("%s: %d updates of %d lock-steps on %d bins, %d bytes" % (path, U, T, N, os.path.getsize(path)))


if __name__ == "__main__":
    record("rollout_cut2_10", 31)
    record("rollout_cut2_10_rot", 32)
