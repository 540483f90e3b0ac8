#!/usr/bin/env python3
"""Generate tests/golden/placements_<case>.npz by RUNNING THE UNMODIFIED REFERENCE (build container only):

    python tests/golden/make_placements_golden.py

For every rollout fixture of CASES the recorded `pool` and `actions` are replayed through the reference stack make_golden.py
recorded them from (PackingGame + Monitor in a DummyVecEnv, items from ref_shims.make_replay_creator); `done` and `counter` must
reproduce the fixture.  After every lock-step the box the reference appended to `space.boxes` (envs/bpp0/space.py:176-177) is
recorded: box [T][E][7] int16 = Box.standardize() (x, y, z, lx, ly, lz) and space.flags[-1], -1 where nothing was appended (the
failed placement that ends an episode).

placements_pretrained_eval_cut2_10_rot: the recorded greedy actions of the reference's rotation checkpoint
(pretrained_eval_cut2_10_rot.npz) on every EVERY-th trajectory of cut2_dataset_10.npz, one PackingGame per trajectory fed by a
replaying creator built from the npz (the reference's LoadBoxCreator re-reads its .pt file on every reset); `ratio` and `counter`
must reproduce the fixture.  box [n][T][7], traj [n] = the trajectory numbers.

Nothing in the fixtures is computed by this repository's code."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the shims, imports the reference)
from oracle import ref_shims  # noqa: E402

CASES = ["rollout_cut2_10_rot", "rollout_deep_cut2_10_rot", "rollout_deep_cut2_20", "rollout_short_5x4x6", "rollout_wide_8x12x9_rot",
         "rollout_rs_10", "rollout_cut2_10"]
EVERY = 1          # the pretrained fixture holds every EVERY-th trajectory; all 2 100 stay below the largest committed fixture (328 KB)


def last_box(game):
    b = game.space.boxes[-1]
    return list(b.standardize()) + [int(bool(game.space.flags[-1]))]


def rollout_case(name):
    g = np.load(os.path.join(HERE, name + ".npz"))
    size, rot = tuple(int(v) for v in g["size"]), bool(g["rotation"])
    T, E = g["actions"].shape
    dummy, venv = mg.make_stack(g["pool"], size, rot, E)
    venv.reset()
    games = [m.env for m in dummy.envs]
    box = np.full((T, E, 7), -1, np.int16)
    for t in range(T):
        before = [len(gm.space.boxes) for gm in games]
        _, _, done, infos = venv.step(torch.from_numpy(g["actions"][t]).unsqueeze(1))
        assert np.array_equal(np.asarray(done).astype(np.uint8), g["done"][t]), (name, t)
        assert np.array_equal(np.array([i["counter"] for i in infos], np.int32), g["counter"][t]), (name, t)
        for e, gm in enumerate(games):
            if done[e]:
                assert len(gm.space.boxes) == 0         # the auto-reset's fresh Space
                continue
            assert len(gm.space.boxes) == before[e] + 1 == g["counter"][t][e]
            box[t, e] = mg.exact(np.array(last_box(gm)), np.int16)
    path = os.path.join(HERE, "placements_%s.npz" % name)
    np.savez_compressed(path, box=box)
    ok = box[:, :, 0] >= 0
    print("%-40s boxes %d, rotated %d, episodes %d, deepest %d -> %d KB" % (os.path.basename(path), int(ok.sum()), int((box[:, :, 6] == 1).sum()),
                                                                         int(g["done"].sum()), int(g["counter"].max()), os.path.getsize(path) // 1024))


def pretrained_case(name="pretrained_eval_cut2_10_rot"):
    from envs.bpp0 import PackingGame
    g = np.load(os.path.join(HERE, name + ".npz"))
    pool = np.load(os.path.join(HERE, "cut2_dataset_10.npz"))["pool"]
    size, rot = tuple(int(v) for v in g["size"]), bool(g["rotation"])
    seqs = [[tuple(int(v) for v in it[:3]) for it in s] for s in pool]
    traj = np.arange(0, pool.shape[0], EVERY)
    box = np.full((len(traj), g["actions"].shape[1], 7), -1, np.int16)
    for k, i in enumerate(traj):
        game = PackingGame(box_creator=ref_shims.make_replay_creator(seqs, size, env_id=int(i), env_total=len(seqs)), container_size=size,
                           enable_rotation=rot)
        game.reset()
        for t in range(int(g["steps"][i])):
            _, _, done, info = game.step([int(g["actions"][i, t])])
            assert done == (t == g["steps"][i] - 1), (i, t)
            if not done:
                box[k, t] = mg.exact(np.array(last_box(game)), np.int16)
        assert info["ratio"] == g["ratio"][i] and info["counter"] == g["counter"][i] == len(game.space.boxes), i
    path = os.path.join(HERE, "placements_%s.npz" % name)
    np.savez_compressed(path, box=box, traj=traj.astype(np.int32))
    print("%-40s %d trajectories (every %d), boxes %d -> %d KB" % (os.path.basename(path), len(traj), EVERY, int((box[:, :, 0] >= 0).sum()),
                                                                os.path.getsize(path) // 1024))


if __name__ == "__main__":
    for case in CASES:
        rollout_case(case)
    pretrained_case()
