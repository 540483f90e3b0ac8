#!/usr/bin/env python3
"""Golden vectors for native multi-bin packing (online-3d-bpp-drl_amd/multibin.py), recorded by RUNNING THE UNMODIFIED
REFERENCE multi_bin/multi_bin.py (build container only):   python tests/golden/make_multibin_golden.py [--limit N]

The module is loaded as it is; its global `args` gets container_size = (w, w, H) and its `nnModel` becomes the FAKE
nnModel of make_reorder_golden.py (exact in int64; evaluate() runs model_loader.evaluate's post-processing literally,
its logits are distinct, so every argmax is unique).  The reference's own test(env, args) plays every trajectory; the
decisions are recorded by wrapping the module's get_action and the env's step.  A KeyError from test() (the step after a
decision without a window, when window (0, 0) has no history: multi_bin.py:91-93) ends that trajectory and is counted.

  * multibin_fake_20x20x10.npz:     the first 64 trajectories of dataset/4bins_cut_2.pt as the reference's LoadBoxCreator
                                    plays them (index pre-incremented: trajectories 1 .. 64; the appended [10, 10, 10]
                                    is never reached), w = 10, s = 10 (K = 4): the reference's configuration.
  * multibin_fake_20x20x10_s5.npz:  the same trajectories with s = 5 (K = 9, overlapping windows; slipingWindow rebound
                                    with functools.partial(stride=5), bin_num stays 4).
  * multibin_fake_30x30x10.npz:     24 CUT-2 sequences of a 30x30x10 pallet (K = 9), replayed through the reference env.

Per file: `pool` uint8 [N, T, 4] (what the device env plays: terminator = the last entry, never placed), `size`, `w`, `s`,
per decision `action` int64, `adv` float64, `window` int32 (-1: no window), `start` int64 [N + 1], per trajectory `ratio`
float64, `counter` int32, `steps` int32, `keyerror` bool, and `cov` int64 [len(COV_NAMES)].
"""
import argparse
import functools
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import ref_shims  # noqa: E402

ref_shims.install()

from make_reorder_golden import FakeModel  # noqa: E402
from envs.bpp0 import PackingGame  # noqa: E402

COV_NAMES = ("skipped_window", "tie_at_max", "no_window", "chosen_again", "failed_placement", "keyerror")


def load_multi_bin():
    """multi_bin/multi_bin.py as a module of its own (it is a script, not a package)."""
    path = os.path.join(ref_shims.REFERENCE_ROOT, "multi_bin", "multi_bin.py")
    spec = importlib.util.spec_from_file_location("multi_bin_ref", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class Recorder(object):
    """Wraps the module's get_action / get_possible_position and the fake model's evaluate; counts coverage."""

    def __init__(self, mb, size, w, s):
        self.mb, self.size, self.w = mb, size, w
        W, L, H = size
        self.labels = [(dx, dy) for dx in range(0, W - w + 1, s) for dy in range(0, L - w + 1, s)]
        self.bin_num = (W * L) / (w * w)
        self.cov = np.zeros(len(COV_NAMES), np.int64)
        self.decisions = []
        self.values, self.skips = [], []
        fake = FakeModel((w, w, H))
        rec = self

        class Model(object):
            def evaluate(self, obs, use_mask=True):
                value, poss = fake.evaluate(obs, use_mask)
                rec.values.append(value)
                return value, poss

        gpp, get_action = mb.get_possible_position, mb.get_action

        def get_possible_position(obs, container_size):
            mask = gpp(obs, container_size)
            rec.skips.append(int(np.sum(mask)) == len(mask))
            return mask

        def wrapped(env, obs, nmodel, past_rewards, evaluations):
            rec.values, rec.skips = [], []
            had = {k: bool(v) for k, v in past_rewards.items()}
            last = {k: (v[-1] if v else None) for k, v in past_rewards.items()}
            last_eval = {k: (v[-1] if v else None) for k, v in evaluations.items()}
            action, adv, label = get_action(env, obs, nmodel, past_rewards, evaluations)
            window = -1 if adv == -1e8 else rec.labels.index(label)
            # coverage only: the advantages of the windows that were not skipped
            advs = [rec.bin_num * last[lb] + (v - last_eval[lb]) if had.get(lb) else -0.2
                    for lb, v, sk in zip(rec.labels, rec.values, rec.skips) if not sk]
            rec.cov[0] += any(rec.skips)
            rec.cov[1] += len(advs) >= 2 and advs.count(max(advs)) >= 2
            rec.cov[2] += window < 0
            rec.cov[3] += window >= 0 and had.get(label, False)
            rec.decisions.append((int(action), float(adv), window))
            return action, adv, label

        mb.nnModel = lambda url, args: Model()
        mb.get_possible_position = get_possible_position
        mb.get_action = wrapped


def play(mb, rec, env):
    """One call of the reference's test(env, args); returns (ratio, counter, steps, keyerror)."""
    steps = [0]
    step = env.step

    def counted(action):
        out = step(action)
        steps[0] += 1
        rec.cov[4] += bool(out[2])
        return out

    env.step = counted
    try:
        ratio, counter = mb.test(env, mb.args)
        ke = False
    except KeyError:
        ratio, counter, ke = env.space.get_ratio(), len(env.space.boxes), True
        rec.cov[5] += 1
    finally:
        env.step = step
    return float(ratio), int(counter), steps[0], ke


def record(name, pool, size, w, s, env_of, n):
    mb = load_multi_bin()
    mb.args = SimpleNamespace(container_size=(w, w, size[2]))
    if s != 10:
        mb.slipingWindow = functools.partial(mb.slipingWindow, stride=s)
    rec = Recorder(mb, size, w, s)
    starts, ratios, counters, steps, kes = [0], [], [], [], []
    for p in range(n):
        env = env_of(p)
        r, c, st, ke = play(mb, rec, env)
        # the pool's terminator (the last entry) is never placed: the device plays the same items
        term = int(np.flatnonzero((pool[p, :, :3] == pool[p, -1, :3]).all(-1))[0])
        assert c <= term, (name, p)
        starts.append(len(rec.decisions))
        ratios.append(r)
        counters.append(c)
        steps.append(st)
        kes.append(ke)
    act, adv, win = (np.array([d[j] for d in rec.decisions]) for j in range(3))
    out = dict(pool=pool[:n], size=np.array(size, np.int32), w=np.int32(w), s=np.int32(s), action=act.astype(np.int64),
               adv=adv.astype(np.float64), window=win.astype(np.int32), start=np.array(starts, np.int64),
               ratio=np.array(ratios, np.float64), counter=np.array(counters, np.int32), steps=np.array(steps, np.int32),
               keyerror=np.array(kes, bool), cov=rec.cov)
    np.savez_compressed(os.path.join(HERE, name), **out)
    print("%s: %d trajectories, %d decisions, mean ratio %.4f, mean items %.2f, coverage %s" % (
        name, n, len(act), float(np.mean(ratios)), float(np.mean(counters)), dict(zip(COV_NAMES, rec.cov.tolist()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=int)
    a = ap.parse_args()
    import bpp_amd
    size = (20, 20, 10)
    # LoadBoxCreator's pre-incremented index: row r of the device pool is trajectory r + 1 (sequences.from_dataset)
    pool4 = bpp_amd.sequences.from_dataset(os.path.join(HERE, "cut2_dataset_4bins_20x20x10.npz"), size, terminator=(20, 20, 10))
    data = os.path.join(ref_shims.REFERENCE_ROOT, "dataset", "4bins_cut_2.pt")
    n4 = a.limit or 64
    for name, s in (("multibin_fake_20x20x10.npz", 10), ("multibin_fake_20x20x10_s5.npz", 5)):
        env = PackingGame(container_size=size, test=True, data_name=data, enable_rotation=False)
        record(name, pool4, size, 10, s, lambda p: env, n4)
    size30 = (30, 30, 10)
    pool30 = bpp_amd.sequences.cut2_pool(size30, a.limit or 24, seed=7, native=False)

    def env30(p):
        seq = [tuple(int(v) for v in it[:3]) for it in pool30[p]]
        return PackingGame(box_creator=ref_shims.make_replay_creator([seq], seq[-1]), container_size=size30, enable_rotation=False)
    record("multibin_fake_30x30x10.npz", pool30, size30, 10, 10, env30, a.limit or 24)


if __name__ == "__main__":
    main()
