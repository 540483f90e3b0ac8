"""Shared by tests/test_rollout_storage.py and tests/test_gpu_rollout_storage.py: the recorded cases of
tests/golden/returns_golden.npz (make_returns_golden.py), a numpy front-end of bpp_compute_returns_host / the emulated
bpp_compute_returns, and random inputs for the comparisons that need no recording."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "returns_golden.npz")
VARIANTS = [(0, 0), (0, 1), (1, 0), (1, 1)]          # (use_gae, use_proper_time_limits)
INPUTS = ("rewards", "value_preds", "next_value", "masks", "bad_masks", "returns0")


def load_cases():
    """[(case id, dict of inputs, T, N, gamma, gae_lambda, use_gae, proper, returns after, value_preds[T] after)]"""
    g = np.load(GOLDEN)
    out = []
    for c, (s, k, use_gae, proper) in enumerate(g["cases"].tolist()):
        T, N = (int(v) for v in g["shapes"][s])
        d = {name: g["%s_%d" % (name, s)] for name in INPUTS}
        out.append((c, d, T, N, float(g["gl"][k][0]), float(g["gl"][k][1]), use_gae, proper, g["returns_%d" % c], g["vlast_%d" % c]))
    return out


def random_inputs(T, N, seed, bad_ones=False):
    rng = np.random.RandomState(seed)
    d = {"rewards": rng.uniform(0.0, 2.0, (T, N)), "value_preds": rng.normal(0.0, 3.0, (T + 1, N)),
         "next_value": rng.normal(0.0, 3.0, (N,)), "masks": (rng.uniform(size=(T + 1, N)) >= 0.2) * 1.0,
         "bad_masks": np.ones((T + 1, N)) if bad_ones else (rng.uniform(size=(T + 1, N)) >= 0.1) * 1.0,
         "returns0": rng.normal(0.0, 100.0, (T + 1, N))}
    return {k: v.astype(np.float32) for k, v in d.items()}


def done_of(masks):
    """u8 [T][N] done bytes that stand for masks rows 1 .. T (nonzero bytes other than 1 among them: any nonzero byte is 'done')."""
    done = (masks[1:] == 0.0).astype(np.uint8)
    done[done == 1] = np.where(np.arange(int(done.sum())) % 3 == 0, 255, 1).astype(np.uint8)
    return done


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(handle, d, T, N, gamma, lam, use_gae, proper, use_done=False, bad=True, advantages=False, kernel=False, masks_out=True):
    """One call on COPIES of the inputs (numpy, host pointers).  kernel=True: bpp_compute_returns of an emulated library (the device
    kernel on the host), else bpp_compute_returns_host.  Returns dict(returns, value_preds, masks, advantages, rc)."""
    a = {k: np.ascontiguousarray(v.copy()) for k, v in d.items()}
    ret = a["returns0"]
    done = done_of(a["masks"]) if use_done else None
    masks = a["masks"]
    if use_done:
        masks = masks.copy()
        masks[1:] = -7.0                  # outputs on this path: whatever was there must not be read
    adv = np.full((T, N), -7.0, dtype=np.float32) if advantages else None

    def p(x):
        return x.ctypes.data if x is not None else None

    args = [p(a["rewards"]), p(a["value_preds"]), p(a["next_value"]), p(done), p(masks) if (masks_out or not use_done) else None,
            p(a["bad_masks"]) if bad else None, p(ret), p(adv), T, N, int(use_gae), int(proper), gamma, lam]
    rc = handle.bpp_compute_returns(*args, None) if kernel else handle.bpp_compute_returns_host(*args)
    return dict(returns=ret, value_preds=a["value_preds"], masks=masks, advantages=adv, rc=rc)
