"""Shared cases of the policy-forward tests (tests/test_policy_forward.py on the emulator, tests/test_gpu_policy_forward.py on the
device): exact-integer networks whose outputs are known in int64, real-valued networks on states of a recorded rollout with a
float64 reference, and the runners that call bpp_policy_forward (include/bpp_policy.h) with host or device pointers."""
import ctypes
import os

import numpy as np
import torch

from bpp_amd import _lib
from bpp_amd import policy as pol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -1
HEADS = pol.HEADS
FACTOR = 8          # e_native <= FACTOR * e_torch32 (the issue's rule: a 576-term sequential chain against a blocked sum, with room)


def geom_arg(g):
    return (ctypes.c_int32 * len(g))(*[int(v) for v in g])


def info(L, geom, n):
    out = (ctypes.c_int32 * 8)()
    rc = L.bpp_policy_forward_info(geom_arg(geom), int(n), out)
    assert rc == 0, rc
    return dict(zip(_lib.POLICY_INFO, (int(v) for v in out)))


def host_runner(L):
    """runner(obs [n, stride] float32 numpy, geom, blob numpy, want) -> {head: numpy} through host pointers (the emulated library)."""
    def run(obs, geom, blob, want=HEADS):
        obs = np.ascontiguousarray(obs, np.float32)
        n, stride = obs.shape
        S, H, M = geom
        g = geom_arg(geom)
        ws = np.full(L.bpp_policy_forward_workspace(g, n) // 4 + 1, np.nan, np.float32)
        outs = {"value": np.full(n, np.nan, np.float32), "logits": np.full((n, M), np.nan, np.float32), "pred": np.full((n, M), np.nan, np.float32)}
        ptr = [outs[h].ctypes.data if h in want else None for h in HEADS]
        blob = np.ascontiguousarray(blob, np.float32)
        rc = L.bpp_policy_forward(obs.ctypes.data, stride, n, g, blob.ctypes.data, ptr[0], ptr[1], ptr[2], ws.ctypes.data, None)
        assert rc == 0, (rc, L.bpp_last_error())
        for h in HEADS:
            if h not in want:
                assert np.isnan(outs[h]).all(), "%s was not asked for and was written" % h
        return {h: outs[h] for h in want}
    return run


def device_runner(device="cuda:0"):
    """The same through bpp_amd.policy_forward on the device."""
    def run(obs, geom, blob, want=HEADS):
        o = torch.from_numpy(np.ascontiguousarray(obs, np.float32)).to(device)
        out = pol.policy_forward(o, torch.from_numpy(np.ascontiguousarray(blob, np.float32)).to(device), geom, want)
        torch.cuda.synchronize()
        return {h: t.cpu().numpy() for h, t in zip(HEADS, out) if t is not None}
    return run


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- exact cases
def _sparse_layer(rng, shape):
    """Integer weights of `shape` [OC, ...]: at most 4 nonzero taps per output channel at distinct places, their values a
    permutation of (2, 1, -1, 1) for an even channel and of (-1, 2, -1, -1) for an odd one (so that pre-activations of both signs
    occur) -- a swapped i / j or a permuted channel order moves a value to another place and changes the result; biases nonzero,
    of both signs."""
    oc, k = shape[0], int(np.prod(shape[1:]))
    w = np.zeros((oc, k), np.int64)
    for o in range(oc):
        taps = min(4, k)
        w[o, rng.choice(k, taps, replace=False)] = rng.permutation([2, 1, -1, 1] if o % 2 == 0 else [-1, 2, -1, -1])[:taps]
    b = rng.choice([-3, -2, -1, 1, 2, 3], oc)
    b[0], b[-1] = 2, -2
    return w.reshape(shape), b.astype(np.int64)


def _conv64(x, w, b, pad):
    """(pre-activation, bound on every partial sum) of a convolution in int64; x [n, C, S, S]."""
    n, _, S, _ = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    out = np.broadcast_to(b[None, :, None, None], (n, w.shape[0], S, S)).copy()
    mag = np.abs(out)
    for o, c, i, j in zip(*np.nonzero(w)):
        out[:, o] += w[o, c, i, j] * xp[:, c, i:i + S, j:j + S]
        mag[:, o] += abs(w[o, c, i, j]) * np.abs(xp[:, c, i:i + S, j:j + S])
    return out, mag


def _linear64(x, w, b):
    return x @ w.T + b, np.abs(x) @ np.abs(w).T + np.abs(b)


def exact_case(S, H, M, n, seed, stride=None):
    """dict(geom, obs [n, stride] float32, blob float32, want {head: float32 of the int64 result}).  Every partial sum of every
    output stays below 2^24, so float32 is exact in any order; every layer has pre-activations of both signs (asserted)."""
    rng = np.random.RandomState(seed)
    A = S * S
    stride = stride or 4 * A
    img = rng.randint(0, 4, (n, 4, S, S)).astype(np.int64)
    border = np.ones((S, S), bool)
    border[1:-1, 1:-1] = False
    img[:, :, border] = np.maximum(img[:, :, border], 1)               # nonzero on the image border: a lost halo shows
    obs = np.full((n, stride), 7.0, np.float32)                        # the padding of a row is never read
    obs[:, :4 * A] = img.reshape(n, 4 * A)
    w = {}
    for name, shape in pol.layer_shapes(S, H, M):
        w[name + ".weight"], w[name + ".bias"] = _sparse_layer(rng, shape)

    def checked(pre, mag, name):
        assert mag.max() < 2 ** 24, (name, mag.max())
        assert (pre > 0).any() and (pre < 0).any(), "%s: pre-activations of one sign only" % name
        return pre

    x = img
    for name in pol.TRUNK:
        x = np.maximum(checked(*_conv64(x, w[name + ".weight"], w[name + ".bias"], 1), name), 0)

    def head(name):
        h = np.maximum(checked(*_conv64(x, w[name + ".0.weight"], w[name + ".0.bias"], 0), name + ".0"), 0).reshape(n, -1)
        return np.maximum(checked(*_linear64(h, w[name + ".3.weight"], w[name + ".3.bias"]), name + ".3"), 0)

    value, mag = _linear64(head("base.critic"), w["base.critic_linear.weight"], w["base.critic_linear.bias"])
    assert mag.max() < 2 ** 24
    logits = checked(*_linear64(head("base.actor"), w["dist.linear.weight"], w["dist.linear.bias"]), "dist.linear")
    pred = np.maximum(checked(*_linear64(head("base.mask"), w["base.mask.5.weight"], w["base.mask.5.bias"]), "base.mask.5"), 0)
    plain = {k: torch.from_numpy(v.astype(np.float32)) for k, v in w.items()}
    blob = pol.pack_weights(plain, S, H, M).numpy()
    return dict(geom=(S, H, M), obs=obs, blob=blob, plain=plain,
                want=dict(value=value.reshape(n).astype(np.float32), logits=logits.astype(np.float32), pred=pred.astype(np.float32)))


def exact_specs(P, T):
    """name -> arguments of exact_case: the smallest shapes at which each mechanism can go wrong.  P: bins per trunk
    workgroup, T: bins per head tile (both from bpp_policy_forward_info)."""
    specs = {"s10_n1": (10, 256, 100, 1, 1), "s10_nP1": (10, 256, 100, P + 1, 2), "s10_rot_n3": (10, 256, 200, 3, 3),
             "s5_n1": (5, 32, 25, 1, 4), "s5_n2": (5, 32, 25, 2, 5), "s5_nP1": (5, 32, 25, P + 1, 6), "s5_nT1": (5, 32, 25, T + 1, 7),
             "s6_rot": (6, 32, 72, 2, 8), "s5_stride": (5, 32, 25, 3, 9, 4 * 25 + 3)}
    return specs


def check_exact(run, case):
    got = run(case["obs"], case["geom"], case["blob"])
    for h in HEADS:
        assert same_bits(got[h], case["want"][h]), (h, np.abs(got[h].astype(np.float64) - case["want"][h]).max())


# ----------------------------------------------------------------------------------------------------------------- real cases
def real_weights(S, H, M, seed):
    """Plain float32 weights initialised as the reference does (acktr/model.py:268: orthogonal_, gain sqrt(2); dist.linear gain
    0.01, distributions.py:65-67), but with biases uniform in +-0.1 so that a dropped bias shows."""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in pol.layer_shapes(S, H, M):
        wt = torch.empty(shape)
        torch.nn.init.orthogonal_(wt, gain=0.01 if name == "dist.linear" else torch.nn.init.calculate_gain("relu"), generator=gen)
        out[name + ".weight"] = wt
        out[name + ".bias"] = (torch.rand(shape[0], generator=gen) - 0.5) * 0.2
    return out


def deep_states(rot, count=16):
    """`count` observation rows [count, 400] float32 spread over a recorded rollout under a competent policy: heights and item
    planes with the values a rollout has."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "rollout_deep_cut2_10%s.npz" % ("_rot" if rot else "")))
    obs = g["obs"].reshape(-1, g["obs"].shape[-1])
    pick = np.linspace(0, obs.shape[0] - 1, count).astype(int)
    return obs[pick].astype(np.float32)


def real_case(rot, seed=11):
    S, H, M = 10, 256, 200 if rot else 100
    plain = real_weights(S, H, M, seed)
    obs = deep_states(rot)
    with torch.no_grad():
        ref64 = pol.torch_forward({k: v.double() for k, v in plain.items()}, torch.from_numpy(obs).double())
        ref32 = pol.torch_forward(plain, torch.from_numpy(obs))
    return dict(geom=(S, H, M), obs=obs, plain=plain, blob=pol.pack_weights(plain, S, H, M).numpy(),
                ref64={h: t.numpy() for h, t in zip(HEADS, ref64)}, ref32={h: t.numpy() for h, t in zip(HEADS, ref32)})


def rel_err(out, ref64):
    """e = max |out - f64| / max |f64|"""
    return float(np.abs(np.asarray(out, np.float64) - ref64).max() / np.abs(ref64).max())


def check_real(got, ref64, ref32, label=""):
    """Per head e_native <= FACTOR * e_torch32, both measured against the float64 forward; returns {head: (e_native, e_torch32)}."""
    figures = {h: (rel_err(got[h], ref64[h]), rel_err(ref32[h], ref64[h])) for h in HEADS if h in got}
    print(label, "e_native / e_torch32 per head:", {h: "%.3g / %.3g = %.2f" % (a, b, a / b if b else float("inf")) for h, (a, b) in figures.items()})
    for h, (e_native, e_torch) in figures.items():
        assert e_torch > 0 and e_native <= FACTOR * e_torch, (label, h, e_native, e_torch, figures)
    return figures


def check_near_ties(l64, l32, masks, recorded, chosen):
    """Every state in which the native action differs from the recorded one must be a near-tie: with the masked probabilities
    p = softmax(l64 - 14 (1 - mask)) + 1e-5 of the float64 logits l64 [k, M] (acktr/distributions.py:78-79),
    |p[recorded] - p[chosen]| < FACTOR * e_torch32 * max p of that row, where e_torch32 is the relative error of the float32
    logits l32 against l64 on these states.  Returns [(gap, limit)] per state; AssertionError for a state that is no near-tie."""
    l64, l32 = torch.as_tensor(l64, dtype=torch.float64), torch.as_tensor(l32, dtype=torch.float64)
    e_torch32 = rel_err(l32.numpy(), l64.numpy())
    probs = torch.softmax(l64 - 14.0 * (1.0 - torch.as_tensor(masks, dtype=torch.float64)), -1) + 1e-5
    out = []
    for r, (a_rec, a_nat) in enumerate(zip(recorded, chosen)):
        gap, limit = abs(float(probs[r, a_rec] - probs[r, a_nat])), FACTOR * e_torch32 * float(probs[r].max())
        assert gap < limit, (r, a_rec, a_nat, gap, limit, e_torch32)
        out.append((gap, limit))
    return out
