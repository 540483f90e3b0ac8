"""Shared cases of the policy-forward tests (tests/test_policy_forward.py on the emulator, tests/test_gpu_policy_forward.py on the
device): exact-integer networks whose outputs are known in int64, real-valued networks on states of a recorded rollout (10 x 10) or
on synthetic states (every other side) with a float64 reference, the inputs of the recorded chain bits, and the runners that call bpp_policy_forward (include/bpp_policy.h) with host or device pointers."""
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


# The accepted geometries beyond the shipped 10 x 10 network: (S, H, M, bins relative to the P of that side or None, n, seed).
# n is what the seed was chosen for (exact_case asserts its own preconditions); where `relative` is k, n means P + k for the
# side's own P and exact_specs takes P from bpp_policy_forward_info.
WIDE_SPECS = {
    "s1_h32_m2": (1, 32, 2, 1, 3, 42),            # A = 1: K1 = 8 and 4 (a Linear shorter than one batch of MFMAs), 2 rows in a tile of 32
    "s2_h32_m4": (2, 32, 4, 1, 3, 40),            # both bins in one partial tile
    "s3_h64_m9": (3, 64, 9, 1, 3, 40),            # H = 64: two of a wave's four column tiles exist
    "s4_h96_m32": (4, 96, 32, None, 2, 40),       # rows = 32 exactly, M = 2 A = one column tile, H = 96
    "s7_h160_m49": (7, 160, 49, None, 2, 40),     # PW odd, PP = 81; H = 160: the second column group has one tile
    "s8_h288_m64": (8, 288, 64, None, 2, 40),     # a second pass over H with 32 columns
    "s5_h288_m50": (5, 288, 50, 1, 3, 40),
    "s9_h32_m81": (9, 32, 81, None, 2, 40),       # PW = 11
    "s11_h32_m121": (11, 32, 121, 1, 2, 40),      # one bin per trunk workgroup, PP = 169
    "s14_h32_m196": (14, 32, 196, 2, 3, 40),      # PP = 257
    "s12_h64_m288": (12, 64, 288, 1, 2, 40),      # PP = 197, M = 2 A > 256: the second Linear loops
    "s13_h320_m169": (13, 320, 169, None, 1, 40),
    "s15_h512_m225": (15, 512, 225, None, 1, 40), # the largest side and hidden size: both LDS budgets near 150 KB
    "s15_h512_m450": (15, 512, 450, 1, 2, 40),    # and the largest M
    "s5_h512_nT1": (5, 512, 25, None, 65, 40),   # two full passes over H, T + 1 bins
}


def exact_specs(P, T, bins=None):
    """name -> arguments of exact_case: the smallest shapes at which each mechanism can go wrong.  P: bins per trunk
    workgroup at 10 x 10, T: bins per head tile (both from bpp_policy_forward_info); bins: geom -> the bins per trunk workgroup of
    that geometry (None: the names are all that is wanted, n is the figure of WIDE_SPECS)."""
    specs = {"s10_n1": (10, 256, 100, 1, 1), "s10_nP1": (10, 256, 100, P + 1, 2), "s10_rot_n3": (10, 256, 200, 3, 3),
             "s5_n1": (5, 32, 25, 1, 4), "s5_n2": (5, 32, 25, 2, 5), "s5_nP1": (5, 32, 25, P + 1, 6), "s5_nT1": (5, 32, 25, T + 1, 7),
             "s6_rot": (6, 32, 72, 2, 8), "s5_stride": (5, 32, 25, 3, 9, 4 * 25 + 3)}
    for name, (S, H, M, relative, n, seed) in WIDE_SPECS.items():
        if name.endswith("_nT1"):
            n = T + 1
        elif bins is not None and relative is not None:
            n = bins((S, H, M)) + relative
        specs[name] = (S, H, M, n, seed)
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
    return with_references((S, H, M), real_weights(S, H, M, seed), deep_states(rot))


# The shapes of the real-valued cases beyond 10 x 10.  Sides up to 3 are left out: the float32 torch forward of a 9-term network
# is no stable yardstick (ratios up to 6.3 were seen for the logits) and at S = 1 the pred head is identically zero; the exact
# cases and the recorded chain bits (tests/golden/make_mfma_chain_bits.py) cover those sides.
WIDE_REAL = [(15, 512, 450), (15, 512, 225), (13, 320, 338), (12, 96, 144), (7, 160, 49)]


def synthetic_states(S, count=16, seed=5):
    """`count` observation rows [count, 4 A] float32 for a side no rollout was recorded at: plane 0 integers uniform in [0, S],
    planes 1 - 3 each one constant from [1, max(1, S // 2)] (an item's extents).  Sixteen states, as deep_states gives: on three
    the float32 torch error of the value head is three numbers' luck."""
    rng = np.random.RandomState(seed)
    A = S * S
    obs = np.empty((count, 4, A), np.float32)
    obs[:, 0] = rng.randint(0, S + 1, (count, A))
    obs[:, 1:] = rng.randint(1, max(1, S // 2) + 1, (count, 3))[:, :, None]
    return obs.reshape(count, 4 * A)


def with_references(geom, plain, obs):
    """The case dict of real_case for any weights and states: the float64 and the float32 torch forward beside the blob."""
    with torch.no_grad():
        ref64 = pol.torch_forward({k: v.double() for k, v in plain.items()}, torch.from_numpy(obs).double())
        ref32 = pol.torch_forward(plain, torch.from_numpy(obs))
    return dict(geom=tuple(geom), obs=obs, plain=plain, blob=pol.pack_weights(plain, *geom).numpy(),
                ref64={h: t.numpy() for h, t in zip(HEADS, ref64)}, ref32={h: t.numpy() for h, t in zip(HEADS, ref32)})


def wide_real_case(S, H, M, seed=11):
    return with_references((S, H, M), real_weights(S, H, M, seed), synthetic_states(S))


# ---- the recorded bits of the emulator's fmaf chains on real-valued data (tests/golden/make_mfma_chain_bits.py) ----------------
CHAIN_FIXTURE = "mfma_chain_emulator_bits"
CHAIN_CASES = [(10, 256, 100, 3), (5, 32, 25, 3), (3, 64, 9, 3), (12, 96, 144, 2), (15, 512, 450, 2)]        # (S, H, M, n)


def chain_name(S, H, M, n):
    return "policy_s%d_h%d_m%d_n%d" % (S, H, M, n)


def chain_case(S, H, M, n, seed=7):
    """Inputs that numpy.random.RandomState alone determines, so that every machine regenerates the same bytes: weights normal
    * sqrt(2 / fan_in), biases uniform in +-0.1, the states of synthetic_states.  dict(geom, obs, blob, plain)."""
    rng = np.random.RandomState(seed)
    plain = {}
    for name, shape in pol.layer_shapes(S, H, M):
        fan_in = int(np.prod(shape[1:]))
        plain[name + ".weight"] = torch.from_numpy((rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)).astype(np.float32))
        plain[name + ".bias"] = torch.from_numpy(rng.uniform(-0.1, 0.1, shape[0]).astype(np.float32))
    return dict(geom=(S, H, M), obs=synthetic_states(S, n), plain=plain, blob=pol.pack_weights(plain, S, H, M).numpy())


def crc(a):
    import zlib
    return np.uint32(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def chain_entries(run, spec):
    """{key: array} of one case for the fixture: the CRC32 of the bytes of each input and the bits of every head from `run`."""
    case, name = chain_case(*spec), chain_name(*spec)
    out = {name + ".crc.obs": crc(case["obs"]), name + ".crc.blob": crc(case["blob"])}
    got = run(case["obs"], case["geom"], case["blob"])
    for h in HEADS:
        out[name + "." + h] = np.ascontiguousarray(got[h], np.float32).view(np.uint32)
    return out


def ulps(a, b):
    """The largest distance of two float32 arrays (given as floats or as bits) in units of the last place."""
    def ordered(x):
        x = np.ascontiguousarray(x)
        i = (x.view(np.uint32) if x.dtype != np.uint32 else x).astype(np.int64)
        return np.where(i & 0x80000000, 0x80000000 - i, i)
    return int(np.abs(ordered(a) - ordered(b)).max())


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
