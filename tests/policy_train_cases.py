"""Shared cases of the trunk-training tests (tests/test_policy_train.py on the emulator, tests/test_gpu_policy_train.py on the
device): exact-integer networks whose forward, input gradients and weight gradients are known in int64, real-valued networks with
a float64 torch autograd reference, the header's arithmetic stated in numpy (fma32, normative) with the cases whose bits are
recorded in tests/golden/trunk_train_chain_bits.npz, the split identity, and the runners that call
bpp_policy_trunk_forward_train and bpp_policy_trunk_backward (include/bpp_policy_train.h) with host or device pointers, plain
or into guarded buffers.  The forward-side helpers are those of tests/policy_cases.py."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import policy_cases as pc
from bpp_amd import _lib
from bpp_amd import policy as pol

OUTPUTS = ("feat", "acts", "grads", "gf", "gw")
LIMIT = 2 ** 24
H = 32          # the hidden size does not enter the trunk; geom carries the smallest one


def geom_of(S):
    return (S, H, S * S)


def info(L, geom, n):
    out = (ctypes.c_int32 * 8)()
    rc = L.bpp_policy_trunk_backward_info(pc.geom_arg(geom), int(n), out)
    assert rc == 0, rc
    return dict(zip(_lib.POLICY_TRAIN_INFO, (int(v) for v in out)))


def split_outputs(S, n, feat, acts, grads, gw):
    A = S * S
    return dict(feat=feat.reshape(n, 20, A), acts=acts.reshape(5, n, 64, A), grads=grads[:5 * n * 64 * A].reshape(5, n, 64, A),
                gf=grads[5 * n * 64 * A:].reshape(n, 20, A), gw=gw)


def host_runner(L):
    """run(obs [n, stride], geom, blob, blob_bwd, grad_feat [n, 20 A]) -> {feat [n, 20, A], acts [5, n, 64, A], grads [5, n, 64, A],
    gf [n, 20, A], gw [151380]} through host pointers (the emulated library); every output starts as NaN."""
    def run(obs, geom, blob, blob_bwd, grad_feat):
        obs = np.ascontiguousarray(obs, np.float32)
        n, stride = obs.shape
        S = geom[0]
        A = S * S
        g = pc.geom_arg(geom)
        blob, blob_bwd = np.ascontiguousarray(blob, np.float32), np.ascontiguousarray(blob_bwd, np.float32)
        grad_feat = np.ascontiguousarray(grad_feat, np.float32)
        feat = np.full(n * 20 * A, np.nan, np.float32)
        acts = np.full(5 * n * 64 * A, np.nan, np.float32)
        rc = L.bpp_policy_trunk_forward_train(obs.ctypes.data, stride, n, g, blob.ctypes.data, feat.ctypes.data, acts.ctypes.data, None)
        assert rc == 0, (rc, L.bpp_last_error())
        grads = np.full(n * (5 * 64 + 20) * A, np.nan, np.float32)
        gw = np.full(pol.TRUNK_FLOATS, np.nan, np.float32)
        bytes_ = L.bpp_policy_trunk_backward_workspace(g, n)
        ws = np.full(bytes_ // 4, np.nan, np.float32)
        rc = L.bpp_policy_trunk_backward(obs.ctypes.data, stride, n, g, blob_bwd.ctypes.data, feat.ctypes.data, acts.ctypes.data,
                                         grad_feat.ctypes.data, grads.ctypes.data, gw.ctypes.data, ws.ctypes.data, bytes_, None)
        assert rc == 0, (rc, L.bpp_last_error())
        return split_outputs(S, n, feat, acts, grads, gw)
    return run


def device_runner(device="cuda:0"):
    """The same through bpp_amd.policy.trunk_forward_train / trunk_backward on the device."""
    def run(obs, geom, blob, blob_bwd, grad_feat):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)        # noqa: E731
        o = dev(obs)
        feat, acts = pol.trunk_forward_train(o, dev(blob), geom)
        grads, gw = pol.trunk_backward(o, geom, dev(blob_bwd), feat, acts, dev(grad_feat))
        torch.cuda.synchronize()
        return split_outputs(geom[0], o.shape[0], *(t.cpu().numpy().reshape(-1) for t in (feat, acts, grads, gw)))
    return run


def blobs(plain):
    """(forward blob [151380], backward blob [148736]) as numpy from plain weights under the reference's names."""
    return pol.pack_trunk(plain).numpy(), pol.pack_trunk_backward(plain).numpy()


def unpack_gradient(gw):
    """{name: numpy gradient in torch's shape} of a grad_weights vector."""
    return {k: v.numpy() for k, v in pol.unpack_trunk_gradient(torch.from_numpy(np.ascontiguousarray(gw))).items()}


# ---------------------------------------------------------------------------------------------------------------- exact cases
def _taps(rng, shape, taps):
    """Integer weights [OC, C, kh, kw] with `taps` nonzero entries per output channel, values +-1 with one 2, both signs; biases
    in {-2 .. 2} without 0."""
    oc, k = shape[0], int(np.prod(shape[1:]))
    w = np.zeros((oc, k), np.int64)
    for o in range(oc):
        t = min(taps, k)
        vals = np.array([2] + [(-1) ** (q + 1) for q in range(t - 1)]) * (1 if o % 2 == 0 else -1)
        w[o, rng.choice(k, t, replace=False)] = rng.permutation(vals)
    return w.reshape(shape), rng.choice([-2, -1, 1, 2], oc).astype(np.int64)


def _corr(xp, g, S):
    """dW[oc][c][i][j] = sum over (b, y, x) of xp[b, c, y + i, x + j] * g[b, oc, y, x] for a padded input xp, in int64."""
    kk = xp.shape[-1] - S + 1
    out = np.zeros((g.shape[1], xp.shape[1], kk, kk), np.int64)
    for i in range(kk):
        for j in range(kk):
            out[:, :, i, j] = np.einsum("boyx,bcyx->oc", g, xp[:, :, i:i + S, j:j + S])
    return out


def exact_case(S, n, seed, stride=None, taps=3, density=None):
    """dict(geom, obs, blob, blob_bwd, grad_feat, want {feat, acts, grads, gf, gw}) of an integer network: every partial sum of
    every chain -- forward, input gradient, weight-gradient split and the sum of the splits -- stays below 2^24 in the
    absolute-value network (asserted in int64), so float32 is exact in any order.  Every ReLU mask is mixed at every layer,
    every layer's taps are asymmetric under the flip and under a swap of i and j, and every gradient is nonzero (asserted)."""
    rng = np.random.RandomState(seed)
    A = S * S
    stride = stride or 4 * A
    density = density or (0.05 if n * A >= 100 else 0.5)          # of the gradient at feat: a handful of entries at least
    img = rng.randint(0, 4, (n, 4, S, S)).astype(np.int64)
    border = np.ones((S, S), bool)
    border[1:-1, 1:-1] = False
    img[:, :, border] = np.maximum(img[:, :, border], 1)
    obs = np.full((n, stride), np.nan, np.float32)          # the padding of a row: one stray read of it and an output is NaN
    obs[:, :4 * A] = img.reshape(n, 4 * A)
    shapes = pol.layer_shapes(S, H, A)[:8]
    w = {}
    for name, shape in shapes:
        w[name + ".weight"], w[name + ".bias"] = _taps(rng, shape, taps)
        if shape[2] == 3 and S > 1:
            ww = w[name + ".weight"]
            assert not np.array_equal(ww, ww[:, :, ::-1, ::-1]) and not np.array_equal(ww, ww.transpose(0, 1, 3, 2)), name

    def bounded(mag, what):
        assert mag.max() < LIMIT, (what, int(mag.max()))

    def mixed(x, what):
        assert (x > 0).any() and (x == 0).any(), "%s: the mask is not mixed" % what
        return x

    # forward
    x, inputs, acts = img, [], []
    for name in pol.TRUNK:
        inputs.append(x)
        pre, mag = pc._conv64(x, w[name + ".weight"], w[name + ".bias"], 1)
        bounded(mag, name)
        x = mixed(np.maximum(pre, 0), name)
        acts.append(x)
    wh = np.concatenate([w[nm + ".weight"] for nm in pol.HEAD_CONVS], 0)
    bh = np.concatenate([w[nm + ".bias"] for nm in pol.HEAD_CONVS], 0)
    pre, mag = pc._conv64(x, wh, bh, 0)
    bounded(mag, "head convolutions")
    feat = mixed(np.maximum(pre, 0), "head convolutions")
    # the gradient at feat: sparse, of both signs, and present where feat > 0 as well as where it is 0
    gfeat = (rng.random_sample(feat.shape) < density) * rng.choice([-2, -1, 1, 2], feat.shape)
    gfeat = gfeat.astype(np.int64)
    gf = np.where(feat > 0, gfeat, 0)
    assert (gf != 0).any() and (gfeat[feat == 0] != 0).any(), "the gradient at feat does not test the head mask"
    # input gradients
    d = np.einsum("bhyx,hc->bcyx", gf, wh[:, :, 0, 0])
    bounded(np.einsum("bhyx,hc->bcyx", np.abs(gf), np.abs(wh[:, :, 0, 0])), "D5")
    G = [None] * 5
    for l in range(4, -1, -1):
        G[l] = np.where(acts[l] > 0, d, 0)
        assert (G[l] != 0).any() and (d[acts[l] == 0] != 0).any(), "layer %d: the mask removes nothing or everything" % l
        if l == 0:
            break
        ww = w[pol.TRUNK[l] + ".weight"]
        gp, d, mag = np.pad(G[l], ((0, 0), (0, 0), (1, 1), (1, 1))), np.zeros_like(acts[l - 1]), np.zeros_like(acts[l - 1])
        for o, c, i, j in zip(*np.nonzero(ww)):
            d[:, c] += ww[o, c, i, j] * gp[:, o, 2 - i:2 - i + S, 2 - j:2 - j + S]
            mag[:, c] += abs(ww[o, c, i, j]) * np.abs(gp[:, o, 2 - i:2 - i + S, 2 - j:2 - j + S])
        bounded(mag, "D%d" % l)
    # weight gradients: the bound over the whole batch covers every split and the sum of the splits
    grad = {}
    for l, name in enumerate(pol.TRUNK):
        xp = np.pad(inputs[l], ((0, 0), (0, 0), (1, 1), (1, 1)))
        grad[name + ".weight"], grad[name + ".bias"] = _corr(xp, G[l], S), G[l].sum((0, 2, 3))
        bounded(_corr(np.abs(xp), np.abs(G[l]), S), "dW " + name)
        bounded(np.abs(G[l]).sum((0, 2, 3)), "db " + name)
        assert (grad[name + ".weight"] != 0).any() and (grad[name + ".bias"] != 0).any(), name
    dwh, dbh = _corr(acts[4], gf, S), gf.sum((0, 2, 3))
    bounded(_corr(np.abs(acts[4]), np.abs(gf), S), "dW head")
    o = 0
    for nm in pol.HEAD_CONVS:
        m = w[nm + ".weight"].shape[0]
        grad[nm + ".weight"], grad[nm + ".bias"] = dwh[o:o + m], dbh[o:o + m]
        o += m
    plain = {k: torch.from_numpy(v.astype(np.float32)) for k, v in w.items()}
    blob, blob_bwd = blobs(plain)
    gw = pol.pack_trunk({k: torch.from_numpy(v.astype(np.float32)) for k, v in grad.items()}).numpy()
    f32 = lambda a: np.asarray(a).astype(np.float32)        # noqa: E731
    return dict(geom=geom_of(S), obs=obs, blob=blob, blob_bwd=blob_bwd, grad_feat=f32(gfeat).reshape(n, 20 * A), plain=plain,
                want=dict(feat=f32(feat).reshape(n, 20, A), acts=f32(np.stack(acts)).reshape(5, n, 64, A),
                          grads=f32(np.stack(G)).reshape(5, n, 64, A), gf=f32(gf).reshape(n, 20, A), gw=gw))


def exact_spec(L, name):
    """The arguments of exact_case for EXACT_SPECS[name] under library handle L's own P and bins per split."""
    S, nf, seed, taps, pad = EXACT_SPECS[name]
    i = info(L, geom_of(S), 1)
    return dict(S=S, n=nf(i["bins_per_group"], i["bins_per_split"]), seed=seed, taps=taps, stride=4 * S * S + pad if pad else None)


def check_exact(run, case):
    got = run(case["obs"], case["geom"], case["blob"], case["blob_bwd"], case["grad_feat"])
    for key in OUTPUTS:
        assert pc.same_bits(got[key], case["want"][key]), (key, np.abs(got[key].astype(np.float64) - case["want"][key]).max())
    return got


# name -> (side, n as a function of (bins per input-gradient workgroup P, bins per split B) of that side, seed, taps per channel,
# floats of NaN padding behind the 4 A of an obs row: obs_stride = 4 A + padding)
EXACT_SPECS = {
    "s10_n1": (10, lambda P, B: 1, 1, 3, 0), "s10_nP1": (10, lambda P, B: P + 1, 2, 3, 0), "s10_n5": (10, lambda P, B: 5, 3, 3, 0),
    "s5_n2": (5, lambda P, B: 2, 4, 3, 0), "s5_three_splits": (5, lambda P, B: 2 * B + 1, 5, 3, 0),
    "s3_n3": (3, lambda P, B: 3, 6, 3, 0), "s1_n3": (1, lambda P, B: 3, 7, 20, 0),       # A = 1: only the centre taps count, so more of them
    "s11_n3": (11, lambda P, B: 3, 8, 3, 0), "s15_n2": (15, lambda P, B: 2, 9, 3, 0),
    # every other side the header accepts; the 64-bin cap on a split (S <= 4) and the shipped 10 x 10 over more than one split;
    # padded rows of obs
    "s2_three_splits": (2, lambda P, B: 2 * B + 1, 20, 3, 3), "s3_three_splits": (3, lambda P, B: 2 * B + 1, 20, 3, 0),
    "s4_nP1": (4, lambda P, B: P + 1, 20, 3, 5), "s4_two_splits": (4, lambda P, B: B + 1, 20, 3, 0),
    "s6_nP1": (6, lambda P, B: P + 1, 20, 3, 0), "s7_nP1": (7, lambda P, B: P + 1, 20, 3, 1), "s8_nP1": (8, lambda P, B: P + 1, 20, 3, 0),
    "s9_nP1": (9, lambda P, B: P + 1, 20, 3, 0), "s12_n2": (12, lambda P, B: 2, 20, 3, 7), "s13_n2": (13, lambda P, B: 2, 20, 3, 0),
    "s14_n2": (14, lambda P, B: 2, 20, 3, 0), "s10_two_splits": (10, lambda P, B: B + 1, 20, 3, 9),
}
# name -> (splits, bins of the last split) of the cases that are there for their splits
EXACT_SPLITS = {"s5_three_splits": (3, 1), "s2_three_splits": (3, 1), "s3_three_splits": (3, 1), "s4_two_splits": (2, 1),
                "s10_two_splits": (2, 1)}


# ----------------------------------------------------------------------------------------------------------------- real cases
def trunk_autograd(plain, obs, grad_feat, dtype):
    """The trunk and head convolutions of torch_forward with torch autograd in `dtype`: dict(feat [n, 20 A], G1 [n, 64, A] -- the
    gradient at the pre-activation output of share.0 -- and the gradient of every trunk parameter) as numpy."""
    w = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in plain.items() if k in pol.TRUNK_PARAMETERS}
    S = int(round((obs.shape[1] // 4) ** 0.5))
    x = torch.as_tensor(obs).to(dtype)[:, :4 * S * S].reshape(-1, 4, S, S)
    pre1 = None
    for name in pol.TRUNK:
        pre = F.conv2d(x, w[name + ".weight"], w[name + ".bias"], padding=1)
        if pre1 is None:
            pre1 = pre
            pre1.retain_grad()
        x = F.relu(pre)
    feat = torch.cat([F.relu(F.conv2d(x, w[nm + ".weight"], w[nm + ".bias"])) for nm in pol.HEAD_CONVS], 1).flatten(1)
    feat.backward(torch.as_tensor(grad_feat).to(dtype))
    out = {k: v.grad.numpy() for k, v in w.items()}
    out["feat"], out["G1"] = feat.detach().numpy(), pre1.grad.numpy().reshape(pre1.shape[0], 64, S * S)
    return out


def tied_bins(plain, obs):
    """bool [n]: the states in which some pre-activation of the trunk or of the head convolutions lies within float32 rounding
    of zero, |pre| <= 2 * 2^-24 * sum |x_k w_k| (in float64).  There the ReLU mask of a float32 forward is decided by rounding, and
    the gradient -- which jumps when one mask element flips -- is defined for no float32 implementation; the gradient
    comparisons on many states leave such states out.  Decided from the float64 forward alone.  The factor: a chain of K terms
    accumulates about sqrt(K) roundings of half an ulp of its partial sums, each below 2^-24 * sum |x_k w_k|; two such units cover
    it with room, while the worst case K * 2^-24 * sum |x_k w_k| would call every state tied."""
    w = {k: v.detach().cpu().double() for k, v in plain.items()}
    S = int(round((obs.shape[1] // 4) ** 0.5))
    x = torch.as_tensor(obs).double()[:, :4 * S * S].reshape(-1, 4, S, S)
    tied = torch.zeros(x.shape[0], dtype=torch.bool)

    def near_zero(x, names, pad):
        nonlocal tied
        wt, b = torch.cat([w[n + ".weight"] for n in names], 0), torch.cat([w[n + ".bias"] for n in names], 0)
        pre, mag = F.conv2d(x, wt, b, padding=pad), F.conv2d(x.abs(), wt.abs(), b.abs(), padding=pad)
        tied |= (pre.abs() <= 2.0 * 2.0 ** -24 * mag).flatten(1).any(1)
        return F.relu(pre)

    for name in pol.TRUNK:
        x = near_zero(x, (name,), 1)
    near_zero(x, pol.HEAD_CONVS, 0)
    return tied.numpy()


def real_case(S, obs, seed=11, gseed=3):
    """dict(geom, obs, plain, blob, blob_bwd, grad_feat, ref64, ref32): pc.real_weights, a standard-normal gradient at feat, and
    torch autograd over the same layers in float64 and in float32."""
    geom = (S, 256, S * S)
    plain = pc.real_weights(*geom, seed)
    grad_feat = torch.randn(obs.shape[0], 20 * S * S, generator=torch.Generator().manual_seed(gseed)).numpy()
    blob, blob_bwd = blobs(plain)
    return dict(geom=geom, obs=obs, plain=plain, blob=blob, blob_bwd=blob_bwd, grad_feat=grad_feat,
                ref64=trunk_autograd(plain, obs, grad_feat, torch.float64), ref32=trunk_autograd(plain, obs, grad_feat, torch.float32))


def check_real(got, ref64, ref32, label=""):
    """Per gradient tensor -- every dW, every db and G1 -- e_native <= FACTOR * e_torch32, both against float64 autograd.
    got: the runner's outputs.  Returns {name: (e_native, e_torch32)}."""
    mine = unpack_gradient(got["gw"])
    mine["G1"] = got["grads"][0]
    return check_gradients(mine, ref64, ref32, label)


def check_gradients(mine, ref64, ref32, label=""):
    figures = {k: (pc.rel_err(mine[k], ref64[k]), pc.rel_err(ref32[k], ref64[k])) for k in mine}
    print(label, "e_native / e_torch32 per gradient:",
          {k: "%.3g / %.3g = %.2f" % (a, b, a / b if b else float("inf")) for k, (a, b) in figures.items()})
    for k, (e_native, e_torch) in figures.items():
        assert e_torch > 0 and e_native <= pc.FACTOR * e_torch, (label, k, e_native, e_torch)
    return figures


# ------------------------------------------------------------- the header's arithmetic in numpy (include/bpp_policy_train.h)
def fma32(a, b, c):
    """The exactly rounded float32 fused multiply-add float32(a * b + c) of float32 arrays, as libm's fmaf gives it.  In
    float64 the product of two float32 is exact (24 + 24 bits); TwoSum gives the error of the float64 sum s = p + c exactly;
    where that error is not zero and s is even, s moves one float64 towards the error's side, which rounds the true sum to odd
    at 53 bits; a value rounded to odd at 24 + 2 bits or more rounds to float32 as the true sum does."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    fix = (err != 0) & ((s.view(np.int64) & 1) == 0) & np.isfinite(s)
    s = np.where(fix, np.where(err > 0, np.nextafter(s, np.inf), np.nextafter(s, -np.inf)), s)
    return s.astype(np.float32)


def header_bins_per_split(S):
    """`bins per split` as DESIGN.md 3.15 states it: clamp(1024 / A, 1, 64), a function of the geometry alone."""
    return max(1, min(64, 1024 // (S * S)))


def _pad1(x):
    return np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))


def _relu32(x):
    return np.where(x > 0, x, np.float32(0)).astype(np.float32)


def normative(plain, obs, grad_feat, S, bins_per_split):
    """{feat [n, 20, A], acts [5, n, 64, A], grads [5, n, 64, A], gf [n, 20, A], gw [151380]} as include/bpp_policy.h and
    include/bpp_policy_train.h state them, one fma32 per step of every chain, in plain numpy: no convolution of torch and
    nothing of the emulator.
      forward   every output element one chain from the bias over ascending k = c * 9 + i * 3 + j (the head convolutions over c)
      gf'       grad_feat where feat > 0
      D_5       one chain over h = 0 .. 19 from +0;  G_l = acts_l > 0 ? D_l : 0
      D_{l-1}   one chain over ascending k' = oc * 9 + i' * 3 + j' from +0 on W[oc][c][2 - i'][2 - j']
      dW_l      per split of `bins_per_split` consecutive bins one chain per element [k][oc] from +0 over ascending (b, p), the
                bias a row of the patch with the value 1; the splits are added in split order in float64 and cast once
    gw is packed with pol.pack_trunk."""
    w = {k: np.asarray(v, np.float32) for k, v in plain.items()}
    n, A, B = obs.shape[0], S * S, int(bins_per_split)
    x = np.ascontiguousarray(obs[:, :4 * A], np.float32).reshape(n, 4, S, S)
    inputs, acts = [], []
    for name in pol.TRUNK:
        W, bias = w[name + ".weight"], w[name + ".bias"]
        inputs.append(x)
        xp = _pad1(x)
        acc = np.broadcast_to(bias[None, :, None, None], (n, 64, S, S)).astype(np.float32)
        for c in range(W.shape[1]):
            for i in range(3):
                for j in range(3):
                    acc = fma32(xp[:, c, None, i:i + S, j:j + S], W[None, :, c, i, j, None, None], acc)
        x = _relu32(acc)
        acts.append(x)
    Wh = np.concatenate([w[nm + ".weight"] for nm in pol.HEAD_CONVS], 0)[:, :, 0, 0]
    bh = np.concatenate([w[nm + ".bias"] for nm in pol.HEAD_CONVS], 0)
    acc = np.broadcast_to(bh[None, :, None, None], (n, 20, S, S)).astype(np.float32)
    for c in range(64):
        acc = fma32(x[:, c, None], Wh[None, :, c, None, None], acc)
    feat = _relu32(acc)
    gf = np.where(feat > 0, np.asarray(grad_feat, np.float32).reshape(feat.shape), np.float32(0)).astype(np.float32)
    d = np.zeros((n, 64, S, S), np.float32)
    for h in range(20):
        d = fma32(gf[:, h, None], Wh[None, h, :, None, None], d)
    G = [None] * 5
    for l in range(4, -1, -1):
        G[l] = np.where(acts[l] > 0, d, np.float32(0)).astype(np.float32)
        if l == 0:
            break
        W, gp, d = w[pol.TRUNK[l] + ".weight"], _pad1(G[l]), np.zeros((n, 64, S, S), np.float32)
        for oc in range(64):
            for i in range(3):
                for j in range(3):
                    d = fma32(gp[:, oc, None, i:i + S, j:j + S], W[None, oc, :, 2 - i, 2 - j, None, None], d)

    def wgrad(xin, g, taps):
        """xin [n, C, S, S], g [n, OC, S, S] -> (dW [OC, C, taps, taps], db [OC])"""
        C, OC = xin.shape[1], g.shape[1]
        xp = _pad1(xin) if taps == 3 else xin
        total = np.zeros((C * taps * taps + 1, OC), np.float64)
        for b0 in range(0, n, B):
            acc = np.zeros((C * taps * taps + 1, OC), np.float32)
            for b in range(b0, min(n, b0 + B)):
                for y in range(S):
                    for xx in range(S):
                        patch = np.append(xp[b, :, y:y + taps, xx:xx + taps].reshape(-1), np.float32(1))
                        acc = fma32(patch[:, None], g[b, None, :, y, xx], acc)
            total = total + acc.astype(np.float64)
        total = total.astype(np.float32)
        return total[:-1].T.reshape(OC, C, taps, taps), total[-1]

    grad = {}
    for l, name in enumerate(pol.TRUNK):
        grad[name + ".weight"], grad[name + ".bias"] = wgrad(inputs[l], G[l], 3)
    dwh, dbh = wgrad(acts[4], gf, 1)
    o = 0
    for nm in pol.HEAD_CONVS:
        m = w[nm + ".weight"].shape[0]
        grad[nm + ".weight"], grad[nm + ".bias"] = dwh[o:o + m], dbh[o:o + m]
        o += m
    gw = pol.pack_trunk({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in grad.items()}).numpy()
    return dict(feat=feat.reshape(n, 20, A), acts=np.stack(acts).reshape(5, n, 64, A), grads=np.stack(G).reshape(5, n, 64, A),
                gf=gf.reshape(n, 20, A), gw=gw)


# ---- the recorded bits of that reference on real-valued data (tests/golden/make_trunk_train_chain_bits.py) -------------------
TRAIN_CHAIN_FIXTURE = "trunk_train_chain_bits"
# (S, n) -> (splits, bins of the last split, bins per input-gradient workgroup): one split and P = 2 with an absent bin; three
# splits under the 64-bin cap with a last split of 2 bins, even A; two splits, odd A; the shipped geometry in splits of 10 and
# 1; P = 1 with both LDS budgets near their limit
TRAIN_CHAIN_CASES = {(5, 3): (1, 3, 2), (2, 130): (3, 2, None), (3, 66): (2, 2, None), (10, 11): (2, 1, 2), (15, 1): (1, 1, 1)}
TRAIN_CHAIN_INPUTS = ("obs", "blob", "blob_bwd", "grad_feat")
SAMPLE = 2048           # floats of an output kept in the fixture beside the CRC32 of all of them


def train_chain_name(S, n):
    return "trunk_s%d_n%d" % (S, n)


def train_chain_case(S, n, seed=7):
    """dict(geom, obs, plain, blob, blob_bwd, grad_feat) from numpy.random.RandomState alone (pc.chain_case: weights normal *
    sqrt(2 / fan_in), biases uniform in +-0.1, the states of pc.synthetic_states), the gradient at feat standard normal."""
    base = pc.chain_case(S, H, S * S, n, seed)
    plain = {k: v for k, v in base["plain"].items() if k in pol.TRUNK_PARAMETERS}
    assert all(float(v.abs().min()) > 0 for k, v in plain.items() if k.endswith(".bias"))
    grad_feat = np.random.RandomState(seed + 1000).standard_normal((n, 20 * S * S)).astype(np.float32)
    blob, blob_bwd = blobs(plain)
    return dict(geom=geom_of(S), obs=base["obs"], plain=plain, blob=blob, blob_bwd=blob_bwd, grad_feat=grad_feat)


def sample_step(size):
    """The smallest odd step (coprime to 64, so that no lane, tile slot or channel is passed over) that leaves at most SAMPLE."""
    return -(-size // SAMPLE) | 1


def train_chain_entries(case, outputs, name):
    """{key: array} of one case for the fixture: a CRC32 of each input; per output a CRC32 of all its bits and every
    sample_step-th of them."""
    out = {"%s.crc.%s" % (name, k): pc.crc(np.ascontiguousarray(case[k], np.float32)) for k in TRAIN_CHAIN_INPUTS}
    for key in OUTPUTS:
        bits = np.ascontiguousarray(outputs[key], np.float32).reshape(-1).view(np.uint32)
        out["%s.%s.crc" % (name, key)] = pc.crc(bits)
        out["%s.%s.sample" % (name, key)] = bits[::sample_step(bits.size)].copy()
    return out


def check_train_chain(got, fixture, name, label=""):
    """Every output of `got` against the recorded reference: the CRC32 of all its bits.  Where one differs, the largest distance
    in ulps over the recorded sample is printed and reported for every output before the assertion."""
    report = {}
    for key in OUTPUTS:
        bits = np.ascontiguousarray(got[key], np.float32).reshape(-1).view(np.uint32)
        sample, want = fixture["%s.%s.sample" % (name, key)], fixture["%s.%s.crc" % (name, key)]
        mine = bits[::sample_step(bits.size)]
        assert mine.shape == sample.shape, (name, key, mine.shape, sample.shape)
        report[key] = dict(crc_equal=bool(pc.crc(bits) == want), sampled=int(sample.size), sampled_differing=int((mine != sample).sum()),
                           largest_ulps_in_sample=pc.ulps(mine, sample))
    print(label, name, report)
    assert all(r["crc_equal"] for r in report.values()), (label, name, report)


def load_fixture(name):
    import os
    return np.load(os.path.join(pc.ROOT, "tests", "golden", name + ".npz"))


# ------------------------------------------------------------------------------------------------------------ the split identity
def check_split_identity(run, case, B):
    """gw of the whole batch == float32(the float64 sum, in split order, of the gw of every split run as a call of its own), bit
    for bit over all 151 380 floats; every split's rows of feat, acts, grads and gf are the whole batch's; and the float32
    running sum of the same parts does NOT give those bits, so the comparison can tell a float reduce from the stated one.
    Returns the number of floats in which the float32 sum differs."""
    n = case["obs"].shape[0]
    args = lambda lo, hi: (case["obs"][lo:hi], case["geom"], case["blob"], case["blob_bwd"], case["grad_feat"][lo:hi])       # noqa: E731
    whole = run(*args(0, n))
    sum64, sum32 = np.zeros(pol.TRUNK_FLOATS, np.float64), np.zeros(pol.TRUNK_FLOATS, np.float32)
    assert n > 2 * B, (n, B)
    for b0 in range(0, n, B):
        part = run(*args(b0, b0 + B))
        for key in ("feat", "gf"):
            assert pc.same_bits(part[key], whole[key][b0:b0 + B]), (key, b0)
        for key in ("acts", "grads"):
            assert pc.same_bits(part[key], whole[key][:, b0:b0 + B]), (key, b0)
        sum64 = sum64 + part["gw"].astype(np.float64)
        sum32 = sum32 + part["gw"]
    differing = int((sum64.astype(np.float32).view(np.uint32) != whole["gw"].view(np.uint32)).sum())
    assert differing == 0, "gw of the whole batch differs from the double sum of its splits in %d floats, %d ulps at most" % (
        differing, pc.ulps(sum64.astype(np.float32), whole["gw"]))
    in_float = int((sum32.view(np.uint32) != whole["gw"].view(np.uint32)).sum())
    assert in_float > 0, "a float32 sum of the splits gives the same bits: this case cannot tell the two reduces apart"
    return in_float


# --------------------------------------------------------------------------------------------------------------- guarded buffers
GUARD, WS_TAIL = 1024, 4096                       # floats before and after every output; floats of workspace beyond the stated bytes
GUARD_BITS, NAN_BITS = np.uint32(0x5A5A5A5A), np.float32(np.nan).view(np.uint32)


def guarded_buffers(S, n, ws_floats):
    """{name: uint32 [GUARD + size + tail]} for feat, acts, grads, gw and the workspace: GUARD_BITS everywhere, NaN in the
    `size` floats a call may write.  The tail is GUARD floats, and WS_TAIL more behind the workspace."""
    A = S * S
    sizes = dict(feat=n * 20 * A, acts=5 * n * 64 * A, grads=n * (5 * 64 + 20) * A, gw=pol.TRUNK_FLOATS, ws=ws_floats)
    bufs = {}
    for k, size in sizes.items():
        bufs[k] = np.full(GUARD + size + GUARD + (WS_TAIL if k == "ws" else 0), GUARD_BITS, np.uint32)
        bufs[k][GUARD:GUARD + size] = NAN_BITS
    return bufs, sizes


def inactive_tiles(blocks):
    """bool [blocks, 4]: the 32 x 32 tiles of the weight-gradient kernel's 64-row blocks with no row below K + 1 or no column
    below OC (csrc/bpp_policy_train.inl: such a tile `does nothing and writes nothing`)."""
    out = []
    for rows, oc in [(37, 64)] + [(577, 64)] * 4 + [(65, 20)]:
        for f0 in range(0, rows, 64):
            out.append([not (f0 + 32 * (wave >> 1) < rows and 32 * (wave & 1) < oc) for wave in range(4)])
    assert len(out) == blocks, (len(out), blocks)
    return np.array(out)


def check_guards(bufs, sizes, splits, blocks):
    """After a forward and a backward into guarded_buffers: every guard float and the workspace beyond the stated bytes still
    hold GUARD_BITS, no output holds a NaN, and the workspace tiles of inactive waves were not stored to.  Returns the outputs
    as split_outputs gives them (views of bufs)."""
    for k, size in sizes.items():
        for what, part in (("before", bufs[k][:GUARD]), ("behind", bufs[k][GUARD + size:])):
            assert (part == GUARD_BITS).all(), "%d floats %s %s were written" % (int((part != GUARD_BITS).sum()), what, k)
        if k != "ws":
            assert not np.isnan(bufs[k][GUARD:GUARD + size].view(np.float32)).any(), "%s: not every float was written" % k
    assert sizes["ws"] == splits * blocks * 4096
    tiles = bufs["ws"][GUARD:GUARD + sizes["ws"]].reshape(splits, blocks, 4, 1024)
    idle = inactive_tiles(blocks)
    assert idle.sum() == 4 * 2 + 5 and (tiles[:, idle] == NAN_BITS).all() and not np.isnan(tiles[:, ~idle].view(np.float32)).any()
    return {k: bufs[k][GUARD:GUARD + sizes[k]].view(np.float32) for k in ("feat", "acts", "grads", "gw")}


def guarded_host_runner(L):
    """host_runner with every output and the workspace carved out of guarded_buffers, checked by check_guards."""
    def run(obs, geom, blob, blob_bwd, grad_feat):
        obs = np.ascontiguousarray(obs, np.float32)
        n, stride = obs.shape
        g = pc.geom_arg(geom)
        blob, blob_bwd = np.ascontiguousarray(blob, np.float32), np.ascontiguousarray(blob_bwd, np.float32)
        grad_feat = np.ascontiguousarray(grad_feat, np.float32)
        bytes_ = L.bpp_policy_trunk_backward_workspace(g, n)
        bufs, sizes = guarded_buffers(geom[0], n, bytes_ // 4)
        at = {k: v[GUARD:].ctypes.data for k, v in bufs.items()}
        rc = L.bpp_policy_trunk_forward_train(obs.ctypes.data, stride, n, g, blob.ctypes.data, at["feat"], at["acts"], None)
        assert rc == 0, (rc, L.bpp_last_error())
        rc = L.bpp_policy_trunk_backward(obs.ctypes.data, stride, n, g, blob_bwd.ctypes.data, at["feat"], at["acts"], grad_feat.ctypes.data,
                                         at["grads"], at["gw"], at["ws"], bytes_, None)
        assert rc == 0, (rc, L.bpp_last_error())
        i = info(L, geom, n)
        return split_outputs(geom[0], n, **check_guards(bufs, sizes, i["splits"], i["blocks"]))
    return run


def guarded_device_runner(L, device="cuda:0"):
    """device_runner with every output and the workspace a slice of a larger device tensor filled as guarded_buffers fills it;
    workspace_bytes is what bpp_policy_trunk_backward_workspace states.  L: the product library, for the sizes."""
    def run(obs, geom, blob, blob_bwd, grad_feat):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)        # noqa: E731
        o = dev(obs)
        n, S = o.shape[0], geom[0]
        bufs, sizes = guarded_buffers(S, n, L.bpp_policy_trunk_backward_workspace(pc.geom_arg(geom), n) // 4)
        whole = {k: torch.from_numpy(v.view(np.float32)).to(device) for k, v in bufs.items()}
        t = {k: v[GUARD:GUARD + sizes[k]] for k, v in whole.items()}
        pol.trunk_forward_train(o, dev(blob), geom, feat=t["feat"].view(n, -1), acts=t["acts"].view(5, n, 64, S, S))
        pol.trunk_backward(o, geom, dev(blob_bwd), t["feat"].view(n, -1), t["acts"].view(5, n, 64, S, S), dev(grad_feat), grads=t["grads"],
                           grad_weights=t["gw"], workspace=t["ws"])
        torch.cuda.synchronize()
        bufs = {k: v.cpu().numpy().view(np.uint32) for k, v in whole.items()}
        i = info(L, geom, n)
        return split_outputs(S, n, **check_guards(bufs, sizes, i["splits"], i["blocks"]))
    return run
