"""Shared cases of the trunk-training tests (tests/test_policy_train.py on the emulator, tests/test_gpu_policy_train.py on the
device): exact-integer networks whose forward, input gradients and weight gradients are known in int64, real-valued networks with
a float64 torch autograd reference, and the runners that call bpp_policy_trunk_forward_train and bpp_policy_trunk_backward
(include/bpp_policy_train.h) with host or device pointers.  The forward-side helpers are those of tests/policy_cases.py."""
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
    obs = np.full((n, stride), 7.0, np.float32)
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
    S, nf, seed, taps = EXACT_SPECS[name]
    i = info(L, geom_of(S), 1)
    return dict(S=S, n=nf(i["bins_per_group"], i["bins_per_split"]), seed=seed, taps=taps)


def check_exact(run, case):
    got = run(case["obs"], case["geom"], case["blob"], case["blob_bwd"], case["grad_feat"])
    for key in OUTPUTS:
        assert pc.same_bits(got[key], case["want"][key]), (key, np.abs(got[key].astype(np.float64) - case["want"][key]).max())
    return got


# name -> (side, n as a function of (bins per input-gradient workgroup P, bins per split B) of that side, seed, taps per channel)
EXACT_SPECS = {
    "s10_n1": (10, lambda P, B: 1, 1, 3), "s10_nP1": (10, lambda P, B: P + 1, 2, 3), "s10_n5": (10, lambda P, B: 5, 3, 3),
    "s5_n2": (5, lambda P, B: 2, 4, 3), "s5_three_splits": (5, lambda P, B: 2 * B + 1, 5, 3),
    "s3_n3": (3, lambda P, B: 3, 6, 3), "s1_n3": (1, lambda P, B: 3, 7, 20),       # A = 1: only the centre taps count, so more of them
    "s11_n3": (11, lambda P, B: 3, 8, 3), "s15_n2": (15, lambda P, B: 2, 9, 3),
}


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
