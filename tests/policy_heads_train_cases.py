"""Shared cases of the head-training tests (tests/test_policy_heads_train.py on the emulator, tests/test_gpu_policy_heads_train.py
on the device): exact-integer heads whose forward, input gradients and weight gradients are known in int64, real-valued heads with
a float64 torch autograd reference, the header's arithmetic stated in numpy (normative_heads, on tc.fma32) with the cases whose
bits are recorded in tests/golden/heads_train_chain_bits.npz, the split identity, guarded buffers, and the runners that call
bpp_policy_heads_forward_train and bpp_policy_heads_backward (include/bpp_policy_heads_train.h) with host or device pointers."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import policy_cases as pc
import policy_train_cases as tc
from bpp_amd import _lib
from bpp_amd import policy as pol

OUTPUTS = ("value", "logits", "pred", "hidden", "grad_hidden", "grad_out_mask", "grad_feat", "gw")
ROW_OUTPUTS = ("value", "logits", "pred", "grad_out_mask", "grad_feat")           # [n, ...]; hidden and grad_hidden are [3, n, H]
HEADS3 = (("base.actor.3", "dist.linear"), ("base.mask.3", "base.mask.5"), ("base.critic.3", "base.critic_linear"))
BINS_PER_SPLIT = 128        # include/bpp_policy_heads_train.h: `bins per split`, whatever geom and n are
TRUNK = pol.TRUNK_FLOATS


def info(L, geom, n):
    out = (ctypes.c_int32 * 8)()
    rc = L.bpp_policy_heads_backward_info(pc.geom_arg(geom), int(n), out)
    assert rc == 0, rc
    return dict(zip(_lib.POLICY_HEADS_TRAIN_INFO, (int(v) for v in out)))


def sizes(geom, n):
    """{output: floats}"""
    S, H, M = geom
    A = S * S
    return dict(value=n, logits=n * M, pred=n * M, hidden=3 * n * H, grad_hidden=3 * n * H, grad_out_mask=n * M, grad_feat=n * 20 * A,
                gw=(8 * A + 1) * H * 2 + (4 * A + 1) * H + (H + 1) * (2 * M + 1))


def shaped(geom, n, flat):
    S, H, M = geom
    shapes = dict(value=(n,), logits=(n, M), pred=(n, M), hidden=(3, n, H), grad_hidden=(3, n, H), grad_out_mask=(n, M), grad_feat=(n, 20 * S * S),
                  gw=(-1,))
    return {k: flat[k].reshape(shapes[k]) for k in OUTPUTS}


def blobs(plain, geom):
    """(the forward blob: the trunk's 151 380 floats as zeros -- the heads never read them -- then the six Linear layers; the
    backward blob) as numpy."""
    tail = pol.pack_heads(plain).numpy()
    return np.concatenate([np.zeros(TRUNK, np.float32), tail]), pol.pack_heads_backward(plain).numpy()


def _call(L, geom, n, ptr, gptr, ws_ptr, ws_bytes):
    g = pc.geom_arg(geom)
    rc = L.bpp_policy_heads_forward_train(ptr["feat"], n, g, ptr["blob"], ptr["value"], ptr["logits"], ptr["pred"], ptr["hidden"], None)
    assert rc == 0, (rc, L.bpp_last_error())
    rc = L.bpp_policy_heads_backward(ptr["feat"], ptr["hidden"], ptr["pred"], gptr[0], gptr[1], gptr[2], n, g, ptr["blob_bwd"], ptr["grad_feat"],
                                     ptr["grad_hidden"], ptr["grad_out_mask"], ptr["gw"], ws_ptr, ws_bytes, None)
    assert rc == 0, (rc, L.bpp_last_error())


def host_runner(L):
    """run(feat [n, 20 A], geom, blob, blob_bwd, grad_value, grad_logits, grad_pred) -> {output: numpy} through host pointers (the
    emulated library); a gradient may be None; every output starts as NaN."""
    def run(feat, geom, blob, blob_bwd, gv, gl, gp):
        n = feat.shape[0]
        c = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)       # noqa: E731
        ins = dict(feat=c(feat), blob=c(blob), blob_bwd=c(blob_bwd))
        grads = [c(gv), c(gl), c(gp)]
        out = {k: np.full(v, np.nan, np.float32) for k, v in sizes(geom, n).items()}
        bytes_ = L.bpp_policy_heads_backward_workspace(pc.geom_arg(geom), n)
        ws = np.full(bytes_ // 4, np.nan, np.float32)
        ptr = {k: v.ctypes.data for k, v in list(ins.items()) + list(out.items())}
        _call(L, geom, n, ptr, [None if a is None else a.ctypes.data for a in grads], ws.ctypes.data, bytes_)
        return shaped(geom, n, out)
    return run


def device_runner(device="cuda:0"):
    """The same through bpp_amd.policy.heads_forward_train / heads_backward on the device."""
    def run(feat, geom, blob, blob_bwd, gv, gl, gp):
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)        # noqa: E731
        f = dev(feat)
        value, logits, pred, hidden = pol.heads_forward_train(f, dev(blob), geom)
        gf, gh, gom, gw = pol.heads_backward(f, hidden, pred, dev(gv), dev(gl), dev(gp), geom, dev(blob_bwd))
        torch.cuda.synchronize()
        flat = dict(zip(OUTPUTS, (t.cpu().numpy().reshape(-1) for t in (value, logits, pred, hidden, gh, gom, gf, gw))))
        return shaped(geom, f.shape[0], flat)
    return run


def run_case(run, case, **replace):
    a = dict(case, **replace)
    return run(a["feat"], a["geom"], a["blob"], a["blob_bwd"], a["grad_value"], a["grad_logits"], a["grad_pred"])


# --------------------------------------------------------------------------------------------------------------- guarded buffers
GUARD = 1024
GUARD_BITS, NAN_BITS = tc.GUARD_BITS, tc.NAN_BITS


def guarded_buffers(geom, n, ws_floats):
    """({name: uint32 [GUARD + size + GUARD]} for every output and the workspace, sizes): GUARD_BITS in the guards, NaN in the
    `size` floats a call may write."""
    sz = dict(sizes(geom, n), ws=ws_floats)
    bufs = {}
    for k, size in sz.items():
        bufs[k] = np.full(2 * GUARD + size, GUARD_BITS, np.uint32)
        bufs[k][GUARD:GUARD + size] = NAN_BITS
    return bufs, sz


def check_guards(bufs, sz):
    """Every guard float still holds GUARD_BITS and no output holds a NaN.  Returns the flat outputs (views of bufs)."""
    for k, size in sz.items():
        for what, part in (("before", bufs[k][:GUARD]), ("behind", bufs[k][GUARD + size:])):
            assert (part == GUARD_BITS).all(), "%d floats %s %s were written" % (int((part != GUARD_BITS).sum()), what, k)
        if k != "ws":
            assert not np.isnan(bufs[k][GUARD:GUARD + size].view(np.float32)).any(), "%s: not every float was written" % k
    return {k: bufs[k][GUARD:GUARD + sz[k]].view(np.float32) for k in OUTPUTS}


def guarded_host_runner(L):
    """host_runner with every output and the workspace carved out of guarded_buffers, checked by check_guards."""
    def run(feat, geom, blob, blob_bwd, gv, gl, gp):
        n = feat.shape[0]
        c = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)       # noqa: E731
        ins = dict(feat=c(feat), blob=c(blob), blob_bwd=c(blob_bwd))
        grads = [c(gv), c(gl), c(gp)]
        bytes_ = L.bpp_policy_heads_backward_workspace(pc.geom_arg(geom), n)
        bufs, sz = guarded_buffers(geom, n, bytes_ // 4)
        ptr = {k: v.ctypes.data for k, v in ins.items()}
        ptr.update({k: v[GUARD:].ctypes.data for k, v in bufs.items()})
        _call(L, geom, n, ptr, [None if a is None else a.ctypes.data for a in grads], ptr["ws"], bytes_)
        return shaped(geom, n, check_guards(bufs, sz))
    return run


def guarded_device_runner(L, device="cuda:0"):
    """device_runner with every output and the workspace a slice of a larger device tensor filled as guarded_buffers fills it;
    workspace_bytes is what bpp_policy_heads_backward_workspace states.  L: the product library, for the sizes."""
    def run(feat, geom, blob, blob_bwd, gv, gl, gp):
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)        # noqa: E731
        f = dev(feat)
        n = f.shape[0]
        bufs, sz = guarded_buffers(geom, n, L.bpp_policy_heads_backward_workspace(pc.geom_arg(geom), n) // 4)
        whole = {k: torch.from_numpy(v.view(np.float32)).to(device) for k, v in bufs.items()}
        t = {k: v[GUARD:GUARD + sz[k]] for k, v in whole.items()}
        pol.heads_forward_train(f, dev(blob), geom, value=t["value"], logits=t["logits"], pred=t["pred"], hidden=t["hidden"])
        pol.heads_backward(f, t["hidden"], t["pred"], dev(gv), dev(gl), dev(gp), geom, dev(blob_bwd), grad_feat=t["grad_feat"],
                           grad_hidden=t["grad_hidden"], grad_out_mask=t["grad_out_mask"], grad_weights=t["gw"], workspace=t["ws"])
        torch.cuda.synchronize()
        return shaped(geom, n, check_guards({k: v.cpu().numpy().view(np.uint32) for k, v in whole.items()}, sz))
    return run


def check_absent_heads(run, case):
    """A NULL output gradient: zeros in that head's slice of grad_feat, its rows of grad_hidden, grad_out_mask for the mask head
    and its weight gradients; the bits of the full call everywhere else."""
    S, H, M = case["geom"]
    A, n = S * S, case["feat"].shape[0]
    full = run_case(run, case)
    zero = lambda a: not np.asarray(a).view(np.uint32).any()       # noqa: E731
    for h, key in enumerate(("grad_logits", "grad_pred", "grad_value")):
        got = run_case(run, case, **{key: None})
        mine, ref = unpack_gradient(got["gw"], case["geom"]), unpack_gradient(full["gw"], case["geom"])
        f0, K1 = h * 8 * A, (4 if h == 2 else 8) * A
        for g in range(3):
            lo, k1 = g * 8 * A, (4 if g == 2 else 8) * A
            names = [nm + s for nm in HEADS3[g] for s in (".weight", ".bias")]
            if g == h:
                assert zero(got["grad_feat"][:, f0:f0 + K1]) and zero(got["grad_hidden"][g]) and all(zero(mine[k]) for k in names), (key, g)
            else:
                assert pc.same_bits(got["grad_feat"][:, lo:lo + k1], full["grad_feat"][:, lo:lo + k1]), (key, g)
                assert pc.same_bits(got["grad_hidden"][g], full["grad_hidden"][g]) and all(pc.same_bits(mine[k], ref[k]) for k in names), (key, g)
        assert zero(got["grad_out_mask"]) if h == 1 else pc.same_bits(got["grad_out_mask"], full["grad_out_mask"])
        assert float(np.abs(full["grad_hidden"][h]).max()) > 0
    only = run_case(run, case, grad_logits=None, grad_pred=None)
    assert zero(only["grad_feat"][:, :16 * A]) and pc.same_bits(only["grad_feat"][:, 16 * A:], full["grad_feat"][:, 16 * A:])
    return n


# ---------------------------------------------------------------------------------------------------------------- exact cases
# (S, H, M, n); the tests add two shapes at EXACT_SPLIT_GEOM with n = B + 1 and 2 B + 1 for the info call's bins per split B
EXACT_SHAPES = [(1, 32, 1, 1), (1, 32, 2, 65), (3, 64, 9, 63), (5, 288, 25, 64), (10, 256, 100, 5), (10, 256, 200, 5), (15, 512, 450, 2),
                (20, 32, 400, 3)]
EXACT_SPLIT_GEOM = (2, 32, 4)


def _sparse(rng, oc, k, taps=3):
    """Integer [oc, k] with `taps` nonzero entries per row from {2, 1, -1} in both sign patterns; biases in {-2 .. 2} without 0."""
    w = np.zeros((oc, k), np.int64)
    for o in range(oc):
        t = min(taps, k)
        vals = np.array([2, -1, 1][:t]) * (1 if o % 2 == 0 else -1)
        w[o, rng.choice(k, t, replace=False)] = rng.permutation(vals)
    return w, rng.choice([-2, -1, 1, 2], oc).astype(np.int64)


def exact_case(S, H, M, n, seed=1):
    """dict(geom, feat, blob, blob_bwd, grad_value, grad_logits, grad_pred, want {every output}) of integer heads: every partial
    sum of every chain -- forward, input gradient, weight-gradient split and the sum of the splits -- stays below 2^24 in the
    absolute-value network (asserted in int64), so float32 is exact in any order.  The hidden masks are mixed, and the mask
    head's output mask wherever there is room for it (asserted)."""
    rng = np.random.RandomState(seed + 1000 * S + n)
    A = S * S
    feat = (rng.randint(0, 4, (n, 20 * A)) * (rng.random_sample((n, 20 * A)) < 0.6)).astype(np.int64)       # post-ReLU values
    w, want, gw = {}, {}, {}
    hidden, ghid = np.zeros((3, n, H), np.int64), np.zeros((3, n, H), np.int64)
    gfeat = np.zeros((n, 20 * A), np.int64)
    go = dict(grad_value=rng.choice([-2, -1, 1, 2], (n, 1)), grad_logits=rng.choice([-2, -1, 1, 2], (n, M)),
              grad_pred=rng.choice([-2, -1, 1, 2], (n, M)))
    go = {k: v.astype(np.int64) for k, v in go.items()}

    def bounded(mag, what):
        assert np.abs(mag).max() < tc.LIMIT, (what, int(np.abs(mag).max()))

    for h, (first, second) in enumerate(HEADS3):
        K1, f0, Mh = (4 if h == 2 else 8) * A, h * 8 * A, 1 if h == 2 else M
        W1, b1 = _sparse(rng, H, K1)
        W2, b2 = _sparse(rng, Mh, H)
        w[first + ".weight"], w[first + ".bias"], w[second + ".weight"], w[second + ".bias"] = W1, b1, W2, b2
        x = feat[:, f0:f0 + K1]
        pre, mag = pc._linear64(x, W1, b1)
        bounded(mag, first)
        hid = np.maximum(pre, 0)
        assert (hid > 0).any() and (hid == 0).any(), "%s: the mask is not mixed" % first
        out, mag = pc._linear64(hid, W2, b2)
        bounded(mag, second)
        g = go[("grad_logits", "grad_pred", "grad_value")[h]]
        if h == 1:
            want["pred"] = np.maximum(out, 0)
            assert n * M < 8 or ((out > 0).any() and (out <= 0).any() and (g[out <= 0] != 0).any()), "the output mask of the mask head is not mixed"
            g = np.where(out > 0, g, 0)
            want["grad_out_mask"] = g
        else:
            want["logits" if h == 0 else "value"] = out
        d = g @ W2
        bounded(np.abs(g) @ np.abs(W2), "Dh " + second)
        G = np.where(hid > 0, d, 0)
        assert n * Mh < 8 or ((G != 0).any() and (d[hid == 0] != 0).any()), "%s: the mask removes nothing or everything" % first
        gfeat[:, f0:f0 + K1] = G @ W1
        bounded(np.abs(G) @ np.abs(W1), "grad_feat " + first)
        hidden[h], ghid[h] = hid, G
        gw[second + ".weight"], gw[second + ".bias"] = g.T @ hid, g.sum(0)
        gw[first + ".weight"], gw[first + ".bias"] = G.T @ x, G.sum(0)
        bounded(np.abs(g).T @ np.abs(hid), "dW " + second)
        bounded(np.abs(G).T @ np.abs(x), "dW " + first)
        assert n * Mh < 8 or ((gw[second + ".weight"] != 0).any() and (gw[first + ".weight"] != 0).any() and (gw[first + ".bias"] != 0).any())
    f32 = lambda a: np.asarray(a).astype(np.float32)        # noqa: E731
    plain = {k: torch.from_numpy(f32(v)) for k, v in w.items()}
    blob, blob_bwd = blobs(plain, (S, H, M))
    want.update(value=want["value"].reshape(n), hidden=hidden, grad_hidden=ghid, grad_feat=gfeat,
                gw=pol.pack_heads({k: torch.from_numpy(f32(v)) for k, v in gw.items()}).numpy())
    return dict(geom=(S, H, M), feat=f32(feat), plain=plain, blob=blob, blob_bwd=blob_bwd, grad_value=f32(go["grad_value"]).reshape(n),
                grad_logits=f32(go["grad_logits"]), grad_pred=f32(go["grad_pred"]), want={k: f32(v) for k, v in want.items()})


def check_exact(run, case):
    got = run_case(run, case)
    for key in OUTPUTS:
        assert pc.same_bits(got[key], case["want"][key]), (key, np.abs(got[key].astype(np.float64) - case["want"][key]).max())
    return got


# ----------------------------------------------------------------------------------------------------------------- real cases
def heads_forward_torch(w, feat):
    """(value, logits, pred) of the six Linear layers of pol.torch_forward on head features [n, 20 A], in the dtype of w."""
    A = feat.shape[1] // 20

    def head(name, lo, hi):
        return F.relu(F.linear(feat[:, lo * A:hi * A], w[name + ".3.weight"], w[name + ".3.bias"]))

    value = F.linear(head("base.critic", 16, 20), w["base.critic_linear.weight"], w["base.critic_linear.bias"]).reshape(-1)
    logits = F.linear(head("base.actor", 0, 8), w["dist.linear.weight"], w["dist.linear.bias"])
    pred = F.relu(F.linear(head("base.mask", 8, 16), w["base.mask.5.weight"], w["base.mask.5.bias"]))
    return value, logits, pred


def heads_autograd(plain, feat, gv, gl, gp, dtype):
    """{every dW and db of the six Linear layers, grad_feat} as numpy from torch autograd in `dtype` over heads_forward_torch."""
    w = {k: plain[k].detach().to(dtype).clone().requires_grad_(True) for k in pol.HEAD_PARAMETERS}
    f = torch.as_tensor(feat).to(dtype).clone().requires_grad_(True)
    outs = heads_forward_torch(w, f)
    torch.autograd.backward(list(outs), [torch.as_tensor(g).to(dtype) for g in (gv, gl, gp)])
    out = {k: v.grad.numpy() for k, v in w.items()}
    out["grad_feat"] = f.grad.numpy()
    return out


def head_ties(plain, feat):
    """bool [n]: the rows in which some pre-activation of the six Linear layers lies within float32 rounding of zero,
    |pre| <= 2 * 2^-24 * sum |x_k w_k| (tc.tied_bins' rule), decided from the float64 forward alone."""
    w = {k: v.detach().cpu().double() for k, v in plain.items()}
    f = torch.as_tensor(feat).double()
    A = f.shape[1] // 20
    tied = torch.zeros(f.shape[0], dtype=torch.bool)
    for h, (first, second) in enumerate(HEADS3):
        x = f[:, h * 8 * A:h * 8 * A + (4 if h == 2 else 8) * A]
        for name in (first, second):
            pre = F.linear(x, w[name + ".weight"], w[name + ".bias"])
            mag = F.linear(x.abs(), w[name + ".weight"].abs(), w[name + ".bias"].abs())
            if name != "dist.linear" and name != "base.critic_linear":          # layers with a ReLU behind them
                tied |= (pre.abs() <= 2.0 * 2.0 ** -24 * mag).any(1)
            x = F.relu(pre)
    return tied.numpy()


def tied_states(plain, obs):
    """bool [n]: tc.tied_bins extended to the pre-activations of the Linear layers with a ReLU behind them, on the float64
    forward of the whole network."""
    zeros = np.zeros((obs.shape[0], 20 * (obs.shape[1] // 4)), np.float32)
    return tc.tied_bins(plain, obs) | head_ties(plain, tc.trunk_autograd(plain, obs, zeros, torch.float64)["feat"])


def trunk_feat(plain, obs):
    """float32 head features [n, 20 A] of torch's trunk on obs (the input of the heads-alone cases)."""
    n = obs.shape[0]
    return tc.trunk_autograd(plain, obs, np.zeros((n, 20 * (obs.shape[1] // 4)), np.float32), torch.float32)["feat"]


def real_case(geom, obs, seed=11, gseed=3):
    """dict(geom, feat, plain, blob, blob_bwd, grad_*, ref64, ref32): pc.real_weights, the float32 torch head features of obs,
    standard-normal output gradients, and torch autograd over the six Linear layers in float64 and float32 on that feat."""
    S, H, M = geom
    plain = pc.real_weights(S, H, M, seed)
    feat = trunk_feat(plain, obs)
    n = feat.shape[0]
    gen = torch.Generator().manual_seed(gseed)
    gv, gl, gp = (torch.randn(shape, generator=gen).numpy() for shape in ((n,), (n, M), (n, M)))
    blob, blob_bwd = blobs(plain, geom)
    return dict(geom=geom, feat=feat, plain=plain, blob=blob, blob_bwd=blob_bwd, grad_value=gv, grad_logits=gl, grad_pred=gp,
                ref64=heads_autograd(plain, feat, gv, gl, gp, torch.float64), ref32=heads_autograd(plain, feat, gv, gl, gp, torch.float32))


def unpack_gradient(gw, geom):
    return {k: v.numpy() for k, v in pol.unpack_heads_gradient(torch.from_numpy(np.ascontiguousarray(gw)), geom[0], geom[1], geom[2]).items()}


def check_real(got, case, label=""):
    """Every dW, every db and grad_feat under tc.check_gradients' 8 x rule."""
    mine = unpack_gradient(got["gw"], case["geom"])
    mine["grad_feat"] = got["grad_feat"]
    return tc.check_gradients(mine, case["ref64"], case["ref32"], label)


# -------------------------------------------------------- the header's arithmetic in numpy (include/bpp_policy_heads_train.h)
def _chain(x, W, start):
    """acc[b][o] = fmaf(x[b][k], W[o][k], acc[b][o]) over ascending k from `start` [b][o]."""
    acc = np.array(start, np.float32)
    for k in range(x.shape[1]):
        acc = tc.fma32(x[:, k, None], W[None, :, k], acc)
    return acc


def normative_heads(plain, feat, gv, gl, gp, geom, bins_per_split=BINS_PER_SPLIT):
    """{every output} as include/bpp_policy.h and include/bpp_policy_heads_train.h state them, one fma32 per step of every
    chain, in plain numpy: nothing of torch's Linear and nothing of the emulator.
      forward    every output one chain from the bias over ascending k; ReLU behind the first Linear and behind mask.5
      go'        grad_pred where pred > 0 for the mask head (grad_out_mask); grad_logits; grad_value as one column
      Dh         one chain over ascending m from +0 on W2[m][h];  Gh = hidden > 0 ? Dh : 0
      grad_feat  one chain over ascending h from +0 on W1[h][k]
      dW, db     per split of `bins_per_split` consecutive bins one chain per element from +0 over ascending b, the bias on an
                 input value of 1; the splits are added in split order in float64 and cast once
    gw is packed with pol.pack_heads."""
    S, H, M = geom
    A, B = S * S, int(bins_per_split)
    w = {k: np.asarray(v, np.float32) for k, v in plain.items()}
    feat = np.ascontiguousarray(feat, np.float32)
    n = feat.shape[0]
    out = dict(hidden=np.zeros((3, n, H), np.float32), grad_hidden=np.zeros((3, n, H), np.float32), grad_feat=np.zeros((n, 20 * A), np.float32))
    grads = (np.asarray(gl, np.float32), np.asarray(gp, np.float32), np.asarray(gv, np.float32).reshape(n, 1))
    relu = lambda v: np.where(v > 0, v, np.float32(0)).astype(np.float32)       # noqa: E731

    def wgrad(x, g):
        """x [n, K], g [n, OC] -> (dW [OC, K], db [OC])"""
        x1 = np.concatenate([x, np.ones((n, 1), np.float32)], 1)
        total = np.zeros((x1.shape[1], g.shape[1]), np.float64)
        for b0 in range(0, n, B):
            acc = np.zeros(total.shape, np.float32)
            for b in range(b0, min(n, b0 + B)):
                acc = tc.fma32(x1[b, :, None], g[b, None, :], acc)
            total = total + acc.astype(np.float64)
        total = total.astype(np.float32)
        return total[:-1].T, total[-1]

    gw = {}
    for h, (first, second) in enumerate(HEADS3):
        K1, f0, Mh = (4 if h == 2 else 8) * A, h * 8 * A, 1 if h == 2 else M
        W1, b1, W2, b2 = w[first + ".weight"], w[first + ".bias"], w[second + ".weight"], w[second + ".bias"]
        x = feat[:, f0:f0 + K1]
        hid = relu(_chain(x, W1, np.broadcast_to(b1, (n, H))))
        o = _chain(hid, W2, np.broadcast_to(b2, (n, Mh)))
        g = grads[h]
        if h == 1:
            o = np.where(o > 0, o, np.float32(0)).astype(np.float32)            # head == 1 && !(v > 0) ? 0 : v
            g = np.where(o > 0, g, np.float32(0)).astype(np.float32)
            out["pred"], out["grad_out_mask"] = o, g
        else:
            out["logits" if h == 0 else "value"] = o if h == 0 else o.reshape(n)
        d = _chain(g, W2.T, np.zeros((n, H), np.float32))
        G = np.where(hid > 0, d, np.float32(0)).astype(np.float32)
        out["grad_feat"][:, f0:f0 + K1] = _chain(G, W1.T, np.zeros((n, K1), np.float32))
        out["hidden"][h], out["grad_hidden"][h] = hid, G
        gw[second + ".weight"], gw[second + ".bias"] = wgrad(hid, g)
        gw[first + ".weight"], gw[first + ".bias"] = wgrad(x, G)
    out["gw"] = pol.pack_heads({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in gw.items()}).numpy()
    return out


# ---- the recorded bits of that reference on real-valued data (tests/golden/make_heads_train_chain_bits.py) -------------------
CHAIN_FIXTURE = "heads_train_chain_bits"
CHAIN_CASES = [(3, 64, 9, 66), (5, 288, 25, 3), (10, 256, 100, 11), (10, 256, 200, 3), (2, 32, 4, 300)]      # the last: three splits
CHAIN_INPUTS = ("feat", "blob", "blob_bwd", "grad_value", "grad_logits", "grad_pred")


def chain_name(S, H, M, n):
    return "heads_s%d_h%d_m%d_n%d" % (S, H, M, n)


def chain_case(S, H, M, n, seed=7):
    """dict(geom, feat, plain, blob, blob_bwd, grad_*) from numpy.random.RandomState alone: weights normal * sqrt(2 / fan_in),
    biases uniform in +-0.1, head features the positive part of a standard normal (about half of them zero, as a ReLU leaves
    them), standard-normal output gradients."""
    rng = np.random.RandomState(seed)
    plain = {}
    for name, shape in pol.layer_shapes(S, H, M)[8:]:
        plain[name + ".weight"] = torch.from_numpy((rng.standard_normal(shape) * np.sqrt(2.0 / shape[1])).astype(np.float32))
        plain[name + ".bias"] = torch.from_numpy(rng.uniform(-0.1, 0.1, shape[0]).astype(np.float32))
    feat = np.maximum(rng.standard_normal((n, 20 * S * S)), 0).astype(np.float32)
    gv, gl, gp = (rng.standard_normal(shape).astype(np.float32) for shape in ((n,), (n, M), (n, M)))
    blob, blob_bwd = blobs(plain, (S, H, M))
    return dict(geom=(S, H, M), feat=feat, plain=plain, blob=blob, blob_bwd=blob_bwd, grad_value=gv, grad_logits=gl, grad_pred=gp)


def chain_reference(case):
    return normative_heads(case["plain"], case["feat"], case["grad_value"], case["grad_logits"], case["grad_pred"], case["geom"])


def chain_entries(case, outputs, name):
    """{key: array} of one case for the fixture: a CRC32 of each input; per output a CRC32 of all its bits and every
    tc.sample_step-th of them."""
    out = {"%s.crc.%s" % (name, k): pc.crc(np.ascontiguousarray(case[k], np.float32)) for k in CHAIN_INPUTS}
    for key in OUTPUTS:
        bits = np.ascontiguousarray(outputs[key], np.float32).reshape(-1).view(np.uint32)
        out["%s.%s.crc" % (name, key)] = pc.crc(bits)
        out["%s.%s.sample" % (name, key)] = bits[::tc.sample_step(bits.size)].copy()
    return out


def check_chain(got, fixture, name, label=""):
    """Every output of `got` against the recorded reference: the CRC32 of all its bits; the largest distance in ulps over the
    recorded sample is printed for every output before the assertion."""
    report = {}
    for key in OUTPUTS:
        bits = np.ascontiguousarray(got[key], np.float32).reshape(-1).view(np.uint32)
        sample, want = fixture["%s.%s.sample" % (name, key)], fixture["%s.%s.crc" % (name, key)]
        mine = bits[::tc.sample_step(bits.size)]
        assert mine.shape == sample.shape, (name, key, mine.shape, sample.shape)
        report[key] = dict(crc_equal=bool(pc.crc(bits) == want), sampled=int(sample.size), sampled_differing=int((mine != sample).sum()),
                           largest_ulps_in_sample=pc.ulps(mine, sample))
    print(label, name, report)
    assert all(r["crc_equal"] for r in report.values()), (label, name, report)


# ------------------------------------------------------------------------------------------------------------ the split identity
def check_split_identity(run, case, B):
    """gw of the whole batch == float32(the float64 sum, in split order, of the gw of every split run as a call of its own), bit
    for bit; every split's rows of the row outputs are the whole batch's; and the float32 running sum of the same parts does NOT
    give those bits.  Returns the number of floats in which the float32 sum differs."""
    n = case["feat"].shape[0]
    assert n > 2 * B, (n, B)
    rows = lambda lo, hi: {k: case[k][lo:hi] for k in ("feat", "grad_value", "grad_logits", "grad_pred")}       # noqa: E731
    whole = run_case(run, case)
    sum64, sum32 = np.zeros(whole["gw"].size, np.float64), np.zeros(whole["gw"].size, np.float32)
    for b0 in range(0, n, B):
        part = run_case(run, case, **rows(b0, b0 + B))
        for key in ROW_OUTPUTS:
            assert pc.same_bits(part[key], whole[key][b0:b0 + B]), (key, b0)
        for key in ("hidden", "grad_hidden"):
            assert pc.same_bits(part[key], whole[key][:, b0:b0 + B]), (key, b0)
        sum64 = sum64 + part["gw"].astype(np.float64)
        sum32 = sum32 + part["gw"]
    differing = int((sum64.astype(np.float32).view(np.uint32) != whole["gw"].view(np.uint32)).sum())
    assert differing == 0, "gw of the whole batch differs from the double sum of its splits in %d floats" % differing
    in_float = int((sum32.view(np.uint32) != whole["gw"].view(np.uint32)).sum())
    assert in_float > 0, "a float32 sum of the splits gives the same bits: this case cannot tell the two reduces apart"
    return in_float
