"""Cases, helpers and bounds shared by tests/test_kfac.py (emulated kernels, CPU) and tests/test_gpu_kfac.py (device):
bpp_kfac_factor (include/bpp_kfac.h) and bpp_amd.KFACOptimizer.

A case is a dict: layout, conv (kernel, stride, padding; PATCH only), x (float32 source), and for the real-valued cases x2 (a
second batch), scale and rho.  `run` is a callable (case, x, m, first, scale, rho) -> new m as numpy, so that one set of checks
serves the emulated library and the device.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

PATCH, ROWS, NCHW = 0, 1, 2
EPS = 2.0 ** -24            # one float32 rounding, relative
BADARG = -1


def conv_of(k=1, s=1, p=0):
    """k, s, p: an int for a square kernel / stride / padding, or a pair (height, width)."""
    def pair(v):
        return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))
    return dict(kernel_size=pair(k), stride=pair(s), padding=pair(p))


def geom(case):
    x = case["x"]
    if case["layout"] == PATCH:
        c = case["conv"]
        return list(x.shape) + list(c["kernel_size"]) + list(c["stride"]) + list(c["padding"])
    if case["layout"] == ROWS:
        return list(x.shape)
    return [x.shape[0], x.shape[1], int(np.prod(x.shape[2:]))]


def rows64(case, x=None):
    """The rows X of the factor, float64 [R, D], by plain loops over the kernel window."""
    x = np.asarray(case["x"] if x is None else x, dtype=np.float64)
    if case["layout"] == ROWS:
        return x
    if case["layout"] == NCHW:
        B, D = x.shape[:2]
        return x.reshape(B, D, -1).transpose(0, 2, 1).reshape(-1, D)
    c = case["conv"]
    (kh, kw), (sh, sw), (ph, pw) = c["kernel_size"], c["stride"], c["padding"]
    B, C, H, W = x.shape
    xp = np.zeros((B, C, H + 2 * ph, W + 2 * pw))
    xp[:, :, ph:ph + H, pw:pw + W] = x
    OH, OW = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    out = np.zeros((B, OH, OW, C, kh, kw))
    for i in range(kh):
        for j in range(kw):
            out[:, :, :, :, i, j] = xp[:, :, i:i + sh * (OH - 1) + 1:sh, j:j + sw * (OW - 1) + 1:sw].transpose(0, 2, 3, 1)
    return out.reshape(B * OH * OW, C * kh * kw)


def positions(case):
    x = case["x"]
    if case["layout"] == ROWS:
        return 1
    if case["layout"] == NCHW:
        return int(np.prod(x.shape[2:]))
    return rows64(case).shape[0] // x.shape[0]


def reference_scale(case, kind):
    """The reference's scalings multiplied out in double (include/bpp_kfac.h cites the lines)."""
    B, P = float(case["x"].shape[0]), float(positions(case))
    return {"conv_a": 1.0 / (B * P * P), "conv_g": B * P, "linear_a": 1.0 / B, "linear_g": B}[kind]


def expected64(case, x, m0, first, scale, rho):
    """(float64 value of the header's expressions with exact rho, scale * sum |x_ri x_rj|)."""
    X = rows64(case, x)
    aa = scale * (X.T @ X)
    mag = scale * (np.abs(X).T @ np.abs(X))
    m = aa if first else np.asarray(m0, dtype=np.float64)
    return rho * m + (1.0 - rho) * aa, mag


def bound(n, mag, m0, first, rho):
    """|err| <= (n + 3) 2^-24 scale sum_r |x_ri x_rj| for a factor that replaces m (first): n roundings of the chain, the cast
    and the running average.  Onto a given m0 the result is rho m0 + (1 - rho) aa, and the same count of roundings applies to
    the magnitudes that enter it: rho |m0| + (1 - rho) scale sum |x_ri x_rj| (for m0 = aa this is the line above)."""
    if first:
        return (n + 3) * EPS * mag
    return (n + 3) * EPS * (rho * np.abs(np.asarray(m0, dtype=np.float64)) + (1.0 - rho) * mag)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the emulated / host library ------------------------------------------------------------------------------------------
def geom_arg(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def info(L, layout, g):
    out = (ctypes.c_int32 * 6)()
    rc = L.bpp_kfac_factor_info(layout, geom_arg(g), out)
    assert rc == 0, L.bpp_last_error()
    return dict(zip(("D", "R", "tile", "rows_per_split", "splits", "chain"), (int(v) for v in out)))


def host_runner(L):
    """run(case, x, m, first, scale, rho) on a library that takes host pointers (the emulator)."""
    def run(case, x, m, first, scale, rho):
        c = dict(case, x=x)
        g = geom_arg(geom(c))
        x = np.ascontiguousarray(x, dtype=np.float32)
        m = np.array(m, dtype=np.float32, copy=True)
        ws = np.full(L.bpp_kfac_factor_workspace(case["layout"], g) // 4 + 2, np.nan, np.float32)
        rc = L.bpp_kfac_factor(x.ctypes.data, case["layout"], g, m.ctypes.data, float(scale), float(rho), int(first), ws.ctypes.data, None)
        assert rc == 0, L.bpp_last_error()
        return m
    return run


def device_runner(dev="cuda:0"):
    """The same through bpp_amd.kfac_factor."""
    import bpp_amd

    def run(case, x, m, first, scale, rho):
        xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
        mt = torch.from_numpy(np.array(m, dtype=np.float32, copy=True)).to(dev)
        bpp_amd.kfac_factor(xt, case["layout"], mt, rho, first, scale, **case.get("conv", {}))
        return mt.cpu().numpy()
    return run


def host_factor_fn(L):
    """A factor_fn for KFACOptimizer on CPU tensors that goes through a host-pointer library."""
    import bpp_amd

    def fn(src, layout, m, stat_decay, first, scale, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0)):
        lay, g, D, R, _ = bpp_amd.kfac.factor_geometry(src, layout, kernel_size, stride, padding)
        x = src.detach().contiguous()
        ga = geom_arg(g)
        ws = torch.empty(L.bpp_kfac_factor_workspace(lay, ga) // 4 + 2, dtype=torch.float32)
        rc = L.bpp_kfac_factor(x.data_ptr(), lay, ga, m.data_ptr(), float(scale), float(stat_decay), int(bool(first)), ws.data_ptr(), None)
        assert rc == 0, L.bpp_last_error()
        return m
    return fn


# ---- exact cases: small integers, powers of two -----------------------------------------------------------------------------
def _ints(shape, seed):
    return np.random.RandomState(seed).randint(-4, 5, size=shape).astype(np.float32)       # |x| <= 4, asymmetric


EXACT = {
    "patch_d36": dict(layout=PATCH, conv=conv_of(3, 1, 1), x=_ints((8, 4, 4, 4), 1), kind="conv_a", running=True),
    "patch_stride2": dict(layout=PATCH, conv=conv_of(3, 2, 0), x=_ints((2, 3, 7, 6), 2), kind=None, running=False),
    "nchw_d8": dict(layout=NCHW, x=_ints((8, 8, 4, 4), 3), kind="conv_g", running=True),
    "rows_d33": dict(layout=ROWS, x=_ints((64, 33), 4), kind="linear_a", running=True),
    "rows_d1": dict(layout=ROWS, x=_ints((4, 1), 5), kind="linear_g", running=True),
}


def _wide(layout, shape, seed, conv=None):
    c = dict(layout=layout, x=_ints(shape, seed), kind=None, running=True)
    if conv:
        c["conv"] = conv
    return c


# the geometries the header accepts beyond the shipped layers
EXACT.update({
    "patch_c10_d90": _wide(PATCH, (3, 10, 4, 5), 1, conv_of(3, 1, 1)),                # a block that straddles channels, D no multiple of 64
    "patch_c15_d135": _wide(PATCH, (2, 15, 3, 3), 2, conv_of(3, 1, 1)),               # three blocks
    "patch_k2x3_s2x1_p0x2": _wide(PATCH, (3, 5, 5, 4), 3, conv_of((2, 3), (2, 1), (0, 2))),
    "patch_k3x2_s1x3_p2x0": _wide(PATCH, (2, 12, 3, 7), 4, conv_of((3, 2), (1, 3), (2, 0))),
    "patch_1x1_c130": _wide(PATCH, (2, 130, 3, 3), 5, conv_of(1, 1, 0)),
    "patch_one_position": _wide(PATCH, (5, 8, 3, 3), 6, conv_of(3, 1, 0)),
    "patch_k5_c3": _wide(PATCH, (2, 3, 6, 5), 7, conv_of(5, 1, 2)),
    "nchw_d70_s65": _wide(NCHW, (2, 70, 5, 13), 8),                                   # two feature blocks; chunks of 33 and 32 positions
    "nchw_d130_s25": _wide(NCHW, (3, 130, 5, 5), 9),
    "nchw_d33_s1": _wide(NCHW, (7, 33, 1, 1), 10),                                    # one position per sample
    "nchw_d8_s129": _wide(NCHW, (2, 8, 3, 43), 11),                                   # three chunks of 43
    "rows_r129_d65": _wide(ROWS, (129, 65), 12),
    "rows_r1_d200": _wide(ROWS, (1, 200), 13),
    "rows_r65_d32": _wide(ROWS, (65, 32), 14),
    "rows_r3_d31": _wide(ROWS, (3, 31), 15),
})


def check_exact(run, case):
    """Every product, sum and scaling is exact in float32, so the result equals an int64 evaluation bit for bit whatever the
    order.  running: also a second accumulation with rho = 0.5 onto the first result (c1 = 1, c2 = 0.5: exact)."""
    X = rows64(case).astype(np.int64)
    raw = (X.T @ X).astype(np.float64)
    D = raw.shape[0]
    assert np.abs(raw).max() < 2 ** 24 and (D == 1 or not np.array_equal(raw, raw[::-1, ::-1]))     # no symmetry beyond X^T X's own
    scale = reference_scale(case, case["kind"]) if case["kind"] else 1.0
    want = (raw * scale).astype(np.float32)
    assert np.array_equal(want.astype(np.float64), raw * scale)
    canary = np.full((D, D), 7.0, np.float32)
    got = run(case, case["x"], canary, True, scale, 0.5)
    assert np.array_equal(bits(got), bits(want))
    if case["running"]:
        x2 = np.ascontiguousarray(case["x"][::-1] * np.float32(2.0))
        X2 = rows64(case, x2).astype(np.int64)
        aa2 = (X2.T @ X2).astype(np.float64) * scale
        want2 = ((want.astype(np.float64) + aa2) * 0.5).astype(np.float32)
        assert np.array_equal(want2.astype(np.float64), (want.astype(np.float64) + aa2) * 0.5)
        got2 = run(case, x2, got, False, scale, 0.5)
        assert np.array_equal(bits(got2), bits(want2))


# ---- real-valued cases ------------------------------------------------------------------------------------------------------
def _real(shape, seed):
    r = np.random.RandomState(seed)
    return (r.standard_normal(shape) * r.uniform(0.5, 2.0)).astype(np.float32), (r.standard_normal(shape) + 0.25).astype(np.float32)


def real_case(layout, shape, seed, kind, conv=None):
    x, x2 = _real(shape, seed)
    c = dict(layout=layout, x=x, x2=x2, kind=kind, rho=0.99)
    if conv:
        c["conv"] = conv
    c["scale"] = reference_scale(c, kind)
    return c


REAL = {
    "patch_d576": lambda: real_case(PATCH, (3, 64, 10, 10), 11, "conv_a", conv_of(3, 1, 1)),
    "patch_d36": lambda: real_case(PATCH, (3, 4, 10, 10), 12, "conv_a", conv_of(3, 1, 1)),
    "patch_d64_k1": lambda: real_case(PATCH, (5, 64, 10, 10), 13, "conv_a", conv_of(1, 1, 0)),
    "nchw_d64": lambda: real_case(NCHW, (3, 64, 10, 10), 14, "conv_g"),
    "nchw_d8": lambda: real_case(NCHW, (3, 8, 10, 10), 15, "conv_g"),
    "nchw_d4": lambda: real_case(NCHW, (3, 4, 10, 10), 16, "conv_g"),
    "rows_d800": lambda: real_case(ROWS, (15, 800), 17, "linear_a"),
    "rows_d400": lambda: real_case(ROWS, (15, 400), 18, "linear_a"),
    "rows_d256": lambda: real_case(ROWS, (15, 256), 19, "linear_g"),
    "rows_d100": lambda: real_case(ROWS, (15, 100), 20, "linear_g"),
    "patch_c10_d90": lambda: real_case(PATCH, (3, 10, 10, 10), 22, "conv_a", conv_of(3, 1, 1)),
    "patch_k3x2_s1x3_p2x0": lambda: real_case(PATCH, (3, 12, 7, 9), 23, "conv_a", conv_of((3, 2), (1, 3), (2, 0))),
    "nchw_d130": lambda: real_case(NCHW, (3, 130, 5, 5), 24, "conv_g"),
    "nchw_d70_s65": lambda: real_case(NCHW, (2, 70, 5, 13), 25, "conv_g"),
    "rows_r129_d65": lambda: real_case(ROWS, (129, 65), 26, "linear_a"),
}

# ---- the recorded bits of the emulator's fmaf chains on real-valued data (tests/golden/make_mfma_chain_bits.py) ----------------
# name -> the arguments of real_case: x and x2 come from numpy.random.RandomState alone, so every machine regenerates them
CHAIN_CASES = {
    "kfac_patch_c10": (PATCH, (3, 10, 10, 10), 31, "conv_a", conv_of(3, 1, 1)),
    "kfac_patch_c15": (PATCH, (3, 15, 10, 10), 32, "conv_a", conv_of(3, 1, 1)),
    "kfac_nchw_d64": (NCHW, (3, 64, 10, 10), 33, "conv_g"),
    "kfac_rows_r15_d100": (ROWS, (15, 100), 34, "linear_g"),
    "kfac_rows_r129_d65": (ROWS, (129, 65), 35, "linear_a"),
}


def crc(a):
    import zlib
    return np.uint32(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def chain_entries(run, name):
    """{key: array} of one case for the fixture: the CRC32 of the bytes of both batches, the bits of m after the first batch
    and after the second (rho = 0.99, the scale of reference_scale); and the case itself."""
    case = real_case(*CHAIN_CASES[name])
    D = rows64(case).shape[1]
    m1 = run(case, case["x"], np.full((D, D), np.nan, np.float32), True, case["scale"], case["rho"])
    m2 = run(case, case["x2"], m1, False, case["scale"], case["rho"])
    return {name + ".crc.x": crc(case["x"]), name + ".crc.x2": crc(case["x2"]), name + ".m1": bits(m1), name + ".m2": bits(m2)}, case


def ulps(a, b):
    """The largest distance of two float32 arrays, given as bits, in units of the last place."""
    def ordered(x):
        i = np.ascontiguousarray(x).view(np.uint32).astype(np.int64)
        return np.where(i & 0x80000000, 0x80000000 - i, i)
    return int(np.abs(ordered(a) - ordered(b)).max())


def split_case(rows_per_split, D=40):
    """R = 2 rows_per_split + 1: two full splits and a third of one row."""
    return real_case(ROWS, (2 * rows_per_split + 1, D), 21, "linear_a")


def check_real(run, case, chain):
    """First path and a second accumulation onto the non-zero result against float64 within `bound`; symmetry and a second
    run bit for bit.  Returns (m after the first batch, m after the second)."""
    D = rows64(case).shape[1]
    rho, scale = case["rho"], case["scale"]
    canary = np.full((D, D), np.nan, np.float32)        # `first` must not read m
    m1 = run(case, case["x"], canary, True, scale, rho)
    want1, mag1 = expected64(case, case["x"], None, True, scale, rho)
    err1, lim1 = np.abs(m1.astype(np.float64) - want1), bound(chain, mag1, None, True, rho)
    print("first: worst err / bound = %.3f" % float((err1 / np.maximum(lim1, 1e-300)).max()))
    assert np.all(err1 <= lim1)
    assert np.array_equal(bits(m1), bits(m1.T))
    assert np.array_equal(bits(run(case, case["x"], canary, True, scale, rho)), bits(m1))
    m2 = run(case, case["x2"], m1, False, scale, rho)
    want2, mag2 = expected64(case, case["x2"], m1, False, scale, rho)
    err2, lim2 = np.abs(m2.astype(np.float64) - want2), bound(chain, mag2, m1, False, rho)
    print("second: worst err / bound = %.3f" % float((err2 / np.maximum(lim2, 1e-300)).max()))
    assert np.all(err2 <= lim2)
    assert np.array_equal(bits(m2), bits(m2.T))
    assert np.array_equal(bits(run(case, case["x2"], m1, False, scale, rho)), bits(m2))
    return m1, m2


# ---- the small net of the optimizer tests ---------------------------------------------------------------------------------
NET_BATCH, NET_STEPS, NET_TF = 64, 4, 2


class SmallNet(nn.Module):
    """conv 3x3 p=1 4->8 on 5x5, conv 1x1 8->2, Linear 50->16, Linear 16->7, ReLUs between."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(4, 8, 3, padding=1)
        self.conv2 = nn.Conv2d(8, 2, 1)
        self.fc1 = nn.Linear(50, 16)
        self.fc2 = nn.Linear(16, 7)

    def forward(self, x):
        x = torch.relu(self.conv1(x))
        x = torch.relu(self.conv2(x))
        x = torch.relu(self.fc1(x.flatten(1)))
        return self.fc2(x)


def net_losses(out, target, noise):
    """(fisher loss, loss) of one batch: out [B, 7] = 6 logits and a value.  The Fisher pass has the shape of
    acktr_pipeline.py:68-84 (a sampled log-likelihood plus a value term against noised values), the loss is cross-entropy
    plus a value regression."""
    logits, value = out[:, :6], out[:, 6]
    logp = torch.log_softmax(logits, dim=1).gather(1, target["action"].view(-1, 1))
    fisher = -logp.mean() - (value - (value + noise).detach()).pow(2).mean()
    loss = -(target["adv"] * logp.view(-1)).mean() + 0.5 * (target["ret"] - value).pow(2).mean()
    return fisher, loss


def run_optimizer(make_optimizer, weights, batches, device="cpu", record_factors=False):
    """Four steps of K-FAC on SmallNet from `weights` over `batches`; returns (parameters after each step as {plain name:
    numpy}, factors after step 0 or None)."""
    import bpp_amd
    net = SmallNet()
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in weights.items()})
    net = net.to(device)
    opt = make_optimizer(net)
    trail, factors = [], None
    for b in batches:
        x = torch.from_numpy(b["x"]).to(device)
        target = {k: torch.from_numpy(b[k]).to(device) for k in ("action", "adv", "ret")}
        out = net(x)
        fisher, loss = net_losses(out, target, torch.from_numpy(b["noise"]).to(device))
        if opt.steps % opt.Ts == 0:
            net.zero_grad()
            opt.acc_stats = True
            fisher.backward(retain_graph=True)
            opt.acc_stats = False
        opt.zero_grad()
        loss.backward()
        opt.step()
        if record_factors and factors is None:
            factors = {}
            for i, m in enumerate(opt.modules):
                factors["aa_%d" % i] = opt.m_aa[m].detach().cpu().numpy().copy()
                factors["gg_%d" % i] = opt.m_gg[m].detach().cpu().numpy().copy()
        trail.append({k: v.detach().cpu().numpy().copy() for k, v in bpp_amd.kfac.plain_state_dict(net.state_dict()).items()})
    return trail, factors


def make_batches(seed):
    r = np.random.RandomState(seed)
    return [dict(x=r.standard_normal((NET_BATCH, 4, 5, 5)).astype(np.float32), action=r.randint(0, 6, NET_BATCH).astype(np.int64),
                 adv=r.standard_normal(NET_BATCH).astype(np.float32), ret=r.standard_normal(NET_BATCH).astype(np.float32),
                 noise=r.standard_normal(NET_BATCH).astype(np.float32)) for _ in range(NET_STEPS)]


def update_distance(trail, ref_trail, start):
    """Relative L2 distance of each step's parameter UPDATE (all parameters as one vector) between two runs."""
    out = []
    prev_a = prev_b = start
    for a, b in zip(trail, ref_trail):
        da = np.concatenate([(a[k].astype(np.float64) - prev_a[k]).ravel() for k in sorted(a)])
        db = np.concatenate([(b[k].astype(np.float64) - prev_b[k]).ravel() for k in sorted(b)])
        out.append(float(np.linalg.norm(da - db) / np.linalg.norm(db)))
        prev_a, prev_b = a, b
    return out


def reference_runs(weights, batches):
    """With the live reference importable: (its trail, its trail with the factors computed in float64 and cast back -- the
    reference against itself --, its factors after step 0)."""
    from acktr.algo import kfac as ref
    trail, factors = run_optimizer(lambda net: ref.KFACOptimizer(net, Tf=NET_TF), weights, batches, record_factors=True)
    cov_a, cov_g = ref.compute_cov_a, ref.compute_cov_g
    ref.compute_cov_a = lambda a, *rest: cov_a(a.double(), *rest).float()
    ref.compute_cov_g = lambda g, *rest: cov_g(g.double(), *rest).float()
    try:
        trail64, _ = run_optimizer(lambda net: ref.KFACOptimizer(net, Tf=NET_TF), weights, batches)
    finally:
        ref.compute_cov_a, ref.compute_cov_g = cov_a, cov_g
    return trail, trail64, factors
