"""The policy-head kernels (csrc/bpp_heads.inl: bpp_masked_act in both its forms, bpp_masked_evaluate / _backward,
bpp_sample_feasible) against a float64 statement of the reference formula (acktr/distributions.py:71-101):
    lx = softmax(x - 14 (1 - m)) + 1e-5,  p = lx / sum(lx),  log-prob = log(clamp(p_a, eps, 1 - eps))   eps = float32 eps
entropy and invalid mass as in tests/test_masked_evaluate.py, gradients by float64 autograd of the same formula.

Inputs go where float32 kernels go wrong: large and offset logits, exact and near ties, rows with nothing / everything /
one dominant cell feasible, M = 1, every PER branch of the 16-lane kernel and the rows only the wave-per-bin kernel
takes, batch sizes that end inside a 16-bin block, global bin ids past 2^32.  The 16-lane kernel runs on 16-byte
aligned rows; the same rows 4 bytes off that boundary force the wave-per-bin kernel, so both see the same data.

Two tiers: the product kernels compiled for the host SIMT emulator (exact libm in place of v_exp_f32 / v_rcp_f32 /
v_log_f32, so it checks the kernel's arithmetic), and the same checks on the MI355X (`-m gpu`, the hardware
approximations included), plus sampling frequencies there."""
import numpy as np
import pytest
import torch

from test_masked_act import make_case, uniform_of
from test_masked_evaluate import GRAD_TOL, forward_tolerances

EPS = float(np.finfo(np.float32).eps)          # torch clamp_probs for float32 probabilities
LP_TOL = 5e-6                                  # log-probability budget against float64
CDF_TOL = 1e-5                                 # a draw sits where the float64 CDF crosses u * total, within this
TIE_TOL = 1e-6                                 # top-2 probability gap above which the deterministic action is determined

M_LANES = [4, 8, 60, 64, 68, 100, 128, 132, 200, 256, 260, 400, 508, 512]   # PER 1/2/3/4/6/8 and the edges between them
M_WAVE = [1, 7, 37, 513, 800, 1023]                                         # M % 4 != 0 or M > 512: wave per bin only
M_ALL = sorted(M_LANES + M_WAVE)
SHIFTS = [50, -50, 200, -200, 1000, -1000]
FAMILIES = ["mild", "shifted", "wide30", "wide100", "tie_all", "tie_half", "near_tie", "none_feasible", "all_feasible",
            "one_feasible_80"]
BASES = [0, 12345, 2 ** 32 - 5]                # the last one wraps the 32-bit hash key inside every batch of > 5 bins


# ---------------------------------------------------------------------------------------------------------------- inputs
def shifted_base(rng, E, M):
    """|x| < 16 on a 2^-8 grid: x + C is exact in float32 for |C| <= 1000, and so is x + C - 14."""
    return (np.round(np.clip(rng.randn(E, M) * 2.0, -15.9, 15.9) * 256.0) / 256.0).astype(np.float32)


def family(name, E, M, seed):
    """(logits, mask) float32 [E, M] of one input family."""
    rng = np.random.RandomState(seed)
    m = (rng.rand(E, M) < 0.3).astype(np.float32)
    if name == "mild":                         # tests/test_masked_act.py's case (its rows 0 / 1: nothing / all feasible)
        x, m = make_case(max(E, 2), M, seed)
        return x[:E], m[:E]
    if name == "shifted":
        x = shifted_base(rng, E, M)
    elif name.startswith("wide"):
        x = (rng.randn(E, M) * float(name[4:])).astype(np.float32)
    elif name == "tie_all":                    # every logit of a row equal; some rows all feasible
        x = np.repeat(np.round(rng.randn(E, 1) * 64.0) / 16.0, M, 1).astype(np.float32)
        m[::3] = 1.0
    elif name == "tie_half":                   # the upper half of a row shares its maximum; odd rows tie in x - 14 (1 - m)
        x = (rng.randn(E, M) - 6.0).astype(np.float32)
        c = np.round(rng.randn(E, 1) * 16.0) / 4.0
        top = np.repeat(c, M - M // 2, 1)
        top[1::2] += 14.0 * (1.0 - m[1::2, M // 2:])
        x[:, M // 2:] = top
    elif name == "near_tie":                   # the two largest feasible logits 1..4 ulp apart (probabilities < 1e-6 apart)
        x = (rng.randn(E, M) * 2.0).astype(np.float32)
        if M > 1:
            for e in range(E):
                i, j = rng.choice(M, 2, replace=False)
                m[e, i] = m[e, j] = 1.0
                x[e, i] = np.float32(9.0 + rng.rand())
                x[e, j] = x[e, i]
                for _ in range(rng.randint(1, 5)):
                    x[e, j] = np.nextafter(x[e, j], np.float32(0.0))
    elif name == "none_feasible":
        x, m = (rng.randn(E, M) * 2.0).astype(np.float32), np.zeros((E, M), np.float32)
    elif name == "all_feasible":
        x, m = (rng.randn(E, M) * 2.0).astype(np.float32), np.ones((E, M), np.float32)
    elif name == "one_feasible_80":
        x, m = (rng.randn(E, M) * 2.0).astype(np.float32), np.zeros((E, M), np.float32)
        j = rng.randint(0, M, E)
        m[np.arange(E), j] = 1.0
        x[np.arange(E), j] = 80.0
    else:
        raise ValueError(name)
    return x, m


def cases(E, M, seed):
    """(label, logits, mask) of every family; the shifted family once per shift C and once unshifted."""
    for k, name in enumerate(FAMILIES):
        x, m = family(name, E, M, seed * 31 + k)
        yield name, x, m
        if name == "shifted":
            for c in SHIFTS:
                yield "shifted%+d" % c, x + np.float32(c), m


# ------------------------------------------------------------------------------------------------- float64 reference
def f64_probs(x, m):
    xd, md = torch.from_numpy(x).double(), torch.from_numpy(m).double()
    lx = torch.softmax(xd - (1.0 - md) * 14.0, dim=-1) + 1e-5
    return (lx / lx.sum(-1, keepdim=True)).numpy()


def f64_log_prob(p, a):
    return np.log(np.clip(p[np.arange(p.shape[0]), a], EPS, 1.0 - EPS))


def f64_evaluate(x, m, a, w):
    """(log-prob, entropy, bad, d(sum w0 logp + w1 ent + w2 bad)/dx) in float64."""
    xd = torch.from_numpy(x).double().requires_grad_(True)
    md = torch.from_numpy(m).double()
    lx = torch.softmax(xd - (1.0 - md) * 14.0, dim=-1) + 1e-5
    p = lx / lx.sum(-1, keepdim=True)
    logc = torch.log(torch.clamp(p, EPS, 1.0 - EPS))
    logp = logc.gather(-1, torch.from_numpy(a).reshape(-1, 1))[:, 0]
    ent = -(p * logc).sum(-1)
    bad = (torch.softmax(xd, dim=-1) * (1.0 - md)).sum(-1)
    wd = [torch.from_numpy(np.asarray(v, np.float64)) for v in w]
    (wd[0] * logp + wd[1] * ent + wd[2] * bad).sum().backward()
    return logp.detach().numpy(), ent.detach().numpy(), bad.detach().numpy(), xd.grad.numpy()


def near_cdf_step(p, u):
    """Rows whose float64 CDF passes within CDF_TOL of u (u * total of the normalised row): a draw may go either way."""
    return (np.abs(np.cumsum(p, 1) - u[:, None]) <= CDF_TOL).any(1)


def uniforms(E, seed, step, base):
    return np.array([uniform_of(seed, base + e, step) for e in range(E)])


# ---------------------------------------------------------------------------------------------------------- the tiers
def placed(a, aligned):
    """A copy of `a` whose data starts on a 16-byte boundary (aligned) or 4 bytes past one."""
    flat = np.ascontiguousarray(a).reshape(-1)
    buf = np.empty(flat.size + 8, flat.dtype)
    off = (-buf.ctypes.data % 16) // flat.itemsize + (0 if aligned else 1)
    out = buf[off:off + flat.size]
    out[:] = flat
    assert (out.ctypes.data % 16 == 0) == aligned
    return out.reshape(a.shape)


class EmuHead:
    """The product kernels on the host SIMT emulator, through the oracle's numpy front-end."""
    rows = 21                                  # bins per family: one full 16-bin block and part of the next

    def __init__(self, emu):
        self.mod = emu

    def act(self, x, m, seed, step, det, base=0, counter=False, aligned=True):
        return self.mod.masked_act(placed(x, aligned), placed(m, aligned), seed, step, det, env_id_base=base, counter=counter)

    def evaluate(self, x, m, a):
        return self.mod.masked_evaluate(x, m, a)

    def backward(self, x, m, a, w):
        return self.mod.masked_evaluate_backward(x, m, a, *w)

    def sample_feasible(self, m, seed, step, base=0, aligned=True):
        return self.mod.sample_feasible(placed(m, aligned), seed, step, env_id_base=base)


class GpuHead:
    """The MI355X through the package's own entry points."""
    rows = 259

    @staticmethod
    def dev(a, aligned=True):
        """Device copy; unaligned = a contiguous view 4 bytes into its storage, which the wrappers pass on unchanged."""
        t = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
        buf = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
        v = buf[(0 if aligned else 1):][:t.numel()].view(a.shape)
        v.copy_(t.view(a.shape))
        assert (v.data_ptr() % 16 == 0) == aligned and v.is_contiguous()
        return v

    def act(self, x, m, seed, step, det, base=0, counter=False, aligned=True):
        import bpp_amd
        xt, mt = self.dev(x, aligned), self.dev(m, aligned)
        if counter:
            ct = torch.tensor([seed, step], dtype=torch.int64, device="cuda")
            a, lp = bpp_amd.masked_act(xt, mt, deterministic=det, env_id_base=base, counter=ct)
        else:
            a, lp = bpp_amd.masked_act(xt, mt, seed, step, det, env_id_base=base)
        return a.cpu().numpy()[:, 0], lp.cpu().numpy()[:, 0]

    def evaluate(self, x, m, a):
        from bpp_amd.masks import _MaskedEvaluate
        out = _MaskedEvaluate.apply(self.dev(x), self.dev(m), self.dev(a))
        return tuple(t.cpu().numpy() for t in out)

    def backward(self, x, m, a, w):
        from bpp_amd.masks import _MaskedEvaluate
        xt = self.dev(x).requires_grad_(True)
        lp, h, b = _MaskedEvaluate.apply(xt, self.dev(m), self.dev(a))
        (self.dev(w[0]) * lp + self.dev(w[1]) * h + self.dev(w[2]) * b).sum().backward()
        return xt.grad.cpu().numpy()

    def sample_feasible(self, m, seed, step, base=0, aligned=True):
        import ctypes
        import bpp_amd
        mt = self.dev(m, aligned)
        a = torch.empty(m.shape[0], dtype=torch.int64, device="cuda")
        bpp_amd._lib.check(bpp_amd._lib.lib().bpp_sample_feasible(mt.data_ptr(), a.data_ptr(), m.shape[0], m.shape[1], int(base),
                                                                  int(seed), int(step),
                                                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return a.cpu().numpy()


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def head(request):
    if request.param == "gpu":
        assert torch.cuda.is_available()
        return GpuHead()
    return EmuHead(request.getfixturevalue("emu"))


def placements(M):
    """(aligned?) of the calls that reach each kernel: 16-lane + wave where the 16-lane kernel takes M, else wave only."""
    return (True, False) if M % 4 == 0 and M <= 512 else (False,)


# ------------------------------------------------------------------------------------------------------ the checks
def check_act(head, x, m, what, seed=5, step=9, base=0, counter=False, aligned=True):
    """One row batch through one masked_act entry point / kernel, both modes, against float64.  Returns the draws."""
    E = x.shape[0]
    p = f64_probs(x, m)
    where = "%s aligned=%d counter=%d base=%d" % (what, aligned, counter, base)
    # deterministic: the first index of the float64 maximum wherever it is determined (a clear gap, or an exact tie)
    a, lp = head.act(x, m, seed, step, True, base, counter, aligned)
    assert ((a >= 0) & (a < x.shape[1])).all(), where
    np.testing.assert_allclose(lp, f64_log_prob(p, a), rtol=0, atol=LP_TOL, err_msg="mode log-prob " + where)
    top2 = np.sort(p, 1)[:, -2:] if x.shape[1] > 1 else np.concatenate([np.zeros((E, 1)), p], 1)
    gap = top2[:, 1] - top2[:, 0]
    decided = (gap > TIE_TOL) | (gap == 0.0)
    np.testing.assert_array_equal(a[decided], p.argmax(1)[decided], err_msg="mode action " + where)
    assert (p[np.arange(E), a] >= top2[:, 1] - TIE_TOL).all(), where
    det = a
    # sampled: the float64 inverse CDF at the counter-based uniform
    a, lp = head.act(x, m, seed, step, False, base, counter, aligned)
    assert ((a >= 0) & (a < x.shape[1])).all(), where
    np.testing.assert_allclose(lp, f64_log_prob(p, a), rtol=0, atol=LP_TOL, err_msg="sampled log-prob " + where)
    u = uniforms(E, seed, step, base)
    cdf = np.cumsum(p, 1)
    hi = cdf[np.arange(E), a]
    lo = np.where(a > 0, cdf[np.arange(E), np.maximum(a - 1, 0)], 0.0)
    bad = ~((lo - CDF_TOL <= u) & (u <= hi + CDF_TOL))
    assert not bad.any(), (where, np.nonzero(bad)[0][:5], a[bad][:5], u[bad][:5])
    return det, a


@pytest.mark.parametrize("M", M_ALL)
def test_policy_head_masked_act_against_float64(head, M):
    """Every family, both kernels where both take M, the by-value and the counter entry point."""
    for name, x, m in cases(head.rows, M, M):
        for aligned in placements(M):
            for counter in (False, True):
                check_act(head, x, m, "%s M=%d" % (name, M), counter=counter, aligned=aligned)


@pytest.mark.parametrize("M", M_ALL)
def test_policy_head_masked_act_is_shift_invariant(head, M):
    """softmax(x + C) = softmax(x): the same deterministic action, and log-probabilities that agree with each other and
    with float64, for every shift C of the exact-shift family."""
    x, m = family("shifted", head.rows, M, 7 * M + 1)
    for aligned in placements(M):
        d0, s0 = check_act(head, x, m, "shifted M=%d" % M, aligned=aligned)
        l0 = head.act(x, m, 5, 9, True, aligned=aligned)[1]
        u = uniforms(x.shape[0], 5, 9, 0)
        steady = ~near_cdf_step(f64_probs(x, m), u)
        for c in SHIFTS:
            xc = x + np.float32(c)
            what = "shifted%+d M=%d" % (c, M)
            dc, sc = check_act(head, xc, m, what, aligned=aligned)
            np.testing.assert_array_equal(dc, d0, err_msg="mode action " + what)
            np.testing.assert_allclose(head.act(xc, m, 5, 9, True, aligned=aligned)[1], l0, rtol=0, atol=LP_TOL, err_msg=what)
            np.testing.assert_array_equal(sc[steady], s0[steady], err_msg="sampled action " + what)


@pytest.mark.parametrize("M", M_LANES)
def test_policy_head_masked_act_kernels_agree(head, M):
    """The 16-lane kernel (aligned rows) and the wave-per-bin kernel (the same rows 4 bytes off) on the same data: the same
    actions except where the float64 CDF passes within 1e-5 of the target, log-probabilities within 5e-6."""
    for name, x, m in cases(head.rows, M, 3 * M):
        p = f64_probs(x, m)
        top2 = np.sort(p, 1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
        for counter in (False, True):
            for det in (True, False):
                a16, l16 = head.act(x, m, 11, 4, det, counter=counter, aligned=True)
                aw, lw = head.act(x, m, 11, 4, det, counter=counter, aligned=False)
                what = "%s M=%d det=%d counter=%d" % (name, M, det, counter)
                same = ((gap > TIE_TOL) | (gap == 0.0)) if det else ~near_cdf_step(p, uniforms(x.shape[0], 11, 4, 0))
                np.testing.assert_array_equal(a16[same], aw[same], err_msg=what)
                eq = a16 == aw
                np.testing.assert_allclose(l16[eq], lw[eq], rtol=0, atol=LP_TOL, err_msg=what)


def check_batch(head, E):
    for M in (100, 37):
        x, m = family("mild", E, M, E + M)
        for base in BASES:
            for aligned in placements(M):
                check_act(head, x, m, "E=%d M=%d" % (E, M), seed=3, step=2 ** 40 + 1, base=base, aligned=aligned)


@pytest.mark.parametrize("E", [1, 3, 15, 16, 17, 4099])
def test_policy_head_masked_act_batch_sizes_and_bin_ids(head, E):
    """Batches that end inside a 16-bin block (and inside a 4-bin workgroup of the wave kernel); env_id_base != 0, one
    that wraps the 32-bit key of the hash."""
    check_batch(head, E)


@pytest.mark.gpu
def test_gpu_policy_head_masked_act_65537_bins():
    check_batch(GpuHead(), 65537)


@pytest.mark.parametrize("M", M_ALL)
def test_policy_head_masked_evaluate_against_float64(head, M):
    """Forward and backward of the training half against float64 autograd, at the tolerances of
    tests/test_masked_evaluate.py, on every family (shifts of +-1000 included); each loss weight on its own as well."""
    tol = forward_tolerances(M)
    for name, x, m in cases(head.rows, M, 5 * M):
        if name.startswith("shifted") and abs(int(name[7:] or 0)) not in (0, 1000):
            continue
        E = x.shape[0]
        rng = np.random.RandomState(M + E)
        a = rng.randint(0, M, E).astype(np.int64)
        a[::2] = np.where(m[::2].any(1), m[::2].argmax(1), a[::2])          # half of the actions on feasible cells
        a[1::4] = f64_probs(x[1::4], m[1::4]).argmax(1)                       # and some on the mode
        w = tuple(rng.randn(E).astype(np.float32) for _ in range(3))
        lp0, h0, b0, g0 = f64_evaluate(x, m, a, w)
        what = "%s M=%d" % (name, M)
        for got, want, t, label in zip(head.evaluate(x, m, a), (lp0, h0, b0), tol, ("log-prob", "entropy", "bad")):
            np.testing.assert_allclose(got, want, rtol=0, atol=t, err_msg="%s %s" % (label, what))
        np.testing.assert_allclose(head.backward(x, m, a, w), g0, rtol=GRAD_TOL[0], atol=GRAD_TOL[1], err_msg="grad " + what)
        for i in range(3):
            wi = tuple(w[j] if j == i else np.zeros(E, np.float32) for j in range(3))
            np.testing.assert_allclose(head.backward(x, m, a, wi), f64_evaluate(x, m, a, wi)[3], rtol=GRAD_TOL[0],
                                       atol=GRAD_TOL[1], err_msg="grad of output %d alone, %s" % (i, what))


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 100, 800])
def test_gpu_policy_head_public_masked_evaluate_against_float64(M):
    """bpp_amd.masked_evaluate, the three scalars the training loop consumes, and their gradient, against float64."""
    import bpp_amd
    for name, x, m in cases(GpuHead.rows, M, 9 * M):
        E = x.shape[0]
        rng = np.random.RandomState(E + M)
        a = np.where(m.any(1), m.argmax(1), rng.randint(0, M, E)).astype(np.int64)
        adv = rng.randn(E).astype(np.float32)
        xt = GpuHead.dev(x).requires_grad_(True)
        logp, ent, prob_loss = bpp_amd.masked_evaluate(xt, GpuHead.dev(m), GpuHead.dev(a).unsqueeze(1))
        (-(GpuHead.dev(adv).unsqueeze(1) * logp).mean() - 0.01 * ent + 0.1 * prob_loss).backward()
        w = (-adv / E, np.full(E, -0.01 / E), np.full(E, 0.1 / (E * M)))
        lp0, h0, b0, g0 = f64_evaluate(x, m, a, w)
        tol = forward_tolerances(M)
        what = "%s M=%d" % (name, M)
        np.testing.assert_allclose(logp.detach().cpu().numpy()[:, 0], lp0, rtol=0, atol=tol[0], err_msg=what)
        np.testing.assert_allclose(ent.item(), h0.mean(), rtol=0, atol=tol[1], err_msg=what)
        np.testing.assert_allclose(prob_loss.item(), b0.sum() / (E * M), rtol=0, atol=tol[2] / M, err_msg=what)
        np.testing.assert_allclose(xt.grad.cpu().numpy(), g0, rtol=GRAD_TOL[0], atol=GRAD_TOL[1] / E + 1e-9, err_msg=what)


def feasible_masks(E, M, seed):
    rng = np.random.RandomState(seed)
    m = (rng.rand(E, M) < rng.choice([0.02, 0.3, 0.9], size=(E, 1))).astype(np.float32)
    m[0] = 0.0
    m[1 % E] = 1.0
    m[2 % E] = 0.0
    m[2 % E, rng.randint(M)] = 1.0                  # one feasible cell
    m[3 % E] = 0.0
    m[3 % E, M - 1] = 1.0                           # ... the last one
    return m


@pytest.mark.parametrize("M", M_ALL)
def test_policy_head_sample_feasible_matches_oracle(head, oracle, M):
    """bpp_sample_feasible, both kernels (16 lanes on aligned rows with M % 4 == 0, M <= 512; one wave per bin otherwise)
    == the oracle bit for bit, at every bin id base."""
    for E in (head.rows, 4099):
        m = feasible_masks(E, M, E + M)
        for base in BASES:
            for step in (0, 2 ** 33 + 7):
                want = oracle.sample_feasible(m, 13, step, env_id_base=base)
                assert (m[np.arange(E), want] == 1.0)[m.any(1)].all()
                for aligned in placements(M):
                    np.testing.assert_array_equal(head.sample_feasible(m, 13, step, base, aligned), want,
                                                  err_msg="M=%d E=%d base=%d aligned=%d" % (M, E, base, aligned))


# ------------------------------------------------------------------------------------------ sampling frequencies (GPU)
N_FREQ = 65536


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["lanes16", "wave"])
def test_gpu_policy_head_masked_act_sampling_frequencies(aligned):
    """One row replicated over 65 536 bins (every bin its own uniform, the hash is keyed by the bin id): each bucket's
    frequency is within the oracle test's bound of the float64 probability -- for a mild row and for the same row + 1000."""
    rng = np.random.RandomState(21)
    M = 100
    x = shifted_base(rng, 1, M) * np.float32(0.75)
    m = (rng.rand(1, M) < 0.4).astype(np.float32)
    for c in (0, 1000):
        xr = np.repeat(x + np.float32(c), N_FREQ, 0)
        mr = np.repeat(m, N_FREQ, 0)
        p = f64_probs(x + np.float32(c), m)[0]
        a, _ = GpuHead().act(xr, mr, 11, 3, False, aligned=aligned)
        freq = np.bincount(a, minlength=M) / N_FREQ
        assert np.abs(freq - p).max() < 4 * np.sqrt(p.max() / N_FREQ) + 1e-3, (c, np.abs(freq - p).max())


@pytest.mark.gpu
@pytest.mark.parametrize("M,aligned", [(100, True), (100, False), (37, False)], ids=["lanes16-100", "wave-100", "wave-37"])
def test_gpu_policy_head_sample_feasible_frequencies(M, aligned):
    """Uniform over the feasible cells of one replicated row, nothing ever drawn from an infeasible one."""
    rng = np.random.RandomState(M)
    m = (rng.rand(1, M) < 0.4).astype(np.float32)
    a = GpuHead().sample_feasible(np.repeat(m, N_FREQ, 0), 17, 5, base=2 ** 32 - N_FREQ // 2, aligned=aligned)
    freq = np.bincount(a, minlength=M) / N_FREQ
    feas = m[0] == 1.0
    q = 1.0 / feas.sum()
    assert (freq[~feas] == 0).all()
    assert np.abs(freq[feas] - q).max() < 4 * np.sqrt(q / N_FREQ) + 1e-3
