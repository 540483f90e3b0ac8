"""Shared by tests/test_ppo.py (emulated kernels, host logic) and tests/test_gpu_ppo.py (device): inputs of the three entry points
of include/bpp_ppo.h, their normative float32 expressions in numpy (in the header's order), the reference's expressions
(acktr/algo/ppo.py:60-80 on the masked head of acktr/distributions.py:71-101) in float64 torch, and the checks both suites run on
whatever produced the outputs."""
import ctypes

import numpy as np
import torch

from a2c_cases import CANARY, EPS, F32, bits, ulp_apart  # noqa: F401
from test_masked_evaluate import GRAD_TOL, forward_tolerances

GUARD = 16                                     # canary floats on either side of every output
COEFS = (0.5, 0.01, 0.0, 0.0)                  # value_loss_coef, entropy_coef, invalid_coef, mask_coef: bpp_amd.PPO's defaults
ALL_COEFS = (0.5, 0.01, 2.0, 5.0)
# |kernel ratio - exp64(float32(logp - old))| / exp64: the largest value over every case of both suites is 5.84e-8 with the emulator
# (glibc expf; M = 257, one of the sizes of PPO_MS) and 7.16e-8 on the device, where the cases of PPO_MS reach 7.01e-8 (DESIGN.md
# 3.16); the bound is twice the larger
RATIO_RTOL = 2 * 7.16e-8
MAX_EXCLUDED = 0.03


def guarded(shape, dtype=np.float32):
    """(whole buffer, the view an entry point writes): GUARD canaries on either side, the view canary-filled too."""
    n = int(np.prod(shape))
    whole = np.full(n + 2 * GUARD, CANARY, dtype)
    return whole, whole[GUARD:GUARD + n].reshape(shape)


def guards_intact(whole):
    return bool(np.all(whole[:GUARD] == CANARY) and np.all(whole[-GUARD:] == CANARY))


# ---------------------------------------------------------------------------------------------------------------- loss: inputs
def logp64(x, m, a):
    x, m = torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(m, np.float64))
    return head64(x, m, torch.from_numpy(a))[0].numpy()


def make_case(B, M, E, seed, spread=0.3):
    """A rollout of E rows (masks with 1 .. M feasible entries, row 0 all infeasible and row 1 all feasible; actions on feasible
    and infeasible cells; old values, returns, advantages; old log-probabilities of "old" logits at scale 3) and a mini-batch of B
    rows of it: idx is a permutation with duplicates that holds rows 0 and E - 1, the new logits are the old ones moved by
    `spread` * N(0, 1), the new values the old ones moved by 0.3 * N(0, 1) (clip 0.2: both sides of the value clip)."""
    rng = np.random.RandomState(seed)
    xo = (rng.randn(E, M) * 3.0).astype(np.float32)
    m = np.zeros((E, M), np.float32)
    for e in range(E):
        m[e, rng.permutation(M)[:rng.randint(1, M + 1)]] = 1.0
    if E >= 3:
        m[0], m[1] = 0.0, 1.0
    a = np.zeros(E, np.int64)
    for e in range(E):
        cells = np.nonzero(m[e] == (1.0 if e % 4 else 0.0))[0]
        a[e] = rng.choice(cells) if cells.size else rng.randint(M)
    vp = (rng.randn(E) * 2.0).astype(np.float32)
    ret = (vp + rng.randn(E)).astype(np.float32)
    adv = rng.randn(E).astype(np.float32)
    old = logp64(xo, m, a).astype(np.float32)
    idx = rng.randint(0, E, size=B).astype(np.int64)
    idx[0] = E - 1
    if B > 1:
        idx[-1] = 0
    if B > 3:
        idx[2] = idx[1]
    x = (xo[idx] + spread * rng.randn(B, M)).astype(np.float32)
    val = (vp[idx] + 0.3 * rng.randn(B)).astype(np.float32)
    pm = rng.rand(B, M).astype(np.float32)
    return dict(x=x, val=val, pm=pm, idx=idx, m=m, a=a, vp=vp, ret=ret, old=old, adv=adv, B=B, E=E, M=M)


def gathered(c):
    """The dense case: every rollout-side array gathered at idx, idx itself the identity."""
    g = dict(c)
    for k in ("m", "a", "vp", "ret", "old", "adv"):
        g[k] = np.ascontiguousarray(c[k][c["idx"]])
    g["idx"], g["E"] = np.arange(c["B"], dtype=np.int64), c["B"]
    return g


def weights(B, M, coefs):
    """The weights of include/bpp_ppo.h: formed in double, cast once."""
    vc, ec, ic, mc = coefs
    return dict(cB=F32(1.0 / B), c_v=F32(vc / B), g_ent=F32(-ec / B), g_bad=F32(ic / (float(B) * M)), c_p=F32(2.0 * mc / (float(B) * M)))


def bind(L):
    from bpp_amd import _lib
    return _lib.bind_ppo(L)


def run_host(L, c, clip=0.2, coefs=COEFS, clipped_value=True, pred=True, rows=True, idx="given"):
    """bpp_ppo_loss of library L on host pointers (the emulated kernels), every output canary-filled between guards.
    idx: "given" = c["idx"], "null" = NULL."""
    B, E, M = c["B"], c["E"], c["M"]
    whole, out = {}, {}
    for k, shape in (("grad_logits", (B, M)), ("grad_values", (B,)), ("grad_pred_mask", (B, M)), ("rows", (B, 7)), ("terms", (7,))):
        whole[k], out[k] = guarded(shape)
    ws = np.zeros(int(L.bpp_ppo_loss_workspace(B, M)) // 8 + 1, np.float64)
    p = lambda v: v.ctypes.data                                                          # noqa: E731
    out["rc"] = L.bpp_ppo_loss(p(c["x"]), p(c["val"]), p(c["pm"]) if pred else None, p(c["idx"]) if idx == "given" else None, p(c["m"]),
                               p(c["a"]), p(c["vp"]), p(c["ret"]), p(c["old"]), p(c["adv"]), float(clip), *[float(v) for v in coefs],
                               int(clipped_value), p(out["grad_logits"]), p(out["grad_values"]), p(out["grad_pred_mask"]),
                               p(out["rows"]) if rows else None, p(out["terms"]), p(ws), B, E, M, None)
    out["guards"] = all(guards_intact(w) for w in whole.values())
    return out


def info(L, B, M):
    out = (ctypes.c_int32 * 4)()
    assert L.bpp_ppo_loss_info(B, M, out) == 0
    return list(out)


# ------------------------------------------------------------------------------------------- loss: the numpy float32 statement
def statement(c, ratio, clip, coefs, clipped_value):
    """include/bpp_ppo.h on the kernel's own `ratio` column: float32, unfused, in the header's order."""
    g = gathered(c)
    w = weights(c["B"], c["M"], coefs)
    A, vp, R, v = g["adv"], g["vp"], g["ret"], c["val"]
    lo, hi, cf = F32(1.0 - clip), F32(1.0 + clip), F32(clip)
    with np.errstate(invalid="ignore", over="ignore"):      # off-contract rows: inf and NaN go where the header's expressions send them
        surr1 = ratio * A
        surr2 = np.fmin(np.fmax(ratio, lo), hi) * A
        g_ratio = np.where(surr1 <= surr2, A, F32(0.0))
        d = v - R
        if clipped_value:
            t = v - vp
            e = (vp + np.fmin(np.fmax(t, -cf), cf)) - R
            d2, e2 = d * d, e * e
            ep = e * ((t >= -cf) & (t <= cf)).astype(np.float32)
            vterm = F32(0.5) * np.fmax(d2, e2)
            g_v = np.where(d2 > e2, d, np.where(d2 < e2, ep, F32(0.5) * d + F32(0.5) * ep))
        else:
            vterm, g_v = F32(0.5) * (d * d), d
        return dict(surr1=surr1, surr2=surr2, action=-np.fmin(surr1, surr2), g_ratio=g_ratio, value=vterm, grad_values=w["c_v"] * g_v,
                    g_logp=-(g_ratio * ratio) * w["cB"], clipped=((ratio < lo) | (ratio > hi)).astype(np.float32))


def check_pieces(out, c, evaluate, backward, clip=0.2, coefs=COEFS, clipped_value=True, pred=True):
    """Bit for bit: ent and bad against the evaluate kernel on the gathered rows, the clipped terms and the value gradient against
    the numpy statement on the kernel's own ratio, grad_logits against the backward kernel under the normative weights.  Returns the
    largest relative error of the ratio against float64 exp of the same float32 difference."""
    B, M = c["B"], c["M"]
    g = gathered(c)
    w = weights(B, M, coefs)
    logp, ent, bad = evaluate(c["x"], g["m"], g["a"])
    rows = out["rows"]
    assert np.array_equal(bits(rows[:, 2]), bits(ent)) and np.array_equal(bits(rows[:, 3]), bits(bad))
    ratio = rows[:, 5].copy()
    want = np.exp((logp - g["old"]).astype(np.float64))
    ratio_err = float(np.max(np.abs(ratio.astype(np.float64) - want) / want))
    print("ppo_loss B=%d M=%d: ratio max relative error against float64 exp = %.3g" % (B, M, ratio_err))
    assert ratio_err <= RATIO_RTOL, ratio_err
    s = statement(c, ratio, clip, coefs, clipped_value)
    assert np.array_equal(bits(rows[:, 1]), bits(s["action"])) and np.array_equal(bits(rows[:, 0]), bits(s["value"]))
    assert np.array_equal(bits(rows[:, 6]), bits(s["clipped"]))
    assert np.array_equal(bits(out["grad_values"]), bits(s["grad_values"]))
    grad = backward(c["x"], g["m"], g["a"], s["g_logp"], np.full(B, w["g_ent"]), np.full(B, w["g_bad"]))
    assert np.array_equal(bits(out["grad_logits"]), bits(grad))
    if pred:
        d = c["pm"] - g["m"]
        assert np.array_equal(bits(out["grad_pred_mask"]), bits(w["c_p"] * d))
        sq64 = (d * d).astype(np.float64).sum(1)
        assert np.all(np.abs(rows[:, 4].astype(np.float64) - sq64) <= (M - 1) * EPS * sq64)
    else:
        assert not rows[:, 4].any() and np.all(out["grad_pred_mask"] == CANARY)
    return ratio_err


def ordered_sum(col, R, W):
    """The double sum of a `rows` column in the order of include/bpp_update.h: R rows per workgroup, wave w adds rows w, w + 4,
    ..., the workgroup's partial is ((w0 + w1) + w2) + w3; lane t of W adds partials t, t + W, ...; a binary tree adds the lanes."""
    col = np.asarray(col, np.float64)
    partials = []
    for g0 in range(0, len(col), R):
        blk = col[g0:g0 + R]
        wv = [0.0] * 4
        for w in range(4):
            acc = np.float64(0.0)
            for v in blk[w::4]:
                acc = acc + v
            wv[w] = acc
        partials.append(((wv[0] + wv[1]) + wv[2]) + wv[3])
    lanes = np.zeros(W, np.float64)
    for t in range(min(W, len(partials))):
        acc = np.float64(0.0)
        for v in partials[t::W]:
            acc = acc + v
        lanes[t] = acc
    d = W // 2
    while d:
        lanes[:d] = lanes[:d] + lanes[d:2 * d]
        d //= 2
    return lanes[0]


def same_or_nan(got, want):
    """Bit for bit where `want` is a number (infinities included); NaN, whatever its sign and payload, where `want` is NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def check_terms(out, c, shape, coefs=COEFS, nan_ok=False):
    """The terms are the double sums of the rows' columns in the stated order, divided and cast once: bit for bit.  nan_ok (rows
    with off-contract scalars): a term that is NaN by those sums must be NaN, every other one the same bits."""
    B, M = c["B"], c["M"]
    vc, ec, ic, mc = coefs
    R, _, _, W = shape
    with np.errstate(invalid="ignore", over="ignore"):
        means = {j: ordered_sum(out["rows"][:, j], R, W) / (float(B) if j not in (3, 4) else float(B) * float(M)) for j in (0, 1, 2, 3, 4, 6)}
        want = [means[0], means[1], means[2], means[3], means[4], vc * means[0] + means[1] - ec * means[2] + ic * means[3] + mc * means[4], means[6]]
        want = np.array(want).astype(np.float32)
    if nan_ok:
        assert same_or_nan(out["terms"], want), (out["terms"], want)
    else:
        assert np.array_equal(bits(out["terms"]), bits(want)), (out["terms"], want)


# ------------------------------------------------------------------------------------------------------ loss: float64 autograd
def head64(x, m, a):
    """acktr/distributions.py:71-101: (logp, ent, bad) per row."""
    lx = torch.softmax(x - (1.0 - m) * 14.0, dim=-1) + 1e-5
    p = lx / lx.sum(-1, keepdim=True)
    logc = torch.log(torch.clamp(p, EPS, 1.0 - EPS))
    return logc.gather(-1, a.reshape(-1, 1))[:, 0], -(p * logc).sum(-1), (torch.softmax(x, dim=-1) * (1.0 - m)).sum(-1)


def loss64(x, v, pm, m, a, vp, ret, old, adv, clip, coefs, clipped_value):
    """ppo.py:60-80 on float64 torch tensors already gathered (pm may be None), plus the two optional terms."""
    vc, ec, ic, mc = coefs
    logp, ent, bad = head64(x, m, a)
    ratio = torch.exp(logp - old)
    surr1 = ratio * adv
    surr2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv
    action_rows = -torch.min(surr1, surr2)
    if clipped_value:
        value_pred_clipped = vp + (v - vp).clamp(-clip, clip)
        value_rows = 0.5 * torch.max((v - ret).pow(2), (value_pred_clipped - ret).pow(2))
    else:
        value_rows = 0.5 * (ret - v).pow(2)
    prob_loss = bad.mean() / x.shape[1]
    graph_loss = ((pm - m) ** 2).mean() if pm is not None else torch.zeros((), dtype=torch.float64)
    loss = value_rows.mean() * vc + action_rows.mean() - ent.mean() * ec + prob_loss * ic + graph_loss * mc
    return dict(terms=[value_rows.mean(), action_rows.mean(), ent.mean(), prob_loss, graph_loss, loss], logp=logp, ent=ent, bad=bad,
                ratio=ratio, value_rows=value_rows, action_rows=action_rows, surr1=surr1)


def reference64(c, clip=0.2, coefs=COEFS, clipped_value=True, pred=True):
    g = gathered(c)
    f = lambda k: torch.from_numpy(g[k]).double()                                       # noqa: E731
    x, v, pm = (f(k).requires_grad_(True) for k in ("x", "val", "pm"))
    r = loss64(x, v, pm if pred else None, f("m"), torch.from_numpy(g["a"]), f("vp"), f("ret"), f("old"), f("adv"), clip, coefs, clipped_value)
    r["terms"][5].backward()
    out = {k: (t.detach().numpy() if torch.is_tensor(t) else t) for k, t in r.items()}
    out["terms"] = np.array([float(t.detach()) for t in r["terms"]])
    out.update(grad_logits=x.grad.numpy(), grad_values=v.grad.numpy() if v.grad is not None else np.zeros(c["B"]),
               grad_pred_mask=pm.grad.numpy() if pred and pm.grad is not None else None)
    return out


def excluded_rows(c, ref, clip, clipped_value):
    """Rows float32 may put on the other side of a clip edge, decided from float64 alone.  The kernel's log-probability may differ
    from float64 by forward_tolerances(M)[0], so its ratio by that relative amount (plus expf's RATIO_RTOL and the rounding of lo /
    hi, 4 EPS together at most): a row whose float64 ratio lies within (tol + 4 EPS) * ratio of lo or hi is excluded.  v - vp is one
    float32 subtraction of exact inputs (half an ulp) against a bound rounded once: excluded within 2 EPS * max(|v - vp|, clip) of
    +-clip.  The two value branches are each a few roundings (v - R, vp + clamp, - R, the squares: under 8 EPS relative to the
    magnitudes involved): excluded when |d^2 - e^2| <= 16 EPS * (|v| + |vp| + |R| + clip)^2 -- outside the clip interval only: inside
    it the clamp is the identity, e is d up to rounding and so is the gradient whichever branch float32 takes."""
    g = gathered(c)
    tol = forward_tolerances(c["M"])[0] + 4 * EPS
    ratio = ref["ratio"]
    ex = (np.abs(ratio - (1.0 - clip)) <= tol * ratio) | (np.abs(ratio - (1.0 + clip)) <= tol * ratio)
    if clipped_value:
        v, vp, R = (np.asarray(t, np.float64) for t in (c["val"], g["vp"], g["ret"]))
        t = v - vp
        ex |= np.abs(np.abs(t) - clip) <= 2 * EPS * np.maximum(np.abs(t), clip)
        e = vp + np.clip(t, -clip, clip) - R
        ex |= (np.abs(t) > clip) & (np.abs((v - R) ** 2 - e ** 2) <= 16 * EPS * (np.abs(v) + np.abs(vp) + np.abs(R) + clip) ** 2)
    return ex


def check_against_float64(out, c, evaluate, clip=0.2, coefs=COEFS, clipped_value=True, pred=True, verbose=True):
    """Against float64 autograd of the reference's expressions; returns (reference, excluded rows)."""
    B, M = c["B"], c["M"]
    g = gathered(c)
    ref = reference64(c, clip, coefs, clipped_value, pred)
    ex = excluded_rows(c, ref, clip, clipped_value)
    assert ex.mean() <= MAX_EXCLUDED, ex.mean()                           # from float64 alone
    keep = ~ex
    tol = forward_tolerances(M)
    logp = evaluate(c["x"], g["m"], g["a"])[0]
    rows = out["rows"].astype(np.float64)
    assert np.all(np.abs(logp - ref["logp"]) <= tol[0])
    assert np.all(np.abs(rows[:, 2] - ref["ent"]) <= tol[1]) and np.all(np.abs(rows[:, 3] - ref["bad"]) <= tol[2])
    rtol_ratio = tol[0] + 4 * EPS
    assert np.all(np.abs(rows[:, 5] - ref["ratio"]) <= rtol_ratio * ref["ratio"])
    # per-row terms: the action term is (clamped) ratio * A, relative error that of the ratio plus one rounding; the value term a
    # few roundings of quantities of size |v| + |vp| + |R| + clip
    assert np.all(np.abs(rows[keep, 1] - ref["action_rows"][keep]) <= (rtol_ratio + 2 * EPS) * np.abs(ref["surr1"][keep]) + 1e-30)
    mag = (np.abs(c["val"]) + np.abs(g["vp"]) + np.abs(g["ret"]) + clip).astype(np.float64) ** 2
    assert np.all(np.abs(rows[keep, 0] - ref["value_rows"][keep]) <= 8 * EPS * mag[keep])
    # gradients.  GRAD_TOL is stated for weights of unit size and the error of the head's backward is linear in them: the atol
    # is scaled by the row's |g_logp| B = |A ratio| where that exceeds 1, and by 1 / B as in a2c_cases
    wrow = np.maximum(1.0, np.abs(g["adv"].astype(np.float64) * ref["ratio"]))[:, None]
    gdiff = np.abs(out["grad_logits"] - ref["grad_logits"])
    gbound = (GRAD_TOL[0] + rtol_ratio) * np.abs(ref["grad_logits"]) + GRAD_TOL[1] * wrow / B + 1e-9
    assert np.all(gdiff[keep] <= gbound[keep]), float((gdiff[keep] / gbound[keep]).max())
    vdiff = np.abs(out["grad_values"] - ref["grad_values"])
    assert np.all(vdiff[keep] <= 8 * EPS * np.sqrt(mag[keep]) * coefs[0] / B + 1e-30)
    if pred:
        np.testing.assert_allclose(out["grad_pred_mask"], ref["grad_pred_mask"], rtol=4 * EPS, atol=0)
    # the means: continuous across the edges, so every row counts
    t, r = out["terms"].astype(np.float64), ref["terms"]
    bounds = [8 * EPS * mag.mean(), (rtol_ratio + 2 * EPS) * np.abs(ref["surr1"]).mean() + 4 * EPS * abs(r[1]), tol[1], tol[2] / M,
              4 * EPS * abs(r[4]) + 1e-30]
    diff = np.abs(t[:5] - r[:5])
    if verbose:
        print("ppo_loss B=%d M=%d clip=%g: excluded %d rows; |term - f64| / bound = %s; grad_logits max |diff| / bound = %.3g"
              % (B, M, clip, int(ex.sum()), ["%.3g" % (d / b) for d, b in zip(diff, bounds)], float((gdiff[keep] / gbound[keep]).max())))
    for j in range(5):
        assert diff[j] <= bounds[j], (j, t[j], r[j], diff[j], bounds[j])
    return ref, ex


# ------------------------------------------------------------------------- loss: the sizes that select a form, and off-contract rows
# bpp_ppo_loss launches ppo_loss_kernel<1 | 2 | 4 | 8 | 0> for M <= 64, <= 128, <= 256, <= 512 and beyond (a2c_regs): every arm of
# that switch at both of its ends, one entry, and the largest M the library allows (32 x 32 with rotation).  The form each M selects:
#          1  1   1   1   2    2    4    4    8    8    8  memory  memory
PPO_MS = [1, 2, 63, 64, 65, 128, 129, 256, 257, 400, 512, 513, 2048]
PPO_BS = (5, 9)
ACTION_MS = (37, 100, 200, 400, 600)           # one M per form, for the actions outside [0, M)
SCALAR_SHAPES = ((9, 100), (9, 400))
OUT_KEYS = ("rows", "grad_logits", "grad_values", "grad_pred_mask")


def edge_case(B, M):
    """The case of PPO_MS.  With these seeds the float64 reference alone excludes no row (excluded_rows) at any M of PPO_MS for
    B = 5 and 9: a single excluded row of so few would break MAX_EXCLUDED, so a changed seed must keep that."""
    return make_case(B, M, E=B + 5, seed=100 * B + M)


def ok(out):
    """The host runner's return code and guards; the device runner has neither (its buffers are torch's)."""
    return out.get("rc", 0) == 0 and out.get("guards", True)


def normative_rows(c, clip=0.2, coefs=COEFS, clipped_value=True, pred=True):
    """The whole row of include/bpp_ppo.h without anything a kernel produced: logp, ent, bad and the head's gradient from
    tests/head_normative.py on the gathered rows, the ratio by libm's expf, then the header's order as `statement` has it, g_logp
    fed back into the head for grad_logits.  For the emulator only: its expf is libm's, the device's is not."""
    import head_normative as hn
    B, M = c["B"], c["M"]
    g = gathered(c)
    w = weights(B, M, coefs)
    g_ent, g_bad = np.full(B, w["g_ent"]), np.full(B, w["g_bad"])
    logp, ent, bad, _ = hn.rows(c["x"], g["m"], g["a"], np.zeros(B, np.float32), g_ent, g_bad)
    ratio = hn.expf(logp - g["old"])
    s = statement(c, ratio, clip, coefs, clipped_value)
    grad = hn.rows(c["x"], g["m"], g["a"], s["g_logp"], g_ent, g_bad)[3]
    return dict(logp=logp, value=s["value"], action=s["action"], ent=ent, bad=bad, ratio=ratio, clipped=s["clipped"],
                grad_values=s["grad_values"], grad_logits=grad, grad_pred_mask=w["c_p"] * (c["pm"] - g["m"]) if pred else None)


def check_normative(out, c, clip=0.2, coefs=COEFS, clipped_value=True, pred=True):
    """rows[:, 0:4], rows[:, 5:7], grad_values, grad_logits (and grad_pred_mask) against normative_rows, bit for bit.  (Column 4,
    sq, is a sum whose order the header leaves to bpp_a2c_loss: check_pieces bounds it.)"""
    n = normative_rows(c, clip, coefs, clipped_value, pred)
    for j, k in ((0, "value"), (1, "action"), (2, "ent"), (3, "bad"), (5, "ratio"), (6, "clipped")):
        assert np.array_equal(bits(out["rows"][:, j]), bits(n[k])), (k, out["rows"][:, j], n[k])
    for k in ("grad_values", "grad_logits") + (("grad_pred_mask",) if pred else ()):
        assert np.array_equal(bits(out[k]), bits(n[k])), k
    return n


def check_edge(out, c, shape, evaluate, backward):
    """The full chain of one case of PPO_MS under ALL_COEFS; returns the ratio's largest relative error."""
    assert ok(out) and shape[2] == int(c["M"] <= 512)
    err = check_pieces(out, c, evaluate, backward, coefs=ALL_COEFS)
    check_terms(out, c, shape, ALL_COEFS)
    check_against_float64(out, c, evaluate, coefs=ALL_COEFS)
    return err


def bad_action_cases(M):
    """(case, the same case with four actions outside [0, M), the mini-batch rows that read them).  The case is edge_case(9, M) with
    rows 3 .. 6 of the mini-batch pointed at four rollout rows no other row of it reads, each a copy of the rollout row it read
    before (so the case computes what edge_case(9, M) does); then those rows' actions become -1, M, 2^40 and the smallest int64."""
    c = edge_case(9, M)
    at = np.array([3, 4, 5, 6])
    rest = np.setdiff1d(np.arange(c["B"]), at)
    idx = c["idx"].copy()
    free = np.setdiff1d(np.arange(c["E"]), idx[rest])[:4]
    good = dict(c, idx=idx)
    for k in ("m", "a", "vp", "ret", "old", "adv"):
        good[k] = c[k].copy()
        good[k][free] = c[k][idx[at]]
    idx[at] = free
    a = good["a"].copy()
    a[free] = (-1, M, 2 ** 40, np.iinfo(np.int64).min)
    return good, dict(good, a=a), at


def check_bad_actions(M, run, shape, evaluate, backward, normative=False):
    """Actions outside [0, M) are no entry of the row (tests/head_normative.py::row): logp = logf(EPS), no entry receives the
    log-probability gradient, every other row is untouched.  run(c) -> outputs under ALL_COEFS."""
    good_c, bad_c, at = bad_action_cases(M)
    B = bad_c["B"]
    rest = np.setdiff1d(np.arange(B), at)
    good, bad = run(good_c), run(bad_c)
    assert ok(good) and ok(bad)
    check_pieces(bad, bad_c, evaluate, backward, coefs=ALL_COEFS)          # the evaluate and backward kernels take the same actions
    check_terms(bad, bad_c, shape, ALL_COEFS)
    g = gathered(bad_c)
    logp = evaluate(bad_c["x"][at], g["m"][at], g["a"][at])[0]
    # logf of the device is not libm's: both are within an ulp of log(EPS), and an ulp of a number in [8, 16) is 2^-20
    assert np.all(np.abs(logp.astype(np.float64) - np.log(np.float64(np.float32(EPS)))) <= 2.0 ** -20), logp
    # the gradient of such a row is the one of a row whose log-probability has no weight
    w = weights(B, M, ALL_COEFS)
    none = backward(bad_c["x"][at], g["m"][at], np.zeros(len(at), np.int64), np.zeros(len(at), np.float32), np.full(len(at), w["g_ent"]),
                    np.full(len(at), w["g_bad"]))
    assert np.array_equal(bits(bad["grad_logits"][at]), bits(none))
    for k in OUT_KEYS:
        assert np.array_equal(bits(bad[k][rest]), bits(good[k][rest])), k
    # float64 gathers at the action and cannot state the four rows: it checks the run with the actions in range, whose other five
    # rows are these bits.  (Left out by construction: not exclusions in the sense of MAX_EXCLUDED.)
    check_against_float64(good, good_c, evaluate, coefs=ALL_COEFS)
    if normative:
        n = check_normative(bad, bad_c, coefs=ALL_COEFS)
        import head_normative as hn
        assert np.array_equal(bits(n["logp"][at]), bits(np.repeat(hn.logf(np.array([hn.EPS])), len(at))))


def scalar_changes(c, r):
    """(name, what rollout row r gets, the header's expressions stay free of NaN in the per-row terms)."""
    A = abs(c["adv"][r]) + np.float32(0.25)
    return [("ratio = inf, A > 0", dict(old=-200.0, adv=A), True), ("ratio = inf, A < 0", dict(old=-200.0, adv=-A), True),
            ("ratio = 0", dict(old=200.0), True), ("A = 0", dict(adv=0.0), True), ("A = NaN", dict(adv=np.nan), False),
            ("R = inf", dict(ret=np.inf), False)]


def check_off_contract_scalars(B, M, run, shape, evaluate, backward):
    """One mini-batch row reads a rollout row with an off-contract scalar: every other row keeps its bits, the row itself is what
    the header's expressions give on the kernel's ratio -- bit for bit where they give a number (0 * inf is NaN: a ratio of inf
    whose surrogate is clipped away makes g_logp, and with it the row's grad_logits, NaN), NaN where they give NaN.  Then three
    clips outside the usual range on the clean case.  run(c, clip) -> outputs under ALL_COEFS."""
    c = edge_case(B, M)
    clean = run(c, 0.2)
    assert ok(clean)
    check_pieces(clean, c, evaluate, backward, coefs=ALL_COEFS)
    b = next(b for b in range(B) if (c["idx"] == c["idx"][b]).sum() == 1)
    r = int(c["idx"][b])
    rest = np.setdiff1d(np.arange(B), [b])
    w = weights(B, M, ALL_COEFS)
    for name, change, finite in scalar_changes(c, r):
        cc = dict(c)
        for k, v in change.items():
            cc[k] = c[k].copy()
            cc[k][r] = v
        out = run(cc, 0.2)
        assert ok(out), name
        for k in OUT_KEYS:
            assert np.array_equal(bits(out[k][rest]), bits(clean[k][rest])), (name, k)
        ratio = out["rows"][:, 5].copy()
        if "ratio" in name:
            assert ratio[b] == (np.inf if "inf" in name else 0.0), (name, ratio[b])
        s = statement(cc, ratio, 0.2, ALL_COEFS, True)
        g = gathered(cc)
        grad = backward(cc["x"][b:b + 1], g["m"][b:b + 1], g["a"][b:b + 1], s["g_logp"][b:b + 1], np.full(1, w["g_ent"]), np.full(1, w["g_bad"]))
        pairs = [(out["rows"][b, 0], s["value"][b]), (out["rows"][b, 1], s["action"][b]), (out["rows"][b, 6], s["clipped"][b]),
                 (out["grad_values"][b], s["grad_values"][b]), (out["grad_logits"][b], grad[0])]
        for got, want in pairs:
            if finite:
                assert same_or_nan(got, want), (name, got, want)
            else:
                assert np.array_equal(np.isnan(got), np.isnan(want)), (name, got, want)
        check_terms(out, cc, shape, ALL_COEFS, nan_ok=True)
        if finite:
            assert not np.isnan(out["rows"][b]).any(), name
        elif name == "A = NaN":         # surr1 and surr2 are NaN and so is their fminf; g_ratio = (NaN <= NaN) ? A : 0 = 0
            assert np.isnan(out["rows"][b, 1]) and np.isnan(out["terms"][[1, 5]]).all() and not np.isnan(out["grad_logits"][b]).any()
        else:                           # d = e = -inf: the value term is inf, g_v is -inf, or NaN where the clamp does not pass
            assert out["rows"][b, 0] == np.inf and out["terms"][0] == np.inf and not np.isfinite(out["grad_values"][b])
    for clip in (0.0, 1.5, 1e30):           # lo = hi = 1; lo negative; lo and hi past every ratio and value difference
        out = run(c, clip)
        assert ok(out), clip
        check_pieces(out, c, evaluate, backward, clip=clip, coefs=ALL_COEFS)
        check_terms(out, c, shape, ALL_COEFS)
        assert bool(out["rows"][:, 6].any()) == (clip == 0.0)           # ratio != 1 is clipped at clip = 0, nothing from 1.5 on


# ------------------------------------------------------------------------------------------------------------------ advantages
ADV_EDGES = (255, 256, 257, 256 * 1024 - 1, 256 * 1024, 2 * 256 * 1024 + 1)      # iters 1 -> 2 and blocks 1024 -> 513 behind 256 * 1024


def adv_shape_rule(E):
    """bpp_ppo_advantages_info restated: 256 lanes, at most 1024 blocks; a block takes `iters` chunks of 256 elements."""
    chunks = -(-E // 256)
    iters = -(-chunks // 1024)
    return [256 * iters, -(-chunks // iters), 256]


def advantages_constant(E, seed=0):
    """returns - value_preds = 0.75 in every element, exactly: the values are eighths."""
    vp = (np.random.RandomState(seed + E).randint(-64, 65, E) / 8.0).astype(np.float32)
    return (vp + np.float32(0.75)).astype(np.float32), vp


def advantages_offset(E, seed=0):
    """A large common offset: returns = 1e4 + noise of unit size, value_preds = 0."""
    return (1e4 + np.random.RandomState(seed + E).randn(E)).astype(np.float32), np.zeros(E, np.float32)


def check_advantages_constant(adv, stats):
    """Every raw advantage is 0.75: the double sums are exact, mean = 0.75, std = 0, every advantage 0 / 1e-5 = 0."""
    assert stats[0] == 0.75 and stats[1] == 0.0 and not adv.any(), (stats, np.abs(adv).max())


def advantages_statement(ret, vp, C, W):
    """include/bpp_ppo.h: raw in float32, both sums in double in the stated order (blocks of C elements, W lanes, binary trees), one
    cast each, the normalisation in float32: (adv float32, mean, std)."""
    raw = np.asarray(ret, np.float32) - np.asarray(vp, np.float32)
    E = raw.size

    def tree(lanes):
        lanes = lanes.copy()
        d = W // 2
        while d:
            lanes[:d] = lanes[:d] + lanes[d:2 * d]
            d //= 2
        return lanes[0]

    def total(vals):
        parts = []
        for g0 in range(0, E, C):
            blk = vals[g0:g0 + C]
            lanes = np.zeros(W, np.float64)
            for i in range(0, len(blk), W):
                seg = blk[i:i + W]
                lanes[:len(seg)] = lanes[:len(seg)] + seg
            parts.append(tree(lanes))
        parts = np.array(parts, np.float64)
        lanes = np.zeros(W, np.float64)
        for i in range(0, len(parts), W):
            seg = parts[i:i + W]
            lanes[:len(seg)] = lanes[:len(seg)] + seg
        return tree(lanes)

    mean = total(raw.astype(np.float64)) / float(E)
    dv = raw.astype(np.float64) - mean
    std = np.sqrt(total(dv * dv) / float(E - 1))
    return (raw - F32(mean)) / (F32(std) + F32(1e-5)), mean, std


def advantages_case(E, seed=0):
    rng = np.random.RandomState(seed + E)
    vp = (rng.randn(E) * 2.0).astype(np.float32)
    return (vp + 0.5 + rng.randn(E)).astype(np.float32), vp


def check_advantages(adv, stats, ret, vp, C, W):
    want, mean, std = advantages_statement(ret, vp, C, W)
    assert np.array_equal(bits(adv), bits(want))
    assert stats[0] == mean and stats[1] == std
    raw = ret.astype(np.float64) - vp.astype(np.float64)
    m64, s64 = raw.mean(), raw.std(ddof=1)
    assert abs(mean - m64) <= 1e-12 * np.abs(raw).max() + 4 * EPS * abs(m64) and abs(std - s64) <= 4 * EPS * s64
    # float32 rounding: raw is half an ulp of itself off, the casts of mean and std half an ulp each, the subtraction, the sum
    # with 1e-5 and the division one rounding each
    a64 = (raw - m64) / (s64 + 1e-5)
    assert np.all(np.abs(adv - a64) <= 4 * EPS * (np.abs(a64) + (np.abs(raw) + abs(m64)) / s64))


# ---------------------------------------------------------------------------------------------------------------------- gather
def gather_case(B, n, seed=0):
    """(src with NaN padding behind every row, row stride, idx with duplicates and the first and last row)."""
    rng = np.random.RandomState(seed + 7 * B + n)
    rows, stride = 9, n + 3
    src = np.full((rows, stride), np.nan, np.float32)
    src[:, :n] = rng.randn(rows, n)
    idx = rng.randint(0, rows, size=B).astype(np.int64)
    idx[0] = rows - 1
    if B > 2:
        idx[-1], idx[1] = 0, idx[2]
    return src, stride, idx


# a wave copies kGatherPart = 512 floats: lengths on both sides of one and of two parts, batches that leave every remainder of
# B * parts modulo the four waves of a workgroup
GATHER_LENS = (511, 512, 513, 1024, 1025)
GATHER_BS = (1, 2, 3, 5)
GATHER_ROWS = 7
I64 = np.iinfo(np.int64)
# the last row, the first, a duplicate; `rows`, -1 and the int64 extremes: rows of NaN
GATHER_SEQ = (GATHER_ROWS - 1, 0, 0, GATHER_ROWS, 3, -1, 3, I64.max, GATHER_ROWS - 1, I64.min, 0)


def gather_edge_case(n, pad, seed=0):
    """(src [GATHER_ROWS, n + pad] with NaN in the padding, row stride)."""
    rng = np.random.RandomState(seed + 13 * n + pad)
    src = np.full((GATHER_ROWS, n + pad), np.nan, np.float32)
    src[:, :n] = rng.randn(GATHER_ROWS, n)
    return src, n + pad


def gather_index_vectors(B):
    """Windows of B indices that together walk GATHER_SEQ (wrapping): one call each."""
    k = len(GATHER_SEQ)
    return [np.array([GATHER_SEQ[(s + j) % k] for j in range(B)], np.int64) for s in range(0, k, B)]


def gather_expected(src, idx, n):
    want = np.full((len(idx), n), np.nan, np.float32)
    inside = (idx >= 0) & (idx < src.shape[0])
    want[inside] = src[idx[inside], :n]
    return want


# ------------------------------------------------------------------------------------- PPO.update beyond the recorded defaults
class MaskNet(torch.nn.Module):
    """net(obs) -> (logits, values, pred_mask): two layers, the mask prediction a sigmoid of its own outputs."""

    def __init__(self, D, M, H, dtype):
        super().__init__()
        self.M = M
        self.body = torch.nn.Sequential(torch.nn.Linear(D, H), torch.nn.Tanh(), torch.nn.Linear(H, 2 * M + 1)).to(dtype)

    def forward(self, obs):
        out = self.body(obs)
        return out[:, :self.M], out[:, self.M:self.M + 1], torch.sigmoid(out[:, self.M + 1:])


# T * N = 38 rows of M = 400 (the 20 x 20 bin: ppo_loss_kernel<8>).  38 is divisible by neither 4 nor 3: the generator drops the
# remainder as the reference's BatchSampler(drop_last=True) does, so no mini-batch is shorter than the others; the two updates, at 4
# and then at 3 mini-batches, are what gives the native path two (B, M) shapes, (9, 400) and (12, 400).
UPDATE = dict(T=2, N=19, M=400, D=24, H=16, epochs=2, mini=(4, 3), clip=0.2, lr=1e-3, eps=1e-5, norm=0.5, coefs=ALL_COEFS, seed=5)
_update = {}


def update_data():
    """The synthetic rollout and the initial parameters (float64), made once: masks with 1 .. M feasible entries, actions on
    feasible and infeasible cells, old log-probabilities those of the initial network moved by 0.15 * N(0, 1) (ratios on both sides
    of the clip interval from the first mini-batch on)."""
    if not _update:
        u = UPDATE
        T, N, M, D = u["T"], u["N"], u["M"], u["D"]
        rng = np.random.RandomState(17)
        torch.manual_seed(17)
        net = MaskNet(D, M, u["H"], torch.float64)
        obs = rng.randn(T + 1, N, D)
        m = np.zeros((T + 1, N, M))
        for row in m.reshape(-1, M):
            row[rng.permutation(M)[:rng.randint(1, M + 1)]] = 1.0
        a = rng.randint(0, M, (T, N, 1))
        vp = rng.randn(T + 1, N, 1) * 2.0
        ret = vp + 0.5 + rng.randn(T + 1, N, 1)
        with torch.no_grad():
            logits = net(torch.from_numpy(obs[:-1].reshape(T * N, D)))[0]
            old = head64(logits, torch.from_numpy(m[:-1].reshape(T * N, M)), torch.from_numpy(a.reshape(-1)))[0].numpy()
        old = (old + 0.15 * rng.randn(T * N)).reshape(T, N, 1)
        _update.update(obs=obs, location_masks=m, actions=a, value_preds=vp, returns=ret, action_log_probs=old,
                       init={k: v.clone() for k, v in net.state_dict().items()})
    return _update


def run_update(dtype, device):
    """Two PPO.update calls (UPDATE["mini"] mini-batches each) on the synthetic rollout: (the six means, the final parameters)."""
    import bpp_amd
    u, d = UPDATE, update_data()
    st = bpp_amd.RolloutStorage(u["T"], u["N"], (u["D"],), bpp_amd.Discrete(u["M"]))
    st._slabs = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in st._slabs.items()}
    st._bind()
    for k in ("obs", "location_masks", "value_preds", "returns", "actions", "action_log_probs"):
        getattr(st, k).copy_(torch.from_numpy(d[k]))
    st.to(device)
    net = MaskNet(u["D"], u["M"], u["H"], dtype)
    net.load_state_dict({k: v.to(dtype) for k, v in d["init"].items()})
    net.to(device)
    vc, ec, ic, mc = u["coefs"]
    agent = bpp_amd.PPO(net, u["clip"], u["epochs"], u["mini"][0], vc, ec, lr=u["lr"], eps=u["eps"], max_grad_norm=u["norm"], invalid_coef=ic,
                        mask_coef=mc)
    torch.manual_seed(u["seed"])
    means = []
    for mini in u["mini"]:
        agent.num_mini_batch = mini
        means += list(agent.update(st))
    return means, {k: v.detach().cpu().double().numpy() for k, v in net.state_dict().items()}
