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
# |kernel ratio - exp64(float32(logp - old))| / exp64: the largest value over every case of both suites is 5.45e-8 with the emulator
# (glibc expf) and 7.16e-8 on the device; the bound is twice the larger
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
    surr1 = ratio * A
    surr2 = np.minimum(np.maximum(ratio, lo), hi) * A
    g_ratio = np.where(surr1 <= surr2, A, F32(0.0))
    d = v - R
    if clipped_value:
        t = v - vp
        e = (vp + np.minimum(np.maximum(t, -cf), cf)) - R
        d2, e2 = d * d, e * e
        ep = e * ((t >= -cf) & (t <= cf)).astype(np.float32)
        vterm = F32(0.5) * np.maximum(d2, e2)
        g_v = np.where(d2 > e2, d, np.where(d2 < e2, ep, F32(0.5) * d + F32(0.5) * ep))
    else:
        vterm, g_v = F32(0.5) * (d * d), d
    return dict(surr1=surr1, surr2=surr2, action=-np.minimum(surr1, surr2), g_ratio=g_ratio, value=vterm, grad_values=w["c_v"] * g_v,
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


def check_terms(out, c, shape, coefs=COEFS):
    """The terms are the double sums of the rows' columns in the stated order, divided and cast once: bit for bit."""
    B, M = c["B"], c["M"]
    vc, ec, ic, mc = coefs
    R, _, _, W = shape
    means = {j: ordered_sum(out["rows"][:, j], R, W) / (float(B) if j not in (3, 4) else float(B) * float(M)) for j in (0, 1, 2, 3, 4, 6)}
    want = [means[0], means[1], means[2], means[3], means[4], vc * means[0] + means[1] - ec * means[2] + ic * means[3] + mc * means[4], means[6]]
    assert np.array_equal(bits(out["terms"]), bits(np.array(want).astype(np.float32))), (out["terms"], want)


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


# ------------------------------------------------------------------------------------------------------------------ advantages
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
