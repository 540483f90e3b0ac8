"""Shared by tests/test_a2c_loss.py (emulated kernels) and tests/test_gpu_a2c_loss.py (device): inputs of bpp_a2c_loss
(include/bpp_update.h), its normative float32 expressions in numpy, the reference's expressions in float64 torch
(acktr/distributions.py:71-101 as tests/test_policy_head_f64.py restates them, acktr/algo/acktr_pipeline.py:55-66 and 88-92) and
the checks both suites run on whatever produced the outputs."""
import ctypes

import numpy as np
import torch

from test_masked_evaluate import GRAD_TOL, forward_tolerances

EPS = float(np.finfo(np.float32).eps)
COEFS = (0.5, 0.01, 2.0, 5.0)                  # value_loss_coef, entropy_coef, invalid_coef, mask_coef: the reference's
CANARY = np.float32(-777.25)
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_case(E, M, seed):
    """Logits at scale 3; masks with 1 .. M feasible entries, row 0 all infeasible and row 1 all feasible where E allows;
    actions on feasible cells (even rows) and infeasible ones (odd rows); pred_mask in [0, 1]; returns and values of both signs."""
    rng = np.random.RandomState(seed)
    x = (rng.randn(E, M) * 3.0).astype(np.float32)
    m = np.zeros((E, M), np.float32)
    for e in range(E):
        m[e, rng.permutation(M)[:rng.randint(1, M + 1)]] = 1.0
    if E >= 3:
        m[0], m[1] = 0.0, 1.0
    a = np.zeros(E, np.int64)
    for e in range(E):
        want = 1.0 if e % 2 == 0 else 0.0
        idx = np.nonzero(m[e] == want)[0]
        a[e] = rng.choice(idx) if idx.size else rng.randint(M)
    pm = rng.rand(E, M).astype(np.float32)
    ret = (rng.randn(E) * 2.0).astype(np.float32)
    val = (rng.randn(E) * 2.0).astype(np.float32)
    return dict(x=x, m=m, a=a, pm=pm, ret=ret, val=val, E=E, M=M)


def weights(E, M, coefs=COEFS):
    """The weights of include/bpp_update.h: formed in double, cast once."""
    vc, ec, ic, mc = coefs
    return dict(cE=F32(1.0 / E), cEM=F32(1.0 / (float(E) * M)), g_ent=F32(-ec / E), g_bad=F32(ic / (float(E) * M)),
                c_v=F32(-2.0 * vc / E), c_p=F32(2.0 * mc / (float(E) * M)))


def run_host(L, c, coefs=COEFS, pred=True, rows=True):
    """bpp_a2c_loss of library L (bound by _lib.bind_update) on host pointers: the emulated kernels."""
    E, M = c["E"], c["M"]
    out = dict(grad_logits=np.full((E, M), CANARY), grad_values=np.full(E, CANARY), grad_pred_mask=np.full((E, M), CANARY),
               rows=np.full((E, 5), CANARY), terms=np.full(6, CANARY))
    ws = np.zeros(int(L.bpp_a2c_loss_workspace(E, M)) // 8 + 1, np.float64)
    p = lambda v: v.ctypes.data                                                          # noqa: E731
    out["rc"] = L.bpp_a2c_loss(p(c["x"]), p(c["m"]), p(c["a"]), p(c["val"]), p(c["ret"]), p(c["pm"]) if pred else None, *coefs,
                               p(out["grad_logits"]), p(out["grad_values"]), p(out["grad_pred_mask"]), p(out["rows"]) if rows else None,
                               p(out["terms"]), p(ws), E, M, None)
    return out


def info(L, E, M):
    out = (ctypes.c_int32 * 4)()
    assert L.bpp_a2c_loss_info(E, M, out) == 0
    return list(out)


def loss64(x, v, pm, m, a, ret, coefs=COEFS):
    """acktr/distributions.py:71-101 and acktr/algo/acktr_pipeline.py:55-66, 88-92 on float64 torch tensors (pm may be None):
    (value_loss, action_loss, dist_entropy, prob_loss, graph_loss, loss, adv, logp)."""
    vc, ec, ic, mc = coefs
    lx = torch.softmax(x - (1.0 - m) * 14.0, dim=-1) + 1e-5
    p = lx / lx.sum(-1, keepdim=True)
    logc = torch.log(torch.clamp(p, EPS, 1.0 - EPS))
    logp = logc.gather(-1, a.reshape(-1, 1))[:, 0]
    dist_entropy = (-(p * logc).sum(-1)).mean()
    prob_loss = (torch.softmax(x, dim=-1) * (1.0 - m)).mean()
    adv = ret.reshape(-1) - v.reshape(-1)
    value_loss = adv.pow(2).mean()
    action_loss = -(adv.detach() * logp).mean()
    graph_loss = ((pm - m) ** 2).mean() if pm is not None else torch.zeros((), dtype=torch.float64)
    loss = value_loss * vc + action_loss + prob_loss * ic - dist_entropy * ec + mc * graph_loss
    return value_loss, action_loss, dist_entropy, prob_loss, graph_loss, loss, adv, logp


def reference64(c, coefs=COEFS, pred=True):
    """The reference's update in float64 torch autograd: five terms and loss [6], d loss / d logits, d values, d pred_mask."""
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    v = torch.from_numpy(c["val"]).double().requires_grad_(True)
    pm = torch.from_numpy(c["pm"]).double().requires_grad_(True)
    out = loss64(x, v, pm if pred else None, torch.from_numpy(c["m"]).double(), torch.from_numpy(c["a"]), torch.from_numpy(c["ret"]).double(),
                 coefs)
    out[5].backward()
    return dict(terms=np.array([float(t.detach()) for t in out[:6]]), grad_logits=x.grad.numpy(), grad_values=v.grad.numpy(),
                grad_pred_mask=pm.grad.numpy() if pred else None, adv=out[6].detach().numpy(), logp=out[7].detach().numpy())


def ulp_apart(got, want):
    """Distance in float32 ulps of two finite float32 values."""
    key = lambda f: (lambda i: i if i >= 0 else -(i & 0x7FFFFFFF))(int(np.float32(f).view(np.int32)))     # noqa: E731
    return abs(key(got) - key(want))


def check_pieces(out, c, evaluate, backward, coefs=COEFS, pred=True):
    """Checks 1 and 2: against the masked_evaluate kernels under the normative weights (bit for bit) and the numpy expressions."""
    E, M = c["E"], c["M"]
    w = weights(E, M, coefs)
    adv = c["ret"] - c["val"]                                                            # float32
    logp, ent, bad = evaluate(c["x"], c["m"], c["a"])
    assert np.array_equal(bits(out["rows"][:, 1]), bits(-(adv * logp)))
    assert np.array_equal(bits(out["rows"][:, 2]), bits(ent))
    assert np.array_equal(bits(out["rows"][:, 3]), bits(bad))
    g_logp = -(adv * w["cE"])
    grad = backward(c["x"], c["m"], c["a"], g_logp, np.full(E, w["g_ent"]), np.full(E, w["g_bad"]))
    assert np.array_equal(bits(out["grad_logits"]), bits(grad))
    assert np.array_equal(bits(out["grad_values"]), bits(w["c_v"] * adv))
    assert np.array_equal(bits(out["rows"][:, 0]), bits(adv * adv))
    if pred:
        d = c["pm"] - c["m"]
        assert np.array_equal(bits(out["grad_pred_mask"]), bits(w["c_p"] * d))
        sq64 = (d * d).astype(np.float64).sum(1)                                        # float64 sum of the float32 squares
        assert np.all(np.abs(out["rows"][:, 4].astype(np.float64) - sq64) <= (M - 1) * EPS * sq64)
    else:
        assert not out["rows"][:, 4].any()


def check_terms(out, c, coefs=COEFS):
    """Check 3: the terms are the double sums of the rows' columns, the loss its double expression, each within 1 ulp."""
    E, M = c["E"], c["M"]
    vc, ec, ic, mc = coefs
    means = [out["rows"][:, j].astype(np.float64).sum() / (E if j < 3 else float(E) * M) for j in range(5)]
    for j in range(5):
        assert ulp_apart(out["terms"][j], np.float32(means[j])) <= 1, (j, out["terms"][j], means[j])
    loss = vc * means[0] + means[1] + ic * means[3] - ec * means[2] + mc * means[4]
    assert ulp_apart(out["terms"][5], np.float32(loss)) <= 1, (out["terms"][5], loss)


def check_against_float64(out, c, coefs=COEFS, pred=True, verbose=True):
    """Check 4: against float64 autograd of the reference's expressions."""
    E, M = c["E"], c["M"]
    ref = reference64(c, coefs, pred)
    tol = forward_tolerances(M)
    t, r = out["terms"].astype(np.float64), ref["terms"]
    mean_adv = np.abs(ref["adv"]).mean()
    bounds = [4 * EPS * abs(r[0]), tol[0] * mean_adv + 4 * EPS * np.abs(ref["adv"] * ref["logp"]).mean(), tol[1], tol[2] / M,
              4 * EPS * abs(r[4])]
    diff = np.abs(t[:5] - r[:5])
    gdiff = np.abs(out["grad_logits"] - ref["grad_logits"])
    gbound = GRAD_TOL[0] * np.abs(ref["grad_logits"]) + GRAD_TOL[1] / E + 1e-9
    if verbose:
        print("a2c_loss E=%d M=%d: |term - f64| / bound = %s; grad_logits max |diff| / bound = %.3g"
              % (E, M, ["%.3g" % (d / b if b else d) for d, b in zip(diff, bounds)], float((gdiff / gbound).max())))
    for j in range(5):
        assert diff[j] <= bounds[j], (j, t[j], r[j], diff[j], bounds[j])
    assert np.all(gdiff <= gbound), float((gdiff / gbound).max())
    return ref
