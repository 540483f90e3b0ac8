"""The masked policy head stated once more, independently of csrc/ (tests/test_masked_evaluate.py, tests/test_a2c_loss.py):

    lx = softmax(x - 14 (1 - mask)) + 1e-5,  p = lx / sum(lx),  logp = log(clamp(p[a])),  ent = -sum p log(clamp(p)),
    bad = sum softmax(x) (1 - mask),  grad = d (g_logp logp + g_ent ent + g_bad bad) / dx

as the kernels are specified to compute it: float32 throughout, no contraction, one row in 64 lanes.  Entry k
lives in lane k % 64; a lane fills each of its accumulators over k = lane, lane + 64, ... in ascending order; a row sum or
maximum is then the butterfly  v = op(v, v[lane ^ d])  for d = 32 ... 1.  expf / logf are the C library's, through ctypes:
the host emulator of the kernels calls the same two functions, so the bits compared do not depend on the libm version.

Plain numpy on np.float32 arrays; nothing here reads or calls the code under test."""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
WAVE = 64
PENALTY, FLOOR = F(14.0), F(1e-5)
EPS = F(np.finfo(np.float32).eps)        # torch's probs_to_logits clamp
ONE = F(1.0)
HI = ONE - EPS

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _name in ("expf", "logf"):
    getattr(_libm, _name).argtypes = [ctypes.c_float]
    getattr(_libm, _name).restype = ctypes.c_float


def expf(v):
    return np.array([_libm.expf(float(t)) for t in v], F)


def logf(v):
    return np.array([_libm.logf(float(t)) for t in v], F)


def clamp(p):
    return np.minimum(np.maximum(p, EPS), HI)


def butterfly(v, op):
    idx = np.arange(WAVE)
    for d in (32, 16, 8, 4, 2, 1):
        v = op(v, v[idx ^ d])
    return v[0]


def lanes(terms, op, start):
    """The 64 lane accumulators over terms[k], k = lane, lane + 64, ... ascending, then the butterfly."""
    acc = np.full(WAVE, start, F)
    for k0 in range(0, len(terms), WAVE):
        chunk = terms[k0:k0 + WAVE]
        acc[:len(chunk)] = op(acc[:len(chunk)], chunk)
    return butterfly(acc, op)


def row_sum(terms):
    return lanes(terms, np.add, 0.0)


def row_max(terms):
    return lanes(terms, np.maximum, -np.inf)


def row(x, m, a, g_logp, g_ent, g_bad):
    """(logp, entropy, bad, grad [M]) of one row: logits x [M], mask m [M], action a (any int64), the three weights."""
    x, m = np.asarray(x, F), np.asarray(m, F)
    gl, ge, gb = F(g_logp), F(g_ent), F(g_bad)
    M = len(x)
    om = ONE - m
    z = x - om * PENALTY
    mq, ma = row_max(z), row_max(x)
    eq, ea = expf(z - mq), expf(x - ma)
    sq, sa = row_sum(eq), row_sum(ea)
    q = eq / sq
    tot = row_sum(q + FLOOR)
    p = (q + FLOOR) / tot
    lg = logf(clamp(p))
    av = ea / sa
    ent = row_sum(-(p * lg))                 # h -= p * lg: the same bits as adding the negated product
    bad = row_sum(av * om)
    # h_k = d / d p_k: the entropy term, and the log-probability term on the entry taken; the clamp's derivative is 0 outside
    inside = (p > EPS) & (p < HI)
    pc = clamp(p)
    h = -ge * (lg + np.where(inside, p / pc, F(0.0)))
    taken = 0 <= a < M
    if taken:
        h[a] = h[a] + (gl / pc[a] if inside[a] else F(0.0))
    c = row_sum(p * h)
    v = row_sum(q * (h - c) / tot)
    u = (h - c) / tot
    grad = q * (u - v) + gb * av * (om - bad)
    logp = logf(clamp(np.array([p[a] if taken else EPS], F)))[0]
    return logp, ent, bad, grad.astype(F)


def rows(x, m, a, g_logp, g_ent, g_bad):
    """row() over [E, M] inputs and [E] weights: logp [E], entropy [E], bad [E], grad [E, M], all float32."""
    out = [row(x[e], m[e], int(a[e]), g_logp[e], g_ent[e], g_bad[e]) for e in range(len(x))]
    return tuple(np.array([o[i] for o in out], F) for i in range(4))


# ---- the cases both suites pin: every register template of bpp_a2c_loss (1, 2, 4, 8 entries per lane) on both sides of its
# edge, the looped path with a tail, fewer entries than lanes
MS = [15, 64, 65, 100, 129, 200, 257, 400, 512, 513]
_cache = {}


def case(M):
    """(inputs, expected) for M, computed once and never modified.  inputs: a2c_cases.make_case(5, M) (row 0 all infeasible,
    row 1 all feasible) and two more rows, copies of rows 2 and 3 with the actions -1 and M: E = 7.  The weights are the
    normative ones of include/bpp_update.h for that E.  expected: logp, ent, bad, grad of the statement above."""
    if M not in _cache:
        import a2c_cases as ac
        c = ac.make_case(5, M, seed=7000 + M)
        for k in ("x", "m", "a", "pm", "ret", "val"):
            c[k] = np.concatenate([c[k], c[k][2:4]])
        c["a"][5:] = (-1, M)
        c["E"] = E = 7
        w = ac.weights(E, M)
        adv = c["ret"] - c["val"]
        c["adv"] = adv
        c["g"] = (-(adv * w["cE"]), np.full(E, w["g_ent"]), np.full(E, w["g_bad"]))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        want = dict(zip(("logp", "ent", "bad", "grad"), rows(c["x"], c["m"], c["a"], *c["g"])))
        _cache[M] = (c, want)
    return _cache[M]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
