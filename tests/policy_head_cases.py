"""The calls whose device bits tests/golden/policy_head_device_bits.npz holds: made by tests/golden/make_policy_head_bits.py (the
recorder) and replayed by tests/test_gpu_policy_head_bits.py.  Inputs are regenerated from seeds (a2c_cases.make_case, the input
families of tests/test_policy_head_f64.py); only outputs are stored.  Needs a HIP device."""
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import a2c_cases as ac  # noqa: E402
from test_policy_head_f64 import FAMILIES, family  # noqa: E402

FIXTURE = "policy_head_device_bits"
# E = 37 ends inside a four-row workgroup; M: every register template of bpp_a2c_loss and its looped path
EVAL_SHAPES = [(E, M) for E in (5, 37) for M in (15, 64, 100, 200, 400, 516)]
ACT_E = 37
ACT_WAVE_MS = (7, 37, 513, 800)            # masked_act_kernel_generic: M % 4 != 0 or M > 512
ACT_LANES_MS = (100, 200, 400)             # masked_act_kernel<PER, DET>
ACT_BASES = (0, 2 ** 32 + 5)               # the second wraps the 32-bit hash key
SAMPLE_MS = (100, 37)                      # sample_kernel<PER>, sample_kernel_generic
SEED, STEP = 5, 9


def toolchain():
    """What compiled the library and supplies the device's expf / logf."""
    from bpp_amd import _lib
    text = subprocess.run([_lib.hipcc(), "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True).stdout
    return " | ".join(line.strip() for line in text.splitlines()[:2])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def head_inputs(E, M, seed):
    """(logits, mask) [E, M]: row r is row r of input family r mod 10 (ties, near-ties, nothing / everything feasible among them)."""
    x, m = np.empty((E, M), np.float32), np.empty((E, M), np.float32)
    for k, name in enumerate(FAMILIES):
        fx, fm = family(name, E, M, seed * 31 + k)
        x[k::len(FAMILIES)], m[k::len(FAMILIES)] = fx[k::len(FAMILIES)], fm[k::len(FAMILIES)]
    return x, m


def eval_case(E, M):
    """({name: output to store}, the backward kernel's gradient under the normative weights) of bpp_masked_evaluate and bpp_a2c_loss."""
    import bpp_amd
    from bpp_amd.masks import _MaskedEvaluate
    c = ac.make_case(E, M, seed=1000 * E + M)
    x, m, a = dev(c["x"]), dev(c["m"]), dev(c["a"])
    out = {}
    xt = x.clone().requires_grad_(True)
    fwd = _MaskedEvaluate.apply(xt, m, a)
    for k, t in zip(("logp", "entropy", "bad"), fwd):
        out["evaluate_%s_E%d_M%d" % (k, E, M)] = t.detach().cpu().numpy()
    res = bpp_amd.a2c_loss(x, dev(c["val"]).view(E, 1), dev(c["pm"]), m, a.view(E, 1), dev(c["ret"]), *ac.COEFS, rows=True)
    for k in ("rows", "terms", "grad_logits"):
        out["a2c_%s_E%d_M%d" % (k, E, M)] = getattr(res, k).cpu().numpy()
    w = ac.weights(E, M)
    g = (-((c["ret"] - c["val"]) * w["cE"]), np.full(E, w["g_ent"]), np.full(E, w["g_bad"]))
    torch.autograd.backward(list(fwd), [dev(np.asarray(v, np.float32)) for v in g])
    return out, xt.grad.cpu().numpy()


def act_case(M):
    """{name: output} of bpp_masked_act: both id bases, deterministic and sampled."""
    import bpp_amd
    x, m = head_inputs(ACT_E, M, seed=M)
    xt, mt = dev(x), dev(m)
    assert xt.data_ptr() % 16 == 0 and mt.data_ptr() % 16 == 0
    out = {}
    for b, base in enumerate(ACT_BASES):
        for det in (True, False):
            a, lp = bpp_amd.masked_act(xt, mt, seed=SEED, step=STEP, deterministic=det, env_id_base=base)
            tag = "M%d_base%d_%s" % (M, b, "mode" if det else "sample")
            out["act_action_" + tag], out["act_logp_" + tag] = a.cpu().numpy()[:, 0], lp.cpu().numpy()[:, 0]
    return out


def sample_case(M):
    """{name: actions} of bpp_sample_feasible on the same masks, both id bases."""
    import ctypes
    from bpp_amd import _lib
    _, m = head_inputs(ACT_E, M, seed=M)
    mt = dev(m)
    out = {}
    for b, base in enumerate(ACT_BASES):
        a = torch.full((ACT_E,), -1, dtype=torch.int64, device="cuda")
        _lib.check(_lib.lib().bpp_sample_feasible(mt.data_ptr(), a.data_ptr(), ACT_E, M, base, SEED, STEP,
                                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        out["sample_M%d_base%d" % (M, b)] = a.cpu().numpy()
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
