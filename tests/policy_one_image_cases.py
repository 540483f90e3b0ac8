"""Shared cases of the one-image policy-forward tests (tests/test_policy_forward_one_image.py on the emulator,
tests/test_gpu_policy_forward_one_image.py on the device): the runners that call bpp_policy_forward_one_image
(include/bpp_policy_one_image.h) with host or device pointers, the shapes of every item, and the inputs of the recorded chain
bits.  The cases themselves -- exact-integer networks, real-valued networks with their float64 reference -- are those of
tests/policy_cases.py, which this module only reads."""
import ctypes
import os
import sys

import numpy as np
import torch

from bpp_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_cases as pc  # noqa: E402

HEADS = pc.HEADS
FORM = "one_image"

# (S, H, M, n): bit for bit against bpp_policy_forward, wherever both accept the shape.  (10, 256, 100): P = 2, an odd n leaves a
# workgroup with one bin; (5, 32, 25): TW = 1; (11, 64, 121): the first side with P = 1; (15, 512, 450): the largest shared side.
SAME_BITS = [(10, 256, 100, 1), (10, 256, 100, 3), (10, 256, 100, 5), (5, 32, 25, 3), (11, 64, 121, 2), (15, 512, 450, 2)]
# (S, H, M, n, seed): exact-integer networks beyond the two-image form.  16: TW = 2; 17: TW = 3 (10 tiles); 20: TW = 4 with 13
# tiles (wave 0 has a fourth tile, the others do not); 22: all 16 tiles; (12, 96, 144): TW = 2 and P = 1 inside the shared range.
EXACT = [(16, 32, 256, 2, 40), (17, 64, 578, 1, 40), (20, 256, 400, 1, 40), (20, 256, 400, 3, 40), (20, 32, 800, 2, 40), (22, 32, 484, 1, 40),
         (12, 96, 144, 3, 40)]
REAL = [(20, 256, 400), (22, 96, 484)]               # real-valued, 16 synthetic states, the rule of pc.check_real
CHAIN_FIXTURE = "mfma_chain_one_image_bits"
CHAIN_CASES = [(20, 256, 400, 2), (16, 64, 256, 3), (22, 32, 484, 1)]        # (S, H, M, n)


def case_id(spec):
    return "s%d_h%d_m%d_n%d" % tuple(spec[:4])


def info(L, geom, n):
    out = (ctypes.c_int32 * 8)()
    rc = L.bpp_policy_forward_one_image_info(pc.geom_arg(geom), int(n), out)
    assert rc == 0, rc
    return dict(zip(_lib.POLICY_ONE_IMAGE_INFO, (int(v) for v in out)))


def host_runner(L):
    """pc.host_runner for bpp_policy_forward_one_image: runner(obs [n, stride], geom, blob, want) -> {head: numpy} through host
    pointers (the emulated library)."""
    def run(obs, geom, blob, want=HEADS):
        obs = np.ascontiguousarray(obs, np.float32)
        n, stride = obs.shape
        S, H, M = geom
        g = pc.geom_arg(geom)
        ws = np.full(L.bpp_policy_forward_one_image_workspace(g, n) // 4 + 1, np.nan, np.float32)
        outs = {"value": np.full(n, np.nan, np.float32), "logits": np.full((n, M), np.nan, np.float32), "pred": np.full((n, M), np.nan, np.float32)}
        ptr = [outs[h].ctypes.data if h in want else None for h in HEADS]
        blob = np.ascontiguousarray(blob, np.float32)
        assert blob.size == L.bpp_policy_one_image_weights_floats(g)
        rc = L.bpp_policy_forward_one_image(obs.ctypes.data, stride, n, g, blob.ctypes.data, ptr[0], ptr[1], ptr[2], ws.ctypes.data, None)
        assert rc == 0, (rc, L.bpp_last_error())
        assert np.isnan(ws[-1]) and not np.isnan(ws[:-1]).any(), "the workspace is n * 20 A floats, all written"
        for h in HEADS:
            if h not in want:
                assert np.isnan(outs[h]).all(), "%s was not asked for and was written" % h
        return {h: outs[h] for h in want}
    return run


def device_runner(device="cuda:0", form=FORM):
    """The same through bpp_amd.policy_forward(..., form=) on the device."""
    def run(obs, geom, blob, want=HEADS):
        o = torch.from_numpy(np.ascontiguousarray(obs, np.float32)).to(device)
        out = pc.pol.policy_forward(o, torch.from_numpy(np.ascontiguousarray(blob, np.float32)).to(device), geom, want, form=form)
        torch.cuda.synchronize()
        return {h: t.cpu().numpy() for h, t in zip(HEADS, out) if t is not None}
    return run


def real_case(S, H, M, seed=11):
    """pc.wide_real_case at any side: pc.real_weights on pc.synthetic_states with the float64 and float32 torch forwards."""
    return pc.with_references((S, H, M), pc.real_weights(S, H, M, seed), pc.synthetic_states(S))


def padded(obs, extra=3, fill=9.0):
    """The rows of obs `extra` floats further apart, the gap filled with a value no row holds."""
    out = np.full((obs.shape[0], obs.shape[1] + extra), fill, np.float32)
    out[:, :obs.shape[1]] = obs
    return out


def check_same_bits(one, two, spec, seed=11):
    """Every head of runner `one` equals that of runner `two` bit for bit on pc.real_weights and pc.synthetic_states."""
    S, H, M, n = spec
    blob = pc.pol.pack_weights(pc.real_weights(S, H, M, seed), S, H, M).numpy()
    obs = pc.synthetic_states(S, n)
    a, b = one(obs, (S, H, M), blob), two(obs, (S, H, M), blob)
    for h in HEADS:
        assert pc.same_bits(a[h], b[h]) and np.isfinite(a[h]).all() and np.abs(a[h]).max() > 0, (spec, h, pc.ulps(a[h], b[h]))


def check_batch_independence(run, geom=(20, 256, 400)):
    """Row i of n = 3 equals the same row evaluated alone, bit for bit, and differs from the other rows."""
    S = geom[0]
    blob = pc.pol.pack_weights(pc.real_weights(*geom, 11), *geom).numpy()
    states = pc.synthetic_states(S, 3)
    batch = run(states, geom, blob)
    for i in range(3):
        alone = run(states[i:i + 1], geom, blob)
        for h in HEADS:
            assert pc.same_bits(alone[h][0], batch[h][i]), (h, i)
            assert not pc.same_bits(batch[h][(i + 1) % 3], batch[h][i]), (h, i)


def chain_entries(run, spec):
    """{key: value} of one case for the fixture: the CRC32 of the bytes of each input (pc.chain_case: numpy's RandomState alone
    determines them) and of every head's output bits from `run`."""
    case, name = pc.chain_case(*spec), pc.chain_name(*spec)
    out = {name + ".crc.obs": pc.crc(case["obs"]), name + ".crc.blob": pc.crc(case["blob"])}
    got = run(case["obs"], case["geom"], case["blob"])
    for h in HEADS:
        out[name + ".crc." + h] = pc.crc(np.ascontiguousarray(got[h], np.float32).view(np.uint32))
    return out
