#!/usr/bin/env python3
"""Records the device's bits of the policy-head kernels:   python tests/golden/make_policy_head_bits.py   (needs an MI355X)

tests/golden/policy_head_device_bits.npz: the outputs of the calls listed in tests/policy_head_cases.py -- bpp_masked_evaluate,
bpp_a2c_loss, bpp_masked_act through both of its kernels, bpp_sample_feasible through both of its -- and the version of the
toolchain that compiled the library (the device's expf / logf are its).  Recorded from the commit BEFORE the head's expressions
and the wave primitives were stated once (csrc/bpp_wave.inl, the top of csrc/bpp_heads.inl); tests/test_gpu_policy_head_bits.py
replays the calls and compares bit for bit, so rerun this only where a result is meant to change, or after a toolchain change
that moves the device library's bits."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import policy_head_cases as pc  # noqa: E402


def main():
    out = {}
    for E, M in pc.EVAL_SHAPES:
        stored, bwd = pc.eval_case(E, M)
        assert pc.same_bits(bwd, stored["a2c_grad_logits_E%d_M%d" % (E, M)]), (E, M)    # one stored gradient serves both kernels
        out.update(stored)
    for M in pc.ACT_WAVE_MS + pc.ACT_LANES_MS:
        out.update(pc.act_case(M))
    for M in pc.SAMPLE_MS:
        out.update(pc.sample_case(M))
    out["toolchain"] = np.array(pc.toolchain())
    path = os.path.join(HERE, pc.FIXTURE + ".npz")
    np.savez_compressed(path, **out)
    print("%d arrays, %d bytes, toolchain: %s" % (len(out) - 1, os.path.getsize(path), out["toolchain"]))


if __name__ == "__main__":
    main()
