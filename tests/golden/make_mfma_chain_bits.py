#!/usr/bin/env python3
"""Records the emulator's bits of the two MFMA kernels on real-valued data:   python tests/golden/make_mfma_chain_bits.py

tests/golden/mfma_chain_emulator_bits.npz: bpp_policy_forward (every head) and bpp_kfac_factor (m after a first batch and after a
second with rho = 0.99) computed by the product kernels under the host SIMT emulator (tests/emu), where policy_chain and kfac_mac
are sequential fmaf chains in ascending k.  The inputs come from numpy.random.RandomState alone (tests/policy_cases.py
chain_case, tests/kfac_cases.py CHAIN_CASES), so any machine regenerates the same bytes; the file holds a CRC32 of each input
beside the output bits.  tests/test_policy_forward.py and tests/test_kfac.py recompute every entry on the emulator;
tests/test_gpu_policy_forward.py and tests/test_gpu_kfac.py compare the device's v_mfma_f32_32x32x2_f32 with it.  Needs no GPU and
reads nothing of the reference.  Rerun only where a result is meant to change."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "emu"))

import emu_binding  # noqa: E402
import kfac_cases as kc  # noqa: E402
import policy_cases as pc  # noqa: E402
from bpp_amd import _lib  # noqa: E402


def main():
    emu = emu_binding.load()
    L = _lib.bind_kfac(_lib.bind_policy(ctypes.CDLL(emu.LIB)))
    L.bpp_last_error.restype = ctypes.c_char_p
    out = {}
    for spec in pc.CHAIN_CASES:
        out.update(pc.chain_entries(pc.host_runner(L), spec))
    for name in kc.CHAIN_CASES:
        out.update(kc.chain_entries(kc.host_runner(L), name)[0])
    assert all(v.size < 20000 for v in out.values())
    path = os.path.join(HERE, pc.CHAIN_FIXTURE + ".npz")
    np.savez_compressed(path, **out)
    print("%d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
