#!/usr/bin/env python3
"""Records the emulator's bits of the one-image policy forward on real-valued data:
    python tests/golden/make_mfma_chain_one_image_bits.py

tests/golden/mfma_chain_one_image_bits.npz: per case of tests/policy_one_image_cases.py CHAIN_CASES -- sides 16, 20 and 22, where
bpp_policy_forward refuses and so gives no yardstick -- the CRC32 of every head's output bits from bpp_policy_forward_one_image
under the host SIMT emulator (tests/emu), where policy_chain is a sequential fmaf chain in ascending k, beside the CRC32 of each
input.  The inputs come from numpy.random.RandomState alone (tests/policy_cases.py chain_case), so any machine regenerates the
same bytes.  tests/test_policy_forward_one_image.py recomputes every entry on the emulator;
tests/test_gpu_policy_forward_one_image.py compares the device's v_mfma_f32_32x32x2_f32 with it.  Needs no GPU and reads nothing
of the reference.  Rerun only where a result is meant to change."""
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
import policy_one_image_cases as oc  # noqa: E402
from bpp_amd import _lib  # noqa: E402


def main():
    emu = emu_binding.load()
    L = _lib.bind_policy_one_image(ctypes.CDLL(emu.LIB))
    L.bpp_last_error.restype = ctypes.c_char_p
    out = {}
    for spec in oc.CHAIN_CASES:
        out.update(oc.chain_entries(oc.host_runner(L), spec))
    path = os.path.join(HERE, oc.CHAIN_FIXTURE + ".npz")
    np.savez_compressed(path, **out)
    print("%d entries, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
