#!/usr/bin/env python3
"""Records what include/bpp_policy_heads_train.h says the heads' training pass computes:   python tests/golden/make_heads_train_chain_bits.py

tests/golden/heads_train_chain_bits.npz: value, logits, pred, hidden, grad_hidden, grad_out_mask, grad_feat and grad_weights of
the real-valued cases tests/policy_heads_train_cases.py CHAIN_CASES as `normative_heads` there computes them -- the header's
float32 fmaf chains in the header's order, the splits added in double -- in plain numpy.  The inputs come from
numpy.random.RandomState alone (chain_case), so any machine regenerates the same bytes; the file holds a CRC32 of each input, and
per output a CRC32 of all its bits beside a strided sample of them, with which a failing comparison states its distance in ulps.
tests/test_policy_heads_train.py recomputes two cases live and runs every case on the emulator;
tests/test_gpu_policy_heads_train.py runs every case on the device.  Needs no GPU and no emulator, reads nothing of the reference,
and takes a few seconds.  The archive is stored uncompressed with a fixed time stamp: the same bytes on every run.  Rerun only
where a result is meant to change."""
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import policy_heads_train_cases as hc  # noqa: E402


def entries():
    out = {}
    for spec in hc.CHAIN_CASES:
        case = hc.chain_case(*spec)
        out.update(hc.chain_entries(case, hc.chain_reference(case), hc.chain_name(*spec)))
    return out


def save(path, arrays):
    """numpy.savez without compression and with one fixed time stamp, so that the bytes depend on the arrays alone."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for key in sorted(arrays):
            with z.open(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[key]), allow_pickle=False)


def main():
    out = entries()
    path = os.path.join(HERE, hc.CHAIN_FIXTURE + ".npz")
    save(path, out)
    assert os.path.getsize(path) < 400000, os.path.getsize(path)
    print("%d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
