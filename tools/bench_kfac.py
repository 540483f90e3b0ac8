#!/usr/bin/env python3
"""Times one Kronecker factor of K-FAC (bpp_kfac_factor through bpp_amd.kfac_factor) per layer shape of the reference's CNNPro
(acktr/model.py:265-323) against this repository's torch restatement of the reference's expression (bpp_amd.kfac.torch_factor:
unfold -> contiguous -> matmul -> running average, acktr/algo/kfac.py:15-70).

    python tools/bench_kfac.py [--out profiles/kfac_factor.json]

Two batch sizes: B = 5 x 4 096 rows of a rollout, where the torch form still fits, with both sides timed in the same process on
the same tensors, alternating batch by batch; and B = 5 x 65 536, the native kernel alone, with the bytes the torch form would
have had to materialise.  Every sample is a batch of back-to-back calls between two device events: device time per call with
the enqueue cost in it.  Reported: median and 10th / 90th percentile over the batches, the ratio of the medians, the FLOP of
the full D x D product (2 R D^2, what the torch form computes; the kernel computes the upper triangle) per second of the native
call, and the largest difference between the two results relative to the largest entry.  Needs a HIP device; there is no CPU
mode.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bpp_amd
from bpp_amd import kfac

CONV3 = dict(kernel_size=(3, 3), stride=(1, 1), padding=(1, 1))
# (name, layout, shape after the batch, conv geometry, scale kind)
LAYERS = [("conv 4->64 3x3, input", "patch", (4, 10, 10), CONV3, "conv_a"),
          ("conv 64->64 3x3, input", "patch", (64, 10, 10), CONV3, "conv_a"),
          ("conv 64->8 1x1, input", "patch", (64, 10, 10), {}, "conv_a"),
          ("conv ->64, grad-output", "nchw", (64, 10, 10), {}, "conv_g"),
          ("conv ->8, grad-output", "nchw", (8, 10, 10), {}, "conv_g"),
          ("linear 800->256, input", "rows", (800,), {}, "linear_a"),
          ("linear 256->100, input", "rows", (256,), {}, "linear_a"),
          ("linear ->100, grad-output", "rows", (100,), {}, "linear_g")]


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def summary(us):
    return {"median_us": float(np.median(us)), "p10_us": float(np.percentile(us, 10)), "p90_us": float(np.percentile(us, 90)), "batches": len(us)}


def bench(layer, B, batches, calls, dev, with_torch):
    name, layout, shape, conv, kind = layer
    torch.manual_seed(B + len(shape))
    x = torch.randn((B,) + shape, device=dev)
    _, geom, D, R, positions = kfac.factor_geometry(x, layout, **conv)
    scale = kfac.factor_scale(kind, B, positions)
    info = (ctypes.c_int32 * 6)()
    bpp_amd._lib.check(bpp_amd._lib.lib().bpp_kfac_factor_info(kfac._LAYOUTS[layout], bpp_amd._lib.kfac_geom(geom), info))
    m = torch.zeros(D, D, device=dev)
    cell = {"layer": name, "layout": layout, "B": B, "D": D, "R": R, "splits": int(info[4]), "rows_per_split": int(info[3]),
            "source_bytes": x.numel() * 4, "rows_bytes_of_the_torch_form": R * D * 4, "flop_full_product": 2.0 * R * D * D}

    def native():
        return kfac.kfac_factor(x, layout, m, 0.99, True, scale, **conv)

    runs = {"native": native}
    first = native().clone()
    cell["native_repeats_bit_for_bit"] = bool(torch.equal(native().view(torch.int32), first.view(torch.int32)))
    cell["native_symmetric_bit_for_bit"] = bool(torch.equal(first.view(torch.int32), first.t().contiguous().view(torch.int32)))
    if with_torch:
        m_t = torch.zeros(D, D, device=dev)

        def plain():
            return kfac.torch_factor(x, layout, m_t, 0.99, True, scale, **conv)

        runs["torch"] = plain
        cell["max_abs_difference_over_max_abs"] = float((plain() - first).abs().max() / first.abs().max())
    samples = {k: [] for k in runs}
    for _ in range(batches):
        for k, fn in runs.items():
            samples[k].append(timed(fn, calls, 2))
    for k, v in samples.items():
        cell[k] = summary(v)
    cell["native"]["flop_per_s_full_product"] = cell["flop_full_product"] / (cell["native"]["median_us"] * 1e-6)
    if with_torch:
        cell["native"]["speedup_over_torch"] = cell["torch"]["median_us"] / cell["native"]["median_us"]
    return cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kfac_factor.json"))
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--large-calls", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kfac.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev),
           "method": "device events around batches of back-to-back calls (%d; %d at B = 5 x 65536), native and torch alternated batch by "
                     "batch; median and 10th / 90th percentile of the per-call time over %d batches" % (args.calls, args.large_calls, args.batches),
           "cells": []}
    for B, with_torch, calls in ((5 * 4096, True, args.calls), (5 * 65536, False, args.large_calls)):
        for layer in LAYERS:
            cell = bench(layer, B, args.batches, calls, dev, with_torch)
            res["cells"].append(cell)
            print(json.dumps(cell), flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
