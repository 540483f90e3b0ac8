#!/usr/bin/env python3
"""Records tests/golden/kfac_reference.npz from the live reference's KFACOptimizer (acktr/algo/kfac.py) on the CPU: the small
net of tests/kfac_cases.py, four steps with Tf = 2.

    w0.<name>            initial weights under the plain (unsplit) names
    batch<t>.<key>       x, action, adv, ret, noise of step t
    factors.<aa|gg>_<i>  the reference's running factors after step 0, module i in its own order
    params<t>.<name>     its parameters after step t
    factor_sensitivity   per step: relative L2 distance of its parameter update from its own run with the factors computed
                         in float64 and cast back (kfac_cases.reference_runs) -- the yardstick of the optimizer tests

The seed is the first for which the reference's own run is finite: its eigendecomposition fails on some tiny batches.

    python tests/golden/make_kfac_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import kfac_cases as kc  # noqa: E402
from oracle import ref_shims  # noqa: E402


def main():
    ref_shims.install()
    for seed in range(100):
        torch.manual_seed(seed)
        weights = {k: v.numpy().copy() for k, v in kc.SmallNet().state_dict().items()}
        batches = kc.make_batches(seed)
        try:
            trail, trail64, factors = kc.reference_runs(weights, batches)
        except Exception as exc:  # noqa: BLE001  (torch.linalg.eigh not converging, math domain error of a negative vg_sum)
            print("seed %d: %s" % (seed, exc))
            continue
        if all(np.isfinite(v).all() for run in (trail, trail64) for step in run for v in step.values()):
            break
    else:
        raise SystemExit("no seed gave a finite reference run")
    sens = kc.update_distance(trail64, trail, weights)
    assert all(np.isfinite(sens)) and all(s > 0 for s in sens), sens
    out = {"seed": np.int64(seed), "factor_sensitivity": np.array(sens, np.float64)}
    out.update({"w0." + k: v for k, v in weights.items()})
    for t, b in enumerate(batches):
        out.update({"batch%d.%s" % (t, k): v for k, v in b.items()})
    out.update({"factors." + k: v for k, v in factors.items()})
    for t, step in enumerate(trail):
        out.update({"params%d.%s" % (t, k): v for k, v in step.items()})
    path = os.path.join(HERE, "kfac_reference.npz")
    np.savez_compressed(path, **out)
    print("seed %d, factor_sensitivity %s -> %s (%d bytes)" % (seed, sens, path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
