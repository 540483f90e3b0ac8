#!/usr/bin/env python3
"""Edge vectors for the native returns (include/bpp_rollout.h), recorded by RUNNING THE UNMODIFIED REFERENCE
acktr/storage.py RolloutStorage.compute_returns (build container only):   python tests/golden/make_returns_edges.py

tests/golden/returns_edges.npz holds what returns_golden.npz holds (make_returns_golden.py), but every kind of array ONCE, the
input sets (rewards, value_preds, next_value, masks, bad_masks) and the cases (returns, vlast) concatenated flat in file order --
hundreds of small members would cost more than their contents -- ; no returns0: `returns` holds -7 before every call; `family`
[S] (unit / denormal / huge) and `tile` int64 [S] per input set.  tests/returns_cases.py's load_edge_cases() cuts it up.  The input sets are
tests/returns_cases.py's edge_plan(): time steps around the kernel's eight-row chunks (1, 7, 8, 9, 13, 16, 17, 33, and 1 000),
bin counts around a lane and a workgroup of its 16-byte form (1, 3, 4, 5, 252, 256, 260), gamma = 0, lambda = 0, gamma = lambda
= 1 and a pair whose double product rounds to another float32 than the product of the float32s, all four variants each; and the
value families of family_inputs(): subnormal numbers, and overflow to +-inf with inf * 0 = NaN behind it.

What the file claims about itself is asserted here, on the reference's own results, before it is written.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_shims  # noqa: E402

ref_shims.install()

import returns_cases as rc  # noqa: E402
from make_returns_golden import reference  # noqa: E402


def check_family(family, returns, T):
    """The properties the tests rely on, per recorded result (rows 0 .. T - 1: what the recurrence produced)."""
    r = returns[:T]
    nan, inf = np.isnan(r), np.isinf(r)
    if family == "huge":
        assert inf.any() and nan.any(), "a 'huge' result must hold both inf and NaN"
    else:
        assert not nan.any() and not inf.any(), family
    if family == "denormal":
        sub = (r != 0.0) & (np.abs(r) < rc.FLT_MIN)
        assert sub.any() and (r != 0.0).any(), "a 'denormal' result must hold subnormal numbers"
    return int(nan.sum()), int(r.size)


def main():
    pairs = rc.edge_pairs()
    g, lam = pairs[-1]
    assert np.float32(g * lam) != np.float32(np.float32(g) * np.float32(lam)), "the product pair must round differently"
    assert pairs[:4] == [(0.99, 0.95), (0.0, 0.95), (0.99, 0.0), (1.0, 1.0)]
    plan = rc.edge_plan()
    shapes = {(T, N) for f, T, N, _, _ in plan if f == "unit"}
    assert all((T, 260) in shapes for T in rc.EDGE_T) and all((13, N) in shapes for N in rc.EDGE_N) and set(rc.EDGE_LONG) <= shapes
    out = {"shapes": np.array([(T, N) for _, T, N, _, _ in plan], dtype=np.int64), "gl": np.array(pairs, dtype=np.float64),
           "family": np.array([f for f, _, _, _, _ in plan]), "tile": np.array([t for _, _, _, t, _ in plan], dtype=np.int64)}
    cases, flat, nans = [], {}, {f: [0, 0] for f in rc.FAMILIES}
    for s, (family, T, N, tile, ks) in enumerate(plan):
        d = rc.family_inputs(family, T, N, seed=7000 + s, tile=tile)
        assert all(np.isfinite(v).all() for v in d.values())
        if family == "denormal":
            for k in ("rewards", "value_preds", "next_value"):
                assert ((d[k] != 0.0) & (np.abs(d[k]) < rc.FLT_MIN)).any(), k
        for k, v in d.items():
            if k != "returns0":
                flat.setdefault(k, []).append(v.ravel())
        for k in ks:
            for use_gae in (0, 1):
                for proper in (0, 1):
                    c = len(cases)
                    ret, vlast = reference(d, T, N, bool(use_gae), pairs[k][0], pairs[k][1], bool(proper))
                    n, size = check_family(family, ret, T)
                    nans[family][0] += n
                    nans[family][1] += size
                    flat.setdefault("returns", []).append(ret.ravel())
                    flat.setdefault("vlast", []).append(vlast.ravel())
                    cases.append((s, k, use_gae, proper))
    # NaN positions are compared as a class by the tests: they stay a minority where they occur and do not occur elsewhere
    assert nans["unit"][0] == 0 and nans["denormal"][0] == 0 and 0 < 2 * nans["huge"][0] < nans["huge"][1], nans
    out["cases"] = np.array(cases, dtype=np.int64)
    out.update({k: np.concatenate(v) for k, v in flat.items()})
    path = os.path.join(HERE, "returns_edges.npz")
    np.savez_compressed(path, **out)
    print("%s: %d input sets, %d cases, %d bytes; NaN share of the huge family %.3f" %
          (path, len(plan), len(cases), os.path.getsize(path), nans["huge"][0] / nans["huge"][1]))


if __name__ == "__main__":
    main()
