#!/usr/bin/env python3
"""Times the native returns (bpp_compute_returns through RolloutStorage.compute_returns) against the reference's recurrence
executed by torch on the same device tensors, and a lock-step into the storage against step_tensors + insert.

    python tools/bench_returns.py [--out profiles/returns_kernel.json]

Cells: N = 65 536 bins, T = 5 and 32, the plain variant (main.py's) and GAE with proper time limits.  Both sides run in the same
process on the same tensors, alternating; every sample is a batch of back-to-back calls between two device events, so a figure
is device time per call with the launches' enqueue cost in it (what a training loop pays).  Reported: the median and the
10th / 90th percentiles over the batches, the ratio of the medians, and the native call's share of the HBM roofline on the bytes
the algorithm moves (counted from the shapes below, not measured).  Needs a HIP device; there is no CPU mode.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bpp_amd

HBM_PEAK = 8.0e12      # bytes/s, MI355X


def torch_returns(st, next_value, use_gae, gamma, lam, proper):
    """The reference's compute_returns (acktr/storage.py:72-111) as its storage executes it: a Python loop over t of elementwise
    tensor operations on [N,1] rows."""
    T = st.rewards.size(0)
    if use_gae:
        st.value_preds[-1] = next_value
        gae = 0
        for t in reversed(range(T)):
            delta = st.rewards[t] + gamma * st.value_preds[t + 1] * st.masks[t + 1] - st.value_preds[t]
            gae = delta + gamma * lam * st.masks[t + 1] * gae
            if proper:
                gae = gae * st.bad_masks[t + 1]
            st.returns[t] = gae + st.value_preds[t]
    else:
        st.returns[-1] = next_value
        for t in reversed(range(T)):
            ret = st.returns[t + 1] * gamma * st.masks[t + 1] + st.rewards[t]
            if proper:
                ret = ret * st.bad_masks[t + 1] + (1 - st.bad_masks[t + 1]) * st.value_preds[t]
            st.returns[t] = ret


def returns_bytes(T, N, use_gae, proper, from_done):
    """Bytes one bpp_compute_returns call reads and writes (include/bpp_rollout.h; no advantages)."""
    per_step = 4 + 4                                   # rewards in, returns out
    per_step += 4 if (use_gae or proper) else 0        # value_preds in
    per_step += (1 + 4) if from_done else 4            # done in + masks out, or masks in
    per_step += 4 if proper else 0                     # bad_masks in
    return N * (T * per_step + 4 + 4)                  # + next_value in, row T of value_preds / returns out


def timed(fn, calls, batches, warmup):
    """Per-call microseconds of `batches` batches of `calls` back-to-back calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return out


def summary(us):
    return {"median_us": float(np.median(us)), "p10_us": float(np.percentile(us, 10)), "p90_us": float(np.percentile(us, 90)), "batches": len(us)}


def bench_returns(N, T, use_gae, proper, batches, dev):
    rng = np.random.RandomState(T)
    st = bpp_amd.RolloutStorage(T, N, (4,), bpp_amd.Discrete(4), device=dev)
    st.rewards.copy_(torch.from_numpy(rng.uniform(0, 2, (T, N, 1)).astype(np.float32)))
    st.value_preds.copy_(torch.from_numpy(rng.normal(0, 3, (T + 1, N, 1)).astype(np.float32)))
    done = torch.from_numpy((rng.uniform(size=(T, N)) < 0.2).astype(np.uint8)).to(dev)
    st.done.copy_(done)
    st.masks[1:].copy_((1.0 - done.float()).unsqueeze(-1))
    next_value = torch.from_numpy(rng.normal(0, 3, (N, 1)).astype(np.float32)).to(dev)
    gamma, lam = 0.99, 0.95
    cell = {"N": N, "T": T, "use_gae": bool(use_gae), "use_proper_time_limits": bool(proper)}
    # same bits first (the torch loop on the device rounds like the reference on the CPU: same IEEE operations, nothing fused)
    torch_returns(st, next_value, use_gae, gamma, lam, proper)
    want = st.returns.clone()
    st.returns.zero_()
    st.compute_returns(next_value, use_gae, gamma, lam, proper)
    rows = T if use_gae else T + 1
    cell["bit_identical_to_torch_loop"] = bool(torch.equal(st.returns[:rows].view(torch.int32), want[:rows].view(torch.int32)))
    runs = {"native_masks": lambda: st.compute_returns(next_value, use_gae, gamma, lam, proper),
            "torch_loop": lambda: torch_returns(st, next_value, use_gae, gamma, lam, proper)}
    samples = {k: [] for k in runs}
    samples["native_done"] = []
    for _ in range(batches):          # alternate the sides batch by batch
        st._from_done = [False] * T
        samples["native_masks"] += timed(runs["native_masks"], 200, 1, 20)
        st._from_done = [True] * T      # the zero-copy storage's path: masks derived from the step kernel's done bytes
        samples["native_done"] += timed(runs["native_masks"], 200, 1, 20)
        st._from_done = [False] * T
        samples["torch_loop"] += timed(runs["torch_loop"], 20, 1, 3)
    for k, v in samples.items():
        cell[k] = summary(v)
    for k, from_done in (("native_masks", False), ("native_done", True)):
        nbytes = returns_bytes(T, N, use_gae, proper, from_done)
        cell[k]["bytes"] = nbytes
        cell[k]["hbm_roofline_fraction"] = nbytes / HBM_PEAK / (cell[k]["median_us"] * 1e-6)
        cell[k]["speedup_over_torch_loop"] = cell["torch_loop"]["median_us"] / cell[k]["median_us"]
    return cell


def bench_lockstep(N, T, batches, dev):
    """One lock-step written into the storage (storage.step) against step_tensors + insert (nine copies), value and
    log-probability recorded on both sides, the action draw (the same on both sides) included."""
    size = (10, 10, 10)
    pool = bpp_amd.sequences.cut2_pool(size, 4096, seed=0)
    out = {"N": N, "T": T}
    value, logp = torch.zeros(N, 1, device=dev), torch.zeros(N, 1, device=dev)
    rnn = torch.zeros(N, 1, device=dev)
    envs = {k: bpp_amd.BppVecEnv(N, size, pool=pool, device=dev) for k in ("storage_step", "step_tensors_insert")}
    sts = {k: bpp_amd.RolloutStorage(T, e, e.observation_space.shape, e.action_space) for k, e in envs.items()}
    sts["storage_step"].reset(envs["storage_step"])
    sts["step_tensors_insert"].obs[0].copy_(envs["step_tensors_insert"].reset())
    acts = {k: torch.empty(N, dtype=torch.int64, device=dev) for k in envs}
    tick = {k: 0 for k in envs}

    def zero_copy():
        k = "storage_step"
        envs[k].sample_feasible(3, tick[k], out=acts[k])
        sts[k].step(envs[k], acts[k], value, logp)
        tick[k] += 1

    def with_insert():
        k = "step_tensors_insert"
        envs[k].sample_feasible(3, tick[k], out=acts[k])
        r = envs[k].step_tensors(acts[k])
        sts[k].insert(r.obs, rnn, acts[k].view(N, 1), logp, value, r.reward, r.masks, r.bad_masks, r.mask)
        tick[k] += 1

    samples = {"storage_step": [], "step_tensors_insert": []}
    for _ in range(batches):
        samples["storage_step"] += timed(zero_copy, 50, 1, 5)
        samples["step_tensors_insert"] += timed(with_insert, 50, 1, 5)
    for k, v in samples.items():
        out[k] = summary(v)
    out["speedup"] = out["step_tensors_insert"]["median_us"] / out["storage_step"]["median_us"]
    for e in envs.values():
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "returns_kernel.json"))
    ap.add_argument("--bins", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_returns.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "hbm_peak_bytes_per_s": HBM_PEAK,
           "method": "device events around batches of back-to-back calls (200 native, 20 torch loops, 50 lock-steps), sides alternated "
                     "batch by batch; median and 10th / 90th percentile of the per-call time over the batches",
           "returns": [], "lockstep": None}
    for T in (5, 32):
        for use_gae, proper in ((0, 0), (1, 1)):
            cell = bench_returns(args.bins, T, use_gae, proper, args.batches, dev)
            res["returns"].append(cell)
            print(json.dumps(cell), flush=True)
    res["lockstep"] = bench_lockstep(args.bins, 5, args.batches, dev)
    print(json.dumps(res["lockstep"]), flush=True)
    res["native_not_slower_in_any_cell"] = all(c[k]["median_us"] <= c["torch_loop"]["median_us"] for c in res["returns"]
                                               for k in ("native_masks", "native_done"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not res["native_not_slower_in_any_cell"]:
        raise SystemExit("the native call is slower than the torch loop in a cell")


if __name__ == "__main__":
    main()
