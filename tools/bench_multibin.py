#!/usr/bin/env python3
"""Time native multi-bin packing (online-3d-bpp-drl_amd/multibin.py) on 20x20x10 pallets of the 4-bin set, w = s = 10
(K = 4), with the int64-exact stand-in policy of the fixtures (bpp_amd.reorder.int_policy, its unused feasibility input a
constant) between emit and choose.  Writes profiles/multibin_bench.json.

    python tools/bench_multibin.py [--ns 2100 16384 65536] [--reps 20] [--out profiles/multibin_bench.json]
    python tools/bench_multibin.py --stats KERNEL_STATS_CSV_OR_DB [--out ...]   merge a rocprofv3 --kernel-trace --stats run

Per n: the wall time of one decision (decide + step_tensors + commit, enqueued back to back, synchronised once at the
end), of decide alone, and of the same decision composed from batched_window_masks and torch ops (for context; that path
keeps no history: it only scores the windows).  --stats adds per-kernel average times, the bytes each kernel must move
per call for n = 65 536 and the fraction of 8 TB/s that makes."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bpp_amd  # noqa: E402
from bpp_amd.reorder import int_policy  # noqa: E402

SIZE, W_, S_ = (20, 20, 10), 10, 10


def policy_of(w, H):
    return int_policy((w, w, H), mask_fn=lambda obs: torch.zeros((obs.shape[0], w * w), dtype=torch.float32, device=obs.device))


def make_env(n):
    pool = bpp_amd.sequences.from_dataset(os.path.join(ROOT, "tests", "golden", "cut2_dataset_4bins_20x20x10.npz"), SIZE,
                                          terminator=(20, 20, 10))
    env = bpp_amd.BppVecEnv(n, SIZE, pool=pool, device="cuda")
    env.reset()
    return env


def torch_decide(env, policy, w, s):
    """One decision's scoring composed from batched_window_masks and torch ops: window rows, masks, forward, softmax,
    masked first argmax, the -0.2 / skip rule (no history) and the first best window."""
    E, (W, L, H) = env.E, SIZE
    hm = env.heightmaps()
    it = env.state[:, 8]
    items = torch.stack([it & 255, (it >> 8) & 255, (it >> 16) & 255], 1)
    masks, offs = bpp_amd.batched_window_masks(hm, items, (w, w, H), stride=s)
    K = masks.shape[1]
    wins = torch.stack([hm[:, dx:dx + w, dy:dy + w].reshape(E, w * w) for dx, dy in offs.tolist()], 1).float()
    rows = torch.cat([wins[:, :, None, :], items[:, None, :, None].float().expand(E, K, 3, w * w)], 2).reshape(E * K, 4 * w * w)
    value, logits, _ = policy(rows)
    poss = torch.softmax(logits, 1).view(E, K, -1) * masks
    pos = poss.argmax(-1)
    skip = masks.sum(-1) == w * w
    adv = torch.where(skip, torch.full_like(value.view(E, K), -1e8, dtype=torch.float64), torch.full((E, K), -0.2, dtype=torch.float64, device=hm.device))
    best = adv.argmax(1)
    p = pos.gather(1, best[:, None])[:, 0]
    o = offs.to(hm.device)[best]
    return (o[:, 0] + p // w) * L + o[:, 1] + p % w


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def run(n, reps):
    env = make_env(n)
    mb = bpp_amd.MultiBinPacker(env, W_, S_)
    policy = policy_of(W_, SIZE[2])

    def decision():
        act, _, _ = mb.decide(policy, check=False)
        mb.commit(env.step_tensors(act).done)

    t_dec = timed(decision, reps)
    t_decide = timed(lambda: mb.decide(policy, check=False), reps)
    t_torch = timed(lambda: torch_decide(env, policy, W_, S_), max(3, reps // 4))
    return dict(n=n, size=list(SIZE), w=W_, s=S_, K=mb.K, decision_us=t_dec * 1e6, decisions_per_s=n / t_dec,
                decide_us=t_decide * 1e6, torch_composed_scoring_us=t_torch * 1e6, policy="int_policy")


def kernel_bytes(n, K=4, w=W_, A=SIZE[0] * SIZE[1]):
    """Bytes a call must move for n slots (reads + writes of the kernel's own buffers, 20x20 pallets, w = 10)."""
    w2, ms = w * w, (w * w + 15) // 16 * 16
    return {"multibin_emit_kernel": n * (8 + A + 4 + K * 16 * w2 + K * ms + 16),
            "multibin_choose_kernel": n * (16 + K * ms + K * 4 * w2 + K * 4 + K * 24 + 8 + 8 + 8 + 4 + 4),
            "multibin_commit_kernel": n * (16 + 1 + 24 + 4)}


def merge_stats(path, out):
    doc = json.load(open(out)) if os.path.exists(out) else dict(rows=[])
    rows = []
    if path.endswith(".db"):            # rocprofv3's rocpd database: top_kernels(name, total_calls, total_duration, average [us])
        import sqlite3
        recs = [dict(Name=n, Calls=c, AverageNs=a * 1e3) for n, c, a in
                sqlite3.connect(path).execute("select name, total_calls, average from top_kernels")]
    else:
        recs = list(csv.DictReader(open(path)))
    for r in recs:
        name = r.get("Name") or r.get("KernelName") or ""
        for k, b in kernel_bytes(65536).items():
            if k in name:
                avg = float(r.get("AverageNs") or r.get("Average") or 0)
                rows.append(dict(kernel=k, calls=int(r.get("Calls", 0)), avg_us=avg / 1e3, bytes_per_call=b,
                                 tb_per_s=b / (avg * 1e-9) / 1e12, fraction_of_8tbps=b / (avg * 1e-9) / 8e12))
    doc["kernels_n65536"] = rows
    doc["kernels_note"] = ("rocprofv3 --kernel-trace --stats of a run at n = 65 536 only; bytes are the minimum each kernel "
                           "must read and write, not measured traffic")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(rows, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, nargs="+", default=[2100, 16384, 65536])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multibin_bench.json"))
    ap.add_argument("--stats")
    a = ap.parse_args()
    if a.stats:
        merge_stats(a.stats, a.out)
        return
    rows = []
    for n in a.ns:
        r = run(n, a.reps)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
