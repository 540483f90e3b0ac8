#!/usr/bin/env python3
"""Rates of the CUT-1 and RS stream kinds (include/bpp_stream_kinds.h) beside the CUT-2 counter stream and the static pools
of the same kinds (tools, not the benchmark): env steps/s of rollout_uniform, and the time of one refill call from HIP events
as a function of the sequences every bin needs.  All configurations live in one process and take turns repeat by repeat, so
that a drift of the machine hits them alike; reported are the median and the extremes of the repeats.  Writes
profiles/stream_kinds.json.
usage: bench_stream_kinds.py [--envs 65536] [--depth 32] [--refill-every 14] [--steps 1500] [--warmup 300] [--reps 5]
                             [--needs 1 2 4] [--out profiles/stream_kinds.json]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bpp_amd  # noqa: E402

SIZE = (10, 10, 10)


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--depth", type=int, default=32)
    ap.add_argument("--refill-every", type=int, default=14)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--needs", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_kinds.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_kinds.py measures on the GPU; there is none here")
    E = args.envs
    ring = dict(seed=0, depth=args.depth, refill_every=args.refill_every)
    make = {
        "stream_cut1": lambda: bpp_amd.BppVecEnv(E, SIZE, stream=dict(ring, kind="cut1")),
        "stream_rs": lambda: bpp_amd.BppVecEnv(E, SIZE, stream=dict(ring, kind="rs")),
        "stream_cut2_counter": lambda: bpp_amd.BppVecEnv(E, SIZE, stream=dict(ring, bound=(2, 5), rng="counter")),
        "pool_cut1": lambda: bpp_amd.BppVecEnv(E, SIZE, pool=bpp_amd.factory.make_pool(SIZE, "cut1")),
        "pool_rs": lambda: bpp_amd.BppVecEnv(E, SIZE, pool=bpp_amd.factory.make_pool(SIZE, "rs")),
    }
    envs = {name: f() for name, f in make.items()}
    step = {name: 0 for name in envs}

    def run(name, n):
        envs[name].rollout_uniform(1, step[name], n)
        step[name] += n
    for name, env in envs.items():
        env.reset()
        run(name, args.warmup)
    torch.cuda.synchronize()
    rates = {name: [] for name in envs}
    for _ in range(args.reps):
        for name in envs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, args.steps)
            torch.cuda.synchronize()
            rates[name].append(E * args.steps / (time.perf_counter() - t0))
    out = {"size": list(SIZE), "envs": E, "depth": args.depth, "refill_every": args.refill_every, "steps": args.steps, "warmup": args.warmup,
           "knobs": bpp_amd._lib.get_knobs(), "device": torch.cuda.get_device_name(0),
           "env_steps_per_s": {name: spread(v) for name, v in rates.items()}, "refill_us": {}}
    # one refill call, every bin `need` episodes on (bench_stream_refill.py's method), HIP events on the launch stream
    for name in ("stream_cut1", "stream_rs", "stream_cut2_counter"):
        env = envs[name]
        out["refill_us"][name] = {}
        for need in args.needs:
            ts = []
            for _ in range(args.reps + 1):
                env.state[:, 1] += need                 # bpp_env_state.episode
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                env.refill()
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            out["refill_us"][name][str(need)] = spread([round(t, 1) for t in ts[1:]])
        assert int(env.stream_overflow.item()) == 0
    base = out["env_steps_per_s"]["stream_cut2_counter"]["median"]
    out["relative_to_cut2_counter_stream"] = {n: round(out["env_steps_per_s"][n]["median"] / base, 3) for n in ("stream_cut1", "stream_rs")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
