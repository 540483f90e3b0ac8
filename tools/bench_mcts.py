#!/usr/bin/env python3
"""Time one batched MCTS decision (MCTSearch.decide + the real step + advance) with a stand-in policy or the CNN as the forward.

    python tools/bench_mcts.py [--n 256 2100 16384] [--sims 100] [--k 4] [--decisions 3] [--checkpoint default_cut_2.pt] [--out FILE]

Prints one JSON object: per policy and n, the µs per decision (median over the timed decisions, host included) and
decisions/s.  10x10x10 bins, CUT-2 pool, real bins [0, n), scratch bins [n, 2n).  Policies: the fixtures' flat policy,
and with --checkpoint also the reference's CNN (examples/multibin_checkpoint.py's ActorCritic) as the forward."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import numpy as np
    import torch
    import bpp_amd
    from bpp_amd.mcts import flat_policy
    size = (10, 10, 10)
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[256, 2100, 16384])
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--decisions", type=int, default=3)
    ap.add_argument("--checkpoint")
    ap.add_argument("--out")
    a = ap.parse_args()
    policies = [("flat", lambda: flat_policy(size))]
    if a.checkpoint:
        sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
        from multibin_checkpoint import load_actor_critic
        net = load_actor_critic(a.checkpoint, 10, 100, torch.device("cuda"))

        def cnn(obs):
            with torch.no_grad():
                v, lg = net(obs)
            return v, lg, None
        policies.append(("cnn", lambda: cnn))
    pool = bpp_amd.sequences.cut2_pool(size, 4096, seed=0)
    res = {"size": size, "sims": a.sims, "k": a.k, "runs": []}
    for name, n in [(p, n) for p, _ in policies for n in a.n]:
        env = bpp_amd.BppVecEnv(2 * n, container_size=size, pool=pool, device="cuda", compute_mask=False)
        env.reset()
        ms = bpp_amd.MCTSearch(env, a.k, sim_times=a.sims)
        pol = dict(policies)[name]()
        ids = torch.arange(n, device="cuda")
        times = []
        for d in range(a.decisions + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            act, vis = ms.decide(pol, ids, ids + n, check=False)
            r = env.step_bins(ids, act, check=False)
            ms.advance(r.done)
            torch.cuda.synchronize()
            if d:                                    # the first decision allocates the work buffers
                times.append(time.perf_counter() - t0)
        us = float(np.median(times)) * 1e6
        run = {"policy": name, "n": n, "us_per_decision": round(us, 1), "decisions_per_s": round(n / us * 1e6, 1),
               "state_GB": round(ms.nbytes / 1e9, 2), "overflow": int(ms.overflow.item())}
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
        del ms, env
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
