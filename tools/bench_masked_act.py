#!/usr/bin/env python3
"""Timing of bpp_masked_act against the equivalent PyTorch ops of Policy.act
(acktr/model.py:56-68, acktr/distributions.py:71-84).  HBM-bound: reads 2 * 4M bytes per bin.

    python tools/bench_masked_act.py [bins]        (default 65 536)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bpp_amd

E = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
out = {}
for M in (100, 200, 400):
    x = torch.randn(E, M, device="cuda")
    m = (torch.rand(E, M, device="cuda") < 0.3).float()

    def fused(t):
        return bpp_amd.masked_act(x, m, seed=1, step=t)

    def eager(t):
        lx = torch.softmax(x - (1.0 - m) * 14.0, dim=-1) + 1e-5
        d = torch.distributions.Categorical(probs=lx)
        a = d.sample()
        return a.unsqueeze(-1), d.log_prob(a).unsqueeze(-1)

    res = {}
    for name, fn in (("fused_hip", fused), ("torch_eager", eager)):
        for t in range(5):
            fn(t)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(50)]
        for t, (a, b) in enumerate(evs):
            a.record()
            fn(t)
            b.record()
        torch.cuda.synchronize()
        ts = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
        res[name + "_us"] = round(sum(ts[5:-5]) / len(ts[5:-5]), 1)
    # the kernel alone: 200 launches back to back through the C ABI (no Python wrapper between them), one event pair -- the
    # figure rocprofv3's kernel stats agree with; `fused_hip_us` above is one WRAPPED call per event pair and is host-bound
    # below ~17 us
    import ctypes
    from bpp_amd import _lib
    L = _lib.lib()
    act = torch.empty((E, 1), dtype=torch.int64, device="cuda")
    lp = torch.empty((E, 1), dtype=torch.float32, device="cuda")
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for det in (0, 1):
        for t in range(20):
            L.bpp_masked_act(x.data_ptr(), m.data_ptr(), act.data_ptr(), lp.data_ptr(), E, M, 0, 1, t, det, sp)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for t in range(200):
            L.bpp_masked_act(x.data_ptr(), m.data_ptr(), act.data_ptr(), lp.data_ptr(), E, M, 0, 1, t, det, sp)
        e1.record()
        torch.cuda.synchronize()
        res["kernel_us_back_to_back_%s" % ("mode" if det else "sample")] = round(e0.elapsed_time(e1) / 200 * 1e3, 2)
    res["algorithmic_GBps_fused"] = round(E * (8 * M + 12) / (res["kernel_us_back_to_back_sample"] * 1e-6) / 1e9, 1)
    res["frac_of_8TBps"] = round(res["algorithmic_GBps_fused"] / 8000.0, 3)
    # training half: log-prob + entropy + invalid mass, forward and backward (acktr/model.py:90-96)
    a = torch.randint(0, M, (E,), device="cuda")
    adv = torch.randn(E, 1, device="cuda")
    xg = x.clone().requires_grad_(True)
    # its two kernels alone, as above: 200 launches back to back through the C ABI, one event pair
    outs = [torch.empty(E, device="cuda") for _ in range(3)]
    gw = [torch.randn(E, device="cuda") for _ in range(3)]
    grad = torch.empty_like(x)
    alone = {"evaluate": lambda: L.bpp_masked_evaluate(x.data_ptr(), m.data_ptr(), a.data_ptr(), *[o.data_ptr() for o in outs], E, M, sp),
             "evaluate_backward": lambda: L.bpp_masked_evaluate_backward(x.data_ptr(), m.data_ptr(), a.data_ptr(), *[g.data_ptr() for g in gw],
                                                                         grad.data_ptr(), E, M, sp)}
    for name, call in alone.items():
        for t in range(20):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for t in range(200):
            call()
        e1.record()
        torch.cuda.synchronize()
        res["kernel_us_back_to_back_%s" % name] = round(e0.elapsed_time(e1) / 200 * 1e3, 2)

    def fused_eval(t):
        xg.grad = None
        logp, ent, bad = bpp_amd.masked_evaluate(xg, m, a)
        (-(adv * logp).mean() - 0.01 * ent + 0.1 * bad).backward()

    def eager_eval(t):
        xg.grad = None
        d = torch.distributions.Categorical(probs=torch.softmax(xg - (1.0 - m) * 14.0, dim=-1) + 1e-5)
        bx = torch.softmax(xg, dim=-1) * (1.0 - m)
        (-(adv * d.log_prob(a).unsqueeze(1)).mean() - 0.01 * d.entropy().mean() + 0.1 * bx.mean()).backward()

    for name, fn in (("fused_hip_evaluate_fwd_bwd", fused_eval), ("torch_eager_evaluate_fwd_bwd", eager_eval)):
        for t in range(5):
            fn(t)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(30)]
        for t, (e0, e1) in enumerate(evs):
            e0.record()
            fn(t)
            e1.record()
        torch.cuda.synchronize()
        ts = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in evs)
        res[name + "_us"] = round(sum(ts[3:-3]) / len(ts[3:-3]), 1)
    out["M=%d" % M] = res
print(json.dumps({"E": E, "results": out}))
