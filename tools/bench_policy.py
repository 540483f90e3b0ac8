#!/usr/bin/env python3
"""bpp_amd.NativePolicy (bpp_policy_forward) against the same network in plain torch layers on the device:
float32, no_grad, batch sizes 64 ... 65 536, rotation off and on, all three heads and logits only.

Method: device events around batches of back-to-back calls, the two forms alternated round by round, medians and p10-p90 over
the rounds.  TF/s is counted on the network's 2 * MAC (31.3 MFLOP per bin at 10 x 10, hidden 256, M = 100) whatever heads are
asked for, so logits-only reads higher than it is; the fraction is of the 155 TF the float32 matrix cores deliver.

Also measures, on 16 recorded states, the error of both forms against a float64 forward (tests/policy_cases.py: the tolerance
rule of the tests).

    python tools/bench_policy.py --out profiles/policy_forward.json
    python tools/bench_policy.py --emulator          # no device needed

--emulator measures the same errors for the kernels compiled for the SIMT emulator of the CPU tests (tests/emu) and merges
them into the file as `accuracy_on_the_emulator`; a device run keeps that block.

    python tools/bench_policy.py --forms --out profiles/policy_forward_forms.json

--forms compares the two forms of the native forward (form="two_images": bpp_policy_forward; form="one_image":
bpp_policy_forward_one_image, include/bpp_policy_one_image.h) by the same method, all forms of a row alternated in one run:
(a) S = 10, H = 256, M = 100: one image against two images against torch_forward; (b) S = 20, H = 256, M = 400, which only the
one-image form accepts: one image against torch_forward.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import bpp_amd
from bpp_amd import policy as pol

PEAK_TF = 155.0


def macs(S, H, M):
    A = S * S
    return A * (36 * 64 + 4 * 576 * 64 + 64 * 20) + 2 * 8 * A * H + 4 * A * H + 2 * H * M + H


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # microseconds per call


def summary(xs):
    xs = np.asarray(xs)
    return {"median_us": float(np.median(xs)), "p10_us": float(np.percentile(xs, 10)), "p90_us": float(np.percentile(xs, 90))}


def load(path):
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        return json.load(f)


def emulator_accuracy():
    import ctypes
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import emu_binding
    import policy_cases as pc
    L = bpp_amd._lib.bind_policy(ctypes.CDLL(emu_binding.build()))
    L.bpp_last_error.restype = ctypes.c_char_p
    out = {"note": "the product kernels compiled by g++ for the SIMT emulator (tests/emu), same 16 states and float64 reference"}
    for rot in (False, True):
        case = pc.real_case(rot)
        got = pc.host_runner(L)(case["obs"], case["geom"], case["blob"])
        out["rotation" if rot else "plain"] = {h: {"e_native": pc.rel_err(got[h], case["ref64"][h]),
                                                    "e_torch32_cpu": pc.rel_err(case["ref32"][h], case["ref64"][h])} for h in pol.HEADS}
    return out


FORMS_SHAPES = [((10, 256, 100), (64, 256, 2100, 16384, 65536), ("one_image", "two_images", "torch")),
                ((20, 256, 400), (64, 2100, 32768), ("one_image", "torch"))]


def bench_forms(args):
    """The --forms mode: per shape, batch size and set of heads one row with every form's median and p10 - p90."""
    import policy_cases as pc
    dev = torch.device("cuda:0")
    rows, info = [], {}
    for (S, H, M), sizes, forms in FORMS_SHAPES:
        plain = pc.real_weights(S, H, M, 11)
        native = {f: bpp_amd.NativePolicy(S, M, H, form=f).load_state_dict(plain).to(dev) for f in forms if f != "torch"}
        on_dev = {k: v.to(dev) for k, v in plain.items()}
        states = torch.from_numpy(pc.synthetic_states(S, 64)).to(dev)
        info["s%d" % S] = {f: pol.forward_info((S, H, M), 64, form=f) for f in native}
        for n in sizes:
            obs = states[torch.arange(n, device=dev) % states.shape[0]].contiguous()
            for want in (pol.HEADS, ("logits",)):
                def call(f):
                    if f == "torch":
                        with torch.no_grad():
                            pol.torch_forward(on_dev, obs, want)
                    else:
                        native[f](obs, want=want)

                calls = max(1, min(50, 20000 // n))
                for f in forms:                                                     # warm-up
                    timed(lambda: call(f), 2)
                times = {f: [] for f in forms}
                for r in range(args.rounds):
                    for k in range(len(forms)):                                     # the order rotates round by round
                        f = forms[(r + k) % len(forms)]
                        times[f].append(timed(lambda: call(f), calls))
                flop = 2.0 * macs(S, H, M) * n
                row = {"S": S, "H": H, "M": M, "n": n, "heads": "all" if len(want) == 3 else "logits", "calls_per_round": calls, "rounds": args.rounds}
                for f in forms:
                    row[f] = dict(summary(times[f]), tflops=flop / float(np.median(times[f])) * 1e-6)
                row["one_image_over_torch"] = row["one_image"]["median_us"] / row["torch"]["median_us"]
                if "two_images" in forms:
                    row["one_image_over_two_images"] = row["one_image"]["median_us"] / row["two_images"]["median_us"]
                rows.append(row)
                print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "mflop_per_bin": {"s%d" % g[0]: 2e-6 * macs(*g) for g, _, _ in FORMS_SHAPES},
           "method": "device events around `calls_per_round` back-to-back calls, the forms of a row alternated (the order rotates), `rounds` rounds; "
                     "float32, no_grad; TF/s on the network's 2 * MAC whatever heads are asked for",
           "forward_info_at_n64": info, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,2100,16384,65536")
    ap.add_argument("--forms", action="store_true", help="compare the one-image and two-image forms of the native forward (see above)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_forward.json"))
    ap.add_argument("--emulator", action="store_true", help="measure the emulated kernels' error on the CPU and merge it into --out")
    args = ap.parse_args()
    if args.emulator:
        out = load(args.out)
        out["accuracy_on_the_emulator"] = emulator_accuracy()
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out["accuracy_on_the_emulator"]))
        return
    if args.forms:
        bench_forms(args)
        return
    dev = torch.device("cuda:0")
    import policy_cases as pc
    rows, accuracy = [], {}
    for rot in (False, True):
        S, H, M = 10, 256, 200 if rot else 100
        case = pc.real_case(rot)
        policy = bpp_amd.NativePolicy(S, M, H).load_state_dict(case["plain"]).to(dev)
        plain = {k: v.to(dev) for k, v in case["plain"].items()}
        states = torch.from_numpy(pc.deep_states(rot, 64)).to(dev)
        with torch.no_grad():
            got = {h: t.cpu().numpy() for h, t in zip(pol.HEADS, policy(torch.from_numpy(case["obs"]).to(dev)))}
            dev32 = {h: t.cpu().numpy() for h, t in zip(pol.HEADS, pol.torch_forward(plain, torch.from_numpy(case["obs"]).to(dev)))}
        accuracy["rotation" if rot else "plain"] = {
            h: {"e_native": pc.rel_err(got[h], case["ref64"][h]), "e_torch32_cpu": pc.rel_err(case["ref32"][h], case["ref64"][h]),
                "e_torch32_device": pc.rel_err(dev32[h], case["ref64"][h])} for h in pol.HEADS}
        for n in (int(v) for v in args.sizes.split(",")):
            obs = states[torch.arange(n, device=dev) % states.shape[0]].contiguous()
            for want in (pol.HEADS, ("logits",)):
                def native():
                    policy(obs, want=want)

                def layers():
                    with torch.no_grad():
                        pol.torch_forward(plain, obs, want)

                calls = max(1, min(50, 20000 // n))
                for fn in (native, layers):                                         # warm-up
                    timed(fn, 2)
                t_native, t_torch = [], []
                for r in range(args.rounds):
                    for fn, acc in ((native, t_native), (layers, t_torch)) if r % 2 == 0 else ((layers, t_torch), (native, t_native)):
                        acc.append(timed(fn, calls))
                flop = 2.0 * macs(S, H, M) * n
                a, b = summary(t_native), summary(t_torch)
                row = {"n": n, "rotation": rot, "heads": "all" if len(want) == 3 else "logits", "calls_per_round": calls, "rounds": args.rounds,
                       "native": a, "torch": b, "native_over_torch": a["median_us"] / b["median_us"],
                       "native_tflops": flop / a["median_us"] * 1e-6, "native_fraction_of_155tf": flop / a["median_us"] * 1e-6 / PEAK_TF,
                       "torch_tflops": flop / b["median_us"] * 1e-6}
                rows.append(row)
                print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "mflop_per_bin_plain": 2e-6 * macs(10, 256, 100),
           "method": "device events around `calls_per_round` back-to-back calls, forms alternated, `rounds` rounds; float32, no_grad, eval",
           "accuracy_vs_float64_on_16_recorded_states": accuracy, "rows": rows}
    kept = load(args.out).get("accuracy_on_the_emulator")
    if kept is not None:
        out["accuracy_on_the_emulator"] = kept
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
