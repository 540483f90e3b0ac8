"""bpp_kfac_factor and bpp_amd.KFACOptimizer on the device (include/bpp_kfac.h): the cases and checks of
tests/test_kfac.py through bpp_amd.kfac_factor -- here the MFMA itself runs --, the optimizer against the recorded reference run
of tests/golden/kfac_reference.npz, the hooks, and examples/train_with_storage.py --acktr.  Reads nothing of the reference."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfac_cases as kc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def bpp():
    import bpp_amd
    assert torch.cuda.is_available()
    return bpp_amd


@pytest.fixture(scope="module")
def example():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_with_storage as ex
    return ex


def chain_of(bpp, case):
    return kc.info(bpp._lib.lib(), case["layout"], kc.geom(case))["chain"]


@pytest.mark.parametrize("name", sorted(kc.EXACT))
def test_gpu_exact_integer_cases_equal_int64_numpy_bit_for_bit(bpp, name):
    kc.check_exact(kc.device_runner(DEV), kc.EXACT[name])


@pytest.mark.parametrize("name", sorted(kc.REAL) + ["rows_three_splits"])
def test_gpu_real_cases_within_the_derived_bound_symmetric_and_repeatable(bpp, name):
    case = kc.REAL[name]() if name in kc.REAL else kc.split_case(kc.info(bpp._lib.lib(), kc.ROWS, [1000, 40])["rows_per_split"])
    kc.check_real(kc.device_runner(DEV), case, chain_of(bpp, case))


def test_gpu_the_mfma_gives_the_bits_of_the_emulators_fmaf_chain(bpp):
    """tests/golden/mfma_chain_emulator_bits.npz: five real-valued factors, m after a first batch and after a second.  The
    inputs are regenerated here and their CRC32 compared first; then v_mfma_f32_32x32x2_f32 on the device against the sequential
    fmaf chain of the emulator, bit for bit.  The largest distance per case is printed in float32 ulps."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "mfma_chain_emulator_bits.npz"))
    for name in kc.CHAIN_CASES:
        got, _ = kc.chain_entries(kc.device_runner(DEV), name)
        for key in got:
            if ".crc." in key:
                assert got[key] == g[key], ("%s: the inputs regenerated here are not the bytes tests/golden/make_mfma_chain_bits.py "
                                            "drew (numpy's RandomState, not the kernel)" % key)
        dist = {k: kc.ulps(got[name + k], g[name + k]) for k in (".m1", ".m2")}
        print("%s: device against emulator, ulps: %r" % (name, dist))
        assert all(d == 0 for d in dist.values()), (name, dist)


def test_gpu_many_splits_and_a_strided_source(bpp):
    """More units than splits (several units per split, a partial last split) and a non-contiguous source."""
    r = np.random.RandomState(5)
    x = r.standard_normal((1100, 4, 6, 6)).astype(np.float32)
    case = dict(layout=kc.PATCH, conv=kc.conv_of(3, 1, 1), x=x, kind="conv_a", rho=0.95)
    case["scale"] = kc.reference_scale(case, "conv_a")
    i = kc.info(bpp._lib.lib(), kc.PATCH, kc.geom(case))
    assert i["splits"] < 1100 and i["rows_per_split"] == 2 * 36 and i["splits"] * i["rows_per_split"] >= i["R"]
    got = kc.device_runner(DEV)(case, x, np.zeros((36, 36), np.float32), True, case["scale"], 0.95)
    want, mag = kc.expected64(case, x, None, True, case["scale"], 0.95)
    assert np.all(np.abs(got - want) <= kc.bound(i["chain"], mag, None, True, 0.95))
    wide = torch.from_numpy(r.standard_normal((40, 2 * 70)).astype(np.float32)).to(DEV)
    view = wide[:, ::2]
    m = torch.zeros(70, 70, device=DEV)
    bpp.kfac_factor(view, "rows", m, 0.9, True, 1.0 / 40)
    m2 = torch.zeros(70, 70, device=DEV)
    bpp.kfac_factor(view.contiguous(), "rows", m2, 0.9, True, 1.0 / 40)
    assert torch.equal(m.view(torch.int32), m2.view(torch.int32))
    with pytest.raises(ValueError):
        bpp.kfac_factor(view, "rows", torch.zeros(70, 70), 0.9, True, 1.0)           # m on another device


def test_gpu_optimizer_against_the_recorded_reference(bpp):
    """Four steps across two eigendecompositions on the device; every step's parameter update within 8 x the sensitivity the
    reference showed against itself with float64 factors (recorded with the same method by tests/golden/make_kfac_golden.py)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "kfac_reference.npz"))
    weights = {k[len("w0."):]: g[k] for k in g.files if k.startswith("w0.")}
    batches = [{k: g["batch%d.%s" % (t, k)] for k in ("x", "action", "adv", "ret", "noise")} for t in range(kc.NET_STEPS)]
    ref_trail = [{k[len("params%d." % t):]: g[k] for k in g.files if k.startswith("params%d." % t)} for t in range(kc.NET_STEPS)]
    sens = g["factor_sensitivity"]
    made = []

    def make(net):
        made.append(bpp.KFACOptimizer(net, Tf=kc.NET_TF))
        return made[-1]

    ours, factors = kc.run_optimizer(make, weights, batches, device=DEV, record_factors=True)
    print("eigh on a host copy:", made[0].eigh_on_host)
    for k, v in factors.items():
        np.testing.assert_allclose(v, g["factors." + k], rtol=1e-4, atol=1e-6 * np.abs(g["factors." + k]).max(), err_msg=k)
        assert np.array_equal(kc.bits(v), kc.bits(v.T)), k
    dist = kc.update_distance(ours, ref_trail, weights)
    print("device against the recorded reference, per step:", dist, "sensitivity:", sens.tolist())
    assert all(d <= 8 * s for d, s in zip(dist, sens)), (dist, sens.tolist())


def test_gpu_hooks_take_statistics_only_when_the_reference_would(bpp):
    calls = []

    def spy(src, layout, m, stat_decay, first, scale, **conv):
        calls.append((layout, bool(first)))
        return bpp.kfac_factor(src, layout, m, stat_decay, first, scale, **conv)

    torch.manual_seed(0)
    net = kc.SmallNet().to(DEV)
    opt = bpp.KFACOptimizer(net, Ts=2, factor_fn=spy)
    x = torch.randn(6, 4, 5, 5, device=DEV)
    with torch.no_grad():
        net(x)
    assert calls == []                                                        # not under no_grad
    out = net(x)
    assert [c[0] for c in calls] == ["patch", "patch", "rows", "rows"] and all(c[1] for c in calls)
    del calls[:]
    out.sum().backward(retain_graph=True)
    assert calls == []                                                        # G only inside acc_stats
    opt.acc_stats = True
    out.sum().backward()
    opt.acc_stats = False
    assert sorted(c[0] for c in calls) == ["nchw", "nchw"] + ["rows"] * 6
    opt.step()
    del calls[:]
    net(x)
    assert calls == [] and opt.steps == 1                                     # not off a Ts step
    opt.steps = 2
    net(x)
    assert len(calls) == 4 and not any(c[1] for c in calls)


def test_gpu_example_trains_with_acktr(bpp, example, monkeypatch):
    made = []

    class Recorded(example.ActorCritic):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append((self, {n: v.clone() for n, v in self.state_dict().items()}))

    monkeypatch.setattr(example, "ActorCritic", Recorded)
    history = example.train(envs=64, steps=5, updates=2, acktr=True, verbose=False)
    assert len(history) == 2 and all(len(h) == 5 and np.isfinite(h).all() for h in history), history
    net, before = made[0]
    after = bpp.kfac.plain_state_dict(net.state_dict())
    assert sorted(after) == sorted(before)
    for name, v in before.items():
        now = after[name].cpu()
        assert torch.isfinite(now).all() and not torch.equal(now, v), name
    with pytest.raises(ValueError):
        example.train(envs=64, steps=5, updates=1, acktr=True, fused_loss=True, verbose=False)


@pytest.mark.parametrize("fused", [False, True])
def test_gpu_example_paths_without_the_flag_are_what_they_were(example, fused):
    """Same seed, a fresh run each: the terms of the first update come from the forward pass alone and are the same bits; the
    second update's follow an RMSprop step whose gradient sums need not be the same bits."""
    a = example.train(envs=64, steps=5, updates=2, fused_loss=fused, verbose=False)
    b = example.train(envs=64, steps=5, updates=2, fused_loss=fused, acktr=False, verbose=False)
    print(a, b)
    assert a[0] == b[0]
    np.testing.assert_allclose(a[1], b[1], rtol=1e-2, atol=1e-6)
