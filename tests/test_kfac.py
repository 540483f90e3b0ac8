"""bpp_kfac_factor (include/bpp_kfac.h) and bpp_amd.KFACOptimizer without a GPU: the product kernels of
csrc/bpp_kfac.inl compiled by g++ against the SIMT emulator, bound with _lib.bind_kfac.  Exact integer cases bit for bit against
int64 numpy; real-valued cases against float64 within the derived bound and against the live reference's compute_cov_a /
compute_cov_g / update_running_stat; the optimizer against the live reference's KFACOptimizer.  Helpers: tests/kfac_cases.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from bpp_amd import _lib
from oracle import ref_shims

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfac_cases as kc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not ref_shims.available(), reason="reference tree not present")


@pytest.fixture(scope="module")
def emu_lib(emu):
    import emu_binding
    inl = os.path.join(ROOT, "online-3d-bpp-drl_amd", "csrc", "bpp_kfac.inl")
    if os.path.getmtime(inl) > os.path.getmtime(emu.LIB):          # the emulator's own dependency list predates this file
        emu_binding.build(force=True)
    L = _lib.bind_kfac(ctypes.CDLL(emu.LIB))
    L.bpp_last_error.restype = ctypes.c_char_p
    return L


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def real_results(emu_lib):
    """(case, m after the first batch, m after the second) per real-valued case, computed once and never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            case = kc.REAL[name]() if name in kc.REAL else kc.split_case(kc.info(emu_lib, kc.ROWS, [1000, 40])["rows_per_split"])
            chain = kc.info(emu_lib, case["layout"], kc.geom(case))["chain"]
            cache[name] = (case,) + kc.check_real(kc.host_runner(emu_lib), case, chain)
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(kc.EXACT))
def test_exact_integer_cases_equal_int64_numpy_bit_for_bit(emu_lib, name):
    kc.check_exact(kc.host_runner(emu_lib), kc.EXACT[name])


@pytest.mark.parametrize("name", sorted(kc.REAL) + ["rows_three_splits"])
def test_real_cases_within_the_derived_bound_symmetric_and_repeatable(emu_lib, real_results, name):
    case, m1, m2 = real_results(name)
    i = kc.info(emu_lib, case["layout"], kc.geom(case))
    X = kc.rows64(case)
    assert (i["D"], i["R"], i["tile"]) == (X.shape[1], X.shape[0], 32) and i["chain"] <= i["rows_per_split"]
    assert (i["splits"] - 1) * i["rows_per_split"] < i["R"] <= i["splits"] * i["rows_per_split"]
    if name == "rows_three_splits":
        assert i["splits"] == 3 and i["R"] == 2 * i["rows_per_split"] + 1


def test_the_recorded_chain_bits_are_what_the_emulator_computes(emu_lib):
    """tests/golden/mfma_chain_emulator_bits.npz (make_mfma_chain_bits.py) against the emulator as it is now: the fixture the
    device is compared with cannot drift from the code."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "mfma_chain_emulator_bits.npz"))
    for name in kc.CHAIN_CASES:
        for key, v in kc.chain_entries(kc.host_runner(emu_lib), name)[0].items():
            assert np.array_equal(g[key], v), "%s: rerun tests/golden/make_mfma_chain_bits.py if the change is meant" % key


def _reference_factor(case, x, m0, first):
    """compute_cov_a / compute_cov_g and update_running_stat of the live reference on float32 tensors."""
    from acktr.algo import kfac as ref
    t = torch.from_numpy(np.array(x, copy=True))
    kind = case["kind"]
    if kind == "conv_a":
        c = case["conv"]
        aa = ref.compute_cov_a(t, "Conv2d", (c["kernel_size"], c["stride"], c["padding"]), False)
    elif kind == "conv_g":
        aa = ref.compute_cov_g(t, "Conv2d", None, False)
    elif kind == "linear_a":
        aa = ref.compute_cov_a(t, "Linear", None, False)
    else:
        aa = ref.compute_cov_g(t, "Linear", None, False)
    m = aa.clone() if first else torch.from_numpy(np.array(m0, copy=True))
    ref.update_running_stat(aa, m, case["rho"])
    return m.numpy()


@needs_reference
@pytest.mark.parametrize("name", sorted(kc.REAL))
def test_real_cases_against_the_live_reference_factors(emu_lib, real_results, name):
    """Within the sum of both sides' bounds.  The reference's side: R roundings of its dot products in whatever order, three
    of its scalings of the operands (kfac.py:38, :45 / :57, :62-63), six of the running average and its two constants."""
    ref_shims.install()
    case, m1, m2 = real_results(name)
    i = kc.info(emu_lib, case["layout"], kc.geom(case))
    ours, theirs = i["chain"], i["R"] + 3 + 6 - 3          # kc.bound adds 3 itself
    _, mag1 = kc.expected64(case, case["x"], None, True, case["scale"], case["rho"])
    r1 = _reference_factor(case, case["x"], None, True)
    assert np.all(np.abs(m1.astype(np.float64) - r1) <= kc.bound(ours, mag1, None, True, case["rho"]) + kc.bound(theirs, mag1, None, True, case["rho"]))
    _, mag2 = kc.expected64(case, case["x2"], m1, False, case["scale"], case["rho"])
    r2 = _reference_factor(case, case["x2"], m1, False)
    lim = kc.bound(ours, mag2, m1, False, case["rho"]) + kc.bound(theirs, mag2, m1, False, case["rho"])
    assert np.all(np.abs(m2.astype(np.float64) - r2) <= lim)


def test_torch_factor_is_the_same_expression(real_results):
    """The plain-torch routine for CPU tensors against the same float64 values (its own chain: R roundings)."""
    import bpp_amd
    for name in ("patch_d36", "nchw_d8", "rows_d100"):
        case, m1, _ = real_results(name)
        m = torch.full(m1.shape, float("nan"))
        bpp_amd.kfac.torch_factor(torch.from_numpy(case["x"]), case["layout"], m, case["rho"], True, case["scale"], **case.get("conv", {}))
        want, mag = kc.expected64(case, case["x"], None, True, case["scale"], case["rho"])
        assert np.all(np.abs(m.numpy().astype(np.float64) - want) <= kc.bound(kc.rows64(case).shape[0] + 3, mag, None, True, case["rho"]))


def test_invalid_arguments_are_refused_before_any_device_is_touched(lib, emu_lib):
    x, m, ws = np.zeros(4096, np.float32), np.zeros(4096, np.float32), np.zeros(1 << 16, np.float32)
    patch, rows, nchw = [2, 3, 7, 6, 3, 3, 2, 2, 0, 0], [4, 8], [2, 8, 16]

    def call(L, layout=kc.PATCH, g=patch, src=x, out=m, rho=0.5, work=ws, null_geom=False):
        return L.bpp_kfac_factor(src.ctypes.data if src is not None else None, layout, None if null_geom else kc.geom_arg(g),
                                 out.ctypes.data if out is not None else None, 1.0, rho, 1, work.ctypes.data if work is not None else None, None)

    for layout, g in ((kc.PATCH, patch), (kc.ROWS, rows), (kc.NCHW, nchw)):
        assert call(emu_lib, layout, g) == 0

    def changed(g, k, v):
        return g[:k] + [v] + g[k + 1:]

    bad = [dict(src=None), dict(out=None), dict(work=None), dict(null_geom=True), dict(layout=3), dict(layout=-1),
           dict(rho=0.0), dict(rho=1.0), dict(rho=-0.5), dict(rho=1.5), dict(rho=float("nan"))]
    bad += [dict(g=changed(patch, k, 0)) for k in range(8)]                     # B, C, H, W, kh, kw < 1; stride < 1
    bad += [dict(g=changed(patch, 6, -1)), dict(g=changed(patch, 8, -1))]
    bad += [dict(g=changed(patch, 4, 8)), dict(g=changed(patch, 5, 7))]         # kernel larger than the padded image
    bad += [dict(layout=kc.ROWS, g=[0, 8]), dict(layout=kc.ROWS, g=[4, 0]), dict(layout=kc.ROWS, g=[-1, 8])]
    bad += [dict(layout=kc.NCHW, g=[0, 8, 16]), dict(layout=kc.NCHW, g=[2, 0, 16]), dict(layout=kc.NCHW, g=[2, 8, 0])]
    out = (ctypes.c_int32 * 6)()
    for L in (lib, emu_lib):            # the product library has no device here: it must refuse before it looks for one
        for b in bad:
            assert call(L, **b) == kc.BADARG, b
            assert L.bpp_last_error().decode().startswith("bpp_kfac_factor: "), b
        for layout, g in ((3, rows), (kc.ROWS, [0, 8]), (kc.PATCH, changed(patch, 4, 8)), (kc.PATCH, changed(patch, 7, 0))):
            assert L.bpp_kfac_factor_info(layout, kc.geom_arg(g), out) == kc.BADARG and L.bpp_kfac_factor_workspace(layout, kc.geom_arg(g)) == 0
        assert L.bpp_kfac_factor_info(kc.ROWS, kc.geom_arg(rows), None) == kc.BADARG
        assert L.bpp_kfac_factor_info(kc.ROWS, None, out) == kc.BADARG


def test_every_declared_symbol_is_exported(lib):
    src = open(os.path.join(ROOT, "include", "bpp_kfac.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(bpp_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.KFAC_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.bpp_abi_version() == 16


def test_info_tells_the_tiles_and_the_splits(lib, emu_lib):
    for L in (lib, emu_lib):
        # the shipped layers at 5 x 65536 rows: every factor is cut into enough pieces to fill the device
        i = kc.info(L, kc.PATCH, [5 * 65536, 64, 10, 10, 3, 3, 1, 1, 1, 1])
        assert (i["D"], i["R"], i["tile"]) == (576, 5 * 65536 * 100, 32) and i["rows_per_split"] % 100 == 0
        assert 512 <= 45 * i["splits"] <= 1024 + 45
        i = kc.info(L, kc.PATCH, [5 * 65536, 4, 10, 10, 3, 3, 1, 1, 1, 1])
        assert i["D"] == 36 and 512 <= i["splits"] <= 1024
        i = kc.info(L, kc.ROWS, [5 * 65536, 800])
        assert i["D"] == 800 and 512 <= 91 * i["splits"] <= 1024 + 91 and i["rows_per_split"] % 64 == 0
        i = kc.info(L, kc.ROWS, [15, 800])
        assert (i["splits"], i["rows_per_split"], i["chain"]) == (1, 64, 15)
        i = kc.info(L, kc.NCHW, [3, 64, 100])
        assert (i["D"], i["R"], i["splits"], i["rows_per_split"], i["chain"]) == (64, 300, 6, 50, 50)       # S = 100: two chunks of 50
        for layout, g in ((kc.ROWS, [129, 40]), (kc.PATCH, [7, 64, 10, 10, 3, 3, 1, 1, 1, 1]), (kc.NCHW, [3, 64, 100])):
            i = kc.info(L, layout, g)
            assert L.bpp_kfac_factor_workspace(layout, kc.geom_arg(g)) == i["splits"] * (((i["D"] + 31) // 32) * ((i["D"] + 31) // 32 + 1) // 2) * 4096


def test_the_python_entry_point_checks_its_tensors():
    import bpp_amd
    m = torch.zeros(8, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        bpp_amd.kfac_factor(torch.zeros(4, 8), "rows", m, 0.99, True, 1.0)
    for src, layout, kw in ((torch.zeros(4, 8, dtype=torch.float64), "rows", {}), (torch.zeros(4, 8), "patch", {}), (torch.zeros(8), "rows", {}),
                            (torch.zeros(4, 8), "columns", {}), (torch.zeros(2, 3, 4, 4), "patch", dict(kernel_size=5)),
                            (torch.zeros(2, 3, 4, 4), "patch", dict(kernel_size=3, stride=0)), (torch.zeros(0, 8), "rows", {})):
        with pytest.raises(ValueError):
            bpp_amd.kfac_factor(src, layout, m, 0.99, True, 1.0, **kw)
    for bad_m in (torch.zeros(8, 7), torch.zeros(8, 8, dtype=torch.float64), torch.zeros(8, 16)[:, ::2]):
        with pytest.raises(ValueError):
            bpp_amd.kfac.torch_factor(torch.zeros(4, 8), "rows", bad_m, 0.99, True, 1.0)
    assert bpp_amd.kfac_factor is bpp_amd.kfac.kfac_factor and bpp_amd.KFACOptimizer is bpp_amd.kfac.KFACOptimizer


def test_checkpoint_names_are_the_reference_scheme():
    """Splitting the biases gives `<layer>.module.weight` / `<layer>.add_bias._bias` [n, 1] (what the reference's ACKTR run
    saves); plain_state_dict is main.py:70-75 and gives back the names and shapes of the unsplit model, so a checkpoint moves
    either way."""
    import bpp_amd
    torch.manual_seed(3)
    plain = kc.SmallNet()
    before = {k: v.clone() for k, v in plain.state_dict().items()}
    net = kc.SmallNet()
    net.load_state_dict(before)
    opt = bpp_amd.KFACOptimizer(net)
    names = sorted(net.state_dict())
    assert names == sorted(["%s.%s" % (n, s) for n in ("conv1", "conv2", "fc1", "fc2") for s in ("module.weight", "add_bias._bias")])
    assert tuple(net.state_dict()["conv1.add_bias._bias"].shape) == (8, 1)
    assert len(opt.modules) == 8 and [type(m).__name__ for m in opt.modules[:2]] == ["Conv2d", "AddBias"]
    back = bpp_amd.kfac.plain_state_dict(net.state_dict())
    assert sorted(back) == sorted(before) and all(torch.equal(back[k], before[k]) for k in before)
    plain.load_state_dict(back)
    x = torch.randn(5, 4, 5, 5)
    assert torch.allclose(plain(x), net(x), rtol=0, atol=1e-6)          # the bias is added in a step of its own now
    if ref_shims.available():           # and the live reference's own split gives the same names
        ref_shims.install()
        from acktr.algo.kfac import KFACOptimizer as RefKFAC
        other = kc.SmallNet()
        RefKFAC(other)
        assert sorted(other.state_dict()) == names
        other.load_state_dict(net.state_dict())


@needs_reference
def test_optimizer_against_the_live_reference(emu_lib):
    """Four steps across two eigendecompositions, identical weights, data and passes; the parameter UPDATE of every step within
    8 x the sensitivity the reference shows against itself with float64 factors -- once with the plain-torch factors, once
    with the emulated kernel.  (Sensitivity on this net, this CPU: see the printed figures.)"""
    import bpp_amd
    ref_shims.install()
    g = np.load(os.path.join(ROOT, "tests", "golden", "kfac_reference.npz"))
    weights = {k[len("w0."):]: g[k] for k in g.files if k.startswith("w0.")}
    batches = [{k: g["batch%d.%s" % (t, k)] for k in ("x", "action", "adv", "ret", "noise")} for t in range(kc.NET_STEPS)]
    trail, trail64, factors = kc.reference_runs(weights, batches)
    assert all(np.isfinite(v).all() for step in trail for v in step.values())
    sens = kc.update_distance(trail64, trail, weights)
    print("reference against itself with float64 factors, per step:", sens)
    for label, fn in (("torch", None), ("emulated kernel", kc.host_factor_fn(emu_lib))):
        ours, ours_factors = kc.run_optimizer(lambda net: bpp_amd.KFACOptimizer(net, Tf=kc.NET_TF, factor_fn=fn), weights, batches,
                                              record_factors=True)
        dist = kc.update_distance(ours, trail, weights)
        print(label, "against the reference, per step:", dist)
        for k in factors:
            np.testing.assert_allclose(ours_factors[k], factors[k], rtol=1e-4, atol=1e-6 * np.abs(factors[k]).max())
        assert all(d <= 8 * s for d, s in zip(dist, sens)), (label, dist, sens)


def test_hooks_take_statistics_only_when_the_reference_would():
    import bpp_amd
    calls = []

    def spy(src, layout, m, stat_decay, first, scale, **conv):
        calls.append((layout, bool(first)))
        return bpp_amd.kfac.torch_factor(src, layout, m, stat_decay, first, scale, **conv)

    torch.manual_seed(0)
    net = kc.SmallNet()
    opt = bpp_amd.KFACOptimizer(net, Ts=2, factor_fn=spy)
    x = torch.randn(6, 4, 5, 5)
    with torch.no_grad():
        net(x)
    assert calls == []
    out = net(x)
    assert [c[0] for c in calls] == ["patch", "patch", "rows", "rows"] and all(c[1] for c in calls)       # A of the four weight layers
    del calls[:]
    out.sum().backward(retain_graph=True)
    assert calls == []                                                        # no G outside acc_stats
    opt.acc_stats = True
    out.sum().backward()
    opt.acc_stats = False
    assert sorted(c[0] for c in calls) == ["nchw", "nchw"] + ["rows"] * 6
    opt.step()
    del calls[:]
    net(x)                                                                    # steps = 1, Ts = 2: off a Ts step
    assert calls == [] and opt.steps == 1
    opt.steps = 2
    net(x)
    assert len(calls) == 4 and not any(c[1] for c in calls)
