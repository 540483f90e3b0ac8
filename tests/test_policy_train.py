"""bpp_policy_trunk_forward_train / bpp_policy_trunk_backward (include/bpp_policy_train.h) and
bpp_amd.TrainablePolicy without a GPU: the product kernels of csrc/bpp_policy_train.inl compiled by g++ against the SIMT emulator.
Exact-integer networks bit for bit against int64 numpy (forward, every activation, every input gradient, every weight and bias
gradient); the training forward against the inference forward; real-valued networks against float64 torch autograd within 8 x
the error of float32 torch autograd; batch independence; the refusals of the header on the product library, which has no device
here; the packing of the second blob; the module's names and state-dict forms.  Helpers: tests/policy_train_cases.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from bpp_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_cases as pc  # noqa: E402
import policy_train_cases as tc  # noqa: E402

pol = pc.pol
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G10, G5 = (10, 256, 100), (5, 32, 25)


@pytest.fixture(scope="module")
def emu_lib(emu):
    import emu_binding
    csrc = os.path.join(ROOT, "online-3d-bpp-drl_amd", "csrc")
    if any(os.path.getmtime(os.path.join(csrc, f)) > os.path.getmtime(emu.LIB) for f in ("bpp_policy.inl", "bpp_policy_train.inl")):
        emu_binding.build(force=True)
    L = _lib.bind_policy_train(_lib.bind_policy(ctypes.CDLL(emu.LIB)))
    L.bpp_last_error.restype = ctypes.c_char_p
    return L


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.mark.parametrize("name", sorted(tc.EXACT_SPECS))
def test_exact_integer_networks_equal_int64_numpy_bit_for_bit(emu_lib, name):
    spec = tc.exact_spec(emu_lib, name)
    if name == "s5_three_splits":
        i = tc.info(emu_lib, tc.geom_of(5), spec["n"])
        assert i["splits"] == 3 and spec["n"] == 2 * i["bins_per_split"] + 1 and i["chain_rows"] == i["bins_per_split"] * 25
    tc.check_exact(tc.host_runner(emu_lib), tc.exact_case(**spec))


def test_the_shapes_of_the_exact_cases_are_what_their_names_say(emu_lib):
    assert tc.info(emu_lib, G10, 3)["bins_per_group"] == 2 and tc.exact_spec(emu_lib, "s10_nP1")["n"] == 3      # tile 3 straddles two bins
    assert tc.info(emu_lib, tc.geom_of(11), 3)["bins_per_group"] == 1
    i = tc.info(emu_lib, tc.geom_of(15), 2)
    assert i["grad_lds_bytes"] == 151296 and i["wgrad_lds_bytes"] <= 160 * 1024


@pytest.mark.parametrize("S,H,M,n", [(10, 256, 100, 5), (11, 32, 121, 3)])
def test_the_training_forward_leaves_the_bits_of_the_inference_forward(emu_lib, S, H, M, n):
    """feat against the head features bpp_policy_forward writes to its workspace, real-valued weights."""
    geom, A = (S, H, M), S * S
    blob = pol.pack_weights(pc.real_weights(S, H, M, 11), S, H, M).numpy()
    obs = pc.deep_states(False, n) if S == 10 else pc.synthetic_states(S, n)
    g = pc.geom_arg(geom)
    ws, logits = np.full(n * 20 * A, np.nan, np.float32), np.empty((n, M), np.float32)
    assert emu_lib.bpp_policy_forward(obs.ctypes.data, 4 * A, n, g, blob.ctypes.data, None, logits.ctypes.data, None, ws.ctypes.data, None) == 0
    feat, acts = np.full(n * 20 * A, np.nan, np.float32), np.full(5 * n * 64 * A, np.nan, np.float32)
    assert emu_lib.bpp_policy_trunk_forward_train(obs.ctypes.data, 4 * A, n, g, blob.ctypes.data, feat.ctypes.data, acts.ctypes.data, None) == 0
    assert pc.same_bits(feat, ws) and not np.isnan(acts).any() and (feat > 0).any()


@pytest.mark.parametrize("S,n", [(10, 16), (5, 70)])
def test_real_gradients_within_eight_times_the_float32_autograd_error(emu_lib, S, n):
    """Emulator, against float64 torch autograd over the same layers: 16 recorded states at 10 x 10, 70 synthetic states at 5 x 5
    (two splits).  Measured here: e_native / e_torch32 between 0.45 and 4.7 over every dW, every db and G1 (printed)."""
    obs = pc.deep_states(False, n) if S == 10 else pc.synthetic_states(S, n)
    if S == 5:
        assert tc.info(emu_lib, tc.geom_of(S), n)["splits"] == 2
    case = tc.real_case(S, obs)
    got = tc.host_runner(emu_lib)(case["obs"], case["geom"], case["blob"], case["blob_bwd"], case["grad_feat"])
    np.testing.assert_allclose(got["feat"].reshape(n, -1), case["ref64"]["feat"], rtol=0, atol=1e-5 * np.abs(case["ref64"]["feat"]).max())
    tc.check_real(got, case["ref64"], case["ref32"], "emulator, S = %d, n = %d:" % (S, n))


def test_a_bin_gives_the_same_gradient_rows_in_any_batch(emu_lib):
    """feat, acts and the G rows of a bin alone and as first / middle / last of 5 (5 x 5, real-valued)."""
    case = tc.real_case(5, pc.synthetic_states(5, 6))
    run = tc.host_runner(emu_lib)
    one = run(case["obs"][5:], case["geom"], case["blob"], case["blob_bwd"], case["grad_feat"][5:])
    for at in (0, 2, 4):
        obs, gf = case["obs"][:5].copy(), case["grad_feat"][:5].copy()
        obs[at], gf[at] = case["obs"][5], case["grad_feat"][5]
        got = run(obs, case["geom"], case["blob"], case["blob_bwd"], gf)
        for key in ("feat", "gf"):
            assert pc.same_bits(got[key][at], one[key][0]) and not pc.same_bits(got[key][(at + 1) % 5], one[key][0]), (key, at)
        for key in ("acts", "grads"):
            assert pc.same_bits(got[key][:, at], one[key][:, 0]) and not pc.same_bits(got[key][:, (at + 1) % 5], one[key][:, 0]), (key, at)


def test_refusals_come_before_any_device_is_looked_for(lib, emu_lib):
    A = 25
    obs, blob, wb = np.zeros((4, 103), np.float32), np.zeros(pol.TRUNK_FLOATS, np.float32), np.zeros(pol.TRUNK_BWD_FLOATS, np.float32)
    feat, acts, gfeat = np.zeros(4 * 20 * A, np.float32), np.zeros(5 * 4 * 64 * A, np.float32), np.zeros(4 * 20 * A, np.float32)
    grads, gw = np.zeros(4 * 340 * A, np.float32), np.zeros(pol.TRUNK_FLOATS, np.float32)

    def forward(L, g=G5, n=4, stride=100, null_geom=False, **null):
        p = dict(obs=obs, blob=blob, feat=feat, acts=acts)
        ptr = {k: None if k in null else v.ctypes.data for k, v in p.items()}
        return L.bpp_policy_trunk_forward_train(ptr["obs"], stride, n, None if null_geom else pc.geom_arg(g), ptr["blob"], ptr["feat"], ptr["acts"],
                                                None)

    def backward(L, g=G5, n=4, stride=100, null_geom=False, short=0, **null):
        p = dict(obs=obs, wb=wb, feat=feat, acts=acts, gfeat=gfeat, grads=grads, gw=gw, ws=ws)
        ptr = {k: None if k in null else v.ctypes.data for k, v in p.items()}
        return L.bpp_policy_trunk_backward(ptr["obs"], stride, n, None if null_geom else pc.geom_arg(g), ptr["wb"], ptr["feat"], ptr["acts"],
                                           ptr["gfeat"], ptr["grads"], ptr["gw"], ptr["ws"], ws.nbytes - short, None)

    ws = np.zeros(emu_lib.bpp_policy_trunk_backward_workspace(pc.geom_arg(G5), 4) // 4, np.float32)
    assert forward(emu_lib) == 0 and forward(emu_lib, stride=103) == 0 and backward(emu_lib) == 0 and backward(emu_lib, stride=103) == 0
    shared = [dict(null_geom=True), dict(n=0), dict(n=-1), dict(g=(0, 32, 0)), dict(g=(5, 32, 24)), dict(g=(5, 32, 75)), dict(stride=99),
              dict(stride=0), dict(g=(5, 48, 25)), dict(g=(16, 256, 256), stride=1024), dict(g=(20, 256, 400), stride=1600), dict(obs=None),
              dict(feat=None), dict(acts=None)]
    out = (ctypes.c_int32 * 8)()
    for L in (lib, emu_lib):            # the product library has no device here: it must refuse before it looks for one
        for b in shared + [dict(blob=None)]:
            assert forward(L, **b) == pc.BADARG, b
            assert L.bpp_last_error().decode().startswith("bpp_policy_trunk_forward_train: "), b
        for b in shared + [dict(wb=None), dict(gfeat=None), dict(grads=None), dict(gw=None), dict(ws=None), dict(short=4), dict(short=ws.nbytes)]:
            assert backward(L, **b) == pc.BADARG, b
            assert L.bpp_last_error().decode().startswith("bpp_policy_trunk_backward: "), b
        for g in ((20, 256, 400), (16, 256, 256), (5, 48, 25), (5, 32, 26), (0, 32, 0)):
            out[6] = 5
            assert L.bpp_policy_trunk_backward_info(pc.geom_arg(g), 4, out) == pc.BADARG and out[6] == 0
            assert L.bpp_policy_trunk_backward_workspace(pc.geom_arg(g), 4) == 0
            assert L.bpp_policy_trunk_backward_weights_floats(pc.geom_arg(g)) == 0
        assert L.bpp_policy_trunk_backward_info(pc.geom_arg(G5), 0, out) == pc.BADARG
        assert L.bpp_policy_trunk_backward_workspace(pc.geom_arg(G5), 0) == 0
        assert L.bpp_policy_trunk_backward_info(pc.geom_arg(G5), 4, None) == pc.BADARG
        assert L.bpp_policy_trunk_backward_info(None, 4, out) == pc.BADARG


def test_every_declared_symbol_is_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(_lib.POLICY_TRAIN_HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(bpp_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.POLICY_TRAIN_SYMBOLS) and not set(names) & set(_lib.POLICY_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.bpp_abi_version() == 16


def test_info_is_consistent_with_workspace(lib, emu_lib):
    for L in (lib, emu_lib):
        for g, n in ((G10, 1), (G10, 320), (G10, 2100), (G10, 65536), (G5, 81), ((15, 512, 225), 7), ((1, 32, 1), 3)):
            i, f = tc.info(L, g, n), pc.info(L, g, n)
            A = g[0] ** 2
            assert i["path"] == 1 and i["blocks"] == 1 + 4 * 10 + 2
            assert i["bins_per_group"] == f["bins_per_trunk_group"] and i["grad_lds_bytes"] == f["trunk_lds_bytes"]
            assert i["bins_per_split"] == max(1, min(64, 1024 // A)) and i["splits"] == -(-n // i["bins_per_split"])
            assert i["chain_rows"] == min(n, i["bins_per_split"]) * A and i["wgrad_lds_bytes"] <= 160 * 1024
            assert L.bpp_policy_trunk_backward_workspace(pc.geom_arg(g), n) == i["splits"] * i["blocks"] * 4 * 1024 * 4
            assert L.bpp_policy_trunk_backward_weights_floats(pc.geom_arg(g)) == pol.TRUNK_BWD_FLOATS == 4 * 576 * 64 + 20 * 64
        assert tc.info(L, G10, 65536)["bins_per_split"] == tc.info(L, G10, 1)["bins_per_split"]            # geom alone


def test_the_second_blob_and_the_gradient_views():
    plain = pc.real_weights(10, 256, 100, 4)
    wb = pol.pack_trunk_backward(plain)
    assert wb.numel() == pol.TRUNK_BWD_FLOATS
    w4 = plain["base.share.4.weight"]
    oc, c, i, j = 5, 7, 0, 2                                            # k' = oc * 9 + i' * 3 + j' holds W[oc][c][2 - i'][2 - j']
    assert wb[36864 + (oc * 9 + i * 3 + j) * 64 + c] == w4[oc, c, 2 - i, 2 - j]
    assert torch.equal(wb[147456:147456 + 64], plain["base.actor.0.weight"].reshape(8, 64)[0])
    assert torch.equal(wb[147456 + 16 * 64:147456 + 17 * 64], plain["base.critic.0.weight"].reshape(4, 64)[0])
    blob = pol.pack_trunk(plain)
    assert torch.equal(blob, pol.pack_weights(plain, 10, 256, 100)[:pol.TRUNK_FLOATS]) and blob.numel() == 151380
    back = pol.unpack_trunk_gradient(blob)                              # the gradient has the blob's layout
    assert sorted(back) == sorted(pol.TRUNK_PARAMETERS) and all(torch.equal(back[k], plain[k]) for k in back)


def test_policy_trunk_checks_its_tensors():
    import bpp_amd
    plain = pc.real_weights(10, 256, 100, 4)
    with pytest.raises(ValueError, match="with respect to obs"):
        bpp_amd.policy_trunk(torch.zeros(2, 400, requires_grad=True), plain, 10)
    with pytest.raises(RuntimeError, match="HIP device"):
        bpp_amd.policy_trunk(torch.zeros(2, 400), plain, 10)
    with pytest.raises(ValueError):
        bpp_amd.policy_trunk(torch.zeros(2, 1600), plain, 20)
    assert bpp_amd.policy_trunk is pol.policy_trunk and bpp_amd.TrainablePolicy is pol.TrainablePolicy


def test_the_module_carries_the_reference_names_and_loads_the_three_forms():
    import bpp_amd
    torch.manual_seed(2)
    net = bpp_amd.TrainablePolicy(10, 200)
    want = [n + k for n, _ in pol.layer_shapes(10, 256, 200) for k in (".weight", ".bias")]
    assert sorted(net.state_dict()) == sorted(want) == sorted(n for n, _ in net.named_parameters()) and "dist.linear.weight" in want
    for name, shape in pol.layer_shapes(10, 256, 200):
        assert tuple(net.state_dict()[name + ".weight"].shape) == tuple(shape)
    assert float(net.state_dict()["base.share.0.bias"].abs().max()) == 0.0          # the reference starts every bias at 0
    plain = pc.real_weights(10, 256, 200, 4)
    split = {}
    for k, v in plain.items():                                          # `<layer>.module.weight`, `<layer>.add_bias._bias` [C, 1]
        name, kind = k.rsplit(".", 1)
        split[name + (".module.weight" if kind == "weight" else ".add_bias._bias")] = v if kind == "weight" else v.reshape(-1, 1)
    for state in (plain, split, bpp_amd.kfac.plain_state_dict(split)):
        net = bpp_amd.TrainablePolicy(10, 200)
        result = net.load_state_dict(state)                             # nn.Module's result: nothing missing, nothing unexpected
        assert list(result.missing_keys) == [] and list(result.unexpected_keys) == []
        assert all(torch.equal(net.state_dict()[k], plain[k]) for k in plain)
    # NativePolicy.refresh takes the module: rollouts act on the weights being trained
    policy = bpp_amd.NativePolicy(10, 200).refresh(net)
    assert torch.equal(policy.weights, pol.pack_weights(plain, 10, 256, 200))
    obs = torch.from_numpy(pc.deep_states(True, 3))
    with torch.no_grad():                                               # on CPU tensors both run torch_forward
        assert all(torch.equal(a, b) for a, b in zip(net(obs), policy(obs)))
    with pytest.raises(RuntimeError, match="unexpected"):
        net.load_state_dict(dict(plain, **{"base.extra.weight": torch.zeros(1)}))
    assert list(net.load_state_dict(dict(plain, **{"base.extra.weight": torch.zeros(1)}), strict=False).unexpected_keys) == ["base.extra.weight"]
    with pytest.raises(ValueError):
        bpp_amd.TrainablePolicy(20, 400)
    with pytest.raises(ValueError, match="base.mask.5"):
        bpp_amd.TrainablePolicy(10, 200).load_state_dict({k: v for k, v in plain.items() if not k.startswith("base.mask.5")})
