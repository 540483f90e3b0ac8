"""bpp_policy_trunk_forward_train / bpp_policy_trunk_backward (include/bpp_policy_train.h) and
bpp_amd.TrainablePolicy without a GPU: the product kernels of csrc/bpp_policy_train.inl compiled by g++ against the SIMT emulator.
Exact-integer networks bit for bit against int64 numpy (forward, every activation, every input gradient, every weight and bias
gradient); the training forward against the inference forward; real-valued networks against float64 torch autograd within 8 x
the error of float32 torch autograd; real-valued networks bit for bit against the header's arithmetic in numpy (tc.normative,
recorded in tests/golden/trunk_train_chain_bits.npz) and the split identity of grad_weights; stores outside the outputs; batch
independence; the refusals of the header on the product library, which has no device
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
    case = tc.exact_case(**spec)
    assert case["obs"].shape[1] == 4 * spec["S"] ** 2 + tc.EXACT_SPECS[name][4] and np.isnan(case["obs"][:, 4 * spec["S"] ** 2:]).all()
    tc.check_exact(tc.host_runner(emu_lib), case)


def test_the_shapes_of_the_exact_cases_are_what_their_names_say(emu_lib):
    assert tc.info(emu_lib, G10, 3)["bins_per_group"] == 2 and tc.exact_spec(emu_lib, "s10_nP1")["n"] == 3      # tile 3 straddles two bins
    assert tc.info(emu_lib, tc.geom_of(11), 3)["bins_per_group"] == 1
    i = tc.info(emu_lib, tc.geom_of(15), 2)
    assert i["grad_lds_bytes"] == 151296 and i["wgrad_lds_bytes"] <= 160 * 1024
    assert sorted(tc.EXACT_SPLITS) == sorted(k for k in tc.EXACT_SPECS if k.endswith("_splits"))
    for name, (splits, last) in tc.EXACT_SPLITS.items():                # every multi-split name: its splits and its last split's bins
        spec = tc.exact_spec(emu_lib, name)
        i = tc.info(emu_lib, tc.geom_of(spec["S"]), spec["n"])
        assert i["splits"] == splits and spec["n"] - (splits - 1) * i["bins_per_split"] == last, (name, i)
        assert i["chain_rows"] == i["bins_per_split"] * spec["S"] ** 2 and i["bins_per_split"] == tc.header_bins_per_split(spec["S"])
    for name in ("s2_three_splits", "s3_three_splits", "s4_two_splits"):        # the 64-bin cap on a split, with more than one split
        assert tc.info(emu_lib, tc.geom_of(tc.EXACT_SPECS[name][0]), 1)["bins_per_split"] == 64
    assert tc.exact_spec(emu_lib, "s10_two_splits")["n"] == 11 and tc.exact_spec(emu_lib, "s2_three_splits")["n"] == 129
    assert {tc.EXACT_SPECS[k][0] for k in tc.EXACT_SPECS} == set(range(1, 16))             # every side the header accepts
    assert sum(1 for k in tc.EXACT_SPECS if tc.EXACT_SPECS[k][4]) == 5                     # padded rows of obs
    i = tc.info(emu_lib, tc.geom_of(7), 3)
    assert i["bins_per_group"] == 2 and tc.exact_spec(emu_lib, "s7_nP1")["n"] == 3          # the last workgroup has one bin of its two


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


# ------------------------------------------------------------------------- the header's arithmetic, bit for bit (tc.normative)
def _fmaf():
    libm = ctypes.CDLL("libm.so.6")
    libm.fmaf.restype, libm.fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    return lambda a, b, c: np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)


def _boundary_triples():
    """Small-integer triples whose a * b + c lies at or one unit next to a float32 rounding boundary that float64 cannot tell
    from the boundary itself: c = +-m 2^e with m in [2^23, 2^24) and e = 2 h + 1, so that c's neighbours are 2^e apart and the
    boundary lies 2^(2 h) from c; a * b = (2^h + 1)(2^h - 1) = 2^(2 h) - 1 (one short of the boundary) or 2^h 2^h (on it), towards
    either neighbour.  h >= 16: the missing 1 is below half a unit of float64 at c.  Returns (a, b, c, next_to_a_boundary)."""
    rng = np.random.RandomState(3)
    rows = []
    for h in range(16, 24):
        for m in [2 ** 23, 2 ** 24 - 1] + list(rng.randint(2 ** 23, 2 ** 24, 14)):
            for sign_c in (1.0, -1.0):
                for sign_p in (1.0, -1.0):
                    rows.append((sign_p * (2.0 ** h + 1), 2.0 ** h - 1, sign_c * float(m) * 2.0 ** (2 * h + 1), True))
                    rows.append((sign_p * 2.0 ** h, 2.0 ** h, sign_c * float(m) * 2.0 ** (2 * h + 1), False))
    a, b, c, near = (np.array(v) for v in zip(*rows))
    f = lambda v: v.astype(np.float32)        # noqa: E731
    assert (f(a) == a).all() and (f(b) == b).all() and (f(c) == c).all()
    return f(a), f(b), f(c), near.astype(bool)


def test_fma32_is_libm_fmaf_on_random_triples_and_at_rounding_boundaries():
    fmaf = _fmaf()
    rng = np.random.RandomState(0)
    N = 100000
    a, b = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    c = (rng.standard_normal(N) * 10.0 ** rng.randint(-6, 3, N)).astype(np.float32)
    a[:N // 4], b[:N // 4] = rng.randint(1, 1 << 12, N // 4), rng.randint(1, 1 << 12, N // 4)
    c[:N // 4] = rng.randint(1, 1 << 24, N // 4).astype(np.float32) * np.float32(2.0) ** rng.randint(-30, 30, N // 4)
    c[N // 4:N // 2] = -(a[N // 4:N // 2] * b[N // 4:N // 2])                              # cancellation: the result is the product's own rounding error
    assert pc.same_bits(tc.fma32(a, b, c), fmaf(a, b, c))
    a, b, c, near = _boundary_triples()
    want = fmaf(a, b, c)
    assert pc.same_bits(tc.fma32(a, b, c), want)
    naive = (a.astype(np.float64) * b + c).astype(np.float32)            # rounds twice: to float64, then to float32
    wrong = naive.view(np.uint32) != want.view(np.uint32)
    print("float32(float64(a) * b + c) is wrong in %d of %d boundary triples" % (wrong.sum(), wrong.size))
    assert wrong[near].sum() >= near.sum() // 4 and not wrong[~near].any()            # the set is not too easy: double rounding fails it
    z = np.float32(0)
    assert pc.same_bits(tc.fma32(z, np.float32(-3), z), z) and pc.same_bits(tc.fma32(z, np.float32(3), np.float32(-0.0)), z)        # as fmaf: +0


@pytest.fixture(scope="module")
def chain_bits():
    return tc.load_fixture(tc.TRAIN_CHAIN_FIXTURE)


def test_the_recorded_chain_bits_hold_every_case_once(chain_bits):
    names = [tc.train_chain_name(S, n) for S, n in tc.TRAIN_CHAIN_CASES]
    want = ["%s.crc.%s" % (nm, k) for nm in names for k in tc.TRAIN_CHAIN_INPUTS] + \
           ["%s.%s.%s" % (nm, k, what) for nm in names for k in tc.OUTPUTS for what in ("crc", "sample")]
    assert sorted(chain_bits.files) == sorted(want)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", tc.TRAIN_CHAIN_FIXTURE + ".npz")) < 250000
    for S, n in tc.TRAIN_CHAIN_CASES:
        assert all(tc.sample_step(size) % 2 == 1 and -(-size // tc.sample_step(size)) <= tc.SAMPLE <= 4096
                   for size in (n * 20 * S * S, 5 * n * 64 * S * S, pol.TRUNK_FLOATS))


@pytest.mark.parametrize("S,n", [(5, 3), (3, 66)])
def test_the_recorded_chain_bits_are_the_reference_computed_now(chain_bits, S, n):
    """tc.normative live, about 1 s and 9 s: every recorded array of the case."""
    case = tc.train_chain_case(S, n)
    want = tc.normative(case["plain"], case["obs"], case["grad_feat"], S, tc.header_bins_per_split(S))
    for key, v in tc.train_chain_entries(case, want, tc.train_chain_name(S, n)).items():
        assert np.array_equal(chain_bits[key], v), key
    assert not np.isnan(want["gw"]).any() and min(float(np.abs(want[k]).max()) for k in tc.OUTPUTS) > 0


@pytest.mark.parametrize("S,n", sorted(tc.TRAIN_CHAIN_CASES))
def test_real_valued_chains_equal_the_headers_arithmetic_bit_for_bit(emu_lib, chain_bits, S, n):
    """Emulator: feat, acts, grads, gf' and grad_weights on real-valued data against the recorded bits of tc.normative."""
    splits, last, P = tc.TRAIN_CHAIN_CASES[(S, n)]
    i = tc.info(emu_lib, tc.geom_of(S), n)
    assert i["splits"] == splits and n - (splits - 1) * i["bins_per_split"] == last and i["bins_per_split"] == tc.header_bins_per_split(S)
    assert P is None or i["bins_per_group"] == P
    case, name = tc.train_chain_case(S, n), tc.train_chain_name(S, n)
    for k in tc.TRAIN_CHAIN_INPUTS:
        assert pc.crc(case[k]) == chain_bits["%s.crc.%s" % (name, k)], k
    got = tc.host_runner(emu_lib)(case["obs"], case["geom"], case["blob"], case["blob_bwd"], case["grad_feat"])
    tc.check_train_chain(got, chain_bits, name, "emulator:")


@pytest.mark.parametrize("S,n,splits", [(3, 150, 3), (10, 21, 3)])
def test_the_whole_batch_is_the_double_sum_of_its_splits(emu_lib, S, n, splits):
    i = tc.info(emu_lib, tc.geom_of(S), n)
    assert i["splits"] == splits and i["bins_per_split"] == tc.header_bins_per_split(S)
    differing = tc.check_split_identity(tc.host_runner(emu_lib), tc.train_chain_case(S, n), i["bins_per_split"])
    print("S = %d, n = %d: a float32 sum of the splits differs in %d floats" % (S, n, differing))


@pytest.mark.parametrize("name", ["s10_nP1", "s7_nP1", "s15_n2"])
def test_nothing_is_stored_outside_the_outputs(emu_lib, name):
    """Outputs and workspace carved out of guarded buffers (tc.guarded_buffers): guards and the workspace beyond the stated bytes
    untouched, every output float written, the bits of the plain runner."""
    case = tc.exact_case(**tc.exact_spec(emu_lib, name))
    got = tc.check_exact(tc.guarded_host_runner(emu_lib), case)
    plain = tc.host_runner(emu_lib)(case["obs"], case["geom"], case["blob"], case["blob_bwd"], case["grad_feat"])
    assert all(pc.same_bits(got[k], plain[k]) for k in tc.OUTPUTS)
