"""bpp_policy_forward_one_image (include/bpp_policy_one_image.h) and bpp_amd.NativePolicy(form=) without a GPU:
the product kernel of csrc/bpp_policy_one_image.inl compiled by g++ against the SIMT emulator.  The same bits as the two-image
form wherever both accept the shape; exact-integer networks above side 15 bit for bit against int64 numpy; real-valued networks
at 20 x 20 and 22 x 22 against a float64 forward within 8 x the error of the float32 torch forward; batch independence; the form
`info` tells; the refusals of the header on the product library, which has no device here; the Python forms; the recorded chain
bits.  Helpers: tests/policy_one_image_cases.py, tests/policy_cases.py."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest

from bpp_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_cases as pc  # noqa: E402
import policy_one_image_cases as oc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G5, G10, G20 = (5, 32, 25), (10, 256, 100), (20, 256, 400)


@pytest.fixture(scope="module")
def emu_lib(emu):
    import emu_binding
    csrc = os.path.join(ROOT, "online-3d-bpp-drl_amd", "csrc")
    if max(os.path.getmtime(os.path.join(csrc, f)) for f in ("bpp_policy.inl", "bpp_policy_one_image.inl")) > os.path.getmtime(emu.LIB):
        emu_binding.build(force=True)
    L = _lib.bind_policy_one_image(_lib.bind_policy(ctypes.CDLL(emu.LIB)))
    L.bpp_last_error.restype = ctypes.c_char_p
    return L


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.mark.parametrize("spec", oc.SAME_BITS, ids=oc.case_id)
def test_the_same_bits_as_the_two_image_form(emu_lib, spec):
    """Real-valued weights on synthetic states: every head of bpp_policy_forward_one_image is bpp_policy_forward's, bit for bit."""
    oc.check_same_bits(oc.host_runner(emu_lib), pc.host_runner(emu_lib), spec)


def test_the_same_bits_for_every_subset_of_heads_and_a_padded_stride(emu_lib):
    one, two = oc.host_runner(emu_lib), pc.host_runner(emu_lib)
    blob = pc.pol.pack_weights(pc.real_weights(*G5, 11), *G5).numpy()
    obs = pc.synthetic_states(5, 3)
    full = two(obs, G5, blob)
    for k in (1, 2, 3):
        for want in itertools.combinations(pc.HEADS, k):
            got = one(obs, G5, blob, want)                                # the runner checks that the other heads stay untouched
            assert sorted(got) == sorted(want)
            for h in want:
                assert pc.same_bits(got[h], full[h]), (want, h)
    got = one(oc.padded(obs), G5, blob)
    for h in pc.HEADS:
        assert pc.same_bits(got[h], full[h]), h


@pytest.mark.parametrize("spec", oc.EXACT, ids=oc.case_id)
def test_exact_integer_networks_above_side_15_equal_int64_numpy_bit_for_bit(emu_lib, spec):
    pc.check_exact(oc.host_runner(emu_lib), pc.exact_case(*spec))


@pytest.mark.parametrize("geom", oc.REAL, ids=lambda g: "s%d_h%d_m%d" % tuple(g))
def test_real_networks_within_eight_times_the_float32_torch_error(emu_lib, geom):
    """Emulator, 16 synthetic states, against the float64 forward: e_native <= 8 e_torch32 per head (printed).  The first Linear
    of a head is a chain of 3 200 terms at S = 20 and 3 872 at S = 22."""
    case = oc.real_case(*geom)
    pc.check_real(oc.host_runner(emu_lib)(case["obs"], case["geom"], case["blob"]), case["ref64"], case["ref32"], "emulator, one image, %r:" % (geom,))


def test_a_bin_gives_the_same_bits_alone_and_in_a_batch_at_side_20(emu_lib):
    oc.check_batch_independence(oc.host_runner(emu_lib), G20)


def test_info_tells_the_form(lib, emu_lib):
    for L in (lib, emu_lib):
        i = oc.info(L, G10, 5)
        assert i["bins_per_trunk_group"] == 2 and i["trunk_lds_bytes"] == 77440 and i["tiles_per_wave"] == 2 and i["trunk_groups"] == 3
        assert oc.info(L, (11, 64, 121), 5)["bins_per_trunk_group"] == 1 and oc.info(L, (11, 64, 121), 5)["trunk_groups"] == 5
        i = oc.info(L, G20, 3)
        assert i["bins_per_trunk_group"] == 1 and i["trunk_lds_bytes"] == 128128 and i["tiles_per_wave"] == 4 and i["padded_rows"] == 416
        assert oc.info(L, (22, 32, 484), 1)["trunk_lds_bytes"] == 152064 and oc.info(L, (22, 32, 484), 1)["tiles_per_wave"] == 4
        assert oc.info(L, (12, 96, 144), 3)["tiles_per_wave"] == 2 and oc.info(L, (12, 96, 144), 3)["bins_per_trunk_group"] == 1
        assert oc.info(L, (17, 64, 578), 1)["tiles_per_wave"] == 3 and oc.info(L, G5, 1)["tiles_per_wave"] == 1
        for S in range(1, 23):
            for H, M in ((32, S * S), (512, 2 * S * S)):
                for n in (1, 2, 65, 2100):
                    i = oc.info(L, (S, H, M), n)
                    P, A = i["bins_per_trunk_group"], S * S
                    assert i["path"] == 2 and i["tile"] == 32 and P == (2 if S <= 10 else 1), (S, n)
                    assert i["trunk_groups"] == -(-n // P) and i["head_groups"] == 3 * -(-n // 64)
                    assert i["padded_rows"] % 32 == 0 and 0 <= i["padded_rows"] - P * A < 32
                    assert i["tiles_per_wave"] == -(-i["padded_rows"] // 128) <= 4
                    assert i["trunk_lds_bytes"] == (P * 64 * ((S + 2) ** 2 | 1) + 576 + i["padded_rows"]) * 4 <= (80 if P == 2 else 160) * 1024
                    assert 20 * A <= 64 * ((S + 2) ** 2 | 1)             # the head features fit the image they overwrite
                    assert L.bpp_policy_forward_one_image_workspace(pc.geom_arg((S, H, M)), n) == n * 20 * A * 4
                    floats = sum(int(np.prod(s)) + s[0] for _, s in pc.pol.layer_shapes(S, H, M))
                    assert L.bpp_policy_one_image_weights_floats(pc.geom_arg((S, H, M))) == floats
                    if S <= 15:
                        assert floats == L.bpp_policy_weights_floats(pc.geom_arg((S, H, M)))


def test_invalid_arguments_are_refused_before_any_device_is_touched(lib, emu_lib):
    obs, w, ws = np.zeros(4 * 1603, np.float32), np.zeros(1 << 20, np.float32), np.zeros(1 << 16, np.float32)
    v, lg, pr = np.zeros(8, np.float32), np.zeros(8 * 800, np.float32), np.zeros(8 * 800, np.float32)

    def call(L, g=G5, n=2, stride=100, o=obs, weights=w, value=v, logits=lg, pred=pr, work=ws, null_geom=False):
        p = [a.ctypes.data if a is not None else None for a in (o, weights, value, logits, pred, work)]
        return L.bpp_policy_forward_one_image(p[0], stride, n, None if null_geom else pc.geom_arg(g), p[1], p[2], p[3], p[4], p[5], None)

    assert call(emu_lib) == 0 and call(emu_lib, stride=103) == 0 and call(emu_lib, g=(5, 32, 50)) == 0
    bad = [dict(g=(23, 32, 529), stride=2116), dict(g=(0, 32, 0)), dict(g=(5, 48, 25)), dict(g=(5, 544, 25)), dict(g=(5, 32, 26)),
           dict(g=(20, 256, 401), stride=1600), dict(n=0), dict(n=-1), dict(stride=99), dict(g=G20, stride=1599),
           dict(o=None), dict(weights=None), dict(work=None), dict(null_geom=True), dict(value=None, logits=None, pred=None),
           dict(g=(-1, 32, 1)), dict(g=(5, 0, 25)), dict(g=(5, 16, 25)), dict(g=(5, 32, 75)), dict(g=(24, 32, 576), stride=2304)]
    out = (ctypes.c_int32 * 8)()
    for L in (lib, emu_lib):            # the product library has no device here: it must refuse before it looks for one
        for b in bad:
            assert call(L, **b) == pc.BADARG, b
            assert L.bpp_last_error().decode().startswith("bpp_policy_forward_one_image: "), (b, L.bpp_last_error())
        for g in ((23, 32, 529), (0, 32, 0), (5, 48, 25), (5, 544, 25), (5, 32, 26)):
            out[7] = 5
            assert L.bpp_policy_forward_one_image_info(pc.geom_arg(g), 4, out) == pc.BADARG and out[7] == 0
            assert L.bpp_last_error().decode().startswith("bpp_policy_forward_one_image_info: ")
            assert L.bpp_policy_forward_one_image_workspace(pc.geom_arg(g), 4) == 0
            assert L.bpp_policy_one_image_weights_floats(pc.geom_arg(g)) == 0
        out[7] = 5
        assert L.bpp_policy_forward_one_image_info(pc.geom_arg(G20), 0, out) == pc.BADARG and out[7] == 0
        assert L.bpp_policy_forward_one_image_workspace(pc.geom_arg(G20), 0) == 0
        assert L.bpp_policy_forward_one_image_info(pc.geom_arg(G20), 4, None) == pc.BADARG
        assert L.bpp_policy_forward_one_image_info(None, 4, out) == pc.BADARG and out[7] == 0
        assert L.bpp_policy_forward_one_image_info(pc.geom_arg((22, 512, 968)), 4, out) == 0 and out[7] == 2
        # the two-image entry points keep their refusals
        assert L.bpp_policy_forward_info(pc.geom_arg(G20), 4, out) == pc.BADARG and out[7] == 0
        assert L.bpp_policy_weights_floats(pc.geom_arg((16, 256, 256))) == 0


def test_every_declared_symbol_is_exported(lib, emu_lib):
    src = open(_lib.POLICY_ONE_IMAGE_HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(bpp_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.POLICY_ONE_IMAGE_SYMBOLS) and len(names) == 4
    for L in (lib, emu_lib):
        for n in names:
            assert hasattr(L, n), n
    assert lib.bpp_abi_version() == 16


def test_native_policy_takes_a_form():
    import torch
    import bpp_amd
    for form in ("one_image", "auto"):
        policy = bpp_amd.NativePolicy(20, 400, form=form)
        assert policy.form == form and policy.geom == G20
        assert policy.weights.numel() == sum(int(np.prod(s)) + s[0] for _, s in pc.pol.layer_shapes(20, 256, 400))
        plain = pc.real_weights(20, 256, 400, 4)
        back = policy.load_state_dict(plain).unpack()
        assert sorted(back) == sorted(plain) and all(torch.equal(back[k], plain[k]) for k in plain)
        assert torch.equal(policy.weights, pc.pol.pack_weights(plain, 20, 256, 400))
        assert bpp_amd.NativePolicy(22, 968, 512, form=form).weights.numel() > 0 and bpp_amd.NativePolicy(10, 100, form=form).form == form
        with pytest.raises(ValueError):
            bpp_amd.NativePolicy(23, 529, form=form)
        with pytest.raises(ValueError):
            bpp_amd.NativePolicy(0, 0, form=form)
    with pytest.raises(ValueError, match="form"):
        bpp_amd.NativePolicy(20, 400, form="bogus")
    with pytest.raises(ValueError, match="form"):
        bpp_amd.NativePolicy(10, 100, form="bogus")
    with pytest.raises(ValueError):
        bpp_amd.NativePolicy(20, 400)                                   # two images, as before
    with pytest.raises(ValueError):
        bpp_amd.NativePolicy(16, 256, form="two_images")
    assert pc.pol.MAX_SIDE_ONE_IMAGE == 22 and pc.pol.MAX_SIDE == 15
    assert [pc.pol.resolve_form("auto", S) for S in (1, 15, 16, 22)] == ["two_images", "two_images", "one_image", "one_image"]
    with pytest.raises(ValueError, match="form"):
        pc.pol.policy_forward(torch.zeros(2, 1600), torch.zeros(10), G20, form="bogus")
    # CPU tensors go through torch_forward whatever the form
    policy = bpp_amd.NativePolicy(20, 400, form="auto").load_state_dict(plain)
    obs = torch.from_numpy(pc.synthetic_states(20, 2))
    want = pc.pol.torch_forward(plain, obs)
    assert all(torch.equal(a, b) for a, b in zip(policy(obs), want))
    with pytest.raises(RuntimeError, match="HIP device"):
        bpp_amd.policy_forward(obs, policy.weights, policy.geom, form="one_image")


def test_forward_info_takes_a_form(lib):
    assert pc.pol.forward_info(G20, 3, form="one_image") == oc.info(lib, G20, 3) == pc.pol.forward_info(G20, 3, form="auto")
    assert pc.pol.forward_info(G10, 3, form="auto") == pc.info(lib, G10, 3) == pc.pol.forward_info(G10, 3)
    assert pc.pol.forward_info(G10, 3, form="one_image")["path"] == 2
    with pytest.raises(RuntimeError):
        pc.pol.forward_info(G20, 3)
    with pytest.raises(ValueError, match="form"):
        pc.pol.forward_info(G20, 3, form="bogus")


def test_the_recorded_chain_bits_are_what_the_emulator_computes(emu_lib):
    """tests/golden/mfma_chain_one_image_bits.npz (make_mfma_chain_one_image_bits.py) against the emulator as it is now: the
    fixture the device is compared with cannot drift from the code."""
    g = np.load(os.path.join(ROOT, "tests", "golden", oc.CHAIN_FIXTURE + ".npz"))
    for spec in oc.CHAIN_CASES:
        for key, v in oc.chain_entries(oc.host_runner(emu_lib), spec).items():
            assert g[key] == v, "%s: rerun tests/golden/make_mfma_chain_one_image_bits.py if the change is meant" % key
