"""bpp_policy_forward (include/bpp_policy.h) and bpp_amd.NativePolicy without a GPU: the product kernels of
csrc/bpp_policy.inl compiled by g++ against the SIMT emulator, bound with _lib.bind_policy.  Exact-integer networks bit for bit
against int64 numpy at the shipped shapes and across the accepted ones (S = 1 .. 15, H = 32 .. 512); real-valued networks against a
float64 forward within 8 x the error of the float32 torch forward; batch independence; the recorded chain bits; optional heads; the refusals of the header on the product library, which has no device here; the three
state-dict forms; the live reference's own Policy.  Helpers: tests/policy_cases.py."""
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
import policy_cases as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not ref_shims.available(), reason="reference tree not present")
G10, G5 = (10, 256, 100), (5, 32, 25)


@pytest.fixture(scope="module")
def emu_lib(emu):
    import emu_binding
    inl = os.path.join(ROOT, "online-3d-bpp-drl_amd", "csrc", "bpp_policy.inl")
    if os.path.getmtime(inl) > os.path.getmtime(emu.LIB):
        emu_binding.build(force=True)
    L = _lib.bind_policy(ctypes.CDLL(emu.LIB))
    L.bpp_last_error.restype = ctypes.c_char_p
    return L


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def tiles(emu_lib):
    i = pc.info(emu_lib, G10, 1)
    return i["bins_per_trunk_group"], i["bins_per_head_tile"]


@pytest.fixture(scope="module")
def real_results(emu_lib):
    """(case, emulated outputs) per rotation, computed once and never modified."""
    cache = {}

    def get(rot):
        if rot not in cache:
            case = pc.real_case(rot)
            cache[rot] = (case, pc.host_runner(emu_lib)(case["obs"], case["geom"], case["blob"]))
        return cache[rot]
    return get


@pytest.mark.parametrize("name", sorted(pc.exact_specs(2, 64)))
def test_exact_integer_networks_equal_int64_numpy_bit_for_bit(emu_lib, tiles, name):
    spec = pc.exact_specs(*tiles, bins=lambda g: pc.info(emu_lib, g, 1)["bins_per_trunk_group"])[name]
    pc.check_exact(pc.host_runner(emu_lib), pc.exact_case(*spec))


def test_info_tells_one_bin_per_trunk_group_from_side_11_on(lib, emu_lib):
    for L in (lib, emu_lib):
        for S in range(1, 16):
            for H, M in ((32, S * S), (512, 2 * S * S)):
                i = pc.info(L, (S, H, M), 3)
                assert i["bins_per_trunk_group"] == (2 if S <= 10 else 1), S
                assert i["trunk_lds_bytes"] <= 160 * 1024 and i["trunk_groups"] == -(-3 // i["bins_per_trunk_group"])
        assert pc.info(L, (15, 512, 450), 1)["trunk_lds_bytes"] == 151296
    for name, (S, H, M, relative, n, seed) in pc.WIDE_SPECS.items():        # n of a spec is what "P + k" comes to for its side
        if relative is not None:
            assert pc.exact_specs(2, 64, bins=lambda g: pc.info(emu_lib, g, 1)["bins_per_trunk_group"])[name][3] == n, name


@pytest.mark.parametrize("rot", [False, True])
def test_real_networks_within_eight_times_the_float32_torch_error(real_results, rot):
    """Emulator, 16 states of a recorded rollout, against the float64 forward.  Measured here: e_native / e_torch32 between 1.1
    and 2.5 for every head (printed)."""
    case, got = real_results(rot)
    pc.check_real(got, case["ref64"], case["ref32"], "emulator, rotation %d:" % rot)


@pytest.mark.parametrize("geom", pc.WIDE_REAL, ids=lambda g: "s%d_h%d_m%d" % tuple(g))
def test_real_networks_at_the_other_accepted_shapes(emu_lib, geom):
    """Emulator, 16 synthetic states, against the float64 forward under the same rule.  Measured here: e_native / e_torch32
    between 1.1 and 3.7 for every head (printed)."""
    case = pc.wide_real_case(*geom)
    pc.check_real(pc.host_runner(emu_lib)(case["obs"], case["geom"], case["blob"]), case["ref64"], case["ref32"], "emulator, %r:" % (geom,))


@pytest.mark.parametrize("geom", [(12, 96, 144), (15, 512, 450)], ids=lambda g: "s%d_h%d_m%d" % tuple(g))
def test_a_bin_gives_the_same_bits_where_every_workgroup_is_another_bin(emu_lib, geom):
    """P = 1: one state alone, and as first / middle / last row of n = 3."""
    assert pc.info(emu_lib, geom, 3)["bins_per_trunk_group"] == 1
    run = pc.host_runner(emu_lib)
    S = geom[0]
    blob = pc.pol.pack_weights(pc.real_weights(*geom, 11), *geom).numpy()
    states = pc.synthetic_states(S, 4)
    one = run(states[3:4], geom, blob)
    for rows in ((3, 0, 3), (1, 3, 2)):                                 # first and last in one batch, the middle in another
        got = run(states[list(rows)], geom, blob)
        for at, r in enumerate(rows):
            for h in pc.HEADS:
                assert pc.same_bits(got[h][at], one[h][0]) == (r == 3), (h, rows, at)


def test_a_bin_gives_the_same_bits_over_two_passes_of_the_hidden_layer(emu_lib, tiles):
    """(5, 512, 25): n = 1, n = T + 1 in rows 0, 32 and 64 (both row tiles, the second head tile), and under a padded stride."""
    P, T = tiles
    geom = (5, 512, 25)
    run = pc.host_runner(emu_lib)
    blob = pc.pol.pack_weights(pc.real_weights(*geom, 11), *geom).numpy()
    states = pc.synthetic_states(5, T + 2)
    one = run(states[T + 1:], geom, blob)
    batch = states[:T + 1].copy()
    batch[[0, T // 2, T]] = states[T + 1]
    got = run(batch, geom, blob)
    for at in (0, T // 2, T):
        for h in pc.HEADS:
            assert pc.same_bits(got[h][at], one[h][0]) and not pc.same_bits(got[h][at + 1 if at < T else 1], one[h][0]), (h, at)
    padded = np.full((P + 1, 103), 9.0, np.float32)
    padded[:, :100] = states[:P + 1]
    padded[P, :100] = states[T + 1]
    got = run(padded, geom, blob)
    for h in pc.HEADS:
        assert pc.same_bits(got[h][P], one[h][0]), h


def test_the_recorded_chain_bits_are_what_the_emulator_computes(emu_lib):
    """tests/golden/mfma_chain_emulator_bits.npz (make_mfma_chain_bits.py) against the emulator as it is now: the fixture the
    device is compared with cannot drift from the code."""
    g = np.load(os.path.join(ROOT, "tests", "golden", pc.CHAIN_FIXTURE + ".npz"))
    for spec in pc.CHAIN_CASES:
        for key, v in pc.chain_entries(pc.host_runner(emu_lib), spec).items():
            assert np.array_equal(g[key], v), "%s: rerun tests/golden/make_mfma_chain_bits.py if the change is meant" % key


def test_a_bin_gives_the_same_bits_in_every_batch(emu_lib, tiles, real_results):
    """One state alone, as first / middle / last row of n = P + 1 and n = T + 1, and under a padded stride."""
    P, T = tiles
    run = pc.host_runner(emu_lib)
    case, full = real_results(False)
    alone = run(case["obs"][3:4], case["geom"], case["blob"])
    for h in pc.HEADS:
        assert pc.same_bits(alone[h][0], full[h][3]), h
    small = pc.real_weights(5, 32, 25, 5)
    blob = pc.pol.pack_weights(small, 5, 32, 25).numpy()
    rng = np.random.RandomState(2)
    states = rng.randint(0, 6, (T + 1, 100)).astype(np.float32)
    state = states[7:8]
    one = run(state, G5, blob)
    for n in (P + 1, T + 1):
        for at in (0, n // 2, n - 1):
            batch = states[:n].copy()
            batch[at] = state[0]
            got = run(batch, G5, blob)
            for h in pc.HEADS:
                assert pc.same_bits(got[h][at], one[h][0]), (h, n, at)
    padded = np.full((P + 1, 103), 9.0, np.float32)
    padded[:, :100] = states[:P + 1]
    padded[P, :100] = state[0]
    got = run(padded, G5, blob)
    for h in pc.HEADS:
        assert pc.same_bits(got[h][P], one[h][0]), h


def test_a_head_that_is_not_asked_for_changes_nothing(emu_lib):
    run = pc.host_runner(emu_lib)
    case = pc.exact_case(5, 32, 25, 3, 21)
    full = run(case["obs"], case["geom"], case["blob"])
    for want in (("value",), ("logits",), ("pred",), ("value", "logits"), ("value", "pred"), ("logits", "pred")):
        got = run(case["obs"], case["geom"], case["blob"], want)          # the runner checks the others stay untouched
        for h in want:
            assert pc.same_bits(got[h], full[h]), (want, h)


def test_invalid_arguments_are_refused_before_any_device_is_touched(lib, emu_lib):
    obs, w, ws = np.zeros(8 * 403, np.float32), np.zeros(1 << 20, np.float32), np.zeros(1 << 16, np.float32)
    v, lg, pr = np.zeros(8, np.float32), np.zeros(8 * 200, np.float32), np.zeros(8 * 200, np.float32)

    def call(L, g=G5, n=2, stride=100, o=obs, weights=w, value=v, logits=lg, pred=pr, work=ws, null_geom=False):
        p = [a.ctypes.data if a is not None else None for a in (o, weights, value, logits, pred, work)]
        return L.bpp_policy_forward(p[0], stride, n, None if null_geom else pc.geom_arg(g), p[1], p[2], p[3], p[4], p[5], None)

    assert call(emu_lib) == 0 and call(emu_lib, stride=103) == 0 and call(emu_lib, g=(5, 32, 50)) == 0
    bad = [dict(o=None), dict(weights=None), dict(work=None), dict(null_geom=True), dict(value=None, logits=None, pred=None),
           dict(n=0), dict(n=-1), dict(g=(0, 32, 0)), dict(g=(-1, 32, 1)), dict(g=(5, 0, 25)), dict(g=(5, -32, 25)),
           dict(g=(5, 32, 24)), dict(g=(5, 32, 75)), dict(g=(5, 32, 0)), dict(stride=99), dict(stride=0), dict(stride=-100),
           dict(g=(5, 48, 25)), dict(g=(5, 16, 25)), dict(g=(5, 544, 25)),
           dict(g=(20, 256, 400), stride=1600), dict(g=(16, 256, 256), stride=1024), dict(g=(10, 256, 100), stride=399)]
    out = (ctypes.c_int32 * 8)()
    for L in (lib, emu_lib):            # the product library has no device here: it must refuse before it looks for one
        for b in bad:
            assert call(L, **b) == pc.BADARG, b
            assert L.bpp_last_error().decode().startswith("bpp_policy_forward: "), b
        for g in ((20, 256, 400), (5, 48, 25), (5, 32, 26), (0, 32, 0)):
            out[7] = 5
            assert L.bpp_policy_forward_info(pc.geom_arg(g), 4, out) == pc.BADARG and out[7] == 0
            assert L.bpp_policy_forward_workspace(pc.geom_arg(g), 4) == 0 and L.bpp_policy_weights_floats(pc.geom_arg(g)) == 0
        assert L.bpp_policy_forward_info(pc.geom_arg(G5), 0, out) == pc.BADARG and L.bpp_policy_forward_workspace(pc.geom_arg(G5), 0) == 0
        assert L.bpp_policy_forward_info(pc.geom_arg(G5), 4, None) == pc.BADARG
        assert L.bpp_policy_forward_info(None, 4, out) == pc.BADARG
        assert L.bpp_policy_forward_info(pc.geom_arg((15, 512, 450)), 4, out) == 0          # the largest side and hidden size


def test_every_declared_symbol_is_exported(lib):
    src = open(_lib.POLICY_HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(bpp_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.POLICY_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.bpp_abi_version() == 16


def test_info_is_consistent_with_workspace_and_weights(lib, emu_lib):
    import bpp_amd
    for L in (lib, emu_lib):
        for g, n in ((G10, 1), (G10, 2100), (G10, 65536), ((10, 256, 200), 257), (G5, 65), ((6, 32, 72), 3), ((15, 512, 225), 7)):
            i = pc.info(L, g, n)
            S, H, M = g
            A = S * S
            assert i["tile"] == 32 and i["path"] == 1 and i["bins_per_head_tile"] == 64
            assert i["trunk_groups"] == -(-n // i["bins_per_trunk_group"]) and i["head_groups"] == 3 * -(-n // 64)
            assert i["padded_rows"] % 32 == 0 and 0 <= i["padded_rows"] - i["bins_per_trunk_group"] * A < 32
            assert 2 * i["bins_per_trunk_group"] * 64 * (S + 2) ** 2 * 4 <= i["trunk_lds_bytes"] <= 160 * 1024
            assert L.bpp_policy_forward_workspace(pc.geom_arg(g), n) == n * 20 * A * 4
            floats = sum(int(np.prod(s)) + s[0] for _, s in pc.pol.layer_shapes(S, H, M))
            assert L.bpp_policy_weights_floats(pc.geom_arg(g)) == floats == bpp_amd.NativePolicy(S, M, H).weights.numel()
        assert pc.info(L, G10, 1)["bins_per_trunk_group"] == 2          # what 160 KiB of LDS admit at 10 x 10
        # the offsets the header states
        assert L.bpp_policy_weights_floats(pc.geom_arg(G10)) == 151380 + 3 * 256 + 2 * (800 * 256 + 256 * 100 + 100) + 400 * 256 + 256 + 1


def _split_form(plain):
    """The K-FAC-split checkpoint form of plain weights: `<layer>.module.weight`, `<layer>.add_bias._bias` [C, 1]."""
    out = {}
    for k, v in plain.items():
        name, kind = k.rsplit(".", 1)
        out[name + (".module.weight" if kind == "weight" else ".add_bias._bias")] = v if kind == "weight" else v.reshape(-1, 1)
    return out


def test_the_three_state_dict_forms_pack_to_the_same_blob(tmp_path):
    import bpp_amd
    plain = pc.real_weights(10, 256, 100, 4)
    a = bpp_amd.NativePolicy(10, 100).load_state_dict(plain)
    split = _split_form(plain)
    assert "base.share.0.add_bias._bias" in split and tuple(split["base.critic_linear.add_bias._bias"].shape) == (1, 1)
    b = bpp_amd.NativePolicy(10, 100).load_state_dict(split)
    c = bpp_amd.NativePolicy(10, 100).load_state_dict(bpp_amd.kfac.plain_state_dict(split))
    assert torch.equal(a.weights, b.weights) and torch.equal(a.weights, c.weights) and a.weights.abs().sum() > 0
    back = a.unpack()
    assert sorted(back) == sorted(plain) and all(torch.equal(back[k], plain[k]) for k in plain)
    # the first row of share.2's matrix is tap (c, i, j) = (0, 0, 0) of every output channel: [k][oc]
    assert torch.equal(a.weights[2368:2368 + 64], plain["base.share.2.weight"][:, 0, 0, 0])
    assert torch.equal(a.weights[2368 + 576 * 64:2368 + 577 * 64], plain["base.share.2.bias"])
    net = torch.nn.Module()                                             # refresh takes a module as well
    net.state_dict = lambda: {k: v + 1 for k, v in plain.items()}
    assert torch.equal(bpp_amd.NativePolicy(10, 100).refresh(net).weights, a.weights + 1)
    with pytest.raises(ValueError, match="base.mask.5"):
        bpp_amd.NativePolicy(10, 100).load_state_dict({k: v for k, v in plain.items() if not k.startswith("base.mask.5")})
    with pytest.raises(ValueError):
        bpp_amd.NativePolicy(10, 200).load_state_dict(plain)
    with pytest.raises(ValueError):
        bpp_amd.NativePolicy(10, 150)
    path = str(tmp_path / "ckpt.pt")
    torch.save((split, None), path)
    assert torch.equal(bpp_amd.NativePolicy.from_checkpoint(path, 10, 100).weights, a.weights)
    torch.save((split, {"mean": 0}), path)
    with pytest.raises(ValueError, match="observation statistics"):
        bpp_amd.NativePolicy.from_checkpoint(path, 10, 100)


def test_the_searches_accept_what_the_policy_returns():
    """On CPU tensors the policy runs torch_forward: the same contract, (value [n], logits [n, M], pred [n, M])."""
    import bpp_amd
    from bpp_amd.reorder import check_policy_output
    policy = bpp_amd.NativePolicy(10, 200).load_state_dict(pc.real_weights(10, 256, 200, 6))
    obs = torch.from_numpy(pc.deep_states(True, 5))
    out = policy(obs)
    value, logits, pred = check_policy_output(out, 5, 200)
    assert value.shape == (5,) and logits.shape == (5, 200) and pred.shape == (5, 200) and (pred >= 0).all()
    want = pc.pol.torch_forward(policy.unpack(), obs)
    assert all(torch.equal(a, b) for a, b in zip(out, want))
    assert policy(obs, want=("logits",))[0] is None
    with pytest.raises(RuntimeError, match="HIP device"):
        bpp_amd.policy_forward(obs, policy.weights, policy.geom)
    assert bpp_amd.NativePolicy is pc.pol.NativePolicy and bpp_amd.policy_forward is pc.pol.policy_forward


def test_the_python_entry_point_checks_its_tensors():
    import bpp_amd
    w = torch.zeros(10)
    for obs in (torch.zeros(4, 400, dtype=torch.float64), torch.zeros(400), torch.zeros(0, 400)):
        with pytest.raises(ValueError):
            bpp_amd.policy_forward(obs, w, G10)
    with pytest.raises(ValueError):
        bpp_amd.policy_forward(torch.zeros(4, 400), w, G10, want=())
    with pytest.raises(ValueError):
        bpp_amd.policy_forward(torch.zeros(4, 400), w, G10, want=("probs",))


@needs_reference
@pytest.mark.parametrize("rot", [False, True])
def test_against_the_live_reference_policy(emu_lib, rot):
    """The reference's own Policy, seeded, its state dict loaded into NativePolicy; four deep states on the emulator against
    Policy.base + dist.linear in float64, the reference's own float32 forward giving e_torch32."""
    import types
    import bpp_amd
    ref_shims.install()
    from acktr.model import Policy
    M = 200 if rot else 100
    args = types.SimpleNamespace(channel=4, container_size=(10, 10, 10), pallet_size=10, enable_rotation=rot)
    torch.manual_seed(5)
    ref = Policy((400,), bpp_amd.Discrete(M), base_kwargs={"recurrent": False, "hidden_size": 256, "args": args}).eval()
    with torch.no_grad():
        for p in ref.parameters():                                      # the reference starts every bias at 0: make them count
            if p.dim() == 1:
                p.uniform_(-0.1, 0.1)
    policy = bpp_amd.NativePolicy(10, M).load_state_dict(ref.state_dict())
    obs = pc.deep_states(rot, 4)

    def forward(net, x):
        with torch.no_grad():
            value, features, _, pred = net.base(x, None, None)
            return {"value": value.reshape(-1).numpy(), "logits": net.dist.linear(features).numpy(), "pred": pred.numpy()}

    ref32 = forward(ref, torch.from_numpy(obs))
    ref64 = forward(ref.double(), torch.from_numpy(obs).double())
    got = pc.host_runner(emu_lib)(obs, policy.geom, policy.weights.numpy())
    pc.check_real(got, ref64, ref32, "live reference, rotation %d:" % rot)
    ours32 = pc.pol.torch_forward(policy.unpack(), torch.from_numpy(obs))
    for h, t in zip(pc.HEADS, ours32):                                  # torch_forward is the reference's layers
        np.testing.assert_allclose(t.numpy(), ref32[h], rtol=0, atol=1e-5 * np.abs(ref32[h]).max())


@pytest.mark.parametrize("rot,ckpt", [(False, "default_cut_2.pt"), (True, "rotation_cut_2.pt")])
def test_recorded_outputs_of_the_reference_under_its_checkpoints(emu_lib, rot, ckpt):
    """tests/golden/policy_forward_cut2_10{,_rot}.npz (make_policy_golden.py): what the reference's own Policy computed in float32
    for 32 deep states under its pretrained checkpoint.  The checkpoint's weights come from oracle/_ref/ (a copy of the file);
    the emulator's outputs lie within 8 * e_torch32 of the recording, e_torch32 being the recording's own distance from a
    float64 forward."""
    import bpp_amd
    path = os.path.join(ref_shims.REF_COPY, "pretrained_models", ckpt)
    if not ref_shims.copy_available() or not os.path.isfile(path):
        pytest.skip("oracle/_ref/ without the checkpoints (python oracle/make_ref.py)")
    g = np.load(os.path.join(ROOT, "tests", "golden", "policy_forward_cut2_10%s.npz" % ("_rot" if rot else "")))
    rec = {"value": g["value"], "logits": g["logits"], "pred": g["pred_mask"]}
    policy = bpp_amd.NativePolicy.from_checkpoint(path, 10, 200 if rot else 100)
    obs = pc.deep_states(rot, int(g["states"]))
    with torch.no_grad():
        ref64 = pc.pol.torch_forward({k: v.double() for k, v in policy.unpack().items()}, torch.from_numpy(obs).double())
        ours32 = pc.pol.torch_forward(policy.unpack(), torch.from_numpy(obs))
    ref64 = {h: t.numpy() for h, t in zip(pc.HEADS, ref64)}
    got = pc.host_runner(emu_lib)(obs, policy.geom, policy.weights.numpy())
    for h, t in zip(pc.HEADS, ours32):                                  # torch_forward computes what the reference recorded
        np.testing.assert_allclose(t.numpy(), rec[h], rtol=0, atol=1e-5 * np.abs(rec[h]).max())
    for h in pc.HEADS:
        e_torch32 = pc.rel_err(rec[h], ref64[h])
        e_native = pc.rel_err(got[h], rec[h].astype(np.float64))
        print("checkpoint %s, %s: emulator against the recording %.3g, e_torch32 %.3g" % (ckpt, h, e_native, e_torch32))
        assert e_torch32 > 0 and e_native <= pc.FACTOR * e_torch32, (h, e_native, e_torch32)


def test_the_near_tie_check_of_the_teacher_forced_test():
    """pc.check_near_ties on constructed logits: a tie within the float32 error passes, also where an infeasible action has the
    largest logit; a clear gap, or a choice of an infeasible action, does not."""
    rng = np.random.RandomState(4)
    l64 = rng.standard_normal((3, 100)) * 3.0
    l32 = l64.astype(np.float32).astype(np.float64)                    # relative error about 1e-8 .. 6e-8
    masks = np.ones((3, 100))
    for r in range(3):
        l64[r, 10], l64[r, 20] = l64[r].max() + 1.0, l64[r].max() + 1.0 + 1e-12          # 10 and 20 lead and tie
        l32[r, 10], l32[r, 20] = l64[r, 10], l64[r, 10]
    l64[1, 30], masks[1, 30] = l64[1].max() + 5.0, 0.0                  # infeasible and largest: 14 below after masking
    l32[1, 30] = l64[1, 30]
    got = pc.check_near_ties(l64, l32, masks, [10, 10, 20], [20, 20, 10])
    assert len(got) == 3 and all(0 <= gap < limit for gap, limit in got)
    with pytest.raises(AssertionError):
        pc.check_near_ties(l64, l32, masks, [10, 10, 10], [20, 20, 40])         # state 2: action 40 is no tie
    masks[0, 20] = 0.0
    with pytest.raises(AssertionError):
        pc.check_near_ties(l64, l32, masks, [10, 10, 20], [20, 20, 10])         # state 0: the choice is infeasible


def test_native_policy_from_the_example_actor():
    """examples/rollout_with_policy.native_from_actor on the host: the packed policy's logits are the Actor's, bit for bit (the
    same torch layers); the heads the Actor lacks are zeros."""
    import bpp_amd
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import rollout_with_policy as ex
    torch.manual_seed(3)
    actor = ex.Actor(10, 100).eval()
    policy = ex.native_from_actor(actor)
    obs = torch.from_numpy(pc.deep_states(False, 4))
    with torch.no_grad():
        assert torch.equal(policy(obs, want=("logits",))[1], actor(obs))
    assert float(policy(obs)[0].abs().max()) == 0.0
    for kw in (dict(side=20, n_actions=400), dict(side=16, n_actions=256), dict(side=10, n_actions=100, hidden=48),
               dict(side=10, n_actions=100, hidden=544), dict(side=0, n_actions=0)):
        with pytest.raises(ValueError):                                 # refused wherever the tensors live, as the device call does
            bpp_amd.NativePolicy(**kw)
