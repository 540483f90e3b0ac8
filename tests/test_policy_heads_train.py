"""bpp_policy_heads_forward_train / bpp_policy_heads_backward (include/bpp_policy_heads_train.h) and
bpp_amd.policy_heads without a GPU: the product kernels of csrc/bpp_policy_heads_train.inl compiled by g++ against the SIMT
emulator.  Exact-integer heads bit for bit against int64 numpy; the training forward against the inference forward; real-valued
heads bit for bit against the header's arithmetic in numpy (hc.normative_heads, recorded in tests/golden/heads_train_chain_bits.npz)
and the split identity of grad_weights; real-valued gradients against float64 torch autograd within 8 x the error of float32
torch autograd; batch independence; stores outside the outputs and the zeros of an absent head; the refusals of the header on
the product library, which has no device here; the packing of the blobs.  Helpers: tests/policy_heads_train_cases.py."""
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
import policy_heads_train_cases as hc  # noqa: E402
import policy_train_cases as tc  # noqa: E402

pol = pc.pol
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G10, G5 = (10, 256, 100), (5, 32, 25)


@pytest.fixture(scope="module")
def emu_lib(emu):
    import emu_binding
    csrc = os.path.join(ROOT, "online-3d-bpp-drl_amd", "csrc")
    if any(os.path.getmtime(os.path.join(csrc, f)) > os.path.getmtime(emu.LIB) for f in ("bpp_policy.inl", "bpp_policy_heads_train.inl")):
        emu_binding.build(force=True)
    L = _lib.bind_policy_heads_train(_lib.bind_policy(ctypes.CDLL(emu.LIB)))
    L.bpp_last_error.restype = ctypes.c_char_p
    return L


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


def exact_shapes(L):
    i = hc.info(L, hc.EXACT_SPLIT_GEOM, 1)
    assert i["bins_per_split"] == hc.BINS_PER_SPLIT                       # the header's formula: 128, whatever geom and n are
    B = i["bins_per_split"]
    return hc.EXACT_SHAPES + [hc.EXACT_SPLIT_GEOM + (B + 1,), hc.EXACT_SPLIT_GEOM + (2 * B + 1,)]


@pytest.mark.parametrize("at", range(len(hc.EXACT_SHAPES) + 2))
def test_exact_integer_heads_equal_int64_numpy_bit_for_bit(emu_lib, at):
    S, H, M, n = exact_shapes(emu_lib)[at]
    if at >= len(hc.EXACT_SHAPES):
        i = hc.info(emu_lib, (S, H, M), n)
        assert i["splits"] == at - len(hc.EXACT_SHAPES) + 2 and i["chain_rows"] == hc.BINS_PER_SPLIT
    hc.check_exact(hc.host_runner(emu_lib), hc.exact_case(S, H, M, n))


@pytest.mark.parametrize("S,H,M,n", [(10, 256, 100, 5), (11, 32, 121, 3)])
def test_the_training_forward_leaves_the_bits_of_the_inference_forward(emu_lib, S, H, M, n):
    """value / logits / pred of bpp_policy_heads_forward_train on the feat bpp_policy_forward left in its workspace."""
    geom, A = (S, H, M), S * S
    blob = pol.pack_weights(pc.real_weights(S, H, M, 11), S, H, M).numpy()
    obs = pc.deep_states(False, n) if S == 10 else pc.synthetic_states(S, n)
    g = pc.geom_arg(geom)
    ws = np.full(n * 20 * A, np.nan, np.float32)
    want = dict(value=np.empty(n, np.float32), logits=np.empty((n, M), np.float32), pred=np.empty((n, M), np.float32))
    assert emu_lib.bpp_policy_forward(obs.ctypes.data, 4 * A, n, g, blob.ctypes.data, want["value"].ctypes.data, want["logits"].ctypes.data,
                                      want["pred"].ctypes.data, ws.ctypes.data, None) == 0
    got = {k: np.full(v.shape, np.nan, np.float32) for k, v in want.items()}
    hidden = np.full((3, n, H), np.nan, np.float32)
    assert emu_lib.bpp_policy_heads_forward_train(ws.ctypes.data, n, g, blob.ctypes.data, got["value"].ctypes.data, got["logits"].ctypes.data,
                                                  got["pred"].ctypes.data, hidden.ctypes.data, None) == 0
    assert all(pc.same_bits(got[k], want[k]) for k in want) and not np.isnan(hidden).any() and (hidden > 0).any() and (hidden == 0).any()


# --------------------------------------------------------------------- the header's arithmetic, bit for bit (hc.normative_heads)
@pytest.fixture(scope="module")
def chain_bits():
    return tc.load_fixture(hc.CHAIN_FIXTURE)


def test_the_recorded_chain_bits_hold_every_case_once(chain_bits):
    names = [hc.chain_name(*spec) for spec in hc.CHAIN_CASES]
    want = ["%s.crc.%s" % (nm, k) for nm in names for k in hc.CHAIN_INPUTS] + \
           ["%s.%s.%s" % (nm, k, what) for nm in names for k in hc.OUTPUTS for what in ("crc", "sample")]
    assert sorted(chain_bits.files) == sorted(want)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", hc.CHAIN_FIXTURE + ".npz")) < 400000
    assert all(chain_bits["%s.%s.sample" % (nm, k)].size <= 2048 for nm in names for k in hc.OUTPUTS)
    assert sum(1 for S, H, M, n in hc.CHAIN_CASES if -(-n // hc.BINS_PER_SPLIT) > 2) == 1


@pytest.mark.parametrize("spec", [(5, 288, 25, 3), (2, 32, 4, 300)])
def test_the_recorded_chain_bits_are_the_reference_computed_now(chain_bits, spec):
    case = hc.chain_case(*spec)
    want = hc.chain_reference(case)
    for key, v in hc.chain_entries(case, want, hc.chain_name(*spec)).items():
        assert np.array_equal(chain_bits[key], v), key
    assert min(float(np.abs(want[k]).max()) for k in hc.OUTPUTS) > 0 and not any(np.isnan(want[k]).any() for k in hc.OUTPUTS)


@pytest.mark.parametrize("spec", hc.CHAIN_CASES)
def test_real_valued_chains_equal_the_headers_arithmetic_bit_for_bit(emu_lib, chain_bits, spec):
    """Emulator: every output on real-valued data against the recorded bits of hc.normative_heads, 0 ulps everywhere."""
    case, name = hc.chain_case(*spec), hc.chain_name(*spec)
    assert hc.info(emu_lib, spec[:3], spec[3])["splits"] == -(-spec[3] // hc.BINS_PER_SPLIT)
    for k in hc.CHAIN_INPUTS:
        assert pc.crc(case[k]) == chain_bits["%s.crc.%s" % (name, k)], k
    hc.check_chain(hc.run_case(hc.host_runner(emu_lib), case), chain_bits, name, "emulator:")


def test_the_whole_batch_is_the_double_sum_of_its_splits(emu_lib):
    spec = (2, 32, 4, 300)
    i = hc.info(emu_lib, spec[:3], spec[3])
    assert i["splits"] == 3 and i["bins_per_split"] == hc.BINS_PER_SPLIT
    differing = hc.check_split_identity(hc.host_runner(emu_lib), hc.chain_case(*spec), i["bins_per_split"])
    print("%r: a float32 sum of the splits differs in %d floats" % (spec, differing))


# -------------------------------------------------------------------------------------------------------- accuracy and structure
@pytest.mark.parametrize("geom,n", [(G10, 16), (G5, 70)])
def test_real_gradients_within_eight_times_the_float32_autograd_error(emu_lib, geom, n):
    """Emulator, against float64 torch autograd over the same six Linear layers on the same feat: 16 recorded states at 10 x 10,
    70 synthetic states at 5 x 5; no head pre-activation of either lies within 2 * 2^-24 * sum |x_k w_k| of zero (asserted).
    Measured: e_native / e_torch32 between 1.00 and 2.50 at 10 x 10 and between 1.00 and 7.10 (the bias of critic_linear, a sum
    of 70 terms) at 5 x 5, over every dW, every db and grad_feat (printed)."""
    case = hc.real_case(geom, pc.deep_states(False, n) if geom[0] == 10 else pc.synthetic_states(geom[0], n))
    assert not hc.head_ties(case["plain"], case["feat"]).any()
    hc.check_real(hc.run_case(hc.host_runner(emu_lib), case), case, "emulator, %r, n = %d:" % (geom, n))


def test_the_share_of_tied_states_of_the_many_state_module_test_is_below_the_cap():
    """What tests/test_gpu_policy_heads_train.py leaves out of its 320-state comparison, decided on the CPU from the float64
    forward alone: of the 400 states of deep_states(False, 400) under the reference initialisation (torch.manual_seed(5)), 9 are
    tied in the trunk and none more in the heads: 2.25 %, below the project's cap of 3 %."""
    import bpp_amd
    torch.manual_seed(5)
    plain = {k: v.detach() for k, v in bpp_amd.TrainablePolicy(10, 100).state_dict().items()}
    obs = pc.deep_states(False, 400)
    trunk, both = tc.tied_bins(plain, obs), hc.tied_states(plain, obs)
    heads = both & ~trunk
    print("tied: %d in the trunk, %d more in the heads, of %d" % (trunk.sum(), (heads & ~trunk).sum(), obs.shape[0]))
    assert both.sum() <= 0.03 * obs.shape[0]


def test_a_row_gives_the_same_bits_in_any_batch(emu_lib):
    """Outputs, hidden, grad_hidden, grad_out_mask and grad_feat of a row alone and as first / middle / last of 5 (5 x 5)."""
    case = hc.chain_case(5, 32, 25, 6)
    run = hc.host_runner(emu_lib)
    keys = ("feat", "grad_value", "grad_logits", "grad_pred")
    one = hc.run_case(run, case, **{k: case[k][5:] for k in keys})
    for at in (0, 2, 4):
        rows = {k: case[k][:5].copy() for k in keys}
        for k in keys:
            rows[k][at] = case[k][5]
        got = hc.run_case(run, case, **rows)
        for key in hc.ROW_OUTPUTS:
            assert pc.same_bits(got[key][at], one[key][0]) and not pc.same_bits(got[key][(at + 1) % 5], one[key][0]), (key, at)
        for key in ("hidden", "grad_hidden"):
            assert pc.same_bits(got[key][:, at], one[key][:, 0]) and not pc.same_bits(got[key][:, (at + 1) % 5], one[key][:, 0]), (key, at)


# ------------------------------------------------------------------------------------------------------ buffers and refusals
@pytest.mark.parametrize("spec", [(3, 64, 9, 63), (3, 64, 9, 65), (2, 32, 4, 129)])
def test_nothing_is_stored_outside_the_outputs(emu_lib, spec):
    """Outputs and workspace carved out of guarded buffers: guards untouched, every output float written, the bits of the plain
    runner; the zeros of an absent head, also into guarded buffers."""
    case = hc.exact_case(*spec)
    got = hc.check_exact(hc.guarded_host_runner(emu_lib), case)
    plain = hc.run_case(hc.host_runner(emu_lib), case)
    assert all(pc.same_bits(got[k], plain[k]) for k in hc.OUTPUTS)
    hc.check_absent_heads(hc.guarded_host_runner(emu_lib), case)


def test_refusals_come_before_any_device_is_looked_for(lib, emu_lib):
    geom, n = G5, 4
    sz = hc.sizes(geom, n)
    buf = {k: np.zeros(v, np.float32) for k, v in sz.items()}
    buf.update(feat=np.zeros(n * 500, np.float32), blob=np.zeros(emu_lib.bpp_policy_weights_floats(pc.geom_arg(geom)), np.float32),
               blob_bwd=np.zeros(emu_lib.bpp_policy_heads_backward_weights_floats(pc.geom_arg(geom)), np.float32))
    ws = np.zeros(emu_lib.bpp_policy_heads_backward_workspace(pc.geom_arg(geom), n) // 4, np.float32)
    grads = dict(gv=np.ones(n, np.float32), gl=np.ones(n * geom[2], np.float32), gp=np.ones(n * geom[2], np.float32))

    def forward(L, g=geom, n=n, null_geom=False, **null):
        p = {k: None if k in null else buf[k].ctypes.data for k in ("feat", "blob", "value", "logits", "pred", "hidden")}
        return L.bpp_policy_heads_forward_train(p["feat"], n, None if null_geom else pc.geom_arg(g), p["blob"], p["value"], p["logits"], p["pred"],
                                                p["hidden"], None)

    def backward(L, g=geom, n=n, null_geom=False, short=0, **null):
        p = {k: None if k in null else v.ctypes.data for k, v in buf.items()}
        gv, gl, gp = (None if k in null else grads[k].ctypes.data for k in ("gv", "gl", "gp"))
        return L.bpp_policy_heads_backward(p["feat"], p["hidden"], p["pred"], gv, gl, gp, n, None if null_geom else pc.geom_arg(g), p["blob_bwd"], p["grad_feat"],
                                           p["grad_hidden"], None if "gom" in null else buf["grad_out_mask"].ctypes.data, p["gw"],
                                           None if "ws" in null else ws.ctypes.data, ws.nbytes - short, None)

    assert forward(emu_lib) == 0 and backward(emu_lib) == 0 and backward(emu_lib, gv=1, gl=1) == 0
    shared = [dict(null_geom=True), dict(n=0), dict(n=-1), dict(g=(23, 32, 529)), dict(g=(5, 48, 25)), dict(g=(5, 544, 25)), dict(g=(5, 32, 24)),
              dict(g=(5, 32, 75)), dict(g=(0, 32, 0)), dict(feat=None)]
    out = (ctypes.c_int32 * 8)()
    for L in (lib, emu_lib):            # the product library has no device here: it must refuse before it looks for one
        for b in shared + [dict(blob=None), dict(value=None), dict(logits=None), dict(pred=None), dict(hidden=None)]:
            assert forward(L, **b) == pc.BADARG, b
            assert L.bpp_last_error().decode().startswith("bpp_policy_heads_forward_train: "), b
        for b in shared + [dict(hidden=None), dict(pred=None), dict(blob_bwd=None), dict(grad_feat=None), dict(grad_hidden=None), dict(gom=1),
                           dict(gw=None), dict(ws=1), dict(gv=1, gl=1, gp=1), dict(short=4), dict(short=ws.nbytes)]:
            assert backward(L, **b) == pc.BADARG, b
            assert L.bpp_last_error().decode().startswith("bpp_policy_heads_backward: "), b
        for g in ((23, 32, 529), (5, 48, 25), (5, 544, 25), (5, 32, 26), (0, 32, 0)):
            out[6] = 5
            assert L.bpp_policy_heads_backward_info(pc.geom_arg(g), 4, out) == pc.BADARG and out[6] == 0
            assert L.bpp_policy_heads_backward_workspace(pc.geom_arg(g), 4) == 0
            assert L.bpp_policy_heads_backward_weights_floats(pc.geom_arg(g)) == 0
        assert L.bpp_policy_heads_backward_info(pc.geom_arg(geom), 0, out) == pc.BADARG
        assert L.bpp_policy_heads_backward_workspace(pc.geom_arg(geom), 0) == 0
        assert L.bpp_policy_heads_backward_info(pc.geom_arg(geom), 4, None) == pc.BADARG
        assert L.bpp_policy_heads_backward_info(None, 4, out) == pc.BADARG
        assert L.bpp_policy_heads_backward_info(pc.geom_arg((22, 512, 968)), 2 ** 31 - 1, out) == pc.BADARG    # splits x blocks beyond the grid
        assert L.bpp_policy_heads_backward_info(pc.geom_arg((22, 512, 968)), 4, out) == 0                      # a side only the heads accept


def test_the_python_side_refuses():
    import bpp_amd
    with pytest.raises(ValueError, match="heads must be"):
        bpp_amd.TrainablePolicy(10, 100, heads="nonsense")
    plain = pc.real_weights(5, 32, 25, 4)
    with pytest.raises(RuntimeError, match="HIP device"):                      # a tensor on the wrong device
        bpp_amd.policy_heads(torch.zeros(2, 500), plain, 5, 25, 32)
    with pytest.raises(ValueError, match="20 A"):
        bpp_amd.policy_heads(torch.zeros(2, 499), plain, 5, 25, 32)
    with pytest.raises(ValueError, match="HEAD_PARAMETERS"):
        bpp_amd.policy_heads(torch.zeros(2, 500), [plain[k] for k in pol.HEAD_PARAMETERS[:-1]], 5, 25, 32)
    assert bpp_amd.policy_heads is pol.policy_heads and bpp_amd.TrainablePolicy(10, 100).heads == "torch"
    net = bpp_amd.TrainablePolicy(10, 100, heads="native")
    assert net.kept() is None and sorted(net.state_dict()) == sorted(bpp_amd.TrainablePolicy(10, 100).state_dict())
    obs = torch.from_numpy(pc.deep_states(False, 2))
    with torch.no_grad():                                                      # on CPU tensors both modes are torch_forward
        torch.manual_seed(1)
        a = bpp_amd.TrainablePolicy(10, 100, heads="native")(obs)
        torch.manual_seed(1)
        b = bpp_amd.TrainablePolicy(10, 100)(obs)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_the_example_refuses_acktr_with_the_native_heads():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_with_storage as ex
    with pytest.raises(ValueError, match="native-heads"):
        ex.train(envs=64, updates=1, native_heads=True, acktr=True, verbose=False)
    with pytest.raises(ValueError, match="native-trunk"):              # the existing refusal keeps its message
        ex.train(envs=64, updates=1, native_trunk=True, acktr=True, verbose=False)


def test_every_declared_symbol_is_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(_lib.POLICY_HEADS_TRAIN_HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(bpp_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.POLICY_HEADS_TRAIN_SYMBOLS) and not set(names) & set(_lib.POLICY_SYMBOLS + _lib.POLICY_TRAIN_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.bpp_abi_version() == 16


def test_info_is_consistent_with_workspace(lib, emu_lib):
    for L in (lib, emu_lib):
        for g, n in ((G10, 1), (G10, 320), (G10, 2100), (G10, 65536), (G5, 129), ((15, 512, 450), 7), ((1, 32, 1), 3), ((22, 512, 968), 2)):
            i, f = hc.info(L, g, n), None
            S, H, M = g
            A = S * S
            blocks = sum(-(-rows // 64) * -(-cols // 128) for rows, cols in ((8 * A + 1, H), (H + 1, M), (8 * A + 1, H), (H + 1, M), (4 * A + 1, H),
                                                                             (H + 1, 1)))
            assert i["path"] == 1 and i["blocks"] == blocks and i["bins_per_group"] == 64 and i["grad_lds_bytes"] == ((H + 64) * 65 + 64) * 4
            assert i["bins_per_split"] == 128 and i["splits"] == -(-n // 128) and i["chain_rows"] == min(n, 128)
            assert i["wgrad_lds_bytes"] == 32 * (96 + 160) * 4 and i["grad_lds_bytes"] <= 160 * 1024
            assert L.bpp_policy_heads_backward_workspace(pc.geom_arg(g), n) == i["splits"] * blocks * 8 * 1024 * 4
            assert L.bpp_policy_heads_backward_weights_floats(pc.geom_arg(g)) == 2 * M * H + 20 * A * H + H
            if S <= 15:
                assert L.bpp_policy_weights_floats(pc.geom_arg(g)) - pol.TRUNK_FLOATS == hc.sizes(g, n)["gw"]
        assert hc.info(L, G10, 1)["blocks"] == 81


def test_the_blobs_and_the_gradient_views():
    geom = (10, 256, 200)
    S, H, M = geom
    plain = pc.real_weights(S, H, M, 4)
    whole = pol.pack_weights(plain, S, H, M)
    tail = pol.pack_heads(plain)
    assert torch.equal(tail, whole[pol.TRUNK_FLOATS:]) and torch.equal(pol.pack_trunk(plain), whole[:pol.TRUNK_FLOATS])
    back = pol.unpack_heads_gradient(tail, S, H, M)                     # the gradient has the blob's layout
    assert sorted(back) == sorted(pol.HEAD_PARAMETERS) and all(torch.equal(back[k], plain[k]) for k in back)
    both = dict(pol.unpack_trunk_gradient(whole[:pol.TRUNK_FLOATS]), **back)                 # trunk ++ heads is the whole blob's gradient
    ref = pol.unpack_weights(whole, S, H, M)
    assert sorted(both) == sorted(ref) and all(torch.equal(both[k], ref[k]) for k in ref)
    with pytest.raises(ValueError):
        pol.unpack_heads_gradient(tail[:-1], S, H, M)
    wb = pol.pack_heads_backward(plain)
    A = S * S
    assert wb.numel() == 2 * M * H + 20 * A * H + H
    at = 0
    for name in ("dist.linear", "base.actor.3", "base.mask.5", "base.mask.3", "base.critic_linear", "base.critic.3"):       # W2 in front of W1
        w = plain[name + ".weight"]
        assert torch.equal(wb[at:at + w.numel()], w.reshape(-1)), name
        at += w.numel()
    assert at == wb.numel() and wb[M * H + 3 * 8 * A + 5] == plain["base.actor.3.weight"][3, 5]
