"""bpp_policy_forward_one_image and bpp_amd.NativePolicy(form=) on the device (include/bpp_policy_one_image.h):
the cases of tests/test_policy_forward_one_image.py through bpp_amd.policy_forward(..., form="one_image") -- here the MFMA itself
runs and the accumulators live in registers across the barrier --, the emulator's recorded chain bits, runs, streams and a replayed
graph, act(), the grown workspace, and a 20 x 20 x 20 environment stepped under the native policy.  Reads nothing of the
reference."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_cases as pc  # noqa: E402
import policy_one_image_cases as oc  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G5, G20 = (5, 32, 25), (20, 256, 400)


@pytest.fixture(scope="module")
def bpp():
    import bpp_amd
    assert torch.cuda.is_available()
    return bpp_amd


@pytest.fixture(scope="module")
def policy20(bpp):
    """(NativePolicy(20, 400, form="auto") on the device with real weights, 3 synthetic states, its outputs on them), computed once."""
    policy = bpp.NativePolicy(20, 400, form="auto").load_state_dict(pc.real_weights(*G20, 11)).to(DEV)
    obs = torch.from_numpy(pc.synthetic_states(20, 3)).to(DEV)
    out = [t.clone() for t in policy(obs)]
    torch.cuda.synchronize()
    return policy, obs, out


@pytest.mark.parametrize("spec", oc.SAME_BITS, ids=oc.case_id)
def test_gpu_the_same_bits_as_the_two_image_form(bpp, spec):
    oc.check_same_bits(oc.device_runner(DEV), pc.device_runner(DEV), spec)


def test_gpu_the_same_bits_for_every_subset_of_heads_and_a_padded_stride(bpp):
    one = oc.device_runner(DEV)
    blob = pc.pol.pack_weights(pc.real_weights(*G5, 11), *G5).numpy()
    obs = pc.synthetic_states(5, 3)
    full = pc.device_runner(DEV)(obs, G5, blob)
    for k in (1, 2, 3):
        for want in itertools.combinations(pc.HEADS, k):
            got = one(obs, G5, blob, want)
            assert sorted(got) == sorted(want)
            for h in want:
                assert pc.same_bits(got[h], full[h]), (want, h)
    padded = torch.from_numpy(oc.padded(obs)).to(DEV)
    view = padded[:, :100]                                              # a view: rows 103 floats apart
    got = pc.pol.policy_forward(view, torch.from_numpy(blob).to(DEV), G5, form="one_image")
    assert view.stride(0) == 103 and all(pc.same_bits(t.cpu().numpy(), full[h]) for h, t in zip(pc.HEADS, got))


@pytest.mark.parametrize("spec", oc.EXACT, ids=oc.case_id)
def test_gpu_exact_integer_networks_above_side_15_equal_int64_numpy_bit_for_bit(bpp, spec):
    pc.check_exact(oc.device_runner(DEV), pc.exact_case(*spec))


@pytest.mark.parametrize("geom", oc.REAL, ids=lambda g: "s%d_h%d_m%d" % tuple(g))
def test_gpu_real_networks_within_eight_times_the_float32_torch_error(bpp, geom):
    case = oc.real_case(*geom)
    pc.check_real(oc.device_runner(DEV)(case["obs"], case["geom"], case["blob"]), case["ref64"], case["ref32"], "device, one image, %r:" % (geom,))


def test_gpu_a_bin_gives_the_same_bits_alone_and_in_a_batch_at_side_20(bpp):
    oc.check_batch_independence(oc.device_runner(DEV), G20)


def test_gpu_the_mfma_gives_the_bits_of_the_emulators_fmaf_chain(bpp):
    """tests/golden/mfma_chain_one_image_bits.npz: the inputs are regenerated here and their CRC32 compared first; then every
    head of the device against the emulator's sequential fmaf chain, by the CRC32 of the output bits: 0 ulps."""
    g = load_golden(oc.CHAIN_FIXTURE)
    for spec in oc.CHAIN_CASES:
        got = oc.chain_entries(oc.device_runner(DEV), spec)
        for key in sorted(got, key=lambda k: (".crc.obs" not in k and ".crc.blob" not in k, k)):      # the inputs first
            assert got[key] == g[key], key


def test_gpu_two_runs_a_side_stream_and_a_replayed_graph_give_the_same_bits(bpp, policy20):
    policy, obs, out = policy20
    assert all(torch.equal(a, b) for a, b in zip(policy(obs), out))                 # two runs
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    static = obs.clone()
    with torch.cuda.stream(side):
        other = policy(static)                                                      # another stream; the warm-up of the capture
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(other, out))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = policy(static)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(captured, out))
    changed = torch.from_numpy(pc.synthetic_states(20, 6)[3:]).to(DEV)              # 3 other states
    assert not torch.equal(changed, obs)
    static.copy_(changed)
    graph.replay()
    torch.cuda.synchronize()
    eager = policy(changed)
    assert all(torch.equal(a, b) for a, b in zip(captured, eager)) and not torch.equal(eager[1], out[1])


def test_gpu_act_is_masked_act_on_its_own_logits(bpp, policy20):
    policy, obs, out = policy20
    mask = torch.from_numpy((np.random.RandomState(3).rand(3, 400) < 0.3).astype(np.float32)).to(DEV)
    mask[:, 7] = 1.0
    value, action, logp = policy.act(obs, mask, deterministic=True)
    a2, lp2 = bpp.masked_act(out[1], mask, deterministic=True)
    assert torch.equal(action, a2) and torch.equal(logp, lp2) and action.shape == (3, 1) and action.dtype == torch.int64
    assert value.shape == (3, 1) and torch.equal(value.reshape(-1), out[0])
    assert bool((mask.gather(1, action) == 1).all())


def test_gpu_a_grown_workspace_gives_row_0_the_same_bits(bpp, policy20):
    policy, obs, out = policy20
    states = torch.from_numpy(pc.synthetic_states(20, 70)).to(DEV)
    key = (states.device, torch.cuda.current_stream(DEV).cuda_stream, policy.geom)
    pc.pol._WORKSPACE.pop(key, None)
    one = [t.clone() for t in policy(states[:1])]
    small = pc.pol._WORKSPACE[key].numel()
    grown = policy(states)
    assert small == 20 * 400 and pc.pol._WORKSPACE[key].numel() == 70 * small
    assert all(torch.equal(a[0], b[0]) for a, b in zip(grown, one)) and not torch.equal(grown[1][1], one[1][0])
    again = policy(states[:1])                                                      # the grown workspace serves n = 1 as well
    assert pc.pol._WORKSPACE[key].numel() == 70 * small and all(torch.equal(a, b) for a, b in zip(again, one))


def test_gpu_a_20_cubed_environment_steps_under_the_native_policy(bpp):
    """64 bins of 20 x 20 x 20, 12 lock-steps, greedy under NativePolicy(20, 400, form="auto") with fixed real weights: the
    rows the environment emits reach the kernel, and each step's logits are judged against torch_forward in float64 by
    e_native <= 8 e_torch32."""
    size = (20, 20, 20)
    env = bpp.BppVecEnv(64, size, pool=bpp.sequences.cut2_pool(size, 64, seed=0), device=DEV)
    plain = pc.real_weights(*G20, 11)
    policy = bpp.NativePolicy(20, env.action_space.n, form="auto").load_state_dict(plain).to(DEV)
    assert policy.geom == G20 and pc.pol.forward_info(policy.geom, 64, form=policy.form)["path"] == 2
    plain64 = {k: v.double() for k, v in plain.items()}
    obs, mask = env.reset(), env.location_masks
    seen = []
    for t in range(12):
        rows = obs.clone()
        _, logits, _ = policy(rows, want=("logits",))
        action, _ = bpp.masked_act(logits, mask, deterministic=True)
        host = rows.cpu()
        with torch.no_grad():
            l64 = pc.pol.torch_forward(plain64, host.double(), want=("logits",))[1].numpy()
            l32 = pc.pol.torch_forward(plain, host, want=("logits",))[1].numpy()
        pc.check_real({"logits": logits.cpu().numpy()}, {"logits": l64}, {"logits": l32}, "20^3 environment, lock-step %d:" % t)
        seen.append(host)
        res = env.step_tensors(action)
        obs, mask = res.obs, res.mask
    assert not torch.equal(seen[0], seen[-1]) and float(seen[-1][:, :400].max()) > 0    # the height maps have grown
