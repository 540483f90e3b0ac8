"""bpp_policy_forward and bpp_amd.NativePolicy on the device (include/bpp_policy.h): the cases and checks of
tests/test_policy_forward.py through bpp_amd.policy_forward -- here the MFMA itself runs, at the shipped shapes and across the
accepted ones, and is compared with the emulator's recorded chain bits --, batch independence across runs,
streams and a replayed graph, act(), and the reference's checkpoints: every recorded state of the 2 100 trajectories teacher-forced,
then the whole-set evaluation of examples/evaluate_checkpoint.py --native.  Reads nothing of the reference."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_cases as pc  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
G10, G5 = (10, 256, 100), (5, 32, 25)
CHECKPOINTS = [("pretrained_eval_cut2_10", False, "default_cut_2.pt"), ("pretrained_eval_cut2_10_rot", True, "rotation_cut_2.pt")]


@pytest.fixture(scope="module")
def bpp():
    import bpp_amd
    assert torch.cuda.is_available()
    return bpp_amd


@pytest.fixture(scope="module")
def tiles(bpp):
    i = pc.info(bpp._lib.lib(), G10, 1)
    return i["bins_per_trunk_group"], i["bins_per_head_tile"]


@pytest.fixture(scope="module")
def real_policy(bpp):
    """(case, NativePolicy on the device, its outputs on the case's 16 states), computed once."""
    case = pc.real_case(False)
    policy = bpp.NativePolicy(10, 100).load_state_dict(case["plain"]).to(DEV)
    obs = torch.from_numpy(case["obs"]).to(DEV)
    out = [t.clone() for t in policy(obs)]
    return case, policy, obs, out


def tiled(case, n):
    """`case` repeated to n rows: row i is row i mod m."""
    pick = np.arange(n) % case["obs"].shape[0]
    return dict(case, obs=case["obs"][pick], want={h: v[pick] for h, v in case["want"].items()})


@pytest.mark.parametrize("name", sorted(pc.exact_specs(2, 64)))
def test_gpu_exact_integer_networks_equal_int64_numpy_bit_for_bit(bpp, tiles, name):
    spec = pc.exact_specs(*tiles, bins=lambda g: pc.info(bpp._lib.lib(), g, 1)["bins_per_trunk_group"])[name]
    pc.check_exact(pc.device_runner(DEV), pc.exact_case(*spec))


@pytest.mark.parametrize("n", [257, 1025])
def test_gpu_exact_network_on_more_bins_than_compute_units(bpp, n):
    """One more bin than the device has compute units, and 1 025: 41 distinct states repeated."""
    pc.check_exact(pc.device_runner(DEV), tiled(pc.exact_case(10, 256, 100, 41, 31), n))


@pytest.mark.parametrize("rot", [False, True])
def test_gpu_real_networks_within_eight_times_the_float32_torch_error(bpp, rot):
    case = pc.real_case(rot)
    got = pc.device_runner(DEV)(case["obs"], case["geom"], case["blob"])
    pc.check_real(got, case["ref64"], case["ref32"], "device, rotation %d:" % rot)


@pytest.mark.parametrize("geom", pc.WIDE_REAL, ids=lambda g: "s%d_h%d_m%d" % tuple(g))
def test_gpu_real_networks_at_the_other_accepted_shapes(bpp, geom):
    """16 synthetic states against the float64 forward under the same rule; the ratios are printed."""
    case = pc.wide_real_case(*geom)
    pc.check_real(pc.device_runner(DEV)(case["obs"], case["geom"], case["blob"]), case["ref64"], case["ref32"], "device, %r:" % (geom,))


@pytest.mark.parametrize("geom", [(12, 96, 144), (15, 512, 450)], ids=lambda g: "s%d_h%d_m%d" % tuple(g))
def test_gpu_a_bin_gives_the_same_bits_where_every_workgroup_is_another_bin(bpp, geom):
    """P = 1: one state alone, and as first / middle / last row of n = 3."""
    assert pc.info(bpp._lib.lib(), geom, 3)["bins_per_trunk_group"] == 1
    run = pc.device_runner(DEV)
    blob = pc.pol.pack_weights(pc.real_weights(*geom, 11), *geom).numpy()
    states = pc.synthetic_states(geom[0], 4)
    one = run(states[3:4], geom, blob)
    for rows in ((3, 0, 3), (1, 3, 2)):
        got = run(states[list(rows)], geom, blob)
        for at, r in enumerate(rows):
            for h in pc.HEADS:
                assert pc.same_bits(got[h][at], one[h][0]) == (r == 3), (h, rows, at)


def test_gpu_a_bin_gives_the_same_bits_over_two_passes_of_the_hidden_layer(bpp, tiles):
    """(5, 512, 25): n = 1, n = T + 1 in rows 0, 32 and 64, and a view whose rows lie 103 floats apart."""
    P, T = tiles
    policy = bpp.NativePolicy(5, 25, 512).load_state_dict(pc.real_weights(5, 512, 25, 11)).to(DEV)
    states = torch.from_numpy(pc.synthetic_states(5, T + 2)).to(DEV)
    one = policy(states[T + 1:])
    batch = states[:T + 1].clone()
    batch[[0, T // 2, T]] = states[T + 1]
    got = policy(batch)
    for at in (0, T // 2, T):
        assert all(torch.equal(a[at], b[0]) for a, b in zip(got, one)), at
        assert not torch.equal(got[1][at + 1 if at < T else 1], one[1][0])
    padded = torch.full((P + 1, 103), 9.0, device=DEV)
    padded[:, :100] = states[:P + 1]
    padded[P, :100] = states[T + 1]
    got = policy(padded[:, :100])
    assert padded[:, :100].stride(0) == 103 and all(torch.equal(a[P], b[0]) for a, b in zip(got, one))


def test_gpu_the_largest_policy_grows_its_workspace_and_acts(bpp):
    """NativePolicy(15, 450, 512): n = 1, then n = 70 -- the workspace of this stream and geometry grows -- gives the n = 1 bits in
    its row; act() on the 70 bins is masked_act on the same logits."""
    policy = bpp.NativePolicy(15, 450, 512).load_state_dict(pc.real_weights(15, 512, 450, 11)).to(DEV)
    states = torch.from_numpy(pc.synthetic_states(15, 70)).to(DEV)
    key = (states.device, torch.cuda.current_stream(DEV).cuda_stream, policy.geom)
    pc.pol._WORKSPACE.pop(key, None)
    one = [t.clone() for t in policy(states[41:42])]
    small = pc.pol._WORKSPACE[key].numel()
    out = policy(states)
    assert small == 20 * 225 and pc.pol._WORKSPACE[key].numel() == 70 * small
    assert all(torch.equal(a[41], b[0]) for a, b in zip(out, one)) and not torch.equal(out[1][40], one[1][0])
    again = policy(states[41:42])                                                   # the grown workspace serves n = 1 as well
    assert pc.pol._WORKSPACE[key].numel() == 70 * small and all(torch.equal(a, b) for a, b in zip(again, one))
    mask = torch.from_numpy((np.random.RandomState(3).rand(70, 450) < 0.3).astype(np.float32)).to(DEV)
    mask[:, 7] = 1.0
    for det, kw in ((True, {}), (False, dict(seed=5, step=3))):
        value, action, logp = policy.act(states, mask, deterministic=det, **kw)
        a2, lp2 = bpp.masked_act(out[1], mask, deterministic=det, **kw)
        assert torch.equal(action, a2) and torch.equal(logp, lp2) and action.shape == (70, 1)
        assert torch.equal(value.reshape(-1), out[0])


def test_gpu_the_mfma_gives_the_bits_of_the_emulators_fmaf_chain(bpp):
    """tests/golden/mfma_chain_emulator_bits.npz: real-valued networks at five shapes, every head.  The inputs are regenerated
    here and their CRC32 compared first; then v_mfma_f32_32x32x2_f32 on the device against the sequential fmaf chain of the
    emulator, bit for bit.  The largest distance per case is printed in float32 ulps."""
    g = load_golden(pc.CHAIN_FIXTURE)
    for spec in pc.CHAIN_CASES:
        got = pc.chain_entries(pc.device_runner(DEV), spec)
        name = pc.chain_name(*spec)
        for key in got:
            if ".crc." in key:
                assert got[key] == g[key], ("%s: the inputs regenerated here are not the bytes tests/golden/make_mfma_chain_bits.py "
                                            "drew (numpy's RandomState or the packing, not the kernel)" % key)
        dist = {h: pc.ulps(got[name + "." + h], g[name + "." + h]) for h in pc.HEADS}
        print("%s: device against emulator, ulps per head: %r" % (name, dist))
        assert all(d == 0 for d in dist.values()), (name, dist)


def test_gpu_a_bin_gives_the_same_bits_in_every_batch_run_and_stream(bpp, tiles, real_policy):
    P, T = tiles
    case, policy, obs, out = real_policy
    again = policy(obs)
    assert all(torch.equal(a, b) for a, b in zip(again, out))                       # two runs
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = policy(obs)
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(other, out))                       # another stream
    alone = policy(obs[3:4])
    assert all(torch.equal(a[0], b[3]) for a, b in zip(alone, out))                 # n = 1
    rng = np.random.RandomState(2)
    filler = torch.from_numpy(rng.randint(0, 6, (T + 1, 400)).astype(np.float32)).to(DEV)
    for n in (P + 1, T + 1):
        for at in (0, n // 2, n - 1):
            batch = filler[:n].clone()
            batch[at] = obs[3]
            got = policy(batch)
            assert all(torch.equal(a[at], b[3]) for a, b in zip(got, out)), (n, at)
    padded = torch.full((P + 1, 403), 9.0, device=DEV)
    padded[:, :400] = filler[:P + 1]
    padded[P, :400] = obs[3]
    got = policy(padded[:, :400])                                                   # a view: rows 403 floats apart
    assert padded[:, :400].stride(0) == 403 and all(torch.equal(a[P], b[3]) for a, b in zip(got, out))
    for want in (("value",), ("logits",), ("pred",), ("value", "pred")):             # a head left out changes nothing
        got = policy(obs, want=want)
        for h, a, b in zip(pc.HEADS, got, out):
            assert (a is None) if h not in want else torch.equal(a, b), (want, h)


def test_gpu_a_replayed_graph_on_changed_observations_equals_the_eager_call(bpp, real_policy):
    case, policy, obs, out = real_policy
    static = obs.clone()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        policy(static)                                                              # warm-up: workspace and LDS opt-in exist
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = policy(static)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(captured, out))
    changed = torch.from_numpy(pc.deep_states(False, 24)[8:]).to(DEV)               # 16 other states
    assert not torch.equal(changed, obs)
    static.copy_(changed)
    graph.replay()
    torch.cuda.synchronize()
    eager = policy(changed)
    assert all(torch.equal(a, b) for a, b in zip(captured, eager))
    assert not torch.equal(eager[1], out[1])


def test_gpu_act_is_masked_act_on_its_own_logits_and_leaves_value_alone(bpp, real_policy):
    case, policy, obs, out = real_policy
    g = load_golden("rollout_deep_cut2_10")
    masks = g["mask"].reshape(-1, 100)
    mask = torch.from_numpy(masks[np.linspace(0, masks.shape[0] - 1, 16).astype(int)].astype(np.float32)).to(DEV)
    for det, kw in ((True, {}), (False, dict(seed=5, step=3))):
        value, action, logp = policy.act(obs, mask, deterministic=det, **kw)
        a2, lp2 = bpp.masked_act(out[1], mask, deterministic=det, **kw)
        assert torch.equal(action, a2) and torch.equal(logp, lp2) and action.shape == (16, 1) and action.dtype == torch.int64
        assert value.shape == (16, 1) and torch.equal(value.reshape(-1), out[0])
    from bpp_amd.reorder import check_policy_output
    check_policy_output(policy(obs), 16, 100)


def _checkpoint(ckpt):
    from oracle import ref_shims
    path = os.path.join(ref_shims.REF_COPY, "pretrained_models", ckpt)
    if not ref_shims.copy_available() or not os.path.isfile(path):
        pytest.skip("oracle/_ref/ without the checkpoints (python oracle/make_ref.py)")
    return path, os.path.join(ref_shims.REF_COPY, "dataset", "cut_2.pt")


@pytest.mark.parametrize("case,rot,ckpt", CHECKPOINTS)
def test_gpu_teacher_forced_actions_of_the_reference_checkpoints(bpp, case, rot, ckpt):
    """The recorded actions of all 2 100 trajectories replayed as one batch; at every lock-step NativePolicy.act(deterministic)
    on the live bins against the recorded action.  At most 0.1 % of the live states may differ, and each that does must be a
    near-tie: in a float64 torch_forward of that state the masked probabilities of the two actions differ by less than
    8 * e_torch32 * the row's largest probability (e_torch32: the float32 CPU torch_forward's relative logit error on those states)."""
    path, _ = _checkpoint(ckpt)
    g = load_golden(case)
    size = tuple(int(v) for v in g["size"])
    pool = load_golden("cut2_dataset_10")["pool"]
    n, T = g["actions"].shape
    env = bpp.BppVecEnv(n, size, enable_rotation=bool(rot), pool=pool, device=DEV)
    policy = bpp.NativePolicy.from_checkpoint(path, size[0], env.action_space.n).to(DEV)
    recorded = torch.from_numpy(g["actions"].astype(np.int64)).to(DEV)
    steps = torch.from_numpy(g["steps"].astype(np.int64)).to(DEV)
    noop = torch.full((n,), env.NOOP, dtype=torch.int64, device=DEV)
    obs, mask = env.reset(), env.location_masks
    live_states, odd = 0, []
    for t in range(T):
        live = t < steps
        _, action, _ = policy.act(obs, mask, deterministic=True)
        differs = live & (action.reshape(-1) != recorded[:, t])
        live_states += int(live.sum())
        for b in torch.nonzero(differs).reshape(-1).tolist():
            odd.append((obs[b].cpu(), mask[b].cpu(), int(recorded[b, t]), int(action[b, 0])))
        res = env.step_tensors(torch.where(live, recorded[:, t], noop))
        obs, mask = res.obs, res.mask
    print("%s: %d of %d live states differ from the recorded action" % (case, len(odd), live_states))
    assert len(odd) <= 0.001 * live_states, (len(odd), live_states)
    if odd:
        plain = policy.to("cpu").unpack()
        x = torch.stack([o for o, _, _, _ in odd]).float()
        m = torch.stack([k for _, k, _, _ in odd]).double()
        with torch.no_grad():
            l64 = pc.pol.torch_forward({k: v.double() for k, v in plain.items()}, x.double())[1]
            l32 = pc.pol.torch_forward(plain, x)[1]
        pc.check_near_ties(l64, l32, m, [a for _, _, a, _ in odd], [a for _, _, _, a in odd])


def test_gpu_native_policy_from_an_actor_on_the_device(bpp):
    """examples/rollout_with_policy.py --native: the Actor's weights lie on the device, the zeros that stand in for the critic
    and mask heads on the host; the packed policy's logits are the Actor's (float64 on the host as the reference, the Actor's own
    float32 forward on the host giving e_torch32)."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import rollout_with_policy as ex
    import copy
    torch.manual_seed(3)
    actor = ex.Actor(10, 200).eval()
    with torch.no_grad():
        for p in actor.parameters():
            if p.dim() == 1:
                p.uniform_(-0.1, 0.1)
        host = torch.from_numpy(pc.deep_states(True, 16))
        l32 = actor(host).numpy()                                                   # the float32 torch forward on the host
        l64 = copy.deepcopy(actor).double()(host.double()).numpy()
    policy = ex.native_from_actor(actor.to(DEV))
    assert policy.weights.device == torch.device(DEV) and policy.geom == (10, 256, 200)
    obs = host.to(DEV)
    value, logits, pred = policy(obs, want=("logits",))
    assert value is None and pred is None
    e_native, e_torch32 = pc.rel_err(logits.cpu().numpy(), l64), pc.rel_err(l32, l64)
    print("actor on the device: e_native %.3g, e_torch32 %.3g" % (e_native, e_torch32))
    assert e_torch32 > 0 and e_native <= pc.FACTOR * e_torch32, (e_native, e_torch32)
    assert float(policy(obs)[0].abs().max()) == 0.0                                 # the critic head is zeros


@pytest.mark.parametrize("case,rot,ckpt", CHECKPOINTS)
def test_gpu_whole_set_evaluation_with_the_native_policy(bpp, case, rot, ckpt):
    """examples/evaluate_checkpoint.py --native: it finishes and reports its two means, written beside the reference's; at least
    99 % of the trajectories end identical to the recording (the per-state test above is the parity statement)."""
    path, dataset = _checkpoint(ckpt)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_checkpoint as ev
    g = load_golden(case)
    r = ev.evaluate(path, dataset, rotation=rot, native=True)
    same = (r["ratio"] == g["ratio"]) & (r["counter"] == g["counter"])
    out = {"checkpoint": "pretrained_models/" + ckpt, "policy": "bpp_amd.NativePolicy (bpp_policy_forward, logits only)",
           "trajectories": int(len(same)), "lock_steps": int(r["lock_steps"]), "seconds": round(float(r["seconds"]), 3),
           "mean_space_utilisation": float(r["ratio"].mean()), "mean_items_packed": float(r["counter"].mean()),
           "reference": {"mean_space_utilisation": float(g["ratio"].mean()), "mean_items_packed": float(g["counter"].mean())},
           "trajectories_identical_to_the_last_digit": int(same.sum())}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "policy_eval_native_%s.json" % case.replace("pretrained_eval_", "")), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    assert np.isfinite(r["ratio"]).all() and r["ratio"].mean() > 0 and r["counter"].mean() > 0
    assert same.mean() >= 0.99, same.mean()
