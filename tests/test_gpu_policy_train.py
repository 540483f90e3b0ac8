"""The trunk-training kernels (include/bpp_policy_train.h), bpp_amd.policy_trunk and bpp_amd.TrainablePolicy on
the device: the exact-integer networks of tests/policy_train_cases.py bit for bit, the training forward against the inference
forward's workspace, real-valued gradients against float64 torch autograd under the 8 x rule, real-valued outputs bit for bit
against the recorded bits of the header's arithmetic (tc.normative), the split identity, guarded buffers, independence of the batch, the
same bits on every run / on another stream / in a replayed graph / over a retained graph, the module against the reference's own
Policy (oracle/_ref/, where it is present) under a2c_loss, and examples/train_with_storage.py --native-trunk against its torch
stand-in."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_cases as pc  # noqa: E402
import policy_train_cases as tc  # noqa: E402
from oracle import ref_shims  # noqa: E402

pytestmark = pytest.mark.gpu
pol = pc.pol
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
G10 = (10, 256, 100)


@pytest.fixture(scope="module")
def lib():
    from bpp_amd import _lib
    return _lib.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


@pytest.fixture(scope="module")
def real10():
    """The 10 x 10 case on 16 recorded states with its device tensors and the outputs of one run; never modified."""
    case = tc.real_case(10, pc.deep_states(False, 16))
    t = {k: dev(case[k]) for k in ("obs", "blob", "blob_bwd", "grad_feat")}
    feat, acts = pol.trunk_forward_train(t["obs"], t["blob"], case["geom"])
    grads, gw = pol.trunk_backward(t["obs"], case["geom"], t["blob_bwd"], feat, acts, t["grad_feat"])
    torch.cuda.synchronize()
    return case, t, dict(feat=feat, acts=acts, grads=grads, gw=gw)


def run_all(t, geom, obs=None, grad_feat=None):
    obs = t["obs"] if obs is None else obs
    feat, acts = pol.trunk_forward_train(obs, t["blob"], geom)
    grads, gw = pol.trunk_backward(obs, geom, t["blob_bwd"], feat, acts, t["grad_feat"] if grad_feat is None else grad_feat)
    return dict(feat=feat, acts=acts, grads=grads, gw=gw)


def equal_bits(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


@pytest.mark.parametrize("name", sorted(tc.EXACT_SPECS))
def test_exact_integer_networks_equal_int64_numpy_bit_for_bit(lib, name):
    tc.check_exact(tc.device_runner(DEV), tc.exact_case(**tc.exact_spec(lib, name)))


@pytest.mark.parametrize("S,H,M,n", [(10, 256, 100, 5), (11, 32, 121, 3)])
def test_the_training_forward_leaves_the_bits_of_the_inference_forward(S, H, M, n):
    geom, A = (S, H, M), S * S
    blob = dev(pol.pack_weights(pc.real_weights(S, H, M, 11), S, H, M).numpy())
    obs = dev(pc.deep_states(False, n) if S == 10 else pc.synthetic_states(S, n))
    pol.policy_forward(obs, blob, geom)
    ws = pol._WORKSPACE[(obs.device, torch.cuda.current_stream(obs.device).cuda_stream, geom)][:n * 20 * A].clone()
    feat, acts = pol.trunk_forward_train(obs, blob, geom)
    assert torch.equal(feat.reshape(-1).view(torch.int32), ws.view(torch.int32)) and float(feat.max()) > 0
    assert not torch.isnan(acts).any()


def test_real_gradients_on_recorded_states(real10):
    """Device, 10 x 10, 16 recorded states.  Measured: e_native / e_torch32 between 0.84 and 5.5 (printed)."""
    case, _, out = real10
    got = tc.split_outputs(10, 16, *(out[k].cpu().numpy().reshape(-1) for k in ("feat", "acts", "grads", "gw")))
    tc.check_real(got, case["ref64"], case["ref32"], "device, S = 10, n = 16:")


def test_real_gradients_over_more_than_one_split(lib):
    case = tc.real_case(5, pc.synthetic_states(5, 70))
    assert tc.info(lib, case["geom"], 70)["splits"] == 2
    got = tc.device_runner(DEV)(case["obs"], case["geom"], case["blob"], case["blob_bwd"], case["grad_feat"])
    tc.check_real(got, case["ref64"], case["ref32"], "device, S = 5, n = 70:")


def test_real_gradients_at_the_size_of_the_reference_update():
    """n = 5 x 64 = 320 under the reference's initialisation (orthogonal, ReLU gain, biases 0; TrainablePolicy's own, seeded).
    The 320 states are the first of 400 recorded ones in which no pre-activation is within float32 rounding of zero
    (tc.tied_bins: with biases of 0 about one state in 300 has such a tie, and its float32 gradient is undefined)."""
    import bpp_amd
    torch.manual_seed(5)
    plain = {k: v.clone() for k, v in bpp_amd.TrainablePolicy(10, 100).state_dict().items()}
    obs = pc.deep_states(False, 400)
    tied = tc.tied_bins(plain, obs)
    print("states with a pre-activation tied at zero: %d of 400" % tied.sum())
    assert tied.sum() <= 12                                             # at most 3 %: the filter takes out ties, not states at large
    obs = obs[~tied][:320]
    assert obs.shape[0] == 320
    grad_feat = torch.randn(320, 2000, generator=torch.Generator().manual_seed(3)).numpy()
    blob, blob_bwd = tc.blobs(plain)
    got = tc.device_runner(DEV)(obs, G10, blob, blob_bwd, grad_feat)
    ref64, ref32 = (tc.trunk_autograd(plain, obs, grad_feat, dt) for dt in (torch.float64, torch.float32))
    tc.check_real(got, ref64, ref32, "device, S = 10, n = 320:")


def test_a_bin_gives_the_same_rows_alone_and_anywhere_in_a_batch(real10):
    case, t, _ = real10
    one = run_all(t, case["geom"], t["obs"][15:], t["grad_feat"][15:])
    for at in (0, 2, 4):
        obs, gf = t["obs"][:5].clone(), t["grad_feat"][:5].clone()
        obs[at], gf[at] = t["obs"][15], t["grad_feat"][15]
        got = run_all(t, case["geom"], obs, gf)
        A = 100
        G, G1 = got["grads"][:5 * 5 * 64 * A].reshape(5, 5, -1), one["grads"][:5 * 64 * A].reshape(5, 1, -1)
        assert torch.equal(G[:, at].view(torch.int32), G1[:, 0].view(torch.int32)) and not torch.equal(G[:, (at + 1) % 5], G1[:, 0]), at
        assert torch.equal(got["feat"][at].view(torch.int32), one["feat"][0].view(torch.int32)), at
        assert torch.equal(got["grads"][5 * 5 * 64 * A:].reshape(5, -1)[at], one["grads"][5 * 64 * A:]), at


def test_the_same_bits_on_every_run_and_on_another_stream(real10):
    case, t, first = real10
    assert equal_bits(run_all(t, case["geom"]), first)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = run_all(t, case["geom"])
    side.synchronize()
    assert equal_bits(got, first)


def test_a_replayed_graph_gives_the_bits_of_the_eager_calls(real10):
    case, t, first = real10
    geom, n = case["geom"], 16
    obs, gf = t["obs"].clone(), t["grad_feat"].clone()
    need = pol._lib.lib().bpp_policy_trunk_backward_workspace(pol._lib.kfac_geom(geom), n)
    buf = dict(feat=torch.empty_like(first["feat"]), acts=torch.empty_like(first["acts"]), grads=torch.empty_like(first["grads"]),
               gw=torch.empty_like(first["gw"]))
    ws = torch.empty(need // 4, dtype=torch.float32, device=DEV)

    def both():
        pol.trunk_forward_train(obs, t["blob"], geom, feat=buf["feat"], acts=buf["acts"])
        pol.trunk_backward(obs, geom, t["blob_bwd"], buf["feat"], buf["acts"], gf, grads=buf["grads"], grad_weights=buf["gw"], workspace=ws)

    both()                                                              # the opt-in to large LDS happens outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    graph.replay()
    torch.cuda.synchronize()
    assert equal_bits(buf, first)
    obs.copy_(t["obs"].flip(0))                                         # changed observations and a changed gradient
    gf.copy_(t["grad_feat"] * 0.5 + 1.0)
    graph.replay()
    torch.cuda.synchronize()
    replayed = {k: v.clone() for k, v in buf.items()}
    eager = run_all(t, geom, t["obs"].flip(0).contiguous(), t["grad_feat"] * 0.5 + 1.0)
    assert equal_bits(replayed, eager) and not equal_bits(replayed, first)


def test_two_backward_passes_over_a_retained_graph_give_equal_gradients(real10):
    import bpp_amd
    case, t, first = real10
    params = {k: case["plain"][k].to(DEV).requires_grad_(True) for k in pol.TRUNK_PARAMETERS}
    feat = bpp_amd.policy_trunk(t["obs"], params, 10)
    assert feat.requires_grad and torch.equal(feat.view(torch.int32), first["feat"].view(torch.int32))
    order = [params[k] for k in pol.TRUNK_PARAMETERS]
    g1 = torch.autograd.grad(feat, order, t["grad_feat"], retain_graph=True)
    g2 = torch.autograd.grad(feat, order, t["grad_feat"])
    named = pol.unpack_trunk_gradient(first["gw"])
    for k, a, b in zip(pol.TRUNK_PARAMETERS, g1, g2):
        assert a.shape == params[k].shape and torch.equal(a, b) and torch.equal(a, named[k]), k
    stale = bpp_amd.policy_trunk(t["obs"], params, 10)
    newer = bpp_amd.policy_trunk(t["obs"], params, 10)                  # a newer forward of the same key owns the activations now
    with pytest.raises(RuntimeError, match="overwritten"):
        stale.backward(t["grad_feat"])
    newer.backward(t["grad_feat"])
    assert all(torch.equal(p.grad, g) for p, g in zip(order, g1))


def _storage_rows(n=16):
    g = np.load(os.path.join(ROOT, "tests", "golden", "rollout_deep_cut2_10.npz"))
    pick = np.linspace(0, 240 * 8 - 1, n).astype(int)
    obs = g["obs"].reshape(-1, 400)[pick].astype(np.float32)
    mask = g["mask"].reshape(-1, 100)[pick].astype(np.float32)
    action = torch.from_numpy(mask).argmax(1)                          # a feasible action per state
    returns = torch.linspace(0.5, 8.0, n)
    return dev(obs), dev(mask), action.to(DEV), returns.to(DEV)


def _backward_from_outputs(outs, at_outputs):
    torch.autograd.backward(list(outs), [g.detach().cpu().to(o.dtype).reshape(o.shape) for g, o in zip(at_outputs, outs)])


def _plain_autograd(plain, obs, at_outputs, dtype):
    """torch_forward in `dtype` on the CPU, backward from the given gradients at (value, logits, pred): {name: gradient}."""
    w = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in plain.items()}
    _backward_from_outputs(pol.torch_forward(w, obs.cpu().to(dtype)), at_outputs)
    return {k: v.grad.numpy() for k, v in w.items()}


def _gradients_at_outputs(outputs, loss_backward):
    """The gradients loss_backward(*leaves) leaves at detached copies of the network's outputs."""
    leaves = [t.detach().clone().requires_grad_(True) for t in outputs]
    loss_backward(*leaves)
    return [t.grad.clone() for t in leaves]


def _untied(rows, state, count):
    """The first `count` of `rows` (obs first) whose float32 gradient is defined under the weights `state` (tc.tied_bins)."""
    keep = torch.from_numpy(np.nonzero(~tc.tied_bins(state, rows[0].cpu().numpy()))[0][:count]).to(DEV)
    assert keep.numel() == count
    return [r[keep].contiguous() for r in rows]


needs_copy = pytest.mark.skipif(not ref_shims.copy_available(), reason="oracle/_ref/ not present (python oracle/make_ref.py)")


@needs_copy
def test_the_module_against_the_reference_policy_under_a2c_loss():
    """The reference's own Policy (oracle/_ref/acktr/model.py through oracle/ref_shims), seeded, its biases made to count; its
    state dict loaded into TrainablePolicy; the loss is a2c_loss on 16 recorded states.  Every one of the 28 parameter gradients
    against the reference module's own float64 autograd, its own float32 autograd giving e_torch32; both are handed the gradients
    a2c_loss leaves at the module's outputs."""
    import types
    import bpp_amd
    ref_shims.install(ref_shims.REF_COPY)
    from acktr.model import Policy
    args = types.SimpleNamespace(channel=4, container_size=(10, 10, 10), pallet_size=10, enable_rotation=False)
    torch.manual_seed(5)
    ref = Policy((400,), bpp_amd.Discrete(100), base_kwargs={"recurrent": False, "hidden_size": 256, "args": args})
    with torch.no_grad():
        for p in ref.parameters():                                      # the reference starts every bias at 0: make them count
            if p.numel() == p.shape[0]:
                p.uniform_(-0.1, 0.1)
    net = bpp_amd.TrainablePolicy(10, 100).to(DEV)
    result = net.load_state_dict(ref.state_dict())
    assert not result.missing_keys and not result.unexpected_keys
    obs, mask, action, returns = _untied(_storage_rows(24), net.state_dict(), 16)
    net.zero_grad()
    value, logits, pred = net(obs)
    bpp_amd.a2c_loss(logits, value, pred, mask, action, returns).backward()
    mine = {k: p.grad.cpu().numpy() for k, p in net.named_parameters()}
    at_outputs = _gradients_at_outputs((value, logits, pred), lambda v, l, p: bpp_amd.a2c_loss(l, v, p, mask, action, returns).backward())

    def reference_autograd(module, x):
        module.zero_grad()
        v, features, _, p = module.base(x, None, None)
        _backward_from_outputs((v, module.dist.linear(features), p), at_outputs)
        out = {}
        for k, q in module.named_parameters():                          # the K-FAC bias split: <layer>.module.weight, <layer>.add_bias._bias
            name = k.replace("module.", "").replace("add_bias.", "").replace("_bias", "bias")
            out[name] = q.grad.numpy().reshape(mine[name].shape).copy()
        return out

    ref32 = reference_autograd(ref, obs.cpu())
    ref64 = reference_autograd(ref.double(), obs.cpu().double())
    assert sorted(mine) == sorted(ref64) and len(mine) == 28
    tc.check_gradients(mine, ref64, ref32, "module against the reference Policy, a2c_loss, 16 states:")


def test_the_module_round_trips_through_the_native_inference_policy():
    """state_dict() -> NativePolicy.refresh: the same feat bits, and the inference logits equal the module's under the 8 x rule
    (the Linear layers differ in order).  No gradient is taken: the forward keeps no activations."""
    import bpp_amd
    pol.clear_trunk_buffers()
    torch.manual_seed(5)
    net = bpp_amd.TrainablePolicy(10, 100).to(DEV)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.uniform_(-0.1, 0.1)
    obs = _storage_rows(16)[0]
    policy = bpp_amd.NativePolicy(10, 100, device=DEV).refresh(net)
    kept = net(obs)                                                     # a differentiable forward, then one under no_grad of the same n
    with torch.no_grad():
        value, logits, pred = net(obs)
        got = dict(zip(pc.HEADS, (t.cpu().numpy() for t in policy(obs))))
        feat = bpp_amd.policy_trunk(obs, net.named_weights(), 10)
        ws = pol._WORKSPACE[(obs.device, torch.cuda.current_stream(obs.device).cuda_stream, policy.geom)][:16 * 2000]
        assert torch.equal(feat.reshape(-1).view(torch.int32), ws.view(torch.int32))
        plain = {k: v.cpu() for k, v in net.state_dict().items()}
        ref64 = dict(zip(pc.HEADS, (t.numpy() for t in pol.torch_forward({k: v.double() for k, v in plain.items()}, obs.cpu().double()))))
        ref32 = dict(zip(pc.HEADS, (t.numpy() for t in pol.torch_forward(plain, obs.cpu()))))
    pc.check_real(got, ref64, ref32, "NativePolicy refreshed from the module:")
    pc.check_real(dict(value=value.cpu().numpy(), logits=logits.cpu().numpy(), pred=pred.cpu().numpy()), ref64, ref32, "the module's forward:")
    kept[1].sum().backward()                                            # the no_grad forwards did not take the activations away
    grad = dict(net.named_parameters())["base.share.0.weight"].grad
    assert grad is not None and torch.isfinite(grad).all() and float(grad.abs().max()) > 0
    assert len(net._trunk_cache) == 1                                   # the module's own buffers, one batch size
    assert all(b.acts is None for b in pol._TRUNK_BUFFERS.values())     # policy_trunk under no_grad kept no activations
    pol.clear_trunk_buffers()
    assert not pol._TRUNK_BUFFERS
    net.release_buffers()
    assert len(net._trunk_cache) == 0


class _StandIn:
    """The torch stand-in of examples/train_with_storage.NativeTrunkNet: torch_forward on given weights in a given dtype on the
    CPU, outputs in the example's order (logits, values [n, 1], pred_mask)."""

    def __init__(self, plain, dtype):
        self.w = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in plain.items()}
        self.dtype = dtype

    def __call__(self, obs):
        value, logits, pred = pol.torch_forward(self.w, obs.cpu().to(self.dtype))
        return logits, value.reshape(-1, 1), pred

    def gradients(self, obs, at_outputs):
        _backward_from_outputs(self(obs), at_outputs)
        return {k: v.grad.numpy() for k, v in self.w.items()}


@pytest.mark.parametrize("fused_loss", [True, False], ids=["fused_loss", "autograd_loss"])
def test_the_first_update_of_the_example_against_the_torch_stand_in(fused_loss):
    """One update driven through the public pieces of examples/train_with_storage.py as train(native_trunk=True) drives them:
    NativeTrunkNet, collect, then fused_gradients (storage.a2c_loss) or loss_terms + total_loss.  The gradients this leaves on
    the parameters are compared, all 28, against the torch stand-in holding the same weights on the same storage contents in
    float64 (float32 for e_torch32); the stand-in is handed the gradients the example's own loss leaves at the outputs of
    `net`, in `net`'s output order.  States whose float32 gradient is undefined (tc.tied_bins; at most 5 %) are overwritten in
    the storage by the first state that is defined, before the example's update reads it."""
    import bpp_amd
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_with_storage as ex
    size, envs, steps, seed = (10, 10, 10), 64, 5, 0
    torch.manual_seed(seed)
    env = bpp_amd.BppVecEnv(envs, size, pool=bpp_amd.sequences.cut2_pool(size, 1024, seed=seed), device=torch.device(DEV))
    net = ex.NativeTrunkNet(size[0], env.action_space.n).to(DEV)
    actor = bpp_amd.NativePolicy(size[0], env.action_space.n, device=DEV).refresh(net.policy)
    optimizer = torch.optim.RMSprop(net.parameters(), 7e-4, eps=1e-5, alpha=0.99)
    storage = bpp_amd.RolloutStorage(steps, env, env.observation_space.shape, env.action_space)
    storage.reset(env)
    counter = torch.tensor([seed, 0], dtype=torch.int64, device=DEV)
    ex.collect(net, actor, env, storage, counter, 1.0)
    E = steps * envs
    tied = np.nonzero(tc.tied_bins(net.policy.state_dict(), storage.obs[:-1].reshape(E, -1).float().cpu().numpy()))[0]
    print("tied states overwritten in the storage: %d of %d" % (len(tied), E))
    assert len(tied) <= E // 20
    good = next(i for i in range(E) if i not in set(tied))
    for i in tied:
        for name in ("obs", "location_masks", "actions", "returns"):
            storage._slabs[name][i // envs, i % envs] = storage._slabs[name][good // envs, good % envs]
    obs = storage.obs[:-1].view(E, -1)

    if fused_loss:
        ex.fused_gradients(net, optimizer, storage, ex.COEFS)

        def loss_backward(logits, values, pred_mask):
            c = ex.COEFS
            storage.a2c_loss(logits, values, pred_mask, value_loss_coef=c[0], entropy_coef=c[1], invalid_coef=c[2], mask_coef=c[3]).backward()
    else:
        optimizer.zero_grad()
        ex.total_loss(ex.loss_terms(*net(obs), storage), ex.COEFS).backward()

        def loss_backward(logits, values, pred_mask):
            ex.total_loss(ex.loss_terms(logits, values, pred_mask, storage), ex.COEFS).backward()

    mine = {k: p.grad.cpu().numpy().copy() for k, p in net.policy.named_parameters()}
    with torch.no_grad():
        outputs = net(obs)
    assert tuple(outputs[0].shape) == (E, 100) and tuple(outputs[1].shape) == (E, 1) and tuple(outputs[2].shape) == (E, 100)
    at_outputs = _gradients_at_outputs(outputs, loss_backward)
    plain = net.policy.state_dict()
    ref64, ref32 = (_StandIn(plain, dt).gradients(obs, at_outputs) for dt in (torch.float64, torch.float32))
    assert sorted(mine) == sorted(ref64) and len(mine) == 28
    tc.check_gradients(mine, ref64, ref32, "example, first update, %s:" % ("fused loss" if fused_loss else "autograd loss"))
    env.close()


def test_the_example_trains_through_the_native_trunk():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_with_storage as ex
    fused = ex.train(envs=64, updates=2, native_trunk=True, fused_loss=True, verbose=False)
    plain = ex.train(envs=64, updates=2, native_trunk=True, verbose=False)
    for history in (fused, plain):
        assert len(history) == 2 and all(np.isfinite(v) for terms in history for v in terms)
    with pytest.raises(ValueError, match="native-trunk"):
        ex.train(envs=64, updates=1, native_trunk=True, acktr=True, verbose=False)


# ------------------------------------------------------------------------- the header's arithmetic, bit for bit (tc.normative)
@pytest.mark.parametrize("S,n", sorted(tc.TRAIN_CHAIN_CASES))
def test_real_valued_chains_equal_the_headers_arithmetic_bit_for_bit(lib, S, n):
    """Device: feat, acts, grads, gf' and grad_weights on real-valued data against the recorded bits of tc.normative
    (tests/golden/make_trunk_train_chain_bits.py): the CRC32 of every output, one forward and one backward call per case."""
    splits, last, P = tc.TRAIN_CHAIN_CASES[(S, n)]
    i = tc.info(lib, tc.geom_of(S), n)
    assert i["splits"] == splits and n - (splits - 1) * i["bins_per_split"] == last and (P is None or i["bins_per_group"] == P)
    case, name, bits = tc.train_chain_case(S, n), tc.train_chain_name(S, n), tc.load_fixture(tc.TRAIN_CHAIN_FIXTURE)
    for k in tc.TRAIN_CHAIN_INPUTS:
        assert pc.crc(case[k]) == bits["%s.crc.%s" % (name, k)], k
    got = tc.device_runner(DEV)(case["obs"], case["geom"], case["blob"], case["blob_bwd"], case["grad_feat"])
    tc.check_train_chain(got, bits, name, "device:")


@pytest.mark.parametrize("S,n,splits", [(3, 150, 3), (10, 21, 3)])
def test_the_whole_batch_is_the_double_sum_of_its_splits(lib, S, n, splits):
    i = tc.info(lib, tc.geom_of(S), n)
    assert i["splits"] == splits and i["bins_per_split"] == tc.header_bins_per_split(S)
    differing = tc.check_split_identity(tc.device_runner(DEV), tc.train_chain_case(S, n), i["bins_per_split"])
    print("S = %d, n = %d: a float32 sum of the splits differs in %d floats" % (S, n, differing))


@pytest.mark.parametrize("name", ["s10_nP1", "s7_nP1", "s15_n2"])
def test_nothing_is_stored_outside_the_outputs(lib, name):
    """Outputs and workspace as slices of larger device tensors (tc.guarded_buffers): 1024 guard floats on either side of each
    and the workspace beyond the stated bytes untouched, every output float written, the bits of the plain runner."""
    case = tc.exact_case(**tc.exact_spec(lib, name))
    got = tc.check_exact(tc.guarded_device_runner(lib, DEV), case)
    plain = tc.device_runner(DEV)(case["obs"], case["geom"], case["blob"], case["blob_bwd"], case["grad_feat"])
    assert all(pc.same_bits(got[k], plain[k]) for k in tc.OUTPUTS)


@pytest.mark.parametrize("n", [1, 3])
def test_policy_trunk_on_a_column_slice_and_a_strided_gradient(real10, n):
    """obs a column slice of a wider tensor (stride(0) > 4 A, every other column NaN), the backward from feat[:, ::2].sum(), whose
    gradient at feat is not contiguous: the bits of the contiguous call."""
    import bpp_amd
    case, t, _ = real10
    order = lambda p: [p[k] for k in pol.TRUNK_PARAMETERS]        # noqa: E731
    wide = torch.full((n, 5 + 400 + 32), float("nan"), device=DEV)
    wide[:, 5:405] = t["obs"][:n]
    obs = wide[:, 5:405]
    assert obs.stride(0) == 437 and obs.data_ptr() != wide.data_ptr()
    p1 = {k: case["plain"][k].to(DEV).requires_grad_(True) for k in pol.TRUNK_PARAMETERS}
    feat = bpp_amd.policy_trunk(obs, p1, 10, cache={})
    g1 = torch.autograd.grad(feat[:, ::2].sum(), order(p1))
    p2 = {k: case["plain"][k].to(DEV).requires_grad_(True) for k in pol.TRUNK_PARAMETERS}
    same = bpp_amd.policy_trunk(t["obs"][:n].contiguous(), p2, 10, cache={})
    at_feat = torch.zeros(n, 2000, device=DEV)
    at_feat[:, ::2] = 1.0
    g2 = torch.autograd.grad(same, order(p2), at_feat)
    assert torch.equal(feat.view(torch.int32), same.view(torch.int32)) and not torch.isnan(feat).any() and float(feat.detach().max()) > 0
    for k, a, b in zip(pol.TRUNK_PARAMETERS, g1, g2):
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)) and float(a.abs().max()) > 0, k
