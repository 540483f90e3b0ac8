"""The head-training kernels (include/bpp_policy_heads_train.h), bpp_amd.policy_heads and
bpp_amd.TrainablePolicy(heads="native") on the device: the exact-integer heads of tests/policy_heads_train_cases.py bit for bit,
the training forward against both forms of the inference forward, real-valued outputs bit for bit against the recorded bits of
the header's arithmetic (hc.normative_heads), the split identity, real-valued gradients against float64 torch autograd under
the 8 x rule, the whole module under a2c_loss, independence of the batch, guarded buffers, the same bits in a replayed graph /
over a retained graph / from a strided gradient, the Python-side refusals, and examples/train_with_storage.py --native-heads
against its torch stand-in."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_cases as pc  # noqa: E402
import policy_heads_train_cases as hc  # noqa: E402
import policy_train_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu
pol = pc.pol
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
G10, G5 = (10, 256, 100), (5, 32, 25)
KEYS = ("feat", "grad_value", "grad_logits", "grad_pred")


@pytest.fixture(scope="module")
def lib():
    from bpp_amd import _lib
    return _lib.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def exact_shapes(L):
    B = hc.info(L, hc.EXACT_SPLIT_GEOM, 1)["bins_per_split"]
    assert B == hc.BINS_PER_SPLIT
    return hc.EXACT_SHAPES + [hc.EXACT_SPLIT_GEOM + (B + 1,), hc.EXACT_SPLIT_GEOM + (2 * B + 1,)]


@pytest.mark.parametrize("at", range(len(hc.EXACT_SHAPES) + 2))
def test_exact_integer_heads_equal_int64_numpy_bit_for_bit(lib, at):
    hc.check_exact(hc.device_runner(DEV), hc.exact_case(*exact_shapes(lib)[at]))


@pytest.mark.parametrize("S,H,M,n,form", [(10, 256, 100, 5, "two_images"), (11, 32, 121, 3, "two_images"), (20, 32, 400, 3, "one_image")])
def test_the_training_forward_leaves_the_bits_of_the_inference_forward(S, H, M, n, form):
    geom, A = (S, H, M), S * S
    blob = dev(pol.pack_weights(pc.real_weights(S, H, M, 11), S, H, M).numpy())
    obs = dev(pc.deep_states(False, n) if S == 10 else pc.synthetic_states(S, n))
    want = pol.policy_forward(obs, blob, geom, form=form)
    feat = pol._WORKSPACE[(obs.device, torch.cuda.current_stream(obs.device).cuda_stream, geom)][:n * 20 * A].clone().view(n, 20 * A)
    value, logits, pred, hidden = pol.heads_forward_train(feat, blob, geom)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((value, logits, pred), want))
    assert not torch.isnan(hidden).any() and float(hidden.max()) > 0 and float(hidden.min()) == 0


@pytest.mark.parametrize("spec", hc.CHAIN_CASES)
def test_real_valued_chains_equal_the_headers_arithmetic_bit_for_bit(lib, spec):
    """Device: every output on real-valued data against the recorded bits of hc.normative_heads
    (tests/golden/make_heads_train_chain_bits.py): the CRC32 of every output, 0 ulps everywhere."""
    case, name, recorded = hc.chain_case(*spec), hc.chain_name(*spec), tc.load_fixture(hc.CHAIN_FIXTURE)
    assert hc.info(lib, spec[:3], spec[3])["splits"] == -(-spec[3] // hc.BINS_PER_SPLIT)
    for k in hc.CHAIN_INPUTS:
        assert pc.crc(case[k]) == recorded["%s.crc.%s" % (name, k)], k
    hc.check_chain(hc.run_case(hc.device_runner(DEV), case), recorded, name, "device:")


def test_the_whole_batch_is_the_double_sum_of_its_splits(lib):
    spec = (2, 32, 4, 300)
    i = hc.info(lib, spec[:3], spec[3])
    assert i["splits"] == 3 and i["bins_per_split"] == hc.BINS_PER_SPLIT
    differing = hc.check_split_identity(hc.device_runner(DEV), hc.chain_case(*spec), i["bins_per_split"])
    print("%r: a float32 sum of the splits differs in %d floats" % (spec, differing))


@pytest.mark.parametrize("geom,n", [(G10, 16), (G5, 70)])
def test_real_gradients_within_eight_times_the_float32_autograd_error(geom, n):
    """Device, against float64 torch autograd over the same six Linear layers on the same feat.  Measured: e_native / e_torch32
    between 1.00 and 2.24 at 10 x 10 and between 0.87 and 7.10 (the bias of critic_linear) at 5 x 5 (printed)."""
    case = hc.real_case(geom, pc.deep_states(False, n) if geom[0] == 10 else pc.synthetic_states(geom[0], n))
    assert not hc.head_ties(case["plain"], case["feat"]).any()
    hc.check_real(hc.run_case(hc.device_runner(DEV), case), case, "device, %r, n = %d:" % (geom, n))


def test_a_row_gives_the_same_bits_in_any_batch():
    case = hc.chain_case(5, 32, 25, 6)
    run = hc.device_runner(DEV)
    one = hc.run_case(run, case, **{k: case[k][5:] for k in KEYS})
    for at in (0, 2, 4):
        rows = {k: case[k][:5].copy() for k in KEYS}
        for k in KEYS:
            rows[k][at] = case[k][5]
        got = hc.run_case(run, case, **rows)
        for key in hc.ROW_OUTPUTS:
            assert pc.same_bits(got[key][at], one[key][0]) and not pc.same_bits(got[key][(at + 1) % 5], one[key][0]), (key, at)
        for key in ("hidden", "grad_hidden"):
            assert pc.same_bits(got[key][:, at], one[key][:, 0]) and not pc.same_bits(got[key][:, (at + 1) % 5], one[key][:, 0]), (key, at)


@pytest.mark.parametrize("spec", [(3, 64, 9, 63), (3, 64, 9, 65), (2, 32, 4, 129)])
def test_nothing_is_stored_outside_the_outputs(lib, spec):
    """Outputs and workspace as slices of larger device tensors: 1024 guard floats on either side of each untouched, every
    output float written, the bits of the plain runner; the zeros of an absent head, also into guarded buffers."""
    case = hc.exact_case(*spec)
    got = hc.check_exact(hc.guarded_device_runner(lib, DEV), case)
    plain = hc.run_case(hc.device_runner(DEV), case)
    assert all(pc.same_bits(got[k], plain[k]) for k in hc.OUTPUTS)
    hc.check_absent_heads(hc.guarded_device_runner(lib, DEV), case)


# ------------------------------------------------------------------------------------------------------------- the whole module
def _rows(n):
    """(obs, mask, action, returns) on the device: the states of pc.deep_states(False, n) with a feasible action each."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "rollout_deep_cut2_10.npz"))
    obs, mask = g["obs"].reshape(-1, g["obs"].shape[-1]), g["mask"].reshape(-1, 100)
    pick = np.linspace(0, obs.shape[0] - 1, n).astype(int)
    obs, mask = obs[pick].astype(np.float32), mask[np.minimum(pick, mask.shape[0] - 1)].astype(np.float32)
    assert np.array_equal(obs, pc.deep_states(False, n))
    mask[mask.sum(1) == 0, 0] = 1.0
    return obs, mask, torch.from_numpy(mask).argmax(1).numpy(), np.linspace(0.5, 8.0, n).astype(np.float32)


def _module_against_float64(net, obs, mask, action, returns, label):
    """All 28 parameter gradients of `net` under a2c_loss against float64 autograd of torch_forward on the same parameters
    (float32 autograd gives e_torch32), both handed the gradients a2c_loss leaves at the module's outputs; value / logits / pred
    bit-equal to NativePolicy refreshed from the module."""
    import bpp_amd
    obs, mask, returns = dev(obs), dev(mask), dev(returns)
    action = torch.from_numpy(np.asarray(action)).to(DEV)
    net.zero_grad()
    value, logits, pred = net(obs)
    bpp_amd.a2c_loss(logits, value, pred, mask, action, returns).backward()
    mine = {k: p.grad.cpu().numpy().copy() for k, p in net.named_parameters()}
    policy = bpp_amd.NativePolicy(net.side, net.n_actions, net.hidden, device=DEV).refresh(net)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((value, logits, pred), policy(obs)))
    leaves = [t.detach().clone().requires_grad_(True) for t in (value, logits, pred)]
    bpp_amd.a2c_loss(leaves[1], leaves[0], leaves[2], mask, action, returns).backward()
    at_outputs = [t.grad.cpu() for t in leaves]
    plain = {k: v.detach().cpu() for k, v in net.state_dict().items()}

    def autograd(dtype):
        w = {k: v.to(dtype).requires_grad_(True) for k, v in plain.items()}
        outs = pol.torch_forward(w, obs.cpu().to(dtype))
        torch.autograd.backward(list(outs), [g.to(dtype).reshape(o.shape) for g, o in zip(at_outputs, outs)])
        return {k: v.grad.numpy() for k, v in w.items()}

    ref64, ref32 = autograd(torch.float64), autograd(torch.float32)
    assert sorted(mine) == sorted(ref64) and len(mine) == 28
    return tc.check_gradients(mine, ref64, ref32, label)


def test_the_whole_module_under_a2c_loss_on_recorded_states():
    import bpp_amd
    torch.manual_seed(5)
    net = bpp_amd.TrainablePolicy(10, 100, heads="native").to(DEV)
    with torch.no_grad():
        for p in net.parameters():                                      # the reference starts every bias at 0: make them count
            if p.dim() == 1:
                p.uniform_(-0.1, 0.1)
    rows = _rows(24)
    plain = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    keep = np.nonzero(~hc.tied_states(plain, rows[0]))[0][:16]
    assert keep.size == 16
    _module_against_float64(net, *(r[keep] for r in rows), "module, heads native, a2c_loss, 16 states:")
    kept = net.kept()
    assert sorted(kept) == ["acts", "grad_hidden", "grad_out_mask", "grads", "hidden"]
    assert tuple(kept["hidden"].shape) == (3, 16, 256) and tuple(kept["grad_out_mask"].shape) == (16, 100) and tuple(kept["acts"].shape) == (5, 16, 64, 10, 10)
    assert all(torch.isfinite(v).all() and float(v.abs().max()) > 0 for v in kept.values())
    net.release_buffers()
    assert net.kept() is None and not net._heads_cache and not net._trunk_cache


def test_the_whole_module_at_the_size_of_the_reference_update():
    """n = 5 x 64 = 320 under the reference's initialisation (TrainablePolicy's own, torch.manual_seed(5)): the first 320 of the
    400 states of deep_states(False, 400) without a ReLU tie in the trunk or the heads (hc.tied_states, decided from the float64
    forward alone); the share left out is at most 3 %."""
    import bpp_amd
    torch.manual_seed(5)
    net = bpp_amd.TrainablePolicy(10, 100, heads="native").to(DEV)
    rows = _rows(400)
    tied = hc.tied_states({k: v.detach().cpu() for k, v in net.state_dict().items()}, rows[0])
    print("states with a pre-activation tied at zero: %d of 400" % tied.sum())
    assert tied.sum() <= 0.03 * 400
    keep = np.nonzero(~tied)[0][:320]
    assert keep.size == 320
    _module_against_float64(net, *(r[keep] for r in rows), "module, heads native, a2c_loss, 320 states:")


# ------------------------------------------------------------------------------------------------- the same bits on every run
@pytest.fixture(scope="module")
def heads10():
    """The 10 x 10 chain case (11 rows) with its device tensors; never modified."""
    case = hc.chain_case(10, 256, 100, 11)
    return case, {k: dev(case[k]) for k in hc.CHAIN_INPUTS}


def test_a_replayed_graph_gives_the_bits_of_the_eager_calls():
    """trunk_forward_train -> heads_forward_train -> heads_backward -> trunk_backward captured on one stream, every buffer
    allocated before the capture; the replay on changed inputs against the eager calls."""
    geom, n, A = G10, 6, 100
    L = pol._lib.lib()
    plain = pc.real_weights(*geom, 11)
    blob, trunk_bwd, heads_bwd = dev(pol.pack_weights(plain, *geom).numpy()), dev(pol.pack_trunk_backward(plain).numpy()), dev(pol.pack_heads_backward(plain).numpy())
    states = dev(pc.deep_states(False, 2 * n))
    gen = torch.Generator().manual_seed(9)
    grads = [torch.randn(shape, generator=gen).to(DEV) for shape in ((2 * n,), (2 * n, 100), (2 * n, 100))]
    obs, gv, gl, gp = states[:n].clone(), grads[0][:n].clone(), grads[1][:n].clone(), grads[2][:n].clone()
    new = lambda *shape: torch.full(shape, float("nan"), device=DEV)      # noqa: E731

    def buffers():
        g = pol._lib.kfac_geom(geom)
        return dict(feat=new(n, 20 * A), acts=new(5, n, 64, 10, 10), value=new(n), logits=new(n, 100), pred=new(n, 100), hidden=new(3, n, 256),
                    grad_feat=new(n, 20 * A), grad_hidden=new(3, n, 256), grad_out_mask=new(n, 100), gw_heads=new(hc.sizes(geom, n)["gw"]),
                    ws_heads=new(L.bpp_policy_heads_backward_workspace(g, n) // 4), grads=new(n * 340 * A), gw_trunk=new(pol.TRUNK_FLOATS),
                    ws_trunk=new(L.bpp_policy_trunk_backward_workspace(g, n) // 4))

    def chain(b, obs, gv, gl, gp):
        pol.trunk_forward_train(obs, blob, geom, feat=b["feat"], acts=b["acts"])
        pol.heads_forward_train(b["feat"], blob, geom, value=b["value"], logits=b["logits"], pred=b["pred"], hidden=b["hidden"])
        pol.heads_backward(b["feat"], b["hidden"], b["pred"], gv, gl, gp, geom, heads_bwd, grad_feat=b["grad_feat"], grad_hidden=b["grad_hidden"],
                           grad_out_mask=b["grad_out_mask"], grad_weights=b["gw_heads"], workspace=b["ws_heads"])
        pol.trunk_backward(obs, geom, trunk_bwd, b["feat"], b["acts"], b["grad_feat"], grads=b["grads"], grad_weights=b["gw_trunk"], workspace=b["ws_trunk"])

    outputs = [k for k in buffers() if not k.startswith("ws_")]
    captured, eager = buffers(), buffers()
    chain(eager, obs, gv, gl, gp)                                       # the opt-in to large LDS happens outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain(captured, obs, gv, gl, gp)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(bits(captured[k]), bits(eager[k])) and not torch.isnan(eager[k]).any() for k in outputs)
    first = {k: eager[k].clone() for k in outputs}
    obs.copy_(states[n:])                                               # changed observations and changed gradients
    gv.copy_(grads[0][n:]), gl.copy_(grads[1][n:]), gp.copy_(grads[2][n:])
    graph.replay()
    torch.cuda.synchronize()
    chain(eager, states[n:].contiguous(), grads[0][n:].contiguous(), grads[1][n:].contiguous(), grads[2][n:].contiguous())
    torch.cuda.synchronize()
    assert all(torch.equal(bits(captured[k]), bits(eager[k])) for k in outputs)
    assert not any(torch.equal(bits(captured[k]), bits(first[k])) for k in outputs)


def test_two_backward_passes_over_a_retained_graph_and_a_strided_gradient(heads10):
    import bpp_amd
    case, t = heads10
    S, H, M = case["geom"]
    order = lambda p: [p[k] for k in pol.HEAD_PARAMETERS]        # noqa: E731
    params = {k: case["plain"][k].to(DEV).requires_grad_(True) for k in pol.HEAD_PARAMETERS}
    feat = t["feat"].clone().requires_grad_(True)
    outs = bpp_amd.policy_heads(feat, params, S, M, H, cache={})
    at = [t["grad_value"], t["grad_logits"], t["grad_pred"]]
    g1 = torch.autograd.grad(outs, [feat] + order(params), at, retain_graph=True)
    g2 = torch.autograd.grad(outs, [feat] + order(params), at)
    raw = hc.run_case(hc.device_runner(DEV), case)
    named = hc.unpack_gradient(raw["gw"], case["geom"])
    assert pc.same_bits(g1[0].cpu().numpy(), raw["grad_feat"])
    for k, a, b in zip(pol.HEAD_PARAMETERS, g1[1:], g2[1:]):
        assert a.shape == params[k].shape and torch.equal(bits(a), bits(b)) and pc.same_bits(a.cpu().numpy(), named[k]), k
    assert torch.equal(bits(g1[0]), bits(g2[0]))
    # a gradient that is not contiguous (column slices of wider tensors) and an output that takes no part: the bits of the dense call
    wide = torch.full((11, 2 * M + 3), float("nan"), device=DEV)
    wide[:, 3::2] = t["grad_logits"]
    p2 = {k: case["plain"][k].to(DEV).requires_grad_(True) for k in pol.HEAD_PARAMETERS}
    f2 = t["feat"].clone().requires_grad_(True)
    value, logits, pred = bpp_amd.policy_heads(f2, p2, S, M, H, cache={})
    strided = wide[:, 3::2]
    assert not strided.is_contiguous()
    g3 = torch.autograd.grad([value, logits], [f2] + order(p2), [t["grad_value"], strided])
    only = hc.run_case(hc.device_runner(DEV), case, grad_pred=None)
    named = hc.unpack_gradient(only["gw"], case["geom"])
    assert pc.same_bits(g3[0].cpu().numpy(), only["grad_feat"]) and all(pc.same_bits(a.cpu().numpy(), named[k]) for k, a in zip(pol.HEAD_PARAMETERS, g3[1:]))


def test_the_python_side_refuses_on_the_device(heads10):
    import bpp_amd
    case, t = heads10
    S, H, M = case["geom"]
    params = {k: case["plain"][k].to(DEV).requires_grad_(True) for k in pol.HEAD_PARAMETERS}
    cache = {}
    stale = bpp_amd.policy_heads(t["feat"], params, S, M, H, cache=cache)
    with torch.no_grad():                                               # keeps nothing and disturbs nothing
        bpp_amd.policy_heads(t["feat"], params, S, M, H, cache=cache)
    newer = bpp_amd.policy_heads(t["feat"], params, S, M, H, cache=cache)          # a newer forward of the same key owns the hidden vectors now
    with pytest.raises(RuntimeError, match="overwritten"):
        stale[1].sum().backward()
    newer[1].sum().backward()
    assert float(params["dist.linear.weight"].grad.abs().max()) > 0 and params["base.mask.5.weight"].grad is not None
    assert float(params["base.mask.5.weight"].grad.abs().max()) == 0    # pred took no part: zeros, not stale values
    with pytest.raises(ValueError, match="is on"):                      # a parameter on the wrong device
        bpp_amd.policy_heads(t["feat"], dict(params, **{"dist.linear.bias": case["plain"]["dist.linear.bias"]}), S, M, H, cache=cache)
    with pytest.raises(ValueError):
        pol.heads_forward_train(t["feat"], t["blob"][:-1], case["geom"])
    with torch.no_grad():                                               # a changed parameter re-packs the blobs
        before = bpp_amd.policy_heads(t["feat"], params, S, M, H, cache=cache)[0].clone()
        params["base.critic_linear.bias"].add_(1.0)
        after = bpp_amd.policy_heads(t["feat"], params, S, M, H, cache=cache)[0]
    assert torch.allclose(after, before + 1.0)


# -------------------------------------------------------------------------------------------------------------------- the example
class _StandIn:
    """torch_forward on given weights in a given dtype on the CPU, outputs in the example's order (logits, values [n, 1], pred)."""

    def __init__(self, plain, dtype):
        self.w = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in plain.items()}
        self.dtype = dtype

    def gradients(self, obs, at_outputs):
        value, logits, pred = pol.torch_forward(self.w, obs.cpu().to(self.dtype))
        outs = (logits, value.reshape(-1, 1), pred)
        torch.autograd.backward(list(outs), [g.detach().cpu().to(o.dtype).reshape(o.shape) for g, o in zip(at_outputs, outs)])
        return {k: v.grad.numpy() for k, v in self.w.items()}


def test_the_first_update_of_the_example_against_the_torch_stand_in():
    """One update driven through the public pieces of examples/train_with_storage.py as train(native_heads=True) drives them, at
    the envs / steps of the --native-trunk test (64 x 5): all 28 gradients against the torch stand-in holding the same weights on
    the same storage contents in float64 (float32 for e_torch32).  Tied states (hc.tied_states, decided from the float64 forward
    alone) are overwritten in the storage by the first state that is not, before the update reads it; the cap on their share is
    the --native-trunk test's 5 %: the rollout starts from empty bins under biases of 0, where ties are commoner than in the
    recorded states (13 of 320 here)."""
    import bpp_amd
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_with_storage as ex
    size, envs, steps, seed = (10, 10, 10), 64, 5, 0
    torch.manual_seed(seed)
    env = bpp_amd.BppVecEnv(envs, size, pool=bpp_amd.sequences.cut2_pool(size, 1024, seed=seed), device=torch.device(DEV))
    net = ex.NativeTrunkNet(size[0], env.action_space.n, heads="native").to(DEV)
    assert net.policy.heads == "native"
    actor = bpp_amd.NativePolicy(size[0], env.action_space.n, device=DEV).refresh(net.policy)
    optimizer = torch.optim.RMSprop(net.parameters(), 7e-4, eps=1e-5, alpha=0.99)
    storage = bpp_amd.RolloutStorage(steps, env, env.observation_space.shape, env.action_space)
    storage.reset(env)
    counter = torch.tensor([seed, 0], dtype=torch.int64, device=DEV)
    ex.collect(net, actor, env, storage, counter, 1.0)
    E = steps * envs
    plain = {k: v.detach().cpu() for k, v in net.policy.state_dict().items()}
    tied = np.nonzero(hc.tied_states(plain, storage.obs[:-1].reshape(E, -1).float().cpu().numpy()))[0]
    print("tied states overwritten in the storage: %d of %d" % (len(tied), E))
    assert len(tied) <= E // 20
    good = next(i for i in range(E) if i not in set(tied))
    for i in tied:
        for name in ("obs", "location_masks", "actions", "returns"):
            storage._slabs[name][i // envs, i % envs] = storage._slabs[name][good // envs, good % envs]
    obs = storage.obs[:-1].view(E, -1)
    ex.fused_gradients(net, optimizer, storage, ex.COEFS)
    mine = {k: p.grad.cpu().numpy().copy() for k, p in net.policy.named_parameters()}
    with torch.no_grad():
        outputs = net(obs)
    leaves = [o.detach().clone().requires_grad_(True) for o in outputs]
    c = ex.COEFS
    storage.a2c_loss(*leaves, value_loss_coef=c[0], entropy_coef=c[1], invalid_coef=c[2], mask_coef=c[3]).backward()
    at_outputs = [o.grad.clone() for o in leaves]
    ref64, ref32 = (_StandIn(plain, dt).gradients(obs, at_outputs) for dt in (torch.float64, torch.float32))
    assert sorted(mine) == sorted(ref64) and len(mine) == 28
    tc.check_gradients(mine, ref64, ref32, "example, first update, native heads:")
    env.close()


def test_the_example_trains_through_the_native_heads():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_with_storage as ex
    history = ex.train(envs=64, updates=2, native_heads=True, fused_loss=True, verbose=False)
    assert len(history) == 2 and all(np.isfinite(v) for terms in history for v in terms)
    with pytest.raises(ValueError, match="native-heads"):
        ex.train(envs=64, updates=1, native_heads=True, acktr=True, verbose=False)
    with pytest.raises(ValueError, match="native-trunk"):              # the existing refusal keeps its message
        ex.train(envs=64, updates=1, native_trunk=True, acktr=True, verbose=False)
