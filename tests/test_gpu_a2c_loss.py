"""bpp_amd.a2c_loss on the device (include/bpp_update.h): the checks of tests/test_a2c_loss.py against the
device's own bpp_masked_evaluate kernels and float64 torch on the CPU, the gradients a network receives, the storage method,
a captured graph and the example's --fused-loss path.  Reads nothing of the reference."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import a2c_cases as ac  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH = 1024


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_evaluate(x, m, a):
    from bpp_amd.masks import _MaskedEvaluate
    return tuple(t.cpu().numpy() for t in _MaskedEvaluate.apply(dev(x), dev(m), dev(a)))


def dev_backward(x, m, a, g0, g1, g2):
    from bpp_amd.masks import _MaskedEvaluate
    xt = dev(x).requires_grad_(True)
    out = _MaskedEvaluate.apply(xt, dev(m), dev(a))
    torch.autograd.backward(list(out), [dev(np.asarray(g, np.float32)) for g in (g0, g1, g2)])
    return xt.grad.cpu().numpy()


def run_device(c, coefs=ac.COEFS, pred=True):
    import bpp_amd
    E = c["E"]
    res = bpp_amd.a2c_loss(dev(c["x"]), dev(c["val"]).view(E, 1), dev(c["pm"]) if pred else None, dev(c["m"]), dev(c["a"]).view(E, 1),
                           dev(c["ret"]), *coefs, rows=True)
    out = dict(terms=res.terms, rows=res.rows, grad_logits=res.grad_logits, grad_values=res.grad_values)
    if pred:
        out["grad_pred_mask"] = res.grad_pred_mask
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("M", [15, 100, 200, 516])
@pytest.mark.parametrize("E", [3, 257, WIDTH + 1, 4 * WIDTH + 1])
def test_gpu_a2c_loss_pieces_terms_and_float64(E, M):
    from bpp_amd import _lib
    assert ac.info(_lib.lib(), E, M)[2:] == [int(M <= 512), WIDTH]
    c = ac.make_case(E, M, seed=1000 * E + M)
    out = run_device(c)
    ac.check_pieces(out, c, dev_evaluate, dev_backward)
    ac.check_terms(out, c)
    ref = ac.check_against_float64(out, c)
    np.testing.assert_allclose(out["grad_values"], ref["grad_values"], rtol=4 * ac.EPS, atol=0)
    np.testing.assert_allclose(out["grad_pred_mask"], ref["grad_pred_mask"], rtol=4 * ac.EPS, atol=0)
    again = run_device(c)
    for k in out:
        assert np.array_equal(ac.bits(again[k]), ac.bits(out[k])), k
    if E == 257:
        bare = run_device(c, pred=False)
        assert bare["terms"][4] == 0.0 and np.array_equal(ac.bits(bare["terms"][:4]), ac.bits(out["terms"][:4]))
        assert np.array_equal(ac.bits(bare["grad_logits"]), ac.bits(out["grad_logits"]))


def test_gpu_a2c_loss_shape_and_dtype_mismatches_are_value_errors():
    import bpp_amd
    c = ac.make_case(4, 10, seed=0)
    good = dict(logits=dev(c["x"]), values=dev(c["val"]), pred_mask=dev(c["pm"]), location_masks=dev(c["m"]), action=dev(c["a"]),
                returns=dev(c["ret"]))
    assert float(bpp_amd.a2c_loss(**good).loss) == float(bpp_amd.a2c_loss(**good).terms[5])
    for bad in (dict(logits=good["logits"].double()), dict(values=good["values"][:3]), dict(location_masks=good["location_masks"][:, :9]),
                dict(action=good["action"].int()), dict(pred_mask=good["pred_mask"][:2]), dict(returns=good["returns"].half()),
                dict(logits=good["logits"].reshape(-1))):
        with pytest.raises(ValueError):
            bpp_amd.a2c_loss(**dict(good, **bad))
    with pytest.raises(RuntimeError):
        bpp_amd.a2c_loss(**dict(good, returns=good["returns"].cpu()))


@pytest.fixture(scope="module")
def filled_storage():
    """3 lock-steps of 67 bins at 10x10x10 under a one-layer network, returns computed."""
    import bpp_amd
    size, N, T = (10, 10, 10), 67, 3
    env = bpp_amd.BppVecEnv(N, size, pool=bpp_amd.sequences.cut2_pool(size, 64, seed=0), device="cuda:0")
    M = env.action_space.n
    torch.manual_seed(3)
    net = torch.nn.Linear(4 * M, 2 * M + 1).cuda()
    st = bpp_amd.RolloutStorage(T, env, env.observation_space.shape, env.action_space)
    st.reset(env)
    for t in range(T):
        with torch.no_grad():
            o = net(st.obs[t])
        action, logp = bpp_amd.masked_act(o[:, :M], st.location_masks[t], seed=1, step=t)
        st.step(env, action, o[:, M:M + 1], logp)
    with torch.no_grad():
        next_value = net(st.obs[-1])[:, M:M + 1]
    st.compute_returns(next_value, False, 1.0, 0.95, False)
    torch.cuda.synchronize()
    yield st, net, T, N, M
    env.close()


def heads(net, obs, M):
    o = net(obs)
    return o[:, :M], o[:, M:M + 1], torch.sigmoid(o[:, M + 1:])


def test_gpu_a2c_loss_backward_gives_a_network_the_parent_expression_s_gradients(filled_storage):
    import bpp_amd
    st, net, T, N, M = filled_storage
    vc, ec, ic, mc = ac.COEFS
    obs = st.obs[:-1].view(T * N, -1)
    truth = st.location_masks[:-1].view(T * N, M)
    # the lines of examples/train_with_storage.py before this entry point existed
    net.zero_grad()
    logits, values, pred_mask = heads(net, obs, M)
    action_log_probs, dist_entropy, prob_loss = bpp_amd.masked_evaluate(logits, truth, st.actions.view(T * N, 1))
    advantages = st.returns[:-1] - values.view(T, N, 1)
    value_loss = advantages.pow(2).mean()
    action_loss = -(advantages.detach() * action_log_probs.view(T, N, 1)).mean()
    graph_loss = torch.nn.functional.mse_loss(pred_mask, truth)
    (value_loss * vc + action_loss + prob_loss * ic - dist_entropy * ec + mc * graph_loss).backward()
    parent = [p.grad.detach().cpu().double().numpy().copy() for p in net.parameters()]
    parent_terms = [float(v) for v in (value_loss, action_loss, dist_entropy, prob_loss, graph_loss)]
    # the fused call
    net.zero_grad()
    res = st.a2c_loss(*heads(net, obs, M))
    res.backward()
    fused = [p.grad.detach().cpu().double().numpy().copy() for p in net.parameters()]
    # float64 on the CPU
    net64 = torch.nn.Linear(4 * M, 2 * M + 1).double()
    net64.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
    l64 = ac.loss64(*heads(net64, obs.cpu().double(), M), truth.cpu().double(), st.actions.view(-1).cpu(), st.returns[:-1].cpu().double())
    l64[5].backward()
    g64 = [p.grad.numpy() for p in net64.parameters()]
    for name, f, p, g in zip(("weight", "bias"), fused, parent, g64):
        ef, ep = np.abs(f - g).max(), np.abs(p - g).max()
        print("%s: max |fused - g64| = %.3g, max |parent - g64| = %.3g, max |g64| = %.3g" % (name, ef, ep, np.abs(g).max()))
        assert ef <= 4 * ep + 1e-9, name
    print("terms fused", res.terms.tolist(), "parent", parent_terms, "f64", [float(t.detach()) for t in l64[:5]])


def test_gpu_storage_a2c_loss_hands_over_views_and_equals_the_functional_call(filled_storage):
    import bpp_amd
    st, net, T, N, M = filled_storage
    with torch.no_grad():
        logits, values, pred_mask = (t.contiguous() for t in heads(net, st.obs[:-1].view(T * N, -1), M))
    res = st.a2c_loss(logits, values, pred_mask)
    assert res.inputs["location_masks"].data_ptr() == st.location_masks.data_ptr()
    assert res.inputs["action"].data_ptr() == st.actions.data_ptr() and res.inputs["returns"].data_ptr() == st.returns.data_ptr()
    assert res.inputs["logits"].data_ptr() == logits.data_ptr() and res.inputs["pred_mask"].data_ptr() == pred_mask.data_ptr()
    terms, grad = res.terms.clone(), res.grad_logits.clone()
    fn = bpp_amd.a2c_loss(logits, values, pred_mask, st.location_masks[:-1].reshape(T * N, M).clone(), st.actions.reshape(-1).clone(),
                          st.returns[:-1].clone())
    assert torch.equal(terms.view(torch.int32), fn.terms.view(torch.int32)) and torch.equal(grad.view(torch.int32), fn.grad_logits.view(torch.int32))
    for i, name in enumerate(("value_loss", "action_loss", "dist_entropy", "prob_loss", "graph_loss", "loss")):
        t = getattr(fn, name)
        assert t.dim() == 0 and t.is_cuda and t.data_ptr() == fn.terms[i].data_ptr()
    with pytest.raises(TypeError):
        st.a2c_loss(logits, values, pred_mask, gamma=1.0)


def test_gpu_a2c_loss_in_a_captured_graph_equals_the_eager_call():
    import bpp_amd
    E, M = 257, 100
    cases = [ac.make_case(E, M, seed=s) for s in (11, 12, 13)]
    keys = ("x", "val", "pm", "m", "a", "ret")
    static = {k: dev(cases[0][k]) for k in keys}

    def call(t):
        return bpp_amd.a2c_loss(t["x"], t["val"], t["pm"], t["m"], t["a"], t["ret"], rows=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(static)                                  # the cached buffers exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                     # one stream, no parallel branches
        res = call(static)
    for c in cases[1:]:
        for k in keys:
            static[k].copy_(dev(c[k]))
        graph.replay()
        torch.cuda.synchronize()
        got = {k: getattr(res, k).clone() for k in ("terms", "rows", "grad_logits", "grad_values", "grad_pred_mask")}
        eager = call({k: dev(c[k]) for k in keys})
        for k, v in got.items():
            assert torch.equal(v.view(torch.int32), getattr(eager, k).view(torch.int32)), k
        ac.check_terms({k: v.cpu().numpy() for k, v in got.items()}, c)


def test_gpu_example_trains_with_the_fused_loss():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_with_storage as ex
    fused = ex.train(envs=64, steps=3, updates=2, fused_loss=True, verbose=False)
    plain = ex.train(envs=64, steps=3, updates=2, fused_loss=False, verbose=False)
    assert len(fused) == 2 and all(len(h) == 5 and np.isfinite(h).all() for h in fused)
    # Same seed, weights and rollout: the first update's terms differ by float32 summation order only.  Bounds of check 4 for
    # E = 192, M = 100; the action loss bound needs mean |adv| and mean |adv logp|, which train() does not return: both are
    # replaced by lower bounds (mean |adv logp| >= |action_loss|, mean |adv| >= |action_loss| / max |logp|, |logp| <= -log(eps)),
    # so the bound used is never wider than the one they give.
    tol = ac.forward_tolerances(100)
    f, p = fused[0], plain[0]
    print("fused", f, "plain", p)
    bounds = [4 * ac.EPS * abs(p[0]), (tol[0] / -np.log(ac.EPS) + 4 * ac.EPS) * abs(p[1]), tol[1], tol[2] / 100, 4 * ac.EPS * abs(p[4])]
    for j in range(5):
        assert abs(f[j] - p[j]) <= bounds[j], (j, f[j], p[j], bounds[j])
