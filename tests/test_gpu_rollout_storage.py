"""The device side of the rollout storage (include/bpp_rollout.h, bpp_amd.RolloutStorage): bpp_compute_returns against the recorded
reference and against its host twin, bit for bit; the zero-copy lock-step and the pipelined driver writing into the storage; graph
capture of compute_returns; the example's training loop."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import returns_cases as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = rc.load_cases() if os.path.exists(rc.GOLDEN) else []


@pytest.fixture(scope="module")
def bpp():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import bpp_amd
    bpp_amd._lib.lib()
    return bpp_amd


def device_run(bpp, d, T, N, gamma, lam, use_gae, proper, use_done=False, advantages=True, bad=True):
    """bpp_compute_returns on device copies of the inputs; host arrays back."""
    import torch
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
    done = torch.from_numpy(rc.done_of(d["masks"])).to(dev) if use_done else None
    if use_done:
        t["masks"][1:] = -7.0
    adv = torch.full((T, N), -7.0, dtype=torch.float32, device=dev) if advantages else None
    lib = bpp._lib.lib()
    with torch.cuda.device(dev):
        rcode = lib.bpp_compute_returns(t["rewards"].data_ptr(), t["value_preds"].data_ptr(), t["next_value"].data_ptr(),
                                        done.data_ptr() if done is not None else None, t["masks"].data_ptr(),
                                        t["bad_masks"].data_ptr() if bad else None, t["returns0"].data_ptr(),
                                        adv.data_ptr() if adv is not None else None, T, N, use_gae, proper, gamma, lam,
                                        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rcode == 0, lib.bpp_last_error()
    torch.cuda.synchronize(dev)
    return dict(returns=t["returns0"].cpu().numpy(), value_preds=t["value_preds"].cpu().numpy(), masks=t["masks"].cpu().numpy(),
                advantages=adv.cpu().numpy() if adv is not None else None)


def test_the_fixture_is_there():
    assert len(CASES) == 40


@pytest.mark.parametrize("case", CASES, ids=lambda c: "c%d_T%d_N%d_gae%d_proper%d" % (c[0], c[2], c[3], c[6], c[7]))
def test_device_entry_point_matches_the_recorded_reference_bit_for_bit(bpp, case):
    c, d, T, N, gamma, lam, use_gae, proper, want, vlast = case
    for use_done in (False, True):
        out = device_run(bpp, d, T, N, gamma, lam, use_gae, proper, use_done=use_done)
        assert np.array_equal(rc.bits(out["returns"]), rc.bits(want)), use_done       # rows the reference leaves alone included
        assert np.array_equal(rc.bits(out["value_preds"][T]), rc.bits(vlast))
        assert np.array_equal(rc.bits(out["value_preds"][:T]), rc.bits(d["value_preds"][:T]))
        assert np.array_equal(rc.bits(out["masks"]), rc.bits(d["masks"])), use_done   # row 0 untouched; the done path writes exact 0.0 / 1.0
        assert np.array_equal(rc.bits(out["advantages"]), rc.bits(out["returns"][:T] - d["value_preds"][:T]))


@pytest.mark.parametrize("use_gae,proper", rc.VARIANTS)
@pytest.mark.parametrize("T", [5, 32])
@pytest.mark.parametrize("N", [65536, 65537])
def test_device_equals_the_host_entry_point(bpp, N, T, use_gae, proper):
    d = rc.random_inputs(T, N, seed=T + N)
    lib = bpp._lib.lib()
    for use_done, bad in ((False, True), (True, True), (True, False)):
        if not bad:
            d = dict(d, bad_masks=np.ones_like(d["bad_masks"]))
        want = rc.run(lib, d, T, N, 0.99, 0.95, use_gae, proper, use_done=use_done, bad=bad, advantages=True)
        got = device_run(bpp, d, T, N, 0.99, 0.95, use_gae, proper, use_done=use_done, bad=bad)
        assert want["rc"] == 0
        for k in ("returns", "value_preds", "masks", "advantages"):
            assert np.array_equal(rc.bits(got[k]), rc.bits(want[k])), (k, use_done, bad)


def make_env(bpp, E, rot=False, **kw):
    size = (10, 10, 10)
    return bpp.BppVecEnv(E, size, enable_rotation=rot, pool=bpp.sequences.cut2_pool(size, 64, seed=3), **kw)


@pytest.mark.parametrize("rot", [False, True])
def test_lockstep_writes_into_the_storage_without_a_copy(bpp, rot):
    import torch
    E, T = 4096, 5
    env, twin = make_env(bpp, E, rot), make_env(bpp, E, rot)
    st = bpp.RolloutStorage(T, env, env.observation_space.shape, env.action_space)
    obs0 = st.reset(env)
    assert obs0.data_ptr() == st.obs[0].data_ptr() and env.location_masks.data_ptr() == st.location_masks[0].data_ptr()
    assert torch.equal(st.obs[0], twin.reset()) and torch.equal(st.location_masks[0], twin.location_masks)
    ptrs = [st.obs[t].data_ptr() for t in range(T + 1)]
    for update in range(2):
        want = []
        for t in range(T):
            assert st.step == t
            a = env.sample_feasible(seed=11, step=update * T + t, mask=st.location_masks[t])
            if t == 2:
                a[::3] = 0                    # infeasible placements: episodes end
            value, logp = torch.randn(E, 1, device=env.device), torch.randn(E, 1, device=env.device)
            res = st.step(env, a, value, logp)
            assert res.obs.data_ptr() == ptrs[t + 1] == st._slot(t + 1)[1].obs and res.mask.data_ptr() == st.location_masks[t + 1].data_ptr()
            assert env.location_masks.data_ptr() == st.location_masks[t + 1].data_ptr()
            r = twin.step_tensors(a)
            want.append({k: getattr(r, k).clone() for k in ("obs", "mask", "reward", "done", "counter", "ratio", "ep_ret", "ep_len")})
            want[-1]["masks"] = r.masks.clone()
            assert torch.equal(st.actions[t], a.view(E, 1)) and torch.equal(st.value_preds[t], value) and torch.equal(st.action_log_probs[t], logp)
        next_value = torch.randn(E, 1, device=env.device)
        st.compute_returns(next_value, True, 0.99, 0.95, True)
        assert any(bool(w["done"].any()) for w in want)
        for t, w in enumerate(want):
            assert torch.equal(st.obs[t + 1], w["obs"]) and torch.equal(st.location_masks[t + 1], w["mask"]), t
            assert torch.equal(st.rewards[t], w["reward"]) and torch.equal(st.masks[t + 1], w["masks"]), t
            for k in ("done", "counter", "ratio", "ep_ret", "ep_len"):
                assert torch.equal(getattr(st, k)[t], w[k]), (t, k)
        # the returns of the storage = the host twin on the same rows
        d = dict(rewards=st.rewards[:, :, 0].cpu().numpy(), value_preds=st.value_preds[:, :, 0].cpu().numpy(), next_value=next_value[:, 0].cpu().numpy(),
                 masks=st.masks[:, :, 0].cpu().numpy(), bad_masks=st.bad_masks[:, :, 0].cpu().numpy(), returns0=np.zeros((T + 1, E), np.float32))
        host = rc.run(bpp._lib.lib(), d, T, E, 0.99, 0.95, 1, 1)
        assert np.array_equal(rc.bits(st.returns[:T, :, 0].cpu().numpy()), rc.bits(host["returns"][:T]))
        st.after_update()
        assert torch.equal(st.obs[0], st.obs[-1]) and torch.equal(st.location_masks[0], st.location_masks[-1])
    # a lock-step without out= goes back to the env's own buffers and leaves the storage alone
    keep = st.obs[T].clone()
    r = env.step_tensors(env.sample_feasible(seed=1, step=99))
    assert r.obs.data_ptr() not in ptrs and torch.equal(st.obs[T], keep) and env.location_masks.data_ptr() == r.mask.data_ptr()
    env.close()
    twin.close()


def test_caller_owned_buffers_are_refused_where_they_cannot_be_honoured(bpp):
    E = 64
    fresh = make_env(bpp, E, fresh_outputs=True)
    st = bpp.RolloutStorage(3, fresh, fresh.observation_space.shape, fresh.action_space)
    with pytest.raises(RuntimeError, match="fresh_outputs"):
        st.reset(fresh)
    fresh.reset()
    with pytest.raises(RuntimeError, match="fresh_outputs"):
        st.step(fresh, fresh.sample_feasible(seed=0, step=0))
    env = make_env(bpp, E)
    env.reset()
    host = env._staging(mapped=True)
    with pytest.raises(RuntimeError, match="host mirror"):
        env.step_tensors(env.sample_feasible(seed=0, step=0), _host=host, out=st._slot(1))
    other = bpp.RolloutStorage(3, 32, env.observation_space.shape, env.action_space, device=env.device)
    with pytest.raises(ValueError):
        other.step(env, env.sample_feasible(seed=0, step=0))


@pytest.mark.parametrize("E", [32768, 33000])
def test_pipelined_driver_fills_identical_storages(bpp, E, monkeypatch):
    import torch
    monkeypatch.setattr(bpp.vec_env, "_ENV_ROLLOUT_GROUPS", 0)
    T, filled = 6, []
    for groups in (1, 2):
        env = make_env(bpp, E, rollout_groups=groups)
        assert env.rollout_groups == groups
        st = bpp.RolloutStorage(T, env, env.observation_space.shape, env.action_space)
        st.reset(env)
        actions = torch.empty(E, dtype=torch.int64, device=env.device)
        last = env.rollout_uniform_sets(5, 0, T, actions, sets=st.output_sets())
        assert last.obs.data_ptr() == st.obs[T].data_ptr()
        st.compute_returns(torch.ones(E, 1, device=env.device), False, 0.99, 0.95, False)
        torch.cuda.synchronize(env.device)
        filled.append({k: getattr(st, k).cpu() for k in ("obs", "location_masks", "rewards", "masks", "returns", "done", "counter", "ratio",
                                                         "ep_ret", "ep_len")})
        env.close()
    # lock-step t landed in slot t + 1: replay the single-chain rollout one lock-step at a time
    env = make_env(bpp, E, rollout_groups=1)
    env.reset()
    actions = torch.empty(E, dtype=torch.int64, device=env.device)
    for t in range(T):
        r = env.rollout_uniform_sets(5, t, 1, actions, resume=t > 0)
        assert torch.equal(filled[0]["obs"][t + 1], r.obs.cpu()) and torch.equal(filled[0]["rewards"][t], r.reward.cpu()), t
        assert torch.equal(filled[0]["masks"][t + 1], r.masks.cpu()), t
    env.close()
    assert bool((filled[0]["done"] != 0).any())
    for k in filled[0]:
        assert torch.equal(filled[0][k], filled[1][k]), k


def test_compute_returns_replays_from_a_graph(bpp):
    import torch
    T, N = 5, 65536
    dev = torch.device("cuda:0")
    d = rc.random_inputs(T, N, seed=2)
    st = bpp.RolloutStorage(T, N, (4,), bpp.Discrete(4), device=dev)
    for k in ("rewards", "value_preds", "masks", "bad_masks"):
        getattr(st, k).copy_(torch.from_numpy(d[k]).unsqueeze(-1))
    next_value = torch.from_numpy(d["next_value"]).to(dev).unsqueeze(-1)
    st.compute_returns(next_value, True, 0.99, 0.95, True)
    eager = st.returns.clone()
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        st.compute_returns(next_value, True, 0.99, 0.95, True)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                      # one kernel node: a single branch, no parallel streams
        st.compute_returns(next_value, True, 0.99, 0.95, True)
    st.returns.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(st.returns.view(torch.int32), eager.view(torch.int32))
    host = rc.run(bpp._lib.lib(), d, T, N, 0.99, 0.95, 1, 1)
    assert np.array_equal(rc.bits(st.returns[:T, :, 0].cpu().numpy()), rc.bits(host["returns"][:T]))


def test_the_example_trains_for_two_updates(bpp):
    spec = importlib.util.spec_from_file_location("train_with_storage", os.path.join(ROOT, "examples", "train_with_storage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    history = mod.train(envs=2048, steps=5, updates=2, verbose=False)
    assert len(history) == 2 and all(len(h) == 5 and all(np.isfinite(v) for v in h) for h in history)
