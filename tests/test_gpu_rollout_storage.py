"""The device side of the rollout storage (include/bpp_rollout.h, bpp_amd.RolloutStorage): bpp_compute_returns against the recorded
reference (returns_golden.npz, returns_edges.npz) and against its host twin, bit for bit, in both forms of the kernel on the same
data and with every optional pointer left out; the zero-copy lock-step and the pipelined driver writing into the storage, against
the reference's storage and the oracle across updates, on side streams too; who owns which output set afterwards; graph capture
of compute_returns; the example's training loop."""
import contextlib
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
EDGE_CASES = rc.load_edge_cases() if os.path.exists(rc.EDGES) else []


@pytest.fixture(scope="module")
def bpp():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import bpp_amd
    bpp_amd._lib.lib()
    return bpp_amd


def on_device(a, shift=0):
    """Device copy of numpy array `a` that starts `shift` bytes past a 16-byte boundary (a contiguous view into a larger
    allocation: every byte the kernel touches lies inside it)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    pad = 16 // t.element_size()
    buf = torch.zeros(t.numel() + pad, dtype=t.dtype, device="cuda:0")
    assert buf.data_ptr() % 16 == 0 and shift % t.element_size() == 0
    v = buf[shift // t.element_size():][:t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == shift and v.is_contiguous()
    return v.view(a.shape)


def device_run(bpp, d, T, N, gamma, lam, use_gae, proper, use_done=False, advantages=True, bad=True, masks_out=True, moved=None, shift=4):
    """bpp_compute_returns on device copies of the inputs; host arrays back, and `form` = the bins per lane
    bpp_compute_returns_info reports for exactly these arguments.  moved: the one array placed `shift` bytes off."""
    import torch
    dev = torch.device("cuda:0")
    t = {k: on_device(v, shift if k == moved else 0) for k, v in d.items()}
    done = on_device(rc.done_of(d["masks"]), shift if moved == "done" else 0) if use_done else None
    if use_done:
        t["masks"][1:] = -7.0
    adv = on_device(np.full((T, N), -7.0, dtype=np.float32), shift if moved == "advantages" else 0) if advantages else None
    lib = bpp._lib.lib()
    args = [t["rewards"].data_ptr(), t["value_preds"].data_ptr(), t["next_value"].data_ptr(), done.data_ptr() if done is not None else None,
            t["masks"].data_ptr() if (masks_out or not use_done) else None, t["bad_masks"].data_ptr() if bad else None,
            t["returns0"].data_ptr(), adv.data_ptr() if adv is not None else None, T, N, use_gae, proper, gamma, lam]
    info = (ctypes.c_int32 * 3)()
    assert lib.bpp_compute_returns_info(*args, info) == 0, lib.bpp_last_error()
    with torch.cuda.device(dev):
        rcode = lib.bpp_compute_returns(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rcode == 0, lib.bpp_last_error()
    torch.cuda.synchronize(dev)
    return dict(returns=t["returns0"].cpu().numpy(), value_preds=t["value_preds"].cpu().numpy(), masks=t["masks"].cpu().numpy(),
                advantages=adv.cpu().numpy() if adv is not None else None, form=int(info[0]))


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


def edge_id(c):
    return "e%d_%s_T%d_N%d_g%s_l%s_gae%d_proper%d" % (c[0], c[10], c[2], c[3], c[4], c[5], c[6], c[7])


def test_the_edge_fixture_is_there():
    assert len(EDGE_CASES) == 248 and {c[10] for c in EDGE_CASES} == set(rc.FAMILIES)


@pytest.mark.parametrize("case", EDGE_CASES, ids=edge_id)
def test_device_entry_point_matches_the_recorded_edges(bpp, case):
    """Chunk, lane and workgroup edges, gamma / lambda = 0 and 1, the split product, subnormal numbers (the device code must keep
    them, as the reference and the host twin do), inf and NaN (rc.same_bits), masks path and done path."""
    c, d, T, N, gamma, lam, use_gae, proper, want, vlast, family = case
    for use_done in (False, True):
        out = device_run(bpp, d, T, N, gamma, lam, use_gae, proper, use_done=use_done)
        assert out["form"] == (4 if N % 4 == 0 else 1)
        assert rc.same_bits(out["returns"], want), use_done
        if use_gae:
            assert (out["returns"][T] == -7.0).all()
        assert rc.same_bits(out["value_preds"][T], vlast)
        assert np.array_equal(rc.bits(out["value_preds"][:T]), rc.bits(d["value_preds"][:T]))
        assert np.array_equal(rc.bits(out["masks"]), rc.bits(d["masks"])), use_done
        with np.errstate(invalid="ignore", over="ignore"):
            assert rc.same_bits(out["advantages"], out["returns"][:T] - d["value_preds"][:T])


MOVABLE = ("rewards", "value_preds", "next_value", "masks", "bad_masks", "returns0", "advantages", "done")


@pytest.mark.parametrize("T", [5, 13, 32])
@pytest.mark.parametrize("N", [4, 256, 260, 65536])
def test_both_kernel_forms_give_the_same_bits_on_the_same_data(bpp, N, T):
    """returns_kernel<4> and returns_kernel<1> on the same data: every array once 16-byte aligned and once 4 bytes off (`done`: 1
    byte off), one array moved at a time.  That the two placements do take different forms is asserted through
    bpp_compute_returns_info (include/bpp_rollout.h), which runs the dispatch's own condition on the very arguments of the call --
    not through a profiler trace.  Unaligned accesses do not fault on this hardware, so without that assertion equal bits would
    prove nothing.  Every access of a misplaced array lies inside its allocation and is a legal access of the one-bin form."""
    lib = bpp._lib.lib()
    family = {4: "huge", 260: "denormal"}.get(N, "unit")
    d = rc.family_inputs(family, T, N, seed=N + T)
    for use_gae, proper in rc.VARIANTS:
        for use_done in (False, True):
            host = rc.run(lib, d, T, N, 0.99, 0.95, use_gae, proper, use_done=use_done, advantages=True)
            base = device_run(bpp, d, T, N, 0.99, 0.95, use_gae, proper, use_done=use_done)
            assert host["rc"] == 0 and host["form"] == 4 and base["form"] == 4
            for moved in MOVABLE:
                if moved == "done" and not use_done:
                    continue
                got = device_run(bpp, d, T, N, 0.99, 0.95, use_gae, proper, use_done=use_done, moved=moved, shift=1 if moved == "done" else 4)
                assert got["form"] == 1, moved
                for k in ("returns", "value_preds", "masks", "advantages"):
                    # two runs on the same device: every bit, NaN included; against the x86 host twin NaN is a class (rc.same_bits)
                    assert np.array_equal(rc.bits(got[k]), rc.bits(base[k])) and rc.same_bits(base[k], host[k]), (k, moved, use_done, use_gae, proper)


@pytest.mark.parametrize("use_gae,proper", rc.VARIANTS)
@pytest.mark.parametrize("N", [260, 65537])
def test_optional_pointers_on_the_device(bpp, N, use_gae, proper):
    """masks = NULL with done; advantages = NULL (the plain variant then never loads value_preds: NaN there changes nothing);
    bad_masks = NULL under proper time limits -- against the host twin, and nothing else touched."""
    T = 13
    lib = bpp._lib.lib()
    d = rc.family_inputs("unit", T, N, seed=N)
    full = rc.run(lib, d, T, N, 0.99, 0.95, use_gae, proper, use_done=True, advantages=True)

    def untouched(got, masks_are_input):
        assert np.array_equal(rc.bits(got["value_preds"][:T]), rc.bits(d["value_preds"][:T]))
        assert np.array_equal(rc.bits(got["value_preds"][T]), rc.bits(d["next_value"] if use_gae else d["value_preds"][T]))
        assert np.array_equal(rc.bits(got["masks"][0]), rc.bits(d["masks"][0]))
        if use_gae:
            assert (got["returns"][T] == -7.0).all()
        if masks_are_input:
            assert np.array_equal(rc.bits(got["masks"]), rc.bits(d["masks"]))

    # masks = NULL with done: nothing is stored to the masks array, the returns are those of the call that stores them
    got = device_run(bpp, d, T, N, 0.99, 0.95, use_gae, proper, use_done=True, masks_out=False)
    want = rc.run(lib, d, T, N, 0.99, 0.95, use_gae, proper, use_done=True, masks_out=False, advantages=True)
    assert (got["masks"][1:] == -7.0).all() and (want["masks"][1:] == -7.0).all()
    for k in ("returns", "advantages"):
        assert np.array_equal(rc.bits(got[k]), rc.bits(want[k])) and np.array_equal(rc.bits(got[k]), rc.bits(full[k])), k
    untouched(got, False)
    # advantages = NULL, masks path and done path
    for use_done in (False, True):
        got = device_run(bpp, d, T, N, 0.99, 0.95, use_gae, proper, use_done=use_done, advantages=False)
        assert got["advantages"] is None and np.array_equal(rc.bits(got["returns"]), rc.bits(full["returns"])), use_done
        assert np.array_equal(rc.bits(got["masks"]), rc.bits(d["masks"]))
        untouched(got, not use_done)
    if not use_gae and not proper:
        poisoned = dict(d, value_preds=np.full_like(d["value_preds"], np.nan))
        got = device_run(bpp, poisoned, T, N, 0.99, 0.95, 0, 0, advantages=False)
        assert np.array_equal(rc.bits(got["returns"]), rc.bits(full["returns"])) and np.isnan(got["value_preds"]).all()
    # bad_masks = NULL = a row of ones
    ones = dict(d, bad_masks=np.ones_like(d["bad_masks"]))
    want = rc.run(lib, ones, T, N, 0.99, 0.95, use_gae, proper, advantages=True)
    assert np.array_equal(rc.bits(rc.run(lib, d, T, N, 0.99, 0.95, use_gae, proper, bad=False)["returns"]), rc.bits(want["returns"]))
    for use_done in (False, True):
        got = device_run(bpp, d, T, N, 0.99, 0.95, use_gae, proper, use_done=use_done, bad=False)
        for k in ("returns", "advantages"):
            assert np.array_equal(rc.bits(got[k]), rc.bits(want[k])), (k, use_done)
        untouched(got, not use_done)


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


# ------------------------------------------------------------------ the storage against the reference, across updates
SLABS = ("obs", "location_masks", "rewards", "value_preds", "returns", "masks", "bad_masks", "actions", "action_log_probs", "done",
         "counter", "ratio", "ep_ret", "ep_len")


def clones(st, names=SLABS):
    """Device clones of the public slabs, enqueued on the current stream: no synchronise."""
    return {k: getattr(st, k).clone() for k in names}


def to_host(snap):
    return {k: v.cpu().numpy() for k, v in snap.items()}


def replay_into_storage(bpp, name, mixed=False, stream=None):
    """The recorded actions of rollout_<name>.npz through storage.reset / storage.step for U updates of T lock-steps, with the seeded
    values, log-probabilities and next_value of storage_updates_<name>.npz; compute_returns (main.py's variant, then GAE with proper
    time limits) and after_update in between.  mixed: every second row goes in through insert() from a twin env's step_tensors
    instead.  Everything is enqueued on `stream` (default: the current one) and nothing synchronises before the last update's
    clones are enqueued; returns [(host copies of the slabs, `step` after the update)] per update."""
    import torch
    g, s = rc.load_storage_case(name)
    T, U, N = int(s["T"]), int(s["U"]), g["actions"].shape[1]
    size, rot = tuple(int(v) for v in g["size"]), bool(g["rotation"])
    env = bpp.BppVecEnv(N, size, enable_rotation=rot, pool=g["pool"], mask_rule="utils")
    twin = bpp.BppVecEnv(N, size, enable_rotation=rot, pool=g["pool"], mask_rule="utils") if mixed else None
    st = bpp.RolloutStorage(T, env, env.observation_space.shape, env.action_space)
    dev = env.device
    up = {k: torch.from_numpy(s[k]).to(dev) for k in ("values", "log_probs", "next_value")}
    actions = torch.from_numpy(g["actions"][:U * T]).to(dev)
    torch.cuda.synchronize(dev)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
    taken = []
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        st.reset(env)
        if mixed:
            twin.reset()
        for u in range(U):
            for t in range(T):
                assert st.step == t
                a, value, logp = actions[u * T + t], up["values"][u, t].unsqueeze(-1), up["log_probs"][u, t].unsqueeze(-1)
                if mixed and t % 2 == 1:
                    env.step_tensors(a)                      # keeps the env in step; its own buffers, not the storage
                    r = twin.step_tensors(a)
                    st.insert(r.obs, torch.zeros(N, 1, device=dev), a.view(N, 1), logp, value, r.reward, r.masks, r.bad_masks, r.mask)
                else:
                    st.step(env, a, value, logp)
                    if mixed:
                        twin.step_tensors(a)
            after_steps = int(st.step)
            nv = up["next_value"][u].unsqueeze(-1)
            st.compute_returns(nv, bool(s["main"][0]), s["main"][1], s["main"][2], bool(s["main"][3]))
            main = st.returns.clone()
            st.compute_returns(nv, bool(s["gae"][0]), s["gae"][1], s["gae"][2], bool(s["gae"][3]))
            taken.append((dict(clones(st), returns_main=main), after_steps))
            st.after_update()
    torch.cuda.synchronize(dev)
    out = [(to_host(snap), step) for snap, step in taken]
    env.close()
    if twin is not None:
        twin.close()
    return g, s, out


@pytest.mark.parametrize("name", rc.STORAGE_CASES)
@pytest.mark.parametrize("how", ["lockstep", "lockstep_side_stream", "mixed_fill"])
def test_storage_equals_the_reference_storage_across_updates(bpp, name, how):
    """After every update every public slab is what the reference's RolloutStorage held at that point (make_storage_golden.py) and
    what the reference's environment produced (make_golden.py); `step` wrapped to 0.  On a side stream nothing synchronises between
    storage.step, compute_returns and the clones that read them.  mixed_fill: the branch of compute_returns for a rollout filled
    partly by insert() gives identical slabs (and needs the step kernel's done bytes to be exactly 0 or 1 no longer)."""
    import torch
    g, s, out = replay_into_storage(bpp, name, mixed=how == "mixed_fill", stream=torch.cuda.Stream() if how == "lockstep_side_stream" else None)
    T = int(s["T"])
    assert len(out) == int(s["U"]) >= 3
    for u, (snap, step) in enumerate(out):
        assert step == 0
        rc.check_storage_update(snap, g, s, u, small_rows=range(0, T, 2) if how == "mixed_fill" else None)
        rows = list(range(0, T, 2)) if how == "mixed_fill" else list(range(T))
        assert set(np.unique(snap["done"][rows]).tolist()) <= {0, 1}              # what the step kernel writes
        d = g["done"][u * T:(u + 1) * T].astype(bool)
        for t in rows:
            np.testing.assert_array_equal(snap["ep_ret"][t][d[t]], g["ep_r_raw"][u * T + t][d[t]])
            np.testing.assert_array_equal(snap["ep_len"][t][d[t]], g["ep_l"][u * T + t][d[t]])


# ------------------------------------------------------------------ the driver into the storage, across updates
def drive_into_storage(bpp, E, T, U, groups, eps, pool, stream=None):
    """U updates of the native driver writing straight into the storage; clones per update, no synchronise before the end."""
    import torch
    env = bpp.BppVecEnv(E, (10, 10, 10), enable_rotation=True, pool=pool, rollout_groups=groups)
    assert env.rollout_groups == groups
    st = bpp.RolloutStorage(T, env, env.observation_space.shape, env.action_space)
    dev = env.device
    gen = torch.Generator(device="cpu").manual_seed(5)
    values = torch.randn(U, T + 1, E, 1, generator=gen).to(dev)
    nvs = torch.randn(U, E, 1, generator=gen).to(dev)
    actions = torch.empty(E, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
    taken = []
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        st.reset(env)
        for u in range(U):
            last = env.rollout_uniform_sets(5, u * T, T, actions, sets=st.output_sets(), resume=u > 0, eps=eps)
            assert last.obs.data_ptr() == st.obs[T].data_ptr() and st.step == 0
            st.value_preds.copy_(values[u])
            st.compute_returns(nvs[u], True, 0.99, 0.95, True)
            taken.append(dict(clones(st), next_action=actions.clone()))
            st.after_update()
    torch.cuda.synchronize(dev)
    out = [to_host(snap) for snap in taken]
    env.close()
    return out, values.cpu().numpy()[:, :, :, 0], nvs.cpu().numpy()[:, :, 0]


@pytest.mark.parametrize("eps", [0.0, 0.01], ids=["plain", "epsilon"])
def test_driver_fills_the_storage_like_the_oracle_across_updates(bpp, oracle, eps, monkeypatch):
    """rollout_uniform_sets(sets=storage.output_sets(), resume=u > 0) + compute_returns + after_update, three times: every slot
    against oracle.rollout_uniform_sets' per-step outputs, the returns against the host twin on the oracle's rewards and dones;
    one and two bin groups (ragged last group) give identical slabs.  The one-group run is repeated on a side stream of the caller's
    and the two-group run takes place there, so a difference names its cause: the stream (one group, both streams) or the
    grouping (side stream, one and two groups)."""
    import torch
    monkeypatch.setattr(bpp.vec_env, "_ENV_ROLLOUT_GROUPS", 0)
    E, T, U, size = 33000, 6, 3, (10, 10, 10)
    pool = bpp.sequences.cut2_pool(size, 96, seed=8)
    one, values, nvs = drive_into_storage(bpp, E, T, U, 1, eps, pool)
    side = torch.cuda.Stream()
    one_side, _, _ = drive_into_storage(bpp, E, T, U, 1, eps, pool, stream=side)
    for u in range(U):
        for k in sorted(one[u]):
            np.testing.assert_array_equal(one_side[u][k], one[u][k], err_msg="one group, side stream against default: %s u=%d" % (k, u))
    del one_side
    two, _, _ = drive_into_storage(bpp, E, T, U, 2, eps, pool, stream=side)
    ref = oracle.OracleEnv(pool, size, True, E)
    obs0, mask0 = ref.reset()
    ra, prev, finished = None, None, 0
    for u in range(U):
        rs, ra = oracle.rollout_uniform_sets(ref, 5, u * T, T, T, resume=u > 0, actions=ra, first_mask=prev["mask"] if prev else None, eps=eps)
        snap = one[u]
        np.testing.assert_array_equal(snap["next_action"], ra)
        np.testing.assert_array_equal(snap["obs"][0], prev["obs"] if prev else obs0)
        np.testing.assert_array_equal(snap["location_masks"][0], prev["mask"] if prev else mask0)
        for t in range(T):
            w = rs[t]
            np.testing.assert_array_equal(snap["obs"][t + 1], w["obs"], err_msg="obs u=%d t=%d" % (u, t))
            np.testing.assert_array_equal(snap["location_masks"][t + 1], w["mask"], err_msg="mask u=%d t=%d" % (u, t))
            np.testing.assert_array_equal(snap["rewards"][t, :, 0], w["reward"], err_msg="reward u=%d t=%d" % (u, t))
            np.testing.assert_array_equal(snap["masks"][t + 1, :, 0], np.where(w["done"] != 0, 0.0, 1.0).astype(np.float32))
            for k in ("done", "counter", "ratio", "ep_ret", "ep_len"):
                np.testing.assert_array_equal(snap[k][t], w[k], err_msg="%s u=%d t=%d" % (k, u, t))
            finished += int(w["done"].sum())
        masks = np.concatenate([snap["masks"][:1, :, 0]] + [np.where(w["done"] != 0, 0.0, 1.0).astype(np.float32)[None] for w in rs])
        d = dict(rewards=np.stack([w["reward"] for w in rs]), value_preds=values[u], next_value=nvs[u], masks=masks,
                 bad_masks=np.ones((T + 1, E), np.float32), returns0=np.zeros((T + 1, E), np.float32))
        host = rc.run(bpp._lib.lib(), d, T, E, 0.99, 0.95, 1, 1)
        assert host["rc"] == 0 and np.array_equal(rc.bits(snap["returns"][:T, :, 0]), rc.bits(host["returns"][:T]))
        assert np.array_equal(rc.bits(snap["value_preds"][:, :, 0]), rc.bits(host["value_preds"]))
        if u:
            np.testing.assert_array_equal(snap["masks"][0], one[u - 1]["masks"][T])      # after_update carried them over
        prev = {k: v.copy() for k, v in rs[T - 1].items()}
        for k in sorted(snap):
            np.testing.assert_array_equal(two[u][k], snap[k], err_msg="groups 2 against 1: %s u=%d" % (k, u))
    assert finished > E * U * T / 60


# ------------------------------------------------------------------ who owns which output set
@pytest.mark.parametrize("groups", [1, 2])
def test_the_driver_leaves_the_storage_slots_to_the_storage(bpp, groups, monkeypatch):
    """After rollout_uniform_sets(sets=storage.output_sets()) slot T is the env's current result, never its own output set: a
    lock-step and a reset without out= write the env's buffers and no slab changes (_caller_set's guarantee)."""
    import torch
    monkeypatch.setattr(bpp.vec_env, "_ENV_ROLLOUT_GROUPS", 0)
    E, T = 32768, 4
    env, twin = make_env(bpp, E, rollout_groups=groups), make_env(bpp, E, rollout_groups=1)
    st = bpp.RolloutStorage(T, env, env.observation_space.shape, env.action_space)
    st.reset(env)
    twin.reset()
    actions, twin_actions = torch.empty(E, dtype=torch.int64, device=env.device), torch.empty(E, dtype=torch.int64, device=env.device)
    last = env.rollout_uniform_sets(5, 0, T, actions, sets=st.output_sets())
    twin.rollout_uniform_sets(5, 0, T, twin_actions)
    assert last.obs.data_ptr() == st.obs[T].data_ptr() and env.location_masks.data_ptr() == st.location_masks[T].data_ptr()
    st.compute_returns(torch.ones(E, 1, device=env.device), False, 0.99, 0.95, False)
    before = clones(st)
    slots = {getattr(st, k)[j].data_ptr() for k in ("obs", "location_masks") for j in range(T + 1)}
    r = env.step_tensors(actions)
    w = twin.step_tensors(twin_actions)
    assert r.obs.data_ptr() not in slots and r.mask.data_ptr() not in slots and env.location_masks.data_ptr() == r.mask.data_ptr()
    for k in ("obs", "mask", "reward", "done", "counter", "ratio"):
        assert torch.equal(getattr(r, k), getattr(w, k)), k                        # ... and it is the right lock-step
    obs = env.reset()
    assert obs.data_ptr() not in slots and env.location_masks.data_ptr() not in slots and torch.equal(obs, twin.reset())
    torch.cuda.synchronize(env.device)
    for k, v in before.items():
        assert torch.equal(getattr(st, k), v), k
    # a set of the env's own still rotates in: the last one written is what the next lock-step without out= reuses
    own = env.output_sets(3)
    last = env.rollout_uniform_sets(5, 0, 4, actions, sets=own)
    assert last is own[0][0] and env._bufs is own[0][0] and env.step_tensors(actions).obs.data_ptr() == own[0][0].obs.data_ptr()
    for k, v in before.items():
        assert torch.equal(getattr(st, k), v), k
    env.close()
    twin.close()


# ------------------------------------------------------------------ smaller paths
def test_a_storage_moved_to_the_cpu_forgets_its_device_slots(bpp):
    import torch
    E, T = 64, 3
    env = make_env(bpp, E)
    st = bpp.RolloutStorage(T, env, env.observation_space.shape, env.action_space)
    st.reset(env)
    for t in range(T):
        st.step(env, env.sample_feasible(seed=2, step=t, mask=st.location_masks[t]), torch.randn(E, 1, device=env.device))
    assert len(st.output_sets()) == T                     # the slots were handed out
    nv = torch.randn(E, 1, device=env.device)
    st.compute_returns(nv, True, 0.99, 0.95, True)
    on_dev = to_host(clones(st))
    st.to("cpu")
    assert st.device.type == "cpu" and st.obs.device.type == "cpu"
    with pytest.raises(RuntimeError, match=r"a CPU storage is filled with insert\(\)"):
        st._slot(1)
    with pytest.raises(RuntimeError, match=r"a CPU storage is filled with insert\(\)"):
        st.output_sets()
    with pytest.raises(ValueError, match="the storage %d on cpu" % E):           # the env is on the device, the storage no longer
        st.reset(env)
    for k, v in on_dev.items():
        assert np.array_equal(getattr(st, k).numpy(), v), k
    # the host entry point on the moved slabs: the same bits as the device gave
    st.returns.zero_()
    st.compute_returns(nv, True, 0.99, 0.95, True)
    assert np.array_equal(rc.bits(st.returns.numpy()), rc.bits(on_dev["returns"]))
    st.step = 0
    r = env.step_tensors(env.sample_feasible(seed=2, step=9))
    st.insert(r.obs.cpu(), torch.zeros(E, 1), torch.zeros(E, 1, dtype=torch.int64), torch.zeros(E, 1), torch.zeros(E, 1), r.reward.cpu(), r.masks.cpu(),
              r.bad_masks.cpu(), r.mask.cpu())
    assert st.step == 1 and torch.equal(st.obs[1], r.obs.cpu()) and torch.equal(st.masks[1], r.masks.cpu())
    env.close()


@pytest.mark.parametrize("variant", [(False, 0.99, 0.95, False), (True, 0.99, 0.95, True)], ids=["main", "gae_proper"])
def test_compute_returns_twice_in_a_row_changes_nothing(bpp, variant):
    """The done path stores masks and the GAE path overwrites value_preds[T]: a second call reads what the first wrote."""
    import torch
    E, T = 4096, 5
    env = make_env(bpp, E)
    st = bpp.RolloutStorage(T, env, env.observation_space.shape, env.action_space)
    st.reset(env)
    for t in range(T):
        a = env.sample_feasible(seed=3, step=t, mask=st.location_masks[t])
        if t == 1:
            a[::3] = 0
        st.step(env, a, torch.randn(E, 1, device=env.device), torch.randn(E, 1, device=env.device))
    nv = torch.randn(E, 1, device=env.device)
    adv1 = st.compute_returns(nv, *variant, advantages=True)
    first = clones(st)
    adv2 = st.compute_returns(nv, *variant, advantages=True)
    assert bool((st.masks[1:] == 0).any()) and torch.equal(adv1.view(torch.int32), adv2.view(torch.int32))
    for k, v in first.items():
        assert torch.equal(getattr(st, k), v), k
    env.close()


def test_a_storage_of_another_geometry_is_refused_before_anything_is_written(bpp):
    """Wrong obs_shape or action_space.n: reset, step and a driver call over output_sets() raise before a kernel is launched (the
    rows here are longer than the env's, so even a launch would have stayed inside the slabs)."""
    import torch
    E, T = 64, 3
    env = make_env(bpp, E)
    env.reset()
    a = env.sample_feasible(seed=0, step=0)
    keep = env.hmap.clone()
    for shape, n in (((404,), env.action_space.n), (env.observation_space.shape, env.action_space.n + 4)):
        st = bpp.RolloutStorage(T, env, shape, bpp.Discrete(n))
        with pytest.raises(ValueError):
            st.reset(env)
        with pytest.raises(ValueError):
            st.step(env, a)
        with pytest.raises(ValueError):
            env.rollout_uniform_sets(5, 0, T, torch.empty(E, dtype=torch.int64, device=env.device), sets=st.output_sets())
        assert not st.obs.any() and not st.location_masks.any() and torch.equal(env.hmap, keep)
    env.close()
