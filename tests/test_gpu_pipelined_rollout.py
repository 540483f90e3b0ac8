"""The pipelined rollout driver (include/bpp_pipeline.h: the bins split into groups, every group's chain of step-kernel
launches on a stream of its own) computes bit for bit what the single-chain driver computes, and joins the launch stream."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OUTPUTS = ("obs", "mask", "reward", "done", "counter", "ratio", "ep_ret", "ep_len")
# (nsets, eps): the env's single output set, three rotating sets, the epsilon variant
MODES = {"single_set": (1, 0.0), "rotating_sets": (3, 0.0), "epsilon": (1, 0.01)}
CALLS = (31, 29)     # ~60 lock-steps in two calls: resume=False, then resume=True
BASE = 192           # first global bin id of the shard (a group's env_id_base is this plus its first bin)


@pytest.fixture(scope="module")
def bpp():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import bpp_amd
    bpp_amd._lib.lib()
    return bpp_amd


@pytest.fixture(autouse=True)
def no_override(bpp, monkeypatch):
    """The constructor argument decides here, not a BPP_ROLLOUT_GROUPS left in the environment."""
    monkeypatch.setattr(bpp.vec_env, "_ENV_ROLLOUT_GROUPS", 0)


def rollout(bpp, size, rot, E, pool, groups, mode, stream=None):
    """The two-call rollout; returns everything the driver leaves behind as host arrays.  Nothing synchronises between the
    native call and its first readers, which are enqueued on the launch stream."""
    import torch
    nsets, eps = MODES[mode]
    env = bpp.BppVecEnv(E, size, enable_rotation=rot, pool=pool, env_id_base=BASE, env_id_total=E + BASE + 5, rollout_groups=groups)
    assert env.rollout_groups == groups and env._pipe is None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(env.device))      # the constructor's fills ran on the current stream
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        env.reset()
        actions = torch.empty(E, dtype=torch.int64, device=env.device)
        sets = env.output_sets(nsets) if nsets > 1 else None
        t = 0
        for n in CALLS:
            r = env.rollout_uniform_sets(5, t, n, actions, sets=sets, resume=t > 0, eps=eps)
            t += n
        # the join: clones enqueued on the launch stream right behind the call, no synchronise in between
        got = {k: getattr(r, k).clone() for k in OUTPUTS}
        got["actions"] = actions.clone()
        got["hmap"] = env.hmap.clone()
        got["ep_acc"] = env.ep_acc.clone()
        got["state"] = env.state.clone()
        got["stats"] = env.episode_stats().clone()
    torch.cuda.synchronize(env.device)
    assert (env._pipe is not None) == (groups > 1)
    out = {k: v.cpu().numpy() for k, v in got.items()}
    st = out.pop("state").view(env.state_numpy().dtype).reshape(-1)
    for f in st.dtype.names:
        if f != "pad":
            out["state." + f] = st[f]
    if sets is not None:        # the other rotating sets hold the two lock-steps before the last
        for j, (res, _) in enumerate(sets):
            out["set%d.mask" % j] = res.mask.cpu().numpy()
            out["set%d.obs" % j] = res.obs.cpu().numpy()
    env.close()
    assert env._pipe is None
    return out


@pytest.mark.parametrize("groups", [2, 4])
@pytest.mark.parametrize("E", [32768, 33000])       # a multiple of every group size / a ragged last group
@pytest.mark.parametrize("size,rot", [((10, 10, 10), False), ((10, 10, 10), True), ((20, 20, 20), False)])
def test_pipelined_rollout_equals_the_single_chain(bpp, size, rot, E, groups):
    import torch
    plan = bpp._lib.pipeline_plan(E, groups)
    assert len(plan) == groups and (E == 33000) == (plan[-1][1] != plan[0][1])
    pool = bpp.sequences.cut2_pool(size, 96, seed=8)
    side = torch.cuda.Stream()
    for mode in MODES:
        want = rollout(bpp, size, rot, E, pool, 1, mode)
        # once on the default stream, once on a stream of the caller's (group 0 runs there)
        got = rollout(bpp, size, rot, E, pool, groups, mode, stream=side if mode == "rotating_sets" else None)
        assert sorted(got) == sorted(want)
        for k in sorted(want):
            np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (mode, k))
        assert want["stats"][3] > E * sum(CALLS) / 60        # episodes did finish: resets and ep_acc rows are exercised
        if mode == "epsilon":
            plain = rollout(bpp, size, rot, E, pool, groups, "single_set")
            assert np.count_nonzero(plain["hmap"] != got["hmap"]) > 0      # the override launches did run


@pytest.mark.parametrize("mode", sorted(MODES))
def test_pipelined_rollout_equals_the_oracle(bpp, oracle, mode):
    """One configuration against the CPU restatement, as bench.py's parity gate does: ragged last group, rotation on."""
    size, rot, E, groups = (10, 10, 10), True, 33000, 4
    nsets, eps = MODES[mode]
    pool = bpp.sequences.cut2_pool(size, 96, seed=8)
    got = rollout(bpp, size, rot, E, pool, groups, mode)
    ref = oracle.OracleEnv(pool, size, rot, E, env_id_base=BASE, env_id_total=E + BASE + 5)
    ref.reset()
    ra, r_last, t = None, None, 0
    for n in CALLS:
        rs, ra = oracle.rollout_uniform_sets(ref, 5, t, n, nsets, resume=t > 0, actions=ra,
                                             first_mask=r_last["mask"] if r_last else None, eps=eps)
        r_last = rs[(n - 1) % nsets]
        t += n
    np.testing.assert_array_equal(got["actions"], ra)
    for k in OUTPUTS:
        want = r_last[k]
        np.testing.assert_array_equal(got[k].reshape(want.shape), want, err_msg=k)
    np.testing.assert_array_equal(got["hmap"], ref.hmap)
    np.testing.assert_array_equal(got["ep_acc"], ref.ep_acc)
    np.testing.assert_array_equal(got["stats"], ref.episode_stats())
    for f in ref.state.dtype.names:
        if f != "pad":
            np.testing.assert_array_equal(got["state." + f], ref.state[f], err_msg=f)


def test_small_batches_and_one_group_take_the_single_chain(bpp):
    pool = bpp.sequences.cut2_pool((10, 10, 10), 16, seed=8)
    for E, groups, want in ((4099, 4, 1), (16384, 4, 2), (65536, 1, 1), (65536, None, bpp.vec_env.default_rollout_groups(65536, 10, 10)),
                            (16384, None, 1)):
        env = bpp.BppVecEnv(E, (10, 10, 10), pool=pool, rollout_groups=groups)
        assert env.rollout_groups == want
        env.close()
    assert bpp.vec_env.default_rollout_groups(65536, 10, 10) == 2 and bpp.vec_env.default_rollout_groups(32768, 20, 20) == 1
    with pytest.raises(ValueError):
        bpp.BppVecEnv(4099, (10, 10, 10), pool=pool, rollout_groups=5)
