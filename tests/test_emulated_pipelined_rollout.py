"""The pipelined rollout driver (include/bpp_pipeline.h) on the host emulator: its streams and events are no-ops there and a
launch runs at once, so what is left is WHAT it enqueues -- which groups, which slices of every array, which draws and
epsilon overrides behind which lock-step.  That must be what bpp_rollout_uniform_sets enqueues for all bins at once: both run
the one lock-step loop of csrc/bpp_drivers.inl.  (The overlap itself is tests/test_gpu_pipelined_rollout.py's subject.)"""
import ctypes

import numpy as np

SIZE = (10, 10, 10)
FIELDS = ("obs", "mask", "reward", "done", "counter", "ratio", "ep_ret", "ep_len")
CONTINUE = 1


def make_env(emu, E):
    from bpp_amd import sequences
    pool = sequences.cut2_pool(SIZE, 16, seed=4, native=False)
    env = emu.EmuEnv(pool, SIZE, False, E, env_id_base=3, env_id_total=E + 3)
    env.reset()
    return env


def rollout(emu, env, calls, nsets, eps, groups=None, pipe=None):
    """`calls`: [(step0, nsteps)], the first one drawn from the reset's mask, the others resumed.  groups: through
    bpp_rollout_uniform_sets_pipelined, else through bpp_rollout_uniform_sets.  Returns (output sets, actions)."""
    E, A, M = env.E, env.A, env.M
    sets = [dict(obs=np.zeros((E, 4 * A), np.float32), mask=np.zeros((E, M), np.float32), reward=np.zeros(E, np.float32),
                 done=np.zeros(E, np.uint8), counter=np.zeros(E, np.int32), ratio=np.zeros(E, np.float64),
                 ep_ret=np.zeros(E, np.float64), ep_len=np.zeros(E, np.int32)) for _ in range(nsets)]
    outs = (emu.StepOut * nsets)(*[emu.StepOut(*[d[k].ctypes.data for k in FIELDS]) for d in sets])
    actions = np.zeros(E, np.int64)
    lib = emu.lib()
    for i, (step0, n) in enumerate(calls):
        flags = (CONTINUE if i else 0) | (int(round(eps * (1 << 24))) << 8)
        args = (ctypes.byref(env._b), outs, nsets, env.out["mask"].ctypes.data, actions.ctypes.data, 5, step0, n, flags)
        rc = lib.bpp_rollout_uniform_sets_pipelined(*args, pipe, groups, None) if groups else lib.bpp_rollout_uniform_sets(*args, None)
        assert rc == 0, lib.bpp_last_error()
    return sets, actions


def assert_same_rollout(a, b, env_a, env_b):
    (sets_a, act_a), (sets_b, act_b) = a, b
    np.testing.assert_array_equal(act_a, act_b)
    for k, (sa, sb) in enumerate(zip(sets_a, sets_b)):
        for f in FIELDS:
            np.testing.assert_array_equal(sa[f], sb[f], err_msg="%s set %d" % (f, k))
    np.testing.assert_array_equal(env_a.hmap, env_b.hmap)
    for f in env_a.state.dtype.names:
        if f != "pad":
            np.testing.assert_array_equal(env_a.state[f], env_b.state[f], err_msg=f)
    np.testing.assert_array_equal(env_a.ep_acc, env_b.ep_acc)


def test_pipelined_driver_equals_the_single_chain_on_two_ragged_groups(emu):
    """16 448 bins in two groups -- the smallest two the plan makes, the second one ragged, the boundary not at half --, two
    output sets, epsilon = 0.25, 3 lock-steps and 2 more resumed: bit-identical to the same two calls on all bins at once."""
    E = 16448
    first, count = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    assert emu.lib().bpp_pipeline_plan(E, 2, first, count) == 2
    assert [(first[g], count[g]) for g in range(2)] == [(0, 8256), (8256, 8192)]
    pipe = ctypes.c_void_p()
    assert emu.lib().bpp_pipeline_create(ctypes.byref(pipe), 2) == 0 and pipe.value
    try:
        calls = [(0, 3), (3, 2)]
        piped, single, plain = make_env(emu, E), make_env(emu, E), make_env(emu, E)
        got = rollout(emu, piped, calls, 2, 0.25, groups=2, pipe=pipe)
        want = rollout(emu, single, calls, 2, 0.25)
        assert_same_rollout(got, want, piped, single)
        rollout(emu, plain, calls, 2, 0.0, groups=2, pipe=pipe)
        assert not np.array_equal(plain.hmap, piped.hmap)          # the override launches ran
    finally:
        assert emu.lib().bpp_pipeline_destroy(pipe) == 0


def test_a_plan_of_one_group_needs_no_pipe(emu):
    """100 bins asked to run in two groups make one: no pipe, and bpp_rollout_uniform_sets' results -- also for no lock-step at all."""
    E = 100
    for calls in ([(0, 4)], [(0, 0)]):
        piped, single = make_env(emu, E), make_env(emu, E)
        got = rollout(emu, piped, calls, 2, 0.25, groups=2, pipe=None)
        want = rollout(emu, single, calls, 2, 0.25)
        assert_same_rollout(got, want, piped, single)
        assert got[0][0]["obs"].any() == bool(calls[0][1])
