"""CPU checks of the native returns (include/bpp_rollout.h) and of bpp_amd.RolloutStorage on the CPU: the host entry point and
the emulated device kernel against returns recorded from the reference's RolloutStorage.compute_returns
(tests/golden/returns_golden.npz) and against the live reference, bit for bit; the done path against the masks path; argument
validation; exports; and the reference's own ACKTR update on a CPU storage."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import bpp_amd
from bpp_amd import _lib
from oracle import ref_shims

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import returns_cases as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -1
CASES = rc.load_cases() if os.path.exists(rc.GOLDEN) else []


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def emu_lib(emu):
    return _lib.bind_rollout(ctypes.CDLL(emu.LIB))


def check_against_recording(out, d, T, use_gae, want_returns, want_vlast, what):
    assert out["rc"] == 0, what
    assert np.array_equal(rc.bits(out["returns"]), rc.bits(want_returns)), what      # every row: written ones AND returns[T] under GAE
    if use_gae:
        assert np.array_equal(rc.bits(out["returns"][T]), rc.bits(d["returns0"][T])), what   # ... which the reference leaves alone
    assert np.array_equal(rc.bits(out["value_preds"][T]), rc.bits(want_vlast)), what
    assert np.array_equal(rc.bits(out["value_preds"][:T]), rc.bits(d["value_preds"][:T])), what
    assert np.array_equal(rc.bits(out["masks"][0]), rc.bits(d["masks"][0])), what


def test_the_fixture_holds_the_whole_grid():
    assert len(CASES) == 40
    seen = {(T, N, g, lam, u, p) for _, _, T, N, g, lam, u, p, _, _ in CASES}
    for T, N in ((5, 256), (1, 257), (32, 67)):
        for g, lam in ((1.0, 0.95), (0.99, 0.95), (0.9, 0.5)):
            for u, p in rc.VARIANTS:
                assert (T, N, g, lam, u, p) in seen
    d = CASES[-1][1]          # the input set with bad_masks of ones and signed zeros
    assert (d["bad_masks"] == 1.0).all() and np.signbit(d["rewards"][d["rewards"] == 0.0]).any()
    assert np.signbit(d["value_preds"][d["value_preds"] == 0.0]).any()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "c%d_T%d_N%d_g%s_l%s_gae%d_proper%d" % (c[0], c[2], c[3], c[4], c[5], c[6], c[7]))
def test_host_entry_point_matches_the_recorded_reference_bit_for_bit(lib, case):
    c, d, T, N, gamma, lam, use_gae, proper, want, vlast = case
    out = rc.run(lib, d, T, N, gamma, lam, use_gae, proper)
    check_against_recording(out, d, T, use_gae, want, vlast, "masks path")
    assert np.array_equal(rc.bits(out["masks"]), rc.bits(d["masks"]))                 # an input on this path
    # the same through the done bytes: identical returns, masks rows 1 .. T written as exact 0.0 / 1.0, row 0 untouched
    out = rc.run(lib, d, T, N, gamma, lam, use_gae, proper, use_done=True)
    check_against_recording(out, d, T, use_gae, want, vlast, "done path")
    assert np.array_equal(rc.bits(out["masks"]), rc.bits(d["masks"]))
    if (d["bad_masks"] == 1.0).all():                                                 # NULL bad_masks = a row of ones
        out = rc.run(lib, d, T, N, gamma, lam, use_gae, proper, bad=False)
        check_against_recording(out, d, T, use_gae, want, vlast, "bad_masks NULL")


@pytest.mark.parametrize("case", CASES, ids=lambda c: "c%d_T%d_N%d" % (c[0], c[2], c[3]))
def test_emulated_device_kernel_matches_the_recorded_reference_bit_for_bit(emu_lib, case):
    """The device kernel's indexing on the host emulator: N = 256 takes the 16-byte path, 257 and 67 the one-bin-per-lane path."""
    c, d, T, N, gamma, lam, use_gae, proper, want, vlast = case
    for use_done in (False, True):
        out = rc.run(emu_lib, d, T, N, gamma, lam, use_gae, proper, use_done=use_done, advantages=True, kernel=True)
        check_against_recording(out, d, T, use_gae, want, vlast, "done path" if use_done else "masks path")
        assert np.array_equal(rc.bits(out["masks"]), rc.bits(d["masks"]))
        assert np.array_equal(rc.bits(out["advantages"]), rc.bits(out["returns"][:T] - d["value_preds"][:T]))


def test_emulated_kernel_on_misaligned_arrays_takes_the_scalar_path(emu_lib, lib):
    """N % 4 == 0 but an array that does not start on 16 bytes: same bits as the host entry point."""
    T, N = 9, 128
    d = rc.random_inputs(T, N, seed=5)
    buf = np.zeros(T * N + 1, dtype=np.float32)
    buf[1:] = d["rewards"].reshape(-1)
    d["rewards"] = buf[1:].reshape(T, N)
    assert d["rewards"].ctypes.data % 16 != 0
    for use_gae, proper in rc.VARIANTS:
        want = rc.run(lib, d, T, N, 0.99, 0.95, use_gae, proper)
        # (run() copies its inputs: hand the kernel the misaligned view itself)
        ret, vp = d["returns0"].copy(), d["value_preds"].copy()
        r = emu_lib.bpp_compute_returns(d["rewards"].ctypes.data, vp.ctypes.data, d["next_value"].ctypes.data, None, d["masks"].ctypes.data,
                                        d["bad_masks"].ctypes.data, ret.ctypes.data, None, T, N, use_gae, proper, 0.99, 0.95, None)
        assert r == 0 and np.array_equal(rc.bits(ret), rc.bits(want["returns"]))


@pytest.mark.skipif(not ref_shims.available(), reason="reference tree not present")
@pytest.mark.parametrize("T,N", [(7, 1001), (3, 35), (40, 130)])
def test_host_entry_point_matches_the_live_reference(lib, T, N):
    ref_shims.install()
    from acktr.storage import RolloutStorage
    for k, (gamma, lam) in enumerate(((0.99, 0.95), (1.0, 1.0), (0.5, 0.3))):
        d = rc.random_inputs(T, N, seed=100 * T + k)
        for use_gae, proper in rc.VARIANTS:
            st = RolloutStorage(T, N, (1,), bpp_amd.Discrete(1), 1, can_give_up=False, enable_rotation=False, pallet_size=1)
            for name in ("rewards", "value_preds", "masks", "bad_masks"):
                getattr(st, name).copy_(torch.from_numpy(d[name]).unsqueeze(-1))
            st.returns.copy_(torch.from_numpy(d["returns0"]).unsqueeze(-1))
            st.compute_returns(torch.from_numpy(d["next_value"]).unsqueeze(-1), bool(use_gae), gamma, lam, bool(proper))
            out = rc.run(lib, d, T, N, gamma, lam, use_gae, proper, advantages=True)
            check_against_recording(out, d, T, use_gae, st.returns.numpy()[:, :, 0], st.value_preds.numpy()[-1, :, 0], (T, N, gamma, use_gae, proper))
            adv = (st.returns[:-1] - st.value_preds[:-1]).numpy()[:, :, 0]
            assert np.array_equal(rc.bits(out["advantages"]), rc.bits(adv))


@pytest.mark.parametrize("use_gae,proper", rc.VARIANTS)
def test_done_path_and_masks_path_agree_and_masks_may_be_null(lib, use_gae, proper):
    T, N = 11, 203
    d = rc.random_inputs(T, N, seed=9)
    a = rc.run(lib, d, T, N, 0.99, 0.95, use_gae, proper, advantages=True)
    b = rc.run(lib, d, T, N, 0.99, 0.95, use_gae, proper, use_done=True, advantages=True)
    c = rc.run(lib, d, T, N, 0.99, 0.95, use_gae, proper, use_done=True, masks_out=False)
    assert a["rc"] == b["rc"] == c["rc"] == 0
    assert np.array_equal(rc.bits(a["returns"]), rc.bits(b["returns"])) and np.array_equal(rc.bits(a["returns"]), rc.bits(c["returns"]))
    assert np.array_equal(rc.bits(b["masks"]), rc.bits(d["masks"]))              # exact 0.0 / 1.0 in rows 1 .. T, row 0 as it was
    assert set(np.unique(b["masks"][1:]).tolist()) <= {0.0, 1.0}
    for o in (a, b):
        assert np.array_equal(rc.bits(o["advantages"]), rc.bits(o["returns"][:T] - o["value_preds"][:T]))


def test_invalid_arguments_are_refused(lib):
    T, N = 3, 8
    d = rc.random_inputs(T, N, seed=1)
    ret = d["returns0"].copy()
    ptr = {k: v.ctypes.data for k, v in d.items()}
    done = rc.done_of(d["masks"])

    def call(host, **kw):
        a = dict(rewards=ptr["rewards"], value_preds=ptr["value_preds"], next_value=ptr["next_value"], done=None, masks=ptr["masks"],
                 bad_masks=ptr["bad_masks"], returns=ret.ctypes.data, advantages=None, T=T, N=N)
        a.update(kw)
        args = [a[k] for k in ("rewards", "value_preds", "next_value", "done", "masks", "bad_masks", "returns", "advantages", "T", "N")] + \
            [1, 1, 0.99, 0.95]
        return lib.bpp_compute_returns_host(*args) if host else lib.bpp_compute_returns(*args, None)

    assert call(True) == 0
    assert call(True, masks=None, done=done.ctypes.data) == 0
    for host in (True, False):       # the device entry point validates before any device is touched (there is none here)
        for bad in (dict(T=0), dict(T=-1), dict(N=0), dict(N=-5), dict(rewards=None), dict(value_preds=None), dict(next_value=None),
                    dict(returns=None), dict(masks=None)):
            assert call(host, **bad) == BADARG, (host, bad)
            assert lib.bpp_last_error()


def test_every_declared_symbol_is_exported(lib):
    src = open(os.path.join(ROOT, "include", "bpp_rollout.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(bpp_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.ROLLOUT_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.bpp_abi_version() == 16


def test_storage_has_the_reference_layout():
    T, N = 5, 6
    st = bpp_amd.RolloutStorage(T, N, (400,), bpp_amd.Discrete(100), 1)
    shapes = dict(obs=(T + 1, N, 400), recurrent_hidden_states=(T + 1, N, 1), rewards=(T, N, 1), value_preds=(T + 1, N, 1),
                  returns=(T + 1, N, 1), action_log_probs=(T, N, 1), actions=(T, N, 1), masks=(T + 1, N, 1), bad_masks=(T + 1, N, 1),
                  location_masks=(T + 1, N, 100))
    for name, shape in shapes.items():
        t = getattr(st, name)
        assert tuple(t.shape) == shape and t.dtype == (torch.int64 if name == "actions" else torch.float32), name
        assert t.is_contiguous() and t[0].is_contiguous() and t[:-1].reshape(-1).data_ptr() == t.data_ptr(), name
    assert bool((st.masks == 1).all()) and bool((st.bad_masks == 1).all()) and not st.obs.any()
    assert st.num_steps == T and st.step == 0
    with pytest.raises(RuntimeError, match="insert"):
        st.output_sets()              # the step kernel does not write into host memory


@pytest.mark.skipif(not ref_shims.available(), reason="reference tree not present")
def test_cpu_storage_goes_through_the_reference_update(emu):
    """tests/test_training_glue.py's loop with bpp_amd.RolloutStorage (CPU) beside the reference's, fed the same tensors."""
    ref_shims.install()
    from acktr import algo
    from acktr.model import Policy
    from acktr.storage import RolloutStorage
    from bpp_amd.vec_env import StepTensors

    size, E, num_steps = (10, 10, 10), 8, 5
    args = types.SimpleNamespace(channel=4, container_size=size, pallet_size=10, enable_rotation=False, num_processes=E, num_steps=num_steps)
    obs_space, act_space = bpp_amd.Box(0.0, 10, (400,)), bpp_amd.Discrete(100)
    torch.manual_seed(0)
    actor_critic = Policy(obs_space.shape, act_space, base_kwargs={"recurrent": False, "hidden_size": 256, "args": args})
    agent = algo.ACKTR(actor_critic, 0.5, 0.01, 1.0, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5, acktr=False, args=args)
    ref = RolloutStorage(num_steps, E, obs_space.shape, act_space, actor_critic.recurrent_hidden_state_size, can_give_up=False,
                         enable_rotation=False, pallet_size=10)
    mine = bpp_amd.RolloutStorage(num_steps, E, obs_space.shape, act_space, actor_critic.recurrent_hidden_state_size)
    env = emu.EmuEnv(bpp_amd.sequences.cut2_pool(size, 8, seed=0), size, False, E)
    obs, mask = env.reset()
    for st in (ref, mine):
        st.obs[0].copy_(torch.from_numpy(obs))
        st.location_masks[0].copy_(torch.from_numpy(mask))
    location_masks = torch.from_numpy(mask)
    for update in range(2):
        for step in range(num_steps):
            assert mine.step == step
            with torch.no_grad():
                value, action, action_log_prob, rnn = actor_critic.act(mine.obs[step], mine.recurrent_hidden_states[step], mine.masks[step],
                                                                       location_masks)
            o = env.step(action.numpy()[:, 0])
            res = StepTensors(obs=torch.from_numpy(o["obs"]), mask=torch.from_numpy(o["mask"]), reward=torch.from_numpy(o["reward"]).unsqueeze(1),
                              done=torch.from_numpy(o["done"]), counter=torch.from_numpy(o["counter"]), ratio=torch.from_numpy(o["ratio"]),
                              ep_ret=torch.from_numpy(o["ep_ret"]), ep_len=torch.from_numpy(o["ep_len"]))
            location_masks = res.mask
            for st in (ref, mine):
                st.insert(res.obs, rnn, action, action_log_prob, value, res.reward, res.masks, res.bad_masks, location_masks)
        with torch.no_grad():
            next_value = actor_critic.get_value(mine.obs[-1], mine.recurrent_hidden_states[-1], mine.masks[-1]).detach()
        for variant in ((False, 1.0, 0.95, False), (True, 0.99, 0.95, True)):          # main.py's call, and GAE with proper time limits
            ref.compute_returns(next_value, *variant)
            adv = mine.compute_returns(next_value, *variant, advantages=True)
            for name in ("obs", "rewards", "value_preds", "returns", "masks", "bad_masks", "actions", "action_log_probs", "location_masks"):
                assert torch.equal(getattr(ref, name), getattr(mine, name)), (update, variant, name)
            assert np.array_equal(rc.bits(mine.returns.numpy()), rc.bits(ref.returns.numpy()))
            assert torch.equal(adv, ref.returns[:-1] - ref.value_preds[:-1])
        ref.compute_returns(next_value, False, 1.0, 0.95, False)
        assert mine.compute_returns(next_value, False, 1.0, 0.95, False) is None
        out = agent.update(mine)                                                      # the reference's update takes it unchanged
        assert len(out) == 5 and all(np.isfinite(float(v)) for v in out)
        ref.after_update()
        mine.after_update()
        for name in ("obs", "masks", "bad_masks", "location_masks", "recurrent_hidden_states"):
            assert torch.equal(getattr(ref, name)[0], getattr(mine, name)[0]), name
