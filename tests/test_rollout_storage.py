"""CPU checks of the native returns (include/bpp_rollout.h) and of bpp_amd.RolloutStorage on the CPU: the host entry point and
the emulated device kernel against returns recorded from the reference's RolloutStorage.compute_returns
(tests/golden/returns_golden.npz; tests/golden/returns_edges.npz: chunk, lane and workgroup edges, subnormal numbers, inf and
NaN) and against the live reference, bit for bit; the done path against the masks path; which form a call takes; argument
validation; exports; the reference's own ACKTR update on a CPU storage; and a CPU storage fed by the emulated step kernel
against the reference's storage across updates (tests/golden/storage_updates_*.npz)."""
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
EDGE_CASES = rc.load_edge_cases() if os.path.exists(rc.EDGES) else []


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def emu_lib(emu):
    return _lib.bind_rollout(ctypes.CDLL(emu.LIB))


def check_against_recording(out, d, T, use_gae, want_returns, want_vlast, what):
    assert out["rc"] == 0, what
    assert rc.same_bits(out["returns"], want_returns), what      # every row: written ones AND returns[T] under GAE (NaN: rc.same_bits)
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


def edge_id(c):
    return "e%d_%s_T%d_N%d_g%s_l%s_gae%d_proper%d" % (c[0], c[10], c[2], c[3], c[4], c[5], c[6], c[7])


def test_the_edge_fixture_holds_what_it_claims():
    """tests/golden/make_returns_edges.py asserted this of the reference's results when it recorded them; here of the file."""
    assert len(EDGE_CASES) == 248
    seen = {(f, T, N, g, lam, u, p) for _, _, T, N, g, lam, u, p, _, _, f in EDGE_CASES}
    pairs = rc.edge_pairs()
    g, lam = pairs[-1]
    assert np.float32(g * lam) != np.float32(np.float32(g) * np.float32(lam)) and len(pairs) == 5
    shapes = {(T, N) for f, T, N, _, _, _, _ in seen if f == "unit"}
    assert all((T, 260) in shapes for T in rc.EDGE_T) and all((13, N) in shapes for N in rc.EDGE_N) and set(rc.EDGE_LONG) <= shapes
    for f, T, N, _, _, _, _ in list(seen):                       # all four variants wherever a shape and a pair occur
        for u, p in rc.VARIANTS:
            assert any(k[:3] == (f, T, N) and k[5:] == (u, p) for k in seen), (f, T, N, u, p)
    for pair in pairs:                                          # every pair at T = 13, N = 260, and on some other shape
        assert ("unit", 13, 260) + pair + (1, 1) in seen and len({k[1:3] for k in seen if k[3:5] == pair}) > 1, pair
    nan = {f: [0, 0] for f in rc.FAMILIES}
    for c, d, T, N, g, lam, u, p, want, vlast, f in EDGE_CASES:
        r = want[:T]
        sub = (r != 0.0) & (np.abs(r) < rc.FLT_MIN)
        assert all(np.isfinite(d[k]).all() for k in rc.INPUTS), c
        assert set(np.unique(d["masks"]).tolist()) <= {0.0, 1.0} and set(np.unique(d["bad_masks"]).tolist()) <= {0.0, 1.0}
        if f == "denormal":
            assert sub.any() and np.isfinite(r).all(), c
        elif f == "huge":
            assert np.isinf(r).any() and np.isnan(r).any(), c
        else:
            assert np.isfinite(r).all(), c
        nan[f][0] += int(np.isnan(r).sum())
        nan[f][1] += r.size
    # NaN positions are compared as a class (rc.same_bits): a minority where they occur, none anywhere else
    assert nan["unit"][0] == 0 and nan["denormal"][0] == 0 and 0 < 2 * nan["huge"][0] < nan["huge"][1]
    assert {f for *_, f in EDGE_CASES} == set(rc.FAMILIES)


@pytest.mark.parametrize("case", EDGE_CASES, ids=edge_id)
def test_host_entry_point_matches_the_recorded_edges(lib, case):
    c, d, T, N, gamma, lam, use_gae, proper, want, vlast, family = case
    for use_done in (False, True):
        out = rc.run(lib, d, T, N, gamma, lam, use_gae, proper, use_done=use_done, advantages=True)
        check_against_recording(out, d, T, use_gae, want, vlast, "done path" if use_done else "masks path")
        assert np.array_equal(rc.bits(out["masks"]), rc.bits(d["masks"]))
        with np.errstate(invalid="ignore", over="ignore"):
            assert rc.same_bits(out["advantages"], out["returns"][:T] - d["value_preds"][:T])


@pytest.mark.parametrize("case", EDGE_CASES, ids=edge_id)
def test_emulated_device_kernel_matches_the_recorded_edges(emu_lib, case):
    """Both forms of the kernel on the host emulator, masks path and done path: N % 4 == 0 takes four bins per lane (asserted
    through bpp_compute_returns_info), so T = 9, 13, 17, 33 and 1 000 run a full chunk of eight rows and then a partial one there."""
    c, d, T, N, gamma, lam, use_gae, proper, want, vlast, family = case
    for use_done in (False, True):
        out = rc.run(emu_lib, d, T, N, gamma, lam, use_gae, proper, use_done=use_done, advantages=True, kernel=True)
        assert out["form"] == (4 if N % 4 == 0 else 1)
        check_against_recording(out, d, T, use_gae, want, vlast, "done path" if use_done else "masks path")
        assert np.array_equal(rc.bits(out["masks"]), rc.bits(d["masks"]))
        with np.errstate(invalid="ignore", over="ignore"):
            assert rc.same_bits(out["advantages"], out["returns"][:T] - d["value_preds"][:T])


MOVABLE = ("rewards", "value_preds", "next_value", "masks", "bad_masks", "returns0", "advantages", "done")


@pytest.mark.parametrize("moved", MOVABLE)
def test_one_misplaced_array_selects_one_bin_per_lane(lib, emu_lib, moved):
    """N % 4 == 0: any one float array 4 bytes off a 16-byte boundary, or `done` 1, 2 or 3 bytes off a 4-byte boundary, selects the
    one-bin-per-lane form (bpp_compute_returns_info), and the emulated kernel gives the bits of the aligned call."""
    T, N = 13, 260
    d = rc.family_inputs("unit", T, N, seed=77)
    done = rc.done_of(d["masks"])
    want = rc.run(lib, d, T, N, 0.99, 0.95, 1, 1, use_done=True, advantages=True)
    info = (ctypes.c_int32 * 3)()
    for shift in ((1, 2, 3, 5) if moved == "done" else (4, 8, 12)):
        for use_done in (False, True):
            if moved == "done" and not use_done:
                continue
            a = {k: rc.placed(v, shift if k == moved else 0) for k, v in d.items()}
            a["done"] = rc.placed(done, shift if moved == "done" else 0)
            a["advantages"] = rc.placed(np.full((T, N), -7.0, np.float32), shift if moved == "advantages" else 0)
            if use_done:
                a["masks"][1:] = -7.0
            args = [a["rewards"].ctypes.data, a["value_preds"].ctypes.data, a["next_value"].ctypes.data, a["done"].ctypes.data if use_done else None,
                    a["masks"].ctypes.data, a["bad_masks"].ctypes.data, a["returns0"].ctypes.data, a["advantages"].ctypes.data, T, N, 1, 1, 0.99, 0.95]
            for handle in (lib, emu_lib):
                assert handle.bpp_compute_returns_info(*args, info) == 0 and list(info) == [1, 256, 2], (shift, use_done)
            assert emu_lib.bpp_compute_returns(*args, None) == 0
            for k, w in (("returns0", "returns"), ("value_preds", "value_preds"), ("masks", "masks"), ("advantages", "advantages")):
                assert np.array_equal(rc.bits(a[k]), rc.bits(want[w])), (k, shift, use_done)
    a = {k: rc.placed(v, 0) for k, v in d.items()}
    args = [a["rewards"].ctypes.data, a["value_preds"].ctypes.data, a["next_value"].ctypes.data, rc.placed(done, 4).ctypes.data,
            a["masks"].ctypes.data, a["bad_masks"].ctypes.data, a["returns0"].ctypes.data, None, T, N, 1, 1, 0.99, 0.95]
    assert lib.bpp_compute_returns_info(*args, info) == 0 and list(info) == [4, 64, 2]         # 65 lanes: one in the second workgroup
    assert lib.bpp_compute_returns_info(*args[:9], 259, *args[10:], info) == 0 and list(info) == [1, 256, 2]
    assert lib.bpp_compute_returns_info(*args, None) == BADARG


@pytest.mark.skipif(not ref_shims.available(), reason="reference tree not present")
@pytest.mark.parametrize("T,N", [(7, 1001), (3, 35), (40, 130)])
def test_host_entry_point_matches_the_live_reference(lib, T, N):
    ref_shims.install()
    from acktr.storage import RolloutStorage
    draws = [(rc.random_inputs(T, N, seed=100 * T + k), pair) for k, pair in enumerate(((0.99, 0.95), (1.0, 1.0), (0.5, 0.3)))]
    # the value families and the (gamma, lambda) pairs of the edge fixture, drawn afresh
    draws += [(rc.family_inputs(f, T, N, seed=300 * T + k), pair) for k, (f, pair) in
              enumerate([("denormal", (0.99, 0.95)), ("huge", (0.99, 0.95)), ("huge", (1.0, 1.0)), ("unit", (0.0, 0.95)), ("unit", (0.99, 0.0)),
                         ("denormal", rc.split_product_pair()), ("unit", rc.split_product_pair())])]
    for d, (gamma, lam) in draws:
        for use_gae, proper in rc.VARIANTS:
            st = RolloutStorage(T, N, (1,), bpp_amd.Discrete(1), 1, can_give_up=False, enable_rotation=False, pallet_size=1)
            for name in ("rewards", "value_preds", "masks", "bad_masks"):
                getattr(st, name).copy_(torch.from_numpy(d[name]).unsqueeze(-1))
            st.returns.copy_(torch.from_numpy(d["returns0"]).unsqueeze(-1))
            st.compute_returns(torch.from_numpy(d["next_value"]).unsqueeze(-1), bool(use_gae), gamma, lam, bool(proper))
            out = rc.run(lib, d, T, N, gamma, lam, use_gae, proper, advantages=True)
            check_against_recording(out, d, T, use_gae, st.returns.numpy()[:, :, 0], st.value_preds.numpy()[-1, :, 0], (T, N, gamma, use_gae, proper))
            adv = (st.returns[:-1] - st.value_preds[:-1]).numpy()[:, :, 0]
            assert rc.same_bits(out["advantages"], adv)


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


STORAGE_SLABS = ("obs", "location_masks", "rewards", "value_preds", "returns", "masks", "bad_masks", "actions", "action_log_probs")


def snapshot(st, names=STORAGE_SLABS):
    return {k: getattr(st, k).detach().cpu().numpy().copy() for k in names}


@pytest.mark.parametrize("name", rc.STORAGE_CASES)
def test_the_storage_fixture_holds_what_it_claims(name):
    g, s = rc.load_storage_case(name)
    T, U, N = int(s["T"]), int(s["U"]), g["actions"].shape[1]
    assert U >= 3 and T == 5 and s["returns"].shape == (U, T + 1, N) == s["masks"].shape == s["value_preds"].shape
    assert s["main"].tolist() == [0.0, 1.0, 0.95, 0.0] and s["gae"].tolist() == [1.0, 0.99, 0.95, 1.0]
    for u in range(U):
        done = g["done"][u * T:(u + 1) * T]
        assert done.any() and not done.all()                                   # episodes end inside every update
        assert np.array_equal(s["masks"][u][1:], np.where(done != 0, 0.0, 1.0).astype(np.float32))
        assert np.array_equal(s["masks"][u][0], s["masks"][u - 1][T] if u else np.ones(N, np.float32))      # after_update
        assert np.array_equal(rc.bits(s["value_preds"][u][T]), rc.bits(s["next_value"][u]))
        assert np.array_equal(rc.bits(s["returns_main"][u][T]), rc.bits(s["next_value"][u]))
        assert not np.array_equal(s["returns"][u][:T], s["returns_main"][u][:T]) and np.isfinite(s["returns"][u]).all()
    assert (s["masks"][1:, 0] == 0.0).any()                                    # ... and a carried-over row differs from ones


@pytest.mark.parametrize("name", rc.STORAGE_CASES)
def test_cpu_storage_fed_by_the_emulated_step_kernel_equals_the_reference_storage_across_updates(emu, name):
    """The GPU replay of tests/test_gpu_rollout_storage.py without a GPU: the emulated step kernel plays the recorded actions, a CPU
    storage takes every lock-step through insert() and the host entry point computes the returns."""
    g, s = rc.load_storage_case(name)
    T, U, N = int(s["T"]), int(s["U"]), g["actions"].shape[1]
    size, rot = tuple(int(v) for v in g["size"]), bool(g["rotation"])
    env = emu.EmuEnv(g["pool"], size, rot, N, mask_rule=0)
    st = bpp_amd.RolloutStorage(T, N, (g["obs"].shape[2],), bpp_amd.Discrete(g["mask"].shape[2]), 1)
    obs, mask = env.reset()
    st.obs[0].copy_(torch.from_numpy(obs))
    st.location_masks[0].copy_(torch.from_numpy(mask))

    def col(a):
        return torch.from_numpy(np.ascontiguousarray(a)).unsqueeze(-1)

    for u in range(U):
        for t in range(T):
            assert st.step == t
            a = g["actions"][u * T + t]
            o = env.step(a)
            assert set(np.unique(o["done"]).tolist()) <= {0, 1}
            st.insert(torch.from_numpy(o["obs"]), torch.zeros(N, 1), col(a), col(s["log_probs"][u, t]), col(s["values"][u, t]), col(o["reward"]),
                      1.0 - col(o["done"]).to(torch.float32), torch.ones(N, 1), torch.from_numpy(o["mask"]))
        assert st.step == 0
        nv = col(s["next_value"][u])
        assert st.compute_returns(nv, bool(s["main"][0]), s["main"][1], s["main"][2], bool(s["main"][3])) is None
        main = st.returns.numpy().copy()
        st.compute_returns(nv, bool(s["gae"][0]), s["gae"][1], s["gae"][2], bool(s["gae"][3]))
        rc.check_storage_update(dict(snapshot(st), returns_main=main), g, s, u, small_rows=())
        st.after_update()


def filled_cpu_storage(T, N, seed, from_done):
    d = rc.random_inputs(T, N, seed, bad_ones=True)
    st = bpp_amd.RolloutStorage(T, N, (4,), bpp_amd.Discrete(4), 1)
    for k in ("rewards", "value_preds", "masks", "bad_masks"):
        getattr(st, k).copy_(torch.from_numpy(d[k]).unsqueeze(-1))
    st.done.copy_(torch.from_numpy(rc.done_of(d["masks"])))                      # bytes 1 and 255 for "done"
    st._from_done = list(from_done)
    return st, d


@pytest.mark.parametrize("variant", [(False, 0.99, 0.95, False), (True, 0.99, 0.95, True)], ids=["main", "gae_proper"])
def test_a_rollout_filled_both_ways_reads_any_nonzero_done_byte_as_done(lib, variant):
    """compute_returns on rows filled partly by lock-steps (done bytes) and partly by insert() (masks): the masks of the former are
    rebuilt from the bytes, any nonzero byte being 'done' as in the kernel -- hand-written bytes, 255 among them."""
    T, N = 7, 37
    for from_done in ([t % 2 == 0 for t in range(T)], [True] * T, [False] * T):
        st, d = filled_cpu_storage(T, N, 4, from_done)
        assert (st.done == 255).any() and (st.done == 1).any()
        for t in range(T):
            if from_done[t]:
                st.masks[t + 1].fill_(-7.0)                                      # not valid yet on these rows: must not be read
        nv = torch.from_numpy(d["next_value"]).unsqueeze(-1)
        st.compute_returns(nv, *variant)
        want = rc.run(lib, d, T, N, variant[1], variant[2], int(variant[0]), int(variant[3]))
        assert np.array_equal(rc.bits(st.masks.numpy()[:, :, 0]), rc.bits(d["masks"]))
        rows = slice(0, T) if variant[0] else slice(0, T + 1)
        assert np.array_equal(rc.bits(st.returns.numpy()[rows, :, 0]), rc.bits(want["returns"][rows])), from_done
        # a second call in a row changes nothing (GAE: value_preds[T] already holds next_value)
        before = snapshot(st, ("returns", "value_preds", "masks", "rewards"))
        st.compute_returns(nv, *variant)
        for k, v in before.items():
            assert np.array_equal(rc.bits(getattr(st, k).numpy()), rc.bits(v)), k


def test_next_value_of_the_wrong_size_is_refused():
    st, d = filled_cpu_storage(3, 8, 1, [False] * 3)
    for n in (9, 7, 16):
        with pytest.raises(ValueError, match="one value per bin"):
            st.compute_returns(torch.zeros(n, 1), False, 0.99, 0.95, False)
    st.compute_returns(torch.zeros(8), False, 0.99, 0.95, False)
