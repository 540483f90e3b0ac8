"""bpp_a2c_loss (include/bpp_update.h) without a GPU: the product kernels of csrc/bpp_update.inl compiled by g++
against the SIMT emulator, bound with _lib.bind_update.  The five loss terms of acktr/algo/acktr_pipeline.py:45-92 and the
gradients at the three network outputs against (1) the emulated bpp_masked_evaluate kernels bit for bit, (2) the header's
normative float32 expressions in numpy, (3) double sums of the per-row terms, (4) float64 autograd of the reference's
expressions and (7) the live reference's own update().  Helpers and tolerances: tests/a2c_cases.py."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from bpp_amd import _lib
from oracle import ref_shims

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import a2c_cases as ac  # noqa: E402
import head_normative as hn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -1
MS = [15, 64, 91, 100, 200, 400, 516]
ES = [1, 3, 4, 5, 257]
WIDTH = 1024            # first-level width of the reduction (asserted against bpp_a2c_loss_info below)


@pytest.fixture(scope="module")
def emu_lib(emu):
    import emu_binding
    inl = os.path.join(ROOT, "online-3d-bpp-drl_amd", "csrc", "bpp_update.inl")
    if os.path.getmtime(inl) > os.path.getmtime(emu.LIB):          # the emulator's own dependency list predates this file
        emu_binding.build(force=True)
    return _lib.bind_update(ctypes.CDLL(emu.LIB))


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


# every M at one E that fills several workgroups with a partial last one, every E at the shipped M = 100, the corners,
# and rows beyond the first-level width: WIDTH + 1 rows, and 4 * WIDTH + 1 rows = the first size with two row groups per workgroup
SHAPES = [(5, M) for M in MS] + [(E, 100) for E in ES if E != 5] + [(1, 15), (1, 516), (257, 15), (3, 516), (WIDTH + 1, 15),
                                                                    (4 * WIDTH + 1, 15)]


@pytest.fixture(scope="module")
def results(emu_lib):
    """(case, output) per shape, computed once and never modified."""
    cache = {}

    def get(E, M):
        if (E, M) not in cache:
            c = ac.make_case(E, M, seed=1000 * E + M)
            out = ac.run_host(emu_lib, c)
            assert out["rc"] == 0
            cache[(E, M)] = (c, out)
        return cache[(E, M)]
    return get


@pytest.mark.parametrize("E,M", SHAPES)
def test_pieces_equal_the_evaluate_kernels_and_the_normative_expressions_bit_for_bit(emu, results, E, M):
    c, out = results(E, M)
    ac.check_pieces(out, c, emu.masked_evaluate, emu.masked_evaluate_backward)


@pytest.mark.parametrize("E,M", SHAPES)
def test_terms_are_the_double_sums_of_the_rows_and_repeat_bit_for_bit(emu_lib, results, E, M):
    c, out = results(E, M)
    ac.check_terms(out, c)
    again = ac.run_host(emu_lib, c)
    for k in ("terms", "rows", "grad_logits", "grad_values", "grad_pred_mask"):
        assert np.array_equal(ac.bits(again[k]), ac.bits(out[k])), k
    without_rows = ac.run_host(emu_lib, c, rows=False)
    assert np.array_equal(ac.bits(without_rows["terms"]), ac.bits(out["terms"])) and np.all(without_rows["rows"] == ac.CANARY)


@pytest.mark.parametrize("E,M", SHAPES)
def test_terms_and_gradients_against_float64_autograd_of_the_reference(results, E, M):
    c, out = results(E, M)
    ref = ac.check_against_float64(out, c)
    # the two gradients that are one float32 product each
    np.testing.assert_allclose(out["grad_values"], ref["grad_values"], rtol=4 * ac.EPS, atol=0)
    np.testing.assert_allclose(out["grad_pred_mask"], ref["grad_pred_mask"], rtol=4 * ac.EPS, atol=0)


@pytest.mark.parametrize("M", hn.MS)
def test_rows_and_gradient_equal_the_normative_statement_bit_for_bit(emu_lib, M):
    """Against tests/head_normative.py, which shares no code with the kernels (the check above compares them with each other)."""
    c, want = hn.case(M)
    out = ac.run_host(emu_lib, c)
    assert out["rc"] == 0
    rows = np.stack([-(c["adv"] * want["logp"]), want["ent"], want["bad"]], axis=1)
    np.testing.assert_array_equal(hn.bits(out["rows"][:, 1:4]), hn.bits(rows))
    np.testing.assert_array_equal(hn.bits(out["grad_logits"]), hn.bits(want["grad"]))


def test_other_coefficients(emu, emu_lib):
    coefs = (0.25, 0.0, 7.5, 0.125)
    c = ac.make_case(9, 91, seed=5)
    out = ac.run_host(emu_lib, c, coefs)
    assert out["rc"] == 0
    ac.check_pieces(out, c, emu.masked_evaluate, emu.masked_evaluate_backward, coefs)
    ac.check_terms(out, c, coefs)
    ac.check_against_float64(out, c, coefs)


def test_an_action_out_of_range_is_treated_as_masked_evaluate_treats_it(emu, emu_lib):
    for M in (100, 516):
        c = ac.make_case(6, M, seed=M)
        c["a"][[0, 3, 4]] = (-1, M, 1 << 40)
        out = ac.run_host(emu_lib, c)
        assert out["rc"] == 0
        ac.check_pieces(out, c, emu.masked_evaluate, emu.masked_evaluate_backward)
        ac.check_terms(out, c)


@pytest.mark.parametrize("E,M", [(5, 100), (3, 516)])
def test_without_pred_mask_the_graph_loss_is_zero_and_its_gradient_is_not_written(emu, emu_lib, results, E, M):
    c, full = results(E, M)
    out = ac.run_host(emu_lib, c, pred=False)
    assert out["rc"] == 0
    assert out["terms"][4] == 0.0 and not out["rows"][:, 4].any()
    assert np.array_equal(ac.bits(out["terms"][:4]), ac.bits(full["terms"][:4]))
    assert np.all(out["grad_pred_mask"] == ac.CANARY)
    for k in ("grad_logits", "grad_values"):
        assert np.array_equal(ac.bits(out[k]), ac.bits(full[k])), k
    assert np.array_equal(ac.bits(out["rows"][:, :4]), ac.bits(full["rows"][:, :4]))
    ac.check_pieces(out, c, emu.masked_evaluate, emu.masked_evaluate_backward, pred=False)
    ac.check_terms(out, c)
    vc, ec, ic, mc = ac.COEFS
    t = out["terms"].astype(np.float64)
    np.testing.assert_allclose(out["terms"][5], vc * t[0] + t[1] + ic * t[3] - ec * t[2], rtol=4 * ac.EPS)


def test_invalid_arguments_are_refused_before_any_device_is_touched(lib, emu_lib):
    E, M = 3, 8
    c = ac.make_case(E, M, seed=1)
    bufs = dict(logits=c["x"], location_masks=c["m"], action=c["a"], values=c["val"], returns=c["ret"], pred_mask=c["pm"],
                grad_logits=np.zeros((E, M), np.float32), grad_values=np.zeros(E, np.float32), grad_pred_mask=np.zeros((E, M), np.float32),
                rows=np.zeros((E, 5), np.float32), terms=np.zeros(6, np.float32), workspace=np.zeros(64, np.float64))
    order = ("logits", "location_masks", "action", "values", "returns", "pred_mask")
    outs = ("grad_logits", "grad_values", "grad_pred_mask", "rows", "terms", "workspace")

    def call(L, **kw):
        a = {k: v.ctypes.data for k, v in bufs.items()}
        a.update(E=E, M=M)
        a.update(kw)
        return L.bpp_a2c_loss(*[a[k] for k in order], *ac.COEFS, *[a[k] for k in outs], a["E"], a["M"], None)

    assert call(emu_lib) == 0 and call(emu_lib, pred_mask=None, grad_pred_mask=None, rows=None) == 0
    info = (ctypes.c_int32 * 4)()
    for L in (lib, emu_lib):            # the product library has no device here: it must refuse before it looks for one
        for bad in [dict(E=0), dict(E=-3), dict(M=0), dict(M=-1), dict(grad_pred_mask=None)] + \
                [{k: None} for k in ("logits", "location_masks", "action", "values", "returns", "grad_logits", "grad_values", "terms", "workspace")]:
            assert call(L, **bad) == BADARG, bad
            assert L.bpp_last_error()
        for e, m in ((0, 5), (5, 0), (-1, 5)):
            assert L.bpp_a2c_loss_info(e, m, info) == BADARG and L.bpp_a2c_loss_workspace(e, m) == 0
        assert L.bpp_a2c_loss_info(5, 5, None) == BADARG


def test_every_declared_symbol_is_exported(lib):
    src = open(os.path.join(ROOT, "include", "bpp_update.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(bpp_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.UPDATE_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.bpp_abi_version() == 16


def test_info_tells_the_path_and_the_shape_of_the_reduction(lib, emu_lib):
    for L in (lib, emu_lib):
        assert ac.info(L, 5, 400) == [4, 2, 1, WIDTH] and ac.info(L, 5, 512)[2] == 1
        assert ac.info(L, 5, 516) == [4, 2, 0, WIDTH] and ac.info(L, 5, 513)[2] == 0
        assert ac.info(L, 1, 15) == [4, 1, 1, WIDTH]
        assert ac.info(L, 4 * WIDTH, 15) == [4, WIDTH, 1, WIDTH]
        assert ac.info(L, 4 * WIDTH + 1, 15) == [8, 513, 1, WIDTH]           # two row groups per workgroup from here on
        assert ac.info(L, 5 * 65536, 100) == [320, 1024, 1, WIDTH]
        for E, M in ((1, 15), (4 * WIDTH + 1, 15), (5 * 65536, 100)):
            r, g = ac.info(L, E, M)[:2]
            assert L.bpp_a2c_loss_workspace(E, M) == g * 5 * 8 and (g - 1) * r < E <= g * r


def test_the_python_entry_point_refuses_cpu_tensors():
    import bpp_amd
    E, M = 4, 10
    args = (torch.zeros(E, M), torch.zeros(E), torch.zeros(E, M), torch.zeros(E, M), torch.zeros(E, dtype=torch.int64), torch.zeros(E))
    with pytest.raises(RuntimeError, match="HIP device"):
        bpp_amd.a2c_loss(*args)
    assert bpp_amd.a2c_loss is bpp_amd.update.a2c_loss and hasattr(bpp_amd.RolloutStorage, "a2c_loss")


@pytest.mark.skipif(not ref_shims.available(), reason="reference tree not present")
def test_terms_equal_those_of_the_live_reference_update(emu, emu_lib):
    """The reference's Policy, a filled CPU storage and ACKTR(acktr=False).update() with the optimiser step switched off: its
    five numbers against the emulated kernel on the logits, values and predicted mask of the same network."""
    import bpp_amd
    ref_shims.install()
    from acktr import algo
    from acktr.model import Policy
    size, N, T, M = (10, 10, 10), 6, 5, 100
    args = types.SimpleNamespace(channel=4, container_size=size, pallet_size=10, enable_rotation=False, num_processes=N, num_steps=T)
    torch.manual_seed(0)
    policy = Policy((400,), bpp_amd.Discrete(M), base_kwargs={"recurrent": False, "hidden_size": 256, "args": args})
    agent = algo.ACKTR(policy, 0.5, 0.01, 2.0, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5, acktr=False, args=args)
    agent.optimizer.step = lambda *a, **k: None
    st = bpp_amd.RolloutStorage(T, N, (400,), bpp_amd.Discrete(M), policy.recurrent_hidden_state_size)
    env = emu.EmuEnv(bpp_amd.sequences.cut2_pool(size, 8, seed=0), size, False, N)
    obs, mask = env.reset()
    st.obs[0].copy_(torch.from_numpy(obs))
    st.location_masks[0].copy_(torch.from_numpy(mask))
    for t in range(T):
        with torch.no_grad():
            value, action, logp, rnn = policy.act(st.obs[t], st.recurrent_hidden_states[t], st.masks[t], st.location_masks[t])
        if t == 2:
            action[0] = int(np.argmin(st.location_masks[t][0].numpy()))      # one infeasible action
        o = env.step(action.numpy()[:, 0])
        done = torch.from_numpy(o["done"]).float().unsqueeze(1)
        st.insert(torch.from_numpy(o["obs"]), rnn, action, logp, value, torch.from_numpy(o["reward"]).unsqueeze(1), 1.0 - done,
                  torch.ones(N, 1), torch.from_numpy(o["mask"]))
    with torch.no_grad():
        next_value = policy.get_value(st.obs[-1], st.recurrent_hidden_states[-1], st.masks[-1])
    st.compute_returns(next_value, False, 1.0, 0.95, False)
    want = agent.update(st)
    with torch.no_grad():
        value, features, _, graph = policy.base(st.obs[:-1].view(T * N, -1), None, None)
        logits = policy.dist.linear(features)
    c = dict(x=logits.numpy().copy(), m=st.location_masks[:-1].reshape(T * N, M).numpy().copy(), a=st.actions.reshape(-1).numpy().copy(),
             pm=graph.reshape(T * N, M).numpy().copy(), ret=st.returns[:-1].reshape(-1).numpy().copy(), val=value.reshape(-1).numpy().copy(),
             E=T * N, M=M)
    out = ac.run_host(emu_lib, c, (0.5, 0.01, 2.0, 5.0))
    assert out["rc"] == 0
    got = out["terms"]
    print("reference update:", want, "kernel:", got.tolist())
    np.testing.assert_allclose(got[0], want[0], rtol=1e-5)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-5)
    np.testing.assert_allclose(got[2], want[2], rtol=0, atol=2e-5)          # tests/test_masked_evaluate.py:102-103
    np.testing.assert_allclose(got[3], want[3], rtol=0, atol=1e-7)
    np.testing.assert_allclose(got[4], want[4], rtol=1e-5)
