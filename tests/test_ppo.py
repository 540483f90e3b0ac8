"""Native PPO (include/bpp_ppo.h) without a GPU: the product kernels of csrc/bpp_ppo.inl compiled by g++ against the
SIMT emulator, and the host logic of bpp_amd.ppo / RolloutStorage on CPU tensors.  The loss against the emulated
bpp_masked_evaluate kernels and the header's numpy statement bit for bit, against float64 autograd of the reference's
expressions, torch's tie rules, the advantages and the gather bit for bit, the mini-batch generator against torch's samplers
and the live reference's, and PPO.update against the recording of the reference's own (tests/golden/make_ppo_golden.py).
Every entry point also at the sizes that select its form (ppo_cases.PPO_MS, GATHER_LENS, ADV_EDGES), the loss row against a
statement that reads nothing of a kernel, and rows with actions and scalars outside the contract.
Helpers and tolerances: tests/ppo_cases.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from bpp_amd import _lib
from oracle import ref_shims

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heuristic_cases as hc  # noqa: E402
import ppo_cases as pc  # noqa: E402
from conftest import load_golden  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -1
needs_reference = pytest.mark.skipif(not ref_shims.available(), reason="reference tree not present")
SHAPES = [(1, 100), (3, 100), (4, 200), (5, 37), (70, 100), (9, 600)]


@pytest.fixture(scope="module")
def emu_lib(emu):
    return pc.bind(ctypes.CDLL(emu.LIB))


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def results(emu_lib):
    """(case, output with every coefficient set, clipped value loss, pred_mask given) per shape, computed once, never modified."""
    cache = {}

    def get(B, M):
        if (B, M) not in cache:
            c = pc.make_case(B, M, E=B + 5, seed=100 * B + M)
            out = pc.run_host(emu_lib, c, coefs=pc.ALL_COEFS)
            assert out["rc"] == 0 and out["guards"]
            cache[(B, M)] = (c, out)
        return cache[(B, M)]
    return get


# ---------------------------------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("B,M", SHAPES)
def test_loss_pieces_bit_for_bit_terms_in_the_stated_order_and_float64(emu, emu_lib, results, B, M):
    c, out = results(B, M)
    shape = pc.info(emu_lib, B, M)
    assert shape[2] == int(M <= 512)
    err = pc.check_pieces(out, c, emu.masked_evaluate, emu.masked_evaluate_backward, coefs=pc.ALL_COEFS)
    print("ratio: max relative error against float64 exp (emulator) = %.3g" % err)
    pc.check_terms(out, c, shape, pc.ALL_COEFS)
    pc.check_against_float64(out, c, emu.masked_evaluate, coefs=pc.ALL_COEFS)


def test_loss_at_one_row_more_than_a_workgroup_holds(emu, emu_lib):
    B = pc.info(emu_lib, 3, 37)[0] + 1
    c = pc.make_case(B, 37, E=B, seed=9)
    out = pc.run_host(emu_lib, c)
    assert out["rc"] == 0 and out["guards"] and pc.info(emu_lib, B, 37)[1] == 2
    pc.check_pieces(out, c, emu.masked_evaluate, emu.masked_evaluate_backward)
    pc.check_terms(out, c, pc.info(emu_lib, B, 37))


# ------------------------------------------------------------------------ the sizes that select a form, and off-contract rows
@pytest.mark.parametrize("M", pc.PPO_MS)
@pytest.mark.parametrize("B", pc.PPO_BS)
def test_loss_at_every_form_and_on_both_sides_of_every_edge(emu, emu_lib, results, B, M):
    c, out = results(B, M)
    assert c["E"] == B + 5
    err = pc.check_edge(out, c, pc.info(emu_lib, B, M), emu.masked_evaluate, emu.masked_evaluate_backward)
    print("ratio: max relative error against float64 exp (emulator) = %.3g" % err)
    dense = pc.run_host(emu_lib, pc.gathered(c), coefs=pc.ALL_COEFS)
    null = pc.run_host(emu_lib, pc.gathered(c), coefs=pc.ALL_COEFS, idx="null")
    for k in ("terms",) + pc.OUT_KEYS:
        assert np.array_equal(pc.bits(dense[k]), pc.bits(out[k])) and np.array_equal(pc.bits(null[k]), pc.bits(out[k])), k
    assert pc.ok(dense) and pc.ok(null)


@pytest.mark.parametrize("M", pc.PPO_MS)
def test_the_whole_row_against_a_statement_that_reads_nothing_of_a_kernel(emu_lib, results, M):
    """The emulator's expf and logf are libm's, as tests/head_normative.py's are: logp, the ratio and everything behind it bit for bit."""
    c, out = results(5, M)
    pc.check_normative(out, c, coefs=pc.ALL_COEFS)


@pytest.mark.parametrize("M", pc.ACTION_MS)
def test_actions_outside_the_row_are_no_entry_of_it(emu, emu_lib, M):
    pc.check_bad_actions(M, lambda c: pc.run_host(emu_lib, c, coefs=pc.ALL_COEFS), pc.info(emu_lib, 9, M), emu.masked_evaluate,
                         emu.masked_evaluate_backward, normative=True)


@pytest.mark.parametrize("B,M", pc.SCALAR_SHAPES)
def test_off_contract_scalars_stay_in_their_row_and_clips_outside_the_usual_range(emu, emu_lib, B, M):
    pc.check_off_contract_scalars(B, M, lambda c, clip: pc.run_host(emu_lib, c, clip=clip, coefs=pc.ALL_COEFS), pc.info(emu_lib, B, M),
                                  emu.masked_evaluate, emu.masked_evaluate_backward)


@pytest.mark.parametrize("B,M", [(5, 37), (9, 600)])
def test_null_idx_is_the_identity_and_a_permuted_idx_equals_the_dense_call(emu_lib, results, B, M):
    c, out = results(B, M)
    dense = pc.run_host(emu_lib, pc.gathered(c), coefs=pc.ALL_COEFS)
    null = pc.run_host(emu_lib, pc.gathered(c), coefs=pc.ALL_COEFS, idx="null")
    for k in ("terms", "rows", "grad_logits", "grad_values", "grad_pred_mask"):
        assert np.array_equal(pc.bits(dense[k]), pc.bits(out[k])), k
        assert np.array_equal(pc.bits(null[k]), pc.bits(out[k])), k
    assert dense["guards"] and null["guards"]


@pytest.mark.parametrize("clipped_value", [True, False])
@pytest.mark.parametrize("pred", [True, False])
def test_both_value_losses_with_and_without_pred_mask(emu, emu_lib, clipped_value, pred):
    for B, M in ((5, 37), (9, 600)):
        c = pc.make_case(B, M, E=B + 2, seed=B + M)
        out = pc.run_host(emu_lib, c, coefs=pc.ALL_COEFS, clipped_value=clipped_value, pred=pred)
        assert out["rc"] == 0 and out["guards"]
        pc.check_pieces(out, c, emu.masked_evaluate, emu.masked_evaluate_backward, coefs=pc.ALL_COEFS, clipped_value=clipped_value, pred=pred)
        pc.check_terms(out, c, pc.info(emu_lib, B, M), pc.ALL_COEFS)
        pc.check_against_float64(out, c, emu.masked_evaluate, coefs=pc.ALL_COEFS, clipped_value=clipped_value, pred=pred)
        bare = pc.run_host(emu_lib, c, coefs=pc.ALL_COEFS, clipped_value=clipped_value, pred=pred, rows=False)
        assert np.array_equal(pc.bits(bare["terms"]), pc.bits(out["terms"])) and np.all(bare["rows"] == pc.CANARY)


@pytest.mark.parametrize("which", range(4))
def test_every_coefficient_alone(emu, emu_lib, which):
    coefs = tuple(v if j == which else 0.0 for j, v in enumerate((0.25, 0.125, 7.5, 3.0)))
    c = pc.make_case(7, 91, E=10, seed=which)
    out = pc.run_host(emu_lib, c, coefs=coefs)
    assert out["rc"] == 0 and out["guards"]
    pc.check_pieces(out, c, emu.masked_evaluate, emu.masked_evaluate_backward, coefs=coefs)
    pc.check_terms(out, c, pc.info(emu_lib, 7, 91), coefs)
    pc.check_against_float64(out, c, emu.masked_evaluate, coefs=coefs)


def test_an_index_out_of_range_gives_nan_there_and_leaves_the_other_rows_untouched(emu_lib, results):
    for B, M in ((5, 37), (9, 600)):
        c, good = results(B, M)
        bad = dict(c, idx=c["idx"].copy())
        bad["idx"][1], bad["idx"][3] = c["E"], -1
        out = pc.run_host(emu_lib, bad, coefs=pc.ALL_COEFS)
        assert out["rc"] == 0 and out["guards"]
        for k in ("rows", "grad_logits", "grad_values", "grad_pred_mask"):
            assert np.isnan(out[k][[1, 3]]).all(), k
            rest = [b for b in range(B) if b not in (1, 3)]
            assert np.array_equal(pc.bits(out[k][rest]), pc.bits(good[k][rest])), k
        assert np.isnan(out["terms"]).all()


def test_a_far_policy_at_a_narrow_clip_puts_most_rows_outside_the_interval(emu, emu_lib):
    B, M, clip = 70, 100, 0.05
    c = pc.make_case(B, M, E=80, seed=21, spread=3.0)
    ref = pc.reference64(c, clip)
    outside = (ref["ratio"] < 1 - clip) | (ref["ratio"] > 1 + clip)
    assert outside.mean() > 0.5                                            # from float64 alone
    out = pc.run_host(emu_lib, c, clip=clip)
    assert out["rc"] == 0 and out["guards"]
    pc.check_pieces(out, c, emu.masked_evaluate, emu.masked_evaluate_backward, clip=clip)
    pc.check_terms(out, c, pc.info(emu_lib, B, M))
    _, ex = pc.check_against_float64(out, c, emu.masked_evaluate, clip=clip)
    assert np.array_equal(out["rows"][~ex, 6] != 0, outside[~ex]) and abs(out["terms"][6] - outside.mean()) <= (ex.sum() + 0.5) / B
    s = pc.statement(c, out["rows"][:, 5].copy(), clip, pc.COEFS, True)
    assert (s["g_ratio"] == 0).mean() > 0.2 and (s["g_ratio"] != 0).mean() > 0.2          # both sides of the clipped gradient


def tie_case(B=6, M=37):
    c = pc.make_case(B, M, E=B, seed=77)
    c["idx"] = np.arange(B, dtype=np.int64)
    return c


@pytest.mark.parametrize("clip", [0.2, 0.0])
def test_tie_rules_are_those_of_float64_torch_autograd(emu, emu_lib, clip):
    """old = the kernel's own logp: ratio is exactly 1; at clip = 0.2 inside the interval, at clip = 0 on both bounds.  g_ratio must
    be A either way -- what torch gives in float64 for the same expression with the ratio a leaf equal to 1."""
    c = tie_case()
    c["old"] = emu.masked_evaluate(c["x"], c["m"], c["a"])[0].copy()
    coefs = (0.0, 0.0, 0.0, 0.0)                                            # the action term alone
    out = pc.run_host(emu_lib, c, clip=clip, coefs=coefs)
    assert out["rc"] == 0 and np.all(out["rows"][:, 5] == 1.0) and not out["rows"][:, 6].any()
    ratio = torch.ones(c["B"], dtype=torch.float64, requires_grad=True)
    A = torch.from_numpy(c["adv"]).double()
    (-torch.min(ratio * A, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * A)).sum().backward()
    assert torch.equal(-ratio.grad, A)                                      # torch: d(-min) / d ratio = -A, i.e. g_ratio = A
    s = pc.statement(c, out["rows"][:, 5].copy(), clip, coefs, True)
    assert np.array_equal(s["g_ratio"], c["adv"])
    pc.check_pieces(out, c, emu.masked_evaluate, emu.masked_evaluate_backward, clip=clip, coefs=coefs)   # grad_logits under g_logp = -A cB


def test_value_tie_takes_half_of_each_branch_as_torch_does(emu_lib):
    """v = vp: both value branches are the same number; torch's max hands half of the gradient to each, and the clamp passes."""
    c = tie_case()
    c["val"] = c["vp"].copy()
    out = pc.run_host(emu_lib, c, coefs=(1.0, 0.0, 0.0, 0.0))
    v = torch.from_numpy(c["val"]).double().requires_grad_(True)
    vp, R = torch.from_numpy(c["vp"]).double(), torch.from_numpy(c["ret"]).double()
    (0.5 * torch.max((v - R).pow(2), (vp + (v - vp).clamp(-0.2, 0.2) - R).pow(2))).mean().backward()
    np.testing.assert_allclose(out["grad_values"], v.grad.numpy(), rtol=4 * pc.EPS, atol=0)
    # and outside the clip interval with the clipped branch the larger: no gradient
    c["val"] = (c["vp"] + np.where(c["ret"] > c["vp"], -1.0, 1.0)).astype(np.float32)
    out = pc.run_host(emu_lib, c, coefs=(1.0, 0.0, 0.0, 0.0))
    d, e = c["val"] - c["ret"], (c["vp"] + np.clip(c["val"] - c["vp"], -0.2, 0.2)).astype(np.float32) - c["ret"]
    assert np.all(d * d > e * e) and np.array_equal(pc.bits(out["grad_values"]), pc.bits(pc.F32(1.0 / c["B"]) * d))


def test_invalid_arguments_are_refused_before_any_device_is_touched(lib, emu_lib):
    B, E, M = 3, 5, 8
    c = pc.make_case(B, M, E, seed=1)
    bufs = dict(logits=c["x"], values=c["val"], pred_mask=c["pm"], idx=c["idx"], location_masks=c["m"], action=c["a"], value_preds=c["vp"],
                returns=c["ret"], old_log_probs=c["old"], adv=c["adv"], grad_logits=np.zeros((B, M), np.float32),
                grad_values=np.zeros(B, np.float32), grad_pred_mask=np.zeros((B, M), np.float32), rows=np.zeros((B, 7), np.float32),
                terms=np.zeros(7, np.float32), workspace=np.zeros(64, np.float64))
    ins = ("logits", "values", "pred_mask", "idx", "location_masks", "action", "value_preds", "returns", "old_log_probs", "adv")
    outs = ("grad_logits", "grad_values", "grad_pred_mask", "rows", "terms", "workspace")

    def call(L, **kw):
        a = {k: v.ctypes.data for k, v in bufs.items()}
        a.update(B=B, E=E, M=M, clip=0.2)
        a.update(kw)
        return L.bpp_ppo_loss(*[a[k] for k in ins], a["clip"], 0.5, 0.01, 0.0, 0.0, 1, *[a[k] for k in outs], a["B"], a["E"], a["M"], None)

    assert call(emu_lib) == 0 and call(emu_lib, pred_mask=None, grad_pred_mask=None, rows=None, idx=None) == 0
    out3, out4 = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 4)()
    one = np.zeros(4, np.float32)
    for L in (lib, emu_lib):            # the product library has no device here: it must refuse before it looks for one
        for bad in [dict(B=0), dict(B=-2), dict(E=0), dict(M=0), dict(clip=-0.1), dict(clip=float("nan")), dict(grad_pred_mask=None),
                    dict(idx=None, B=E + 1)] + \
                [{k: None} for k in ins if k not in ("pred_mask", "idx")] + [{k: None} for k in ("grad_logits", "grad_values", "terms", "workspace")]:
            assert call(L, **bad) == BADARG, bad
            assert L.bpp_last_error()
        for b, m in ((0, 5), (5, 0), (-1, 5)):
            assert L.bpp_ppo_loss_info(b, m, out4) == BADARG and L.bpp_ppo_loss_workspace(b, m) == 0
        assert L.bpp_ppo_loss_info(5, 5, None) == BADARG
        p = one.ctypes.data
        for e in (1, 0, -4):
            assert L.bpp_ppo_advantages(p, p, p, p, e, p, None) == BADARG
            assert L.bpp_ppo_advantages_info(e, out3) == BADARG and L.bpp_ppo_advantages_workspace(e) == 0
        assert L.bpp_ppo_advantages(None, p, p, p, 4, p, None) == BADARG and L.bpp_ppo_advantages_info(4, None) == BADARG
        idx = np.zeros(2, np.int64).ctypes.data
        for args in ((None, 2, 2, idx, 2, 2, p), (p, 2, 2, None, 2, 2, p), (p, 2, 2, idx, 2, 2, None), (p, 2, 2, idx, 0, 2, p),
                     (p, 2, 2, idx, 2, 0, p), (p, 2, 0, idx, 2, 2, p), (p, 1, 2, idx, 2, 2, p)):
            assert L.bpp_gather_rows(*args, None) == BADARG, args


def test_every_declared_symbol_is_exported_and_the_abi_version_stays(lib):
    src = re.sub(r"/\*.*?\*/", "", open(_lib.PPO_HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(bpp_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.PPO_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.bpp_abi_version() == 16 and _lib.ABI_VERSION == 16


# ---------------------------------------------------------------------------------------------------------------- advantages
def adv_info(L, E):
    out = (ctypes.c_int32 * 3)()
    assert L.bpp_ppo_advantages_info(E, out) == 0
    return list(out)


def test_advantages_bit_for_bit_in_the_stated_order(lib, emu_lib):
    block = adv_info(emu_lib, 320)[0]
    assert adv_info(lib, 5 * 65536) == [512, 640, 256] and adv_info(lib, 320) == [256, 2, 256]
    for E in (2, 3, 320, block + 1):
        C, G, W = adv_info(emu_lib, E)
        assert (G - 1) * C < E <= G * C and emu_lib.bpp_ppo_advantages_workspace(E) == 2 * G * 8
        ret, vp = pc.advantages_case(E)
        runs = []
        for _ in range(2):
            whole, adv = pc.guarded((E,))
            swhole, stats = pc.guarded((2,), np.float64)
            ws = np.zeros(2 * G + 1, np.float64)
            assert emu_lib.bpp_ppo_advantages(ret.ctypes.data, vp.ctypes.data, adv.ctypes.data, stats.ctypes.data, E, ws.ctypes.data, None) == 0
            assert pc.guards_intact(whole) and pc.guards_intact(swhole)
            runs.append((adv, stats))
        pc.check_advantages(runs[0][0], runs[0][1], ret, vp, C, W)
        assert np.array_equal(pc.bits(runs[0][0]), pc.bits(runs[1][0])) and np.array_equal(runs[0][1], runs[1][1])


def emu_advantages(L, ret, vp):
    """(adv, stats) of one emulated bpp_ppo_advantages, guards checked."""
    E = ret.size
    whole, adv = pc.guarded((E,))
    swhole, stats = pc.guarded((2,), np.float64)
    ws = np.zeros(int(L.bpp_ppo_advantages_workspace(E)) // 8 + 1, np.float64)
    assert L.bpp_ppo_advantages(ret.ctypes.data, vp.ctypes.data, adv.ctypes.data, stats.ctypes.data, E, ws.ctypes.data, None) == 0
    assert pc.guards_intact(whole) and pc.guards_intact(swhole)
    return adv, stats


# every size of the device suite runs on the emulator as well (under a second each)
@pytest.mark.parametrize("E", pc.ADV_EDGES)
def test_advantages_at_the_block_shape_change(lib, emu_lib, E):
    assert adv_info(lib, E) == adv_info(emu_lib, E) == pc.adv_shape_rule(E)
    C, G, W = adv_info(emu_lib, E)
    assert (G - 1) * C < E <= G * C and G <= 1024 and emu_lib.bpp_ppo_advantages_workspace(E) == 2 * G * 8
    ret, vp = pc.advantages_case(E)
    adv, stats = emu_advantages(emu_lib, ret, vp)
    pc.check_advantages(adv, stats, ret, vp, C, W)


def test_the_shape_changes_where_1024_blocks_of_one_chunk_no_longer_hold_the_rollout(lib, emu_lib):
    for L in (lib, emu_lib):
        assert adv_info(L, 256 * 1024) == [256, 1024, 256] and adv_info(L, 256 * 1024 + 1) == [512, 513, 256]
        assert adv_info(L, 256) == [256, 1, 256] and adv_info(L, 257) == [256, 2, 256] and adv_info(L, 2 * 256 * 1024 + 1) == [768, 683, 256]


@pytest.mark.parametrize("E", [320, 256 * 1024])
def test_advantages_of_equal_raw_values_are_zero_and_a_large_offset_keeps_the_float64_bound(emu_lib, E):
    C, G, W = adv_info(emu_lib, E)
    ret, vp = pc.advantages_constant(E)
    assert np.all(ret - vp == np.float32(0.75))
    adv, stats = emu_advantages(emu_lib, ret, vp)
    pc.check_advantages_constant(adv, stats)
    ret, vp = pc.advantages_offset(E)
    adv, stats = emu_advantages(emu_lib, ret, vp)
    pc.check_advantages(adv, stats, ret, vp, C, W)


# -------------------------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("n", pc.GATHER_LENS)
def test_gather_rows_at_the_part_boundary_behind_an_inaccessible_page(emu_lib, n):
    """Dense rows and a padded stride, every window of ppo_cases.GATHER_SEQ as the indices.  The dense source and the indices end at
    an inaccessible page: a read past the last row, or past idx[B - 1], is a host fault."""
    for pad in (0, 1000):
        src, stride = pc.gather_edge_case(n, pad)
        held = hc.Fenced(src) if pad == 0 else None
        s = held.array if held else src
        for B in pc.GATHER_BS:
            for idx in pc.gather_index_vectors(B):
                fenced = hc.Fenced(idx, np.int64)
                whole, dst = pc.guarded((B, n))
                assert emu_lib.bpp_gather_rows(s.ctypes.data, stride, pc.GATHER_ROWS, fenced.array.ctypes.data, B, n, dst.ctypes.data, None) == 0
                assert pc.same_or_nan(dst, pc.gather_expected(src, idx, n)) and pc.guards_intact(whole), (pad, B, idx)


@pytest.mark.parametrize("n", [1, 3, 400, 1600])
@pytest.mark.parametrize("B", [1, 65])
def test_gather_rows_bit_for_bit_with_guards(emu_lib, B, n):
    src, stride, idx = pc.gather_case(B, n)
    whole, dst = pc.guarded((B, n))
    assert emu_lib.bpp_gather_rows(src.ctypes.data, stride, src.shape[0], idx.ctypes.data, B, n, dst.ctypes.data, None) == 0
    assert np.array_equal(pc.bits(dst), pc.bits(src[idx, :n])) and pc.guards_intact(whole) and not np.isnan(dst).any()
    if B > 4:
        idx[3], idx[4] = src.shape[0], -1
        whole, dst2 = pc.guarded((B, n))
        assert emu_lib.bpp_gather_rows(src.ctypes.data, stride, src.shape[0], idx.ctypes.data, B, n, dst2.ctypes.data, None) == 0
        keep = [b for b in range(B) if b not in (3, 4)]
        assert np.isnan(dst2[[3, 4]]).all() and np.array_equal(pc.bits(dst2[keep]), pc.bits(dst[keep])) and pc.guards_intact(whole)


# ------------------------------------------------------------------------------------------------- generator and PPO.update
def golden_storage(g, dtype=torch.float64):
    """A CPU bpp_amd.RolloutStorage holding the recorded rollout, its float slabs in `dtype`."""
    import bpp_amd
    T, N, M, F = (int(v) for v in g["shape"][:4])
    st = bpp_amd.RolloutStorage(T, N, (M + F,), bpp_amd.Discrete(M))
    st._slabs = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in st._slabs.items()}
    st._bind()
    for k in ("obs", "location_masks", "value_preds", "returns", "actions", "action_log_probs"):
        getattr(st, k).copy_(torch.from_numpy(g[k]))
    return st


class Stub(torch.nn.Module):
    """The network of tests/golden/make_ppo_golden.py: net(obs) -> (logits, values, None)."""

    def __init__(self, g, dtype=torch.float64):
        super().__init__()
        M, F, H = (int(v) for v in g["shape"][2:5])
        self.M = M
        self.body = torch.nn.Sequential(torch.nn.Linear(M + F, H), torch.nn.Tanh(), torch.nn.Linear(H, M + 1)).to(dtype)
        self.load_state_dict({k[5:]: torch.from_numpy(v).to(dtype) for k, v in g.items() if k.startswith("init.")})

    def forward(self, obs):
        out = self.body(obs)
        return out[:, :self.M], out[:, self.M:], None


def golden_agent(g, net):
    import bpp_amd
    clip, vc, ec, lr, eps, norm = (float(v) for v in g["hyper"])
    return bpp_amd.PPO(net, clip, int(g["shape"][5]), int(g["shape"][6]), vc, ec, lr=lr, eps=eps, max_grad_norm=norm)


@pytest.fixture(scope="module")
def golden():
    return load_golden("ppo_update_reference")


@pytest.mark.parametrize("T,N,mini", [(5, 8, 4), (5, 7, 4), (3, 5, 15), (2, 3, 1)])
def test_generator_draws_the_index_sequence_of_torch_s_own_samplers(T, N, mini):
    import bpp_amd
    from torch.utils.data.sampler import BatchSampler, SubsetRandomSampler
    st = bpp_amd.RolloutStorage(T, N, (6,), bpp_amd.Discrete(4))
    for k in ("obs", "location_masks", "recurrent_hidden_states", "value_preds", "returns", "masks"):
        getattr(st, k).copy_(torch.randn(getattr(st, k).shape))
    st.actions.copy_(torch.randint(0, 4, st.actions.shape))
    st.action_log_probs.copy_(torch.randn(T, N, 1))
    adv = torch.randn(T, N, 1)
    torch.manual_seed(5)
    want = list(BatchSampler(SubsetRandomSampler(range(T * N)), T * N // mini, drop_last=True))
    torch.manual_seed(5)
    got = list(st.feed_forward_generator(adv, mini))
    assert [b.indices.tolist() for b in got] == want and len(got) == (T * N) // (T * N // mini)
    by_size = list(st.feed_forward_generator(adv, mini_batch_size=4, generator=torch.Generator().manual_seed(9)))
    assert [b.indices.tolist() for b in by_size] == list(BatchSampler(SubsetRandomSampler(range(T * N), torch.Generator().manual_seed(9)), 4, True))
    for b in got:
        i = b.indices
        assert i.dtype == torch.int64 and len(b) == 8
        fields = tuple(b)
        want_fields = (st.obs[:-1].reshape(T * N, 6)[i], st.recurrent_hidden_states[:-1].reshape(T * N, 1)[i], st.actions.reshape(T * N, 1)[i],
                       st.value_preds[:-1].reshape(T * N, 1)[i], st.returns[:-1].reshape(T * N, 1)[i], st.masks[:-1].reshape(T * N, 1)[i],
                       st.action_log_probs.reshape(T * N, 1)[i], adv.reshape(T * N, 1)[i])
        for f, w, name in zip(fields, want_fields, b.FIELDS):
            assert torch.equal(f, w) and getattr(b, name) is f, name
        assert torch.equal(b.location_masks_batch, st.location_masks[:-1].reshape(T * N, 4)[i])
    assert tuple(next(iter(st.feed_forward_generator(None, mini))))[7] is None
    with pytest.raises(AssertionError, match="PPO requires"):
        next(iter(st.feed_forward_generator(adv, T * N + 1)))


def test_generator_replays_the_recorded_index_sequence_of_the_reference(golden):
    st = golden_storage(golden)
    T, N, _, _, _, epochs, mini, seed = (int(v) for v in golden["shape"])
    torch.manual_seed(seed)
    got = [b.indices.numpy() for _ in range(epochs) for b in st.feed_forward_generator(None, mini)]
    assert np.array_equal(np.stack(got), golden["indices"])


@needs_reference
def test_generator_yields_the_tuples_of_the_live_reference_generator(golden):
    ref_shims.install()
    from acktr.storage import RolloutStorage as RefStorage
    import bpp_amd
    T, N, M, F = (int(v) for v in golden["shape"][:4])
    ours = golden_storage(golden, torch.float32)
    ref = RefStorage(T, N, (M + F,), bpp_amd.Discrete(M), 1, False, False, 5)
    for k in ("obs", "location_masks", "value_preds", "returns", "actions", "action_log_probs"):
        getattr(ref, k).copy_(getattr(ours, k))
    adv = ours.normalized_advantages()
    for mini in (4, 3):
        torch.manual_seed(2)
        want = list(ref.feed_forward_generator(adv, mini))
        torch.manual_seed(2)
        got = list(ours.feed_forward_generator(adv, mini))
        assert len(got) == len(want)
        for b, w in zip(got, want):
            for f, wf in zip(tuple(b), w):
                assert f.dtype == wf.dtype and f.shape == wf.shape and torch.equal(f, wf)


def test_cpu_normalized_advantages_are_the_reference_s_expression(golden):
    st = golden_storage(golden)
    adv = st.returns[:-1] - st.value_preds[:-1]
    want = (adv - adv.mean()) / (adv.std() + 1e-5)
    got = st.normalized_advantages()
    assert got.shape == (5, 8, 1) and torch.equal(got, want)


def test_cpu_update_reproduces_the_recorded_update_of_the_reference(golden):
    """bpp_amd.PPO on CPU float64 tensors, through ppo_loss_torch, against the unmodified reference's PPO.update."""
    st, net = golden_storage(golden), Stub(golden)
    agent = golden_agent(golden, net)
    torch.manual_seed(int(golden["shape"][7]))
    means = agent.update(st)
    print("means", means, "recorded", golden["means"].tolist())
    np.testing.assert_allclose(means, golden["means"], rtol=0, atol=1e-10)
    for k, v in net.state_dict().items():
        np.testing.assert_allclose(v.numpy(), golden["final." + k], rtol=0, atol=1e-10, err_msg=k)
    assert max(np.abs(golden["final." + k] - golden["init." + k]).max() for k in net.state_dict()) > 1e-3      # it did move


def test_torch_twin_states_what_float64_autograd_of_the_reference_s_expressions_gives():
    import bpp_amd
    c = pc.make_case(9, 37, E=12, seed=4)
    for clipped_value, pred in ((True, True), (False, False)):
        ref = pc.reference64(c, 0.2, pc.ALL_COEFS, clipped_value, pred)
        t = {k: torch.from_numpy(v).double() if v.dtype == np.float32 else torch.from_numpy(v) for k, v in c.items() if isinstance(v, np.ndarray)}
        x, v, pm = (t[k].requires_grad_(True) for k in ("x", "val", "pm"))
        res = bpp_amd.ppo_loss_torch(x, v.view(-1, 1), pm if pred else None, t["m"], t["a"], t["vp"], t["ret"], t["old"], t["adv"], t["idx"], 0.2,
                                     *pc.ALL_COEFS, use_clipped_value_loss=clipped_value, rows=True)
        res.backward()
        np.testing.assert_allclose(res.terms[:6].numpy(), ref["terms"], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(x.grad.numpy(), ref["grad_logits"], rtol=1e-10, atol=1e-14)
        np.testing.assert_allclose(v.grad.numpy(), ref["grad_values"], rtol=1e-10, atol=1e-14)
        np.testing.assert_allclose(res.rows[:, 5].numpy(), ref["ratio"], rtol=1e-12)
        assert float(res.loss) == float(res.terms[5]) and res.clip_fraction.dim() == 0


def test_the_native_entry_points_refuse_cpu_tensors():
    import bpp_amd
    B, M = 4, 10
    z = torch.zeros
    with pytest.raises(RuntimeError, match="HIP device"):
        bpp_amd.ppo_loss(z(B, M), z(B), None, z(B, M), z(B, dtype=torch.int64), z(B), z(B), z(B), z(B))
    with pytest.raises(RuntimeError, match="HIP device"):
        bpp_amd.normalized_advantages(z(B), z(B))
    with pytest.raises(RuntimeError, match="HIP device"):
        bpp_amd.gather_rows(z(B, M), z(2, dtype=torch.int64))
    for name in ("ppo_loss", "normalized_advantages", "feed_forward_generator"):
        assert hasattr(bpp_amd.RolloutStorage, name)
