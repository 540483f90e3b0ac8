"""Native PPO on the device (include/bpp_ppo.h): the checks of tests/test_ppo.py against the device's own
bpp_masked_evaluate kernels and float64 torch on the CPU, the advantages and the gather bit for bit (second stream and replayed
graph included), the generator on a device storage, PPO.update against the recording of the reference's, and the example.
Reads nothing of the reference."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_cases as pc  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_gpu_a2c_loss import dev, dev_backward, dev_evaluate  # noqa: E402
from test_ppo import Stub, golden_agent, golden_storage  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("terms", "rows", "grad_logits", "grad_values", "grad_pred_mask")


def run_device(c, clip=0.2, coefs=pc.COEFS, clipped_value=True, pred=True, idx="given"):
    import bpp_amd
    res = bpp_amd.ppo_loss(dev(c["x"]), dev(c["val"]).view(-1, 1), dev(c["pm"]) if pred else None, dev(c["m"]), dev(c["a"]).view(-1, 1),
                           dev(c["vp"]), dev(c["ret"]), dev(c["old"]), dev(c["adv"]), dev(c["idx"]) if idx == "given" else None, clip, *coefs,
                           use_clipped_value_loss=clipped_value, rows=True)
    out = {k: getattr(res, k) for k in KEYS if pred or k != "grad_pred_mask"}
    out = {k: v.cpu().numpy() for k, v in out.items()}
    if not pred:
        out["grad_pred_mask"] = np.full((c["B"], c["M"]), pc.CANARY)
    return out


def lib_info(B, M):
    from bpp_amd import _lib
    return pc.info(_lib.lib(), B, M)


@pytest.mark.parametrize("B,M", [(1, 100), (3, 100), (4, 200), (5, 37), (70, 100), (9, 600)])
def test_gpu_ppo_loss_pieces_terms_and_float64(B, M):
    c = pc.make_case(B, M, E=B + 5, seed=100 * B + M)
    out = run_device(c, coefs=pc.ALL_COEFS)
    err = pc.check_pieces(out, c, dev_evaluate, dev_backward, coefs=pc.ALL_COEFS)
    print("ratio: max relative error against float64 exp (device) = %.3g" % err)
    pc.check_terms(out, c, lib_info(B, M), pc.ALL_COEFS)
    pc.check_against_float64(out, c, dev_evaluate, coefs=pc.ALL_COEFS)
    again = run_device(c, coefs=pc.ALL_COEFS)
    dense = run_device(pc.gathered(c), coefs=pc.ALL_COEFS)
    null = run_device(pc.gathered(c), coefs=pc.ALL_COEFS, idx="null")
    for k in KEYS:
        for other in (again, dense, null):
            assert np.array_equal(pc.bits(other[k]), pc.bits(out[k])), k


# ------------------------------------------------------------------------ the sizes that select a form, and off-contract rows
@pytest.mark.parametrize("M", pc.PPO_MS)
@pytest.mark.parametrize("B", pc.PPO_BS)
def test_gpu_ppo_loss_at_every_form_and_on_both_sides_of_every_edge(B, M):
    c = pc.edge_case(B, M)
    out = run_device(c, coefs=pc.ALL_COEFS)
    err = pc.check_edge(out, c, lib_info(B, M), dev_evaluate, dev_backward)
    print("ratio: max relative error against float64 exp (device) = %.3g" % err)
    again = run_device(c, coefs=pc.ALL_COEFS)
    dense = run_device(pc.gathered(c), coefs=pc.ALL_COEFS)
    null = run_device(pc.gathered(c), coefs=pc.ALL_COEFS, idx="null")
    for k in KEYS:
        for other in (again, dense, null):
            assert np.array_equal(pc.bits(other[k]), pc.bits(out[k])), k


@pytest.mark.parametrize("M", pc.ACTION_MS)
def test_gpu_ppo_loss_actions_outside_the_row_are_no_entry_of_it(M):
    """The device's expf and logf are not libm's: the evaluate and backward kernels are the comparator here, the statement that reads
    nothing of a kernel runs on the emulator (tests/test_ppo.py)."""
    pc.check_bad_actions(M, lambda c: run_device(c, coefs=pc.ALL_COEFS), lib_info(9, M), dev_evaluate, dev_backward)


@pytest.mark.parametrize("B,M", pc.SCALAR_SHAPES)
def test_gpu_ppo_loss_off_contract_scalars_stay_in_their_row_and_clips_outside_the_usual_range(B, M):
    pc.check_off_contract_scalars(B, M, lambda c, clip: run_device(c, clip=clip, coefs=pc.ALL_COEFS), lib_info(B, M), dev_evaluate, dev_backward)


@pytest.mark.parametrize("clipped_value,pred", [(True, False), (False, True), (False, False)])
def test_gpu_ppo_loss_other_value_loss_and_no_pred_mask(clipped_value, pred):
    for B, M in ((5, 37), (9, 600)):
        c = pc.make_case(B, M, E=B + 2, seed=B + M)
        out = run_device(c, coefs=pc.ALL_COEFS, clipped_value=clipped_value, pred=pred)
        pc.check_pieces(out, c, dev_evaluate, dev_backward, coefs=pc.ALL_COEFS, clipped_value=clipped_value, pred=pred)
        pc.check_terms(out, c, lib_info(B, M), pc.ALL_COEFS)
        pc.check_against_float64(out, c, dev_evaluate, coefs=pc.ALL_COEFS, clipped_value=clipped_value, pred=pred)


@pytest.mark.parametrize("which", range(4))
def test_gpu_ppo_loss_every_coefficient_alone(which):
    coefs = tuple(v if j == which else 0.0 for j, v in enumerate((0.25, 0.125, 7.5, 3.0)))
    c = pc.make_case(7, 91, E=10, seed=which)
    out = run_device(c, coefs=coefs)
    pc.check_pieces(out, c, dev_evaluate, dev_backward, coefs=coefs)
    pc.check_terms(out, c, lib_info(7, 91), coefs)
    pc.check_against_float64(out, c, dev_evaluate, coefs=coefs)


def test_gpu_ppo_loss_one_row_more_than_a_workgroup_and_several_row_groups():
    for B in (lib_info(3, 37)[0] + 1, 4 * 1024 + 1):
        c = pc.make_case(B, 37, E=B, seed=9)
        out = run_device(c)
        assert lib_info(B, 37)[1] > 1
        err = pc.check_pieces(out, c, dev_evaluate, dev_backward)
        print("ratio: max relative error against float64 exp (device) = %.3g" % err)
        pc.check_terms(out, c, lib_info(B, 37))


def test_gpu_ppo_loss_an_index_out_of_range_gives_nan_there_only():
    for B, M in ((5, 37), (9, 600)):
        c = pc.make_case(B, M, E=B + 5, seed=100 * B + M)
        good = run_device(c, coefs=pc.ALL_COEFS)
        bad = dict(c, idx=c["idx"].copy())
        bad["idx"][1], bad["idx"][3] = c["E"], -1
        out = run_device(bad, coefs=pc.ALL_COEFS)
        rest = [b for b in range(B) if b not in (1, 3)]
        for k in KEYS[1:]:
            assert np.isnan(out[k][[1, 3]]).all() and np.array_equal(pc.bits(out[k][rest]), pc.bits(good[k][rest])), k
        assert np.isnan(out["terms"]).all()


def test_gpu_ppo_loss_far_policy_at_a_narrow_clip():
    B, M, clip = 70, 100, 0.05
    c = pc.make_case(B, M, E=80, seed=21, spread=3.0)
    ref = pc.reference64(c, clip)
    outside = (ref["ratio"] < 1 - clip) | (ref["ratio"] > 1 + clip)
    assert outside.mean() > 0.5
    out = run_device(c, clip=clip)
    err = pc.check_pieces(out, c, dev_evaluate, dev_backward, clip=clip)
    print("ratio: max relative error against float64 exp (device) = %.3g" % err)
    pc.check_terms(out, c, lib_info(B, M))
    _, ex = pc.check_against_float64(out, c, dev_evaluate, clip=clip)
    assert np.array_equal(out["rows"][~ex, 6] != 0, outside[~ex])


@pytest.mark.parametrize("clip", [0.2, 0.0])
def test_gpu_ppo_loss_tie_rules(clip):
    c = pc.make_case(6, 37, E=6, seed=77)
    c["idx"] = np.arange(6, dtype=np.int64)
    c["old"] = dev_evaluate(c["x"], c["m"], c["a"])[0].copy()
    coefs = (0.0, 0.0, 0.0, 0.0)
    out = run_device(c, clip=clip, coefs=coefs)
    assert np.all(out["rows"][:, 5] == 1.0) and not out["rows"][:, 6].any()
    s = pc.statement(c, out["rows"][:, 5].copy(), clip, coefs, True)
    assert np.array_equal(s["g_ratio"], c["adv"])                            # torch's rule: tests/test_ppo.py asserts it from autograd
    pc.check_pieces(out, c, dev_evaluate, dev_backward, clip=clip, coefs=coefs)


def test_gpu_ppo_loss_backward_reaches_a_network_and_a_captured_graph_equals_eager():
    import bpp_amd
    B, M = 70, 100
    cases = [pc.make_case(B, M, E=80, seed=s) for s in (31, 32)]
    keys = ("x", "val", "pm", "m", "a", "vp", "ret", "old", "adv", "idx")
    static = {k: dev(cases[0][k]) for k in keys}

    def call(t):
        return bpp_amd.ppo_loss(t["x"], t["val"], t["pm"], t["m"], t["a"], t["vp"], t["ret"], t["old"], t["adv"], t["idx"], 0.2, *pc.ALL_COEFS, rows=True)

    x = static["x"].clone().requires_grad_(True)
    res = call(dict(static, x=x))
    res.backward()
    assert torch.equal(x.grad, res.grad_logits)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = {k: getattr(call(static), k).clone() for k in KEYS}
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                     # one stream, no parallel branches
        res = call(static)
    for i, c in enumerate(cases):
        for k in keys:
            static[k].copy_(dev(c[k]))
        graph.replay()
        torch.cuda.synchronize()
        got = {k: getattr(res, k).clone() for k in KEYS}
        eager = call({k: dev(c[k]) for k in keys})
        for k, v in got.items():
            assert torch.equal(v.view(torch.int32), getattr(eager, k).view(torch.int32)), k
            if i == 0:
                assert torch.equal(v.view(torch.int32), on_side[k].view(torch.int32)), k


# ---------------------------------------------------------------------------------------------------------------- advantages
def test_gpu_advantages_bit_for_bit_on_two_streams_and_in_a_replayed_graph():
    import bpp_amd
    from bpp_amd import _lib
    import ctypes
    for E in (2, 3, 320, 257, 256 * 1024 + 1):
        out = (ctypes.c_int32 * 3)()
        assert _lib.lib().bpp_ppo_advantages_info(E, out) == 0
        C, G, W = list(out)
        ret, vp = pc.advantages_case(E)
        r, v = dev(ret), dev(vp)
        adv, stats = bpp_amd.normalized_advantages(r, v)
        pc.check_advantages(adv.cpu().numpy(), stats.cpu().numpy(), ret, vp, C, W)
        adv2, stats2 = bpp_amd.normalized_advantages(r, v)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            adv3, stats3 = bpp_amd.normalized_advantages(r, v)
        torch.cuda.current_stream().wait_stream(side)
        for a, s in ((adv2, stats2), (adv3, stats3)):
            assert torch.equal(a.view(torch.int32), adv.view(torch.int32)) and torch.equal(s, stats)
    with pytest.raises(RuntimeError, match="E must be >= 2"):
        bpp_amd.normalized_advantages(dev(ret[:1]), dev(vp[:1]))
    E = 320
    ret, vp = pc.advantages_case(E)
    r, v = dev(ret), dev(vp)
    want = bpp_amd.normalized_advantages(r, v)[0].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got, _ = bpp_amd.normalized_advantages(r, v)
    for _ in range(2):
        got.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def adv_info(E):
    import ctypes
    from bpp_amd import _lib
    out = (ctypes.c_int32 * 3)()
    assert _lib.lib().bpp_ppo_advantages_info(E, out) == 0
    return list(out)


@pytest.mark.parametrize("E", pc.ADV_EDGES)
def test_gpu_advantages_at_the_block_shape_change(E):
    import bpp_amd
    C, G, W = adv_info(E)
    assert [C, G, W] == pc.adv_shape_rule(E)
    ret, vp = pc.advantages_case(E)
    adv, stats = bpp_amd.normalized_advantages(dev(ret), dev(vp))
    pc.check_advantages(adv.cpu().numpy(), stats.cpu().numpy(), ret, vp, C, W)


@pytest.mark.parametrize("E", [320, 256 * 1024])
def test_gpu_advantages_of_equal_raw_values_are_zero_and_a_large_offset_keeps_the_float64_bound(E):
    import bpp_amd
    C, G, W = adv_info(E)
    ret, vp = pc.advantages_constant(E)
    adv, stats = bpp_amd.normalized_advantages(dev(ret), dev(vp))
    pc.check_advantages_constant(adv.cpu().numpy(), stats.cpu().numpy())
    ret, vp = pc.advantages_offset(E)
    adv, stats = bpp_amd.normalized_advantages(dev(ret), dev(vp))
    pc.check_advantages(adv.cpu().numpy(), stats.cpu().numpy(), ret, vp, C, W)


# -------------------------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("n", pc.GATHER_LENS)
def test_gpu_gather_rows_at_the_part_boundary(n):
    """Dense rows and a padded stride, every window of ppo_cases.GATHER_SEQ as the indices, guards on both sides of dst.  (On the
    emulator the source and the indices end at an inaccessible page: tests/test_ppo.py.)"""
    import bpp_amd
    for pad in (0, 1000):
        src, stride = pc.gather_edge_case(n, pad)
        view = dev(src)[:, :n]
        assert view.stride(0) == stride
        for B in pc.GATHER_BS:
            for idx in pc.gather_index_vectors(B):
                wd = dev(pc.guarded((B, n))[0])
                bpp_amd.gather_rows(view, dev(idx), out=wd[pc.GUARD:pc.GUARD + B * n].view(B, n))
                back = wd.cpu().numpy()
                assert pc.guards_intact(back), (pad, B, idx)
                assert pc.same_or_nan(back[pc.GUARD:-pc.GUARD].reshape(B, n), pc.gather_expected(src, idx, n)), (pad, B, idx)


@pytest.mark.parametrize("n", [1, 3, 400, 1600])
@pytest.mark.parametrize("B", [1, 65])
def test_gpu_gather_rows_bit_for_bit_with_guards(B, n):
    import bpp_amd
    src, stride, idx = pc.gather_case(B, n)
    whole, _ = pc.guarded((B, n))
    wd = dev(whole)
    out = wd[pc.GUARD:pc.GUARD + B * n].view(B, n)
    sd = dev(src)
    got = bpp_amd.gather_rows(sd[:, :n], dev(idx), out=out)
    assert got.data_ptr() == out.data_ptr()
    back = wd.cpu().numpy()
    assert pc.guards_intact(back) and np.array_equal(pc.bits(back[pc.GUARD:-pc.GUARD].reshape(B, n)), pc.bits(src[idx, :n]))
    if B > 4:
        idx[3], idx[4] = src.shape[0], -1
        bad = bpp_amd.gather_rows(sd[:, :n], dev(idx)).cpu().numpy()
        keep = [b for b in range(B) if b not in (3, 4)]
        assert np.isnan(bad[[3, 4]]).all() and np.array_equal(pc.bits(bad[keep]), pc.bits(src[idx[keep], :n]))


# ------------------------------------------------------------------------------------------------- generator and PPO.update
@pytest.fixture(scope="module")
def golden():
    return load_golden("ppo_update_reference")


def test_gpu_generator_fields_equal_plain_indexing_and_the_storage_hands_over_views(golden):
    st = golden_storage(golden, torch.float32)
    st.to("cuda:0")
    T, N, M, F = (int(v) for v in golden["shape"][:4])
    adv = st.normalized_advantages()
    assert adv.shape == (T, N, 1) and adv.is_cuda
    cpu = golden_storage(golden, torch.float32)
    torch.manual_seed(4)
    want = [b.indices.clone() for b in cpu.feed_forward_generator(None, 3)]
    torch.manual_seed(4)
    got = list(st.feed_forward_generator(adv, 3))
    assert len(got) == len(want) == 3
    for b, w in zip(got, want):
        i = b.indices
        assert i.is_cuda and i.dtype == torch.int64 and torch.equal(i.cpu(), w)
        flat = lambda t: t.reshape(T * N, t.shape[-1])                                  # noqa: E731
        for f, src in zip(tuple(b), (st.obs[:-1], st.recurrent_hidden_states[:-1], st.actions, st.value_preds[:-1], st.returns[:-1], st.masks[:-1],
                                     st.action_log_probs, adv)):
            assert torch.equal(f, flat(src)[i])
        assert torch.equal(b.location_masks_batch, flat(st.location_masks[:-1])[i])
    net = Stub(golden, torch.float32).cuda()
    logits, values, _ = net(got[0].obs_batch)
    res = st.ppo_loss(logits, values, None, got[0], adv, clip_param=0.1)
    assert res.inputs["location_masks"].data_ptr() == st.location_masks.data_ptr() and res.inputs["action"].data_ptr() == st.actions.data_ptr()
    assert res.inputs["returns"].data_ptr() == st.returns.data_ptr() and res.inputs["indices"].data_ptr() == got[0].indices.data_ptr()
    assert res.inputs["advantages"].data_ptr() == adv.data_ptr()
    for i, name in enumerate(("value_loss", "action_loss", "dist_entropy", "prob_loss", "graph_loss", "loss", "clip_fraction")):
        assert getattr(res, name).dim() == 0 and getattr(res, name).data_ptr() == res.terms[i].data_ptr()


def test_gpu_update_reproduces_the_recorded_update_of_the_reference(golden):
    """bpp_amd.PPO on the device through bpp_ppo_loss against the reference's float64 update.  The parameters may differ from the
    recording by the float32 update error: the same update in float32 plain torch (ppo_loss_torch on the CPU) is measured against the
    recording and the native one gets 8 times its distance."""
    seed = int(golden["shape"][7])
    st32, net32 = golden_storage(golden, torch.float32), Stub(golden, torch.float32)
    torch.manual_seed(seed)
    means32 = golden_agent(golden, net32).update(st32)
    st = golden_storage(golden, torch.float32)
    st.to("cuda:0")
    net = Stub(golden, torch.float32).cuda()
    torch.manual_seed(seed)
    means = golden_agent(golden, net).update(st)
    print("means native", means, "float32 torch", means32, "recorded", golden["means"].tolist())
    for k, v in net.state_dict().items():
        want = golden["final." + k]
        d_native = np.abs(v.cpu().double().numpy() - want).max()
        d_torch = np.abs(net32.state_dict()[k].double().numpy() - want).max()
        print("%s: max |native - recorded| = %.3g, max |float32 torch - recorded| = %.3g" % (k, d_native, d_torch))
        assert d_native <= 8 * d_torch, k
    # the three means: the same rule, plus what one float32 evaluation of a term may be off by (forward_tolerances at M = 25 for
    # the log-probability, times mean |A| ~ 1, and the entropy; 4 EPS of the value loss)
    tol = pc.forward_tolerances(int(golden["shape"][2]))
    for j, atol in enumerate((4 * pc.EPS * abs(golden["means"][0]), tol[0], tol[1])):
        assert abs(means[j] - golden["means"][j]) <= 8 * abs(means32[j] - golden["means"][j]) + atol, j


def test_gpu_update_at_m_400_with_every_coefficient_a_pred_mask_and_two_mini_batch_shapes():
    """Two PPO.update calls on a synthetic rollout (ppo_cases.UPDATE: M = 400, T N = 38 rows, every coefficient non-zero, a network
    that returns a pred_mask; 4 and then 3 mini-batches, so two (B, M) entries of the buffer cache).  The reference is the same
    update in float64 on the CPU through ppo_loss_torch; the margin is the rule of the recorded update above: the float32 CPU twin's
    distance from the float64 run is measured, the native update gets 8 times it."""
    from bpp_amd import ppo
    want_means, want = pc.run_update(torch.float64, "cpu")
    means32, twin = pc.run_update(torch.float32, "cpu")
    means, got = pc.run_update(torch.float32, "cuda:0")
    M = pc.UPDATE["M"]
    shapes = {(k[1], k[2]) for k in ppo._CACHE if k[2] == M}
    assert {(38 // mini, M) for mini in pc.UPDATE["mini"]} <= shapes, shapes
    print("means native", means, "float32 torch", means32, "float64 torch", want_means)
    init = pc.update_data()["init"]
    for k in want:
        d_native, d_torch = np.abs(got[k] - want[k]).max(), np.abs(twin[k] - want[k]).max()
        print("%s: max |native - float64| = %.3g, max |float32 torch - float64| = %.3g" % (k, d_native, d_torch))
        assert d_native <= 8 * d_torch, k
        assert np.abs(want[k] - init[k].numpy()).max() > 1e-3, k           # it did move
    tol = pc.forward_tolerances(M)
    for j in range(6):
        atol = (4 * pc.EPS * abs(want_means[j]), tol[0], tol[1])[j % 3]
        assert abs(means[j] - want_means[j]) <= 8 * abs(means32[j] - want_means[j]) + atol, j


def test_gpu_example_trains_with_ppo():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_ppo as ex
    for native_trunk in (False, True):
        hist = ex.train(envs=64, updates=2, native_trunk=native_trunk, verbose=False)
        assert len(hist) == 2 and all(len(h) == 3 and np.isfinite(h).all() for h in hist), hist
