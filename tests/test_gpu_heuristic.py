"""The lowest-top heuristic on the device (include/bpp_heuristic.h): the cases of tests/test_heuristic.py through
bpp_amd.heuristic_act, a second stream and a replayed graph, closed loops of BppVecEnv.heuristic_act against the oracle env under
the oracle heuristic, and examples/evaluate_heuristic.py.  Inputs and checks: tests/heuristic_cases.py.  Reads nothing of the
reference."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heuristic_cases as hc  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def device_runner(want_top=True):
    """run(obs, mask, size, rotation, rule) through bpp_amd.heuristic_act: obs is a numpy array or a device tensor (a row view
    with unit inner stride will do); the outputs lie between guard words, which must be intact."""
    def run(obs, mask, size, rotation, rule):
        import bpp_amd
        o = obs if torch.is_tensor(obs) else dev(obs)
        n = o.shape[0]
        act = torch.full((n + 2 * hc.GUARD,), int(hc.CANARY64), dtype=torch.int64, device="cuda:0")
        top = torch.full((n + 2 * hc.GUARD,), int(hc.CANARY32), dtype=torch.int32, device="cuda:0")
        out = bpp_amd.heuristic_act(o, dev(mask), size, rotation, rule, out=act[hc.GUARD:hc.GUARD + n],
                                    top=top[hc.GUARD:hc.GUARD + n] if want_top else None)
        assert out.data_ptr() == act[hc.GUARD:].data_ptr()
        a, t = act.cpu().numpy(), top.cpu().numpy()
        for buf, canary in ((a, hc.CANARY64), (t, hc.CANARY32)):
            assert (buf[:hc.GUARD] == canary).all() and (buf[hc.GUARD + n:] == canary).all(), "guard words overwritten"
        if not want_top:
            assert (t == hc.CANARY32).all()
        return a[hc.GUARD:hc.GUARD + n], t[hc.GUARD:hc.GUARD + n]
    return run


run = device_runner()


# ------------------------------------------------------------------------------------------------------- 1. recorded deep states
@pytest.mark.parametrize("name", list(hc.DEEP))
def test_gpu_recorded_deep_states_both_rules_one_call_each(name):
    hc.check_deep(name, load_golden(name), run)


# --------------------------------------------------------------------------------------------------------------------- 2. edges
@pytest.mark.parametrize("size,rotation", hc.GEOMS, ids=hc.GEOM_IDS)
def test_gpu_edge_rows_of_every_geometry(size, rotation):
    names, obs, mask = hc.edge_rows(size, rotation)
    hc.check_rows(run, obs, mask, size, rotation, names)
    hc.check_rows(run, obs[:1], mask[:1], size, rotation, names[:1])


@pytest.mark.parametrize("size,rotation", hc.BATCH_GEOMS, ids=hc.BATCH_IDS)
def test_gpu_batch_sizes_with_tails_in_a_wave_a_workgroup_and_a_block_of_bins(size, rotation):
    hc.check_batches(run, size, rotation)


@pytest.mark.parametrize("size,rotation", hc.CARVED_GEOMS, ids=hc.CARVED_IDS)
def test_gpu_rows_carved_from_a_wider_tensor_with_nan_padding_and_top_null(size, rotation):
    import bpp_amd
    W, L, H, A, M = hc.dims(size, rotation)
    obs, mask = hc.batch_rows(size, rotation, 21)
    for before, after in ((0, 9), (3, 4)):
        wide = np.full((21, before + 4 * A + after), np.nan, np.float32)
        wide[:, before:before + 4 * A] = obs
        view = dev(wide)[:, before:before + 4 * A]
        assert not view.is_contiguous()
        hc.check_rows(lambda o, *a: run(view, *a), obs, mask, size, rotation)
    no_top = device_runner(want_top=False)
    hc.check_rows(lambda *a: (no_top(*a)[0], run(*a)[1]), obs, mask, size, rotation)
    fresh = bpp_amd.heuristic_act(dev(obs), dev(mask), size, rotation)          # no out=: a tensor of its own
    np.testing.assert_array_equal(fresh.cpu().numpy(), hc.expected(obs, mask, size, rotation, "lowest_top")[0])
    for bad in (dev(obs)[:, :4 * A - 1], dev(obs).double(), dev(obs)[:, ::2]):
        with pytest.raises(ValueError):
            bpp_amd.heuristic_act(bad, dev(mask), size, rotation)
    with pytest.raises(ValueError):
        bpp_amd.heuristic_act(dev(obs), dev(mask)[:, :-1], size, rotation)


@pytest.mark.parametrize("levels", [2, 3], ids=["binary-times-footprints", "ternary"])
def test_gpu_a_three_by_three_bin_enumerated_completely(levels):
    hc.check_enumerated(run, levels)


# ------------------------------------------------------------------------------------------------------------------- 3. garbage
@pytest.mark.parametrize("size,rotation", hc.GEOMS, ids=hc.GEOM_IDS)
def test_gpu_garbage_stays_in_bounds(size, rotation):
    """No value is compared: the call returns, the guard words are intact and every action lies in [0, M).  (The same rows run on
    the emulator with an inaccessible page behind the inputs: tests/test_heuristic.py.)"""
    W, L, H, A, M = hc.dims(size, rotation)
    obs, mask = hc.garbage_rows(size, rotation)
    for rule in hc.RULES:
        act, top = run(obs, mask, size, rotation, rule)
        assert ((act >= 0) & (act < M)).all()
        assert ((top >= -1) & (top <= 510)).all()


# -------------------------------------------------------------------------------------------------------------- 4. independence
@pytest.mark.parametrize("size,rotation", [((10, 10, 10), True), ((20, 20, 20), False)], ids=["10r", "20"])
def test_gpu_a_row_gives_the_same_action_wherever_it_stands_on_a_second_stream_and_in_a_replayed_graph(size, rotation):
    import bpp_amd
    hc.check_independence(run, size, rotation)
    n = 70
    obs, mask = hc.batch_rows(size, rotation, n)
    want = hc.expected(obs, mask, size, rotation, "lowest_top")
    o, m = dev(obs), dev(mask)
    act = torch.empty(n, dtype=torch.int64, device="cuda:0")
    top = torch.empty(n, dtype=torch.int32, device="cuda:0")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = bpp_amd.heuristic_act(o, m, size, rotation)
    torch.cuda.current_stream().wait_stream(side)
    np.testing.assert_array_equal(on_side.cpu().numpy(), want[0])
    bpp_amd.heuristic_act(o, m, size, rotation, out=act, top=top)       # the kernel's code is loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # this one launch on one stream
        bpp_amd.heuristic_act(o, m, size, rotation, out=act, top=top)
    for shift in (0, 7, 31):                            # changed inputs: the rows rotated
        o.copy_(dev(np.roll(obs, shift, axis=0)))
        m.copy_(dev(np.roll(mask, shift, axis=0)))
        act.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(act.cpu().numpy(), np.roll(want[0], shift))
        np.testing.assert_array_equal(top.cpu().numpy(), np.roll(want[1], shift))


# -------------------------------------------------------------------------------------------------------------- 5. closed loops
@pytest.mark.parametrize("size,rotation,bins,steps,least,full", hc.LOOPS, ids=["10r", "20", "7x13r"])
def test_gpu_closed_loop_against_the_oracle_env_under_the_oracle_heuristic(oracle, size, rotation, bins, steps, least, full):
    import bpp_amd
    want = hc.oracle_loop(oracle, size, rotation, bins, steps, hc.oracle_heuristic(size, rotation))
    print("%s rotation %d: %d episodes, %d completely packed bins, %d fallback rows" % ((size, rotation) + want[2:]))
    assert want[2] >= least and (want[3] >= 1 or not full)
    env = bpp_amd.BppVecEnv(bins, size, enable_rotation=rotation, pool=bpp_amd.sequences.cut2_pool(size, 32, seed=1), device="cuda:0")
    env.reset()
    actions, episodes = [], 0
    for t in range(steps):
        a = env.heuristic_act()
        res = env.step_tensors(a)
        actions.append(a.clone())
        episodes += res.done.sum()
    got = torch.stack(actions).cpu().numpy()
    for t in range(steps):
        np.testing.assert_array_equal(got[t], want[0][t], err_msg="lock-step %d" % t)
    np.testing.assert_array_equal(env.hmap.cpu().numpy().reshape(bins, -1), want[1].reshape(bins, -1))
    assert int(episodes) == want[2]
    with pytest.raises(ValueError, match="unknown heuristic rule"):
        env.heuristic_act("highest_top")
    plain = env.heuristic_act("lowest_top_plain").cpu().numpy()
    np.testing.assert_array_equal(plain, hc.expected(env._res.obs.cpu().numpy(), env.location_masks.cpu().numpy(), size, rotation, "lowest_top_plain")[0])


# ---------------------------------------------------------------------------------------------------------------- 6. the example
@pytest.mark.parametrize("rotation", [False, True])
def test_gpu_example_equals_the_oracle_env_under_the_oracle_heuristic(oracle, tmp_path, rotation):
    import bpp_amd
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_heuristic as ex
    size, n = (10, 10, 10), 128
    r = ex.evaluate(ex.DATASET, rotation=rotation, limit=n, plans=True)
    pool = bpp_amd.sequences.from_dataset(ex.DATASET, size, first_index=0)
    env = oracle.OracleEnv(pool, size, rotation, n)
    obs, mask = env.reset()
    live = np.ones(n, bool)
    ratio, counter = np.zeros(n), np.zeros(n, np.int32)
    while live.any():
        a = hc.policies.lowest_top_actions(obs, mask, size, rotation)
        out = env.step(np.where(live, a, np.iinfo(np.int64).min))          # BPP_ACTION_NOOP
        fin = live & out["done"].astype(bool)
        ratio[fin], counter[fin] = out["ratio"][fin], out["counter"][fin]
        live &= ~fin
        obs, mask = out["obs"], out["mask"]
    np.testing.assert_array_equal(r["ratio"], ratio)
    np.testing.assert_array_equal(r["counter"], counter)
    assert set(r) >= {"ratio", "counter", "steps", "seconds"} and (r["steps"] > 0).all()
    print("rotation %d: %d trajectories, average space utilization %.4f, average put item number %.2f" % (rotation, n, ratio.mean(), counter.mean()))
    sound, same = ex.check_plans(r["plans"], str(tmp_path / "plans.npz"), r["ratio"])
    assert sound == n and same == n
