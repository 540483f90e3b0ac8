"""The tile step kernel's forms with 2 and 4 groups of bins per wave on the device.  configure() picks them by launch size (from
150 001 10x10 bins, 37 501 20x20 bins; bpp_knobs.tile_groups forces one), and they are machine code of their own: another merge of
the window's (max, count) per form (DPP quad_perm / row_ror, the __shfl_xor loop, none at all), NIT staged tiles per lane, tails
that end inside a group, deciding lanes mapped onto owning waves by db / NBW and db % NBW.  Every form against the oracle on every
bin with the cases of tests/tile_group_cases.py, the golden rollouts, the kernel's other callers and the row-cache twin
(bpp_tile_kernel_q).  Everything is bit-exact."""
import numpy as np
import pytest

import tile_group_cases as tg
from conftest import DEEP_CASES, load_golden
from test_gpu_parity import GpuEnv
from test_gpu_pipelined_rollout import rollout
from test_oracle_golden import check_rollout
from test_stream_supply import GpuKnobEnv, knob_check

pytestmark = pytest.mark.gpu

TILE_GOLDENS = ["rollout_cut2_10", "rollout_cut2_10_rot", "rollout_cut2_20"] + DEEP_CASES      # the other goldens never reach the tile kernel


@pytest.fixture(scope="module")
def bpp():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import bpp_amd
    bpp_amd._lib.lib()
    return bpp_amd


@pytest.fixture
def knobs(bpp):
    """Set launch-shape knobs for one test (bpp_set_knobs), restored afterwards."""
    saved = bpp._lib.get_knobs()
    bpp._lib.set_knobs(tile_groups=0, bins_per_wave=0, waves_per_group=0, xcd_remap=1, force_generic=0, legacy_fast=0)
    yield lambda **kw: bpp._lib.set_knobs(**kw)
    bpp._lib.set_knobs(**saved)


@pytest.fixture(params=tg.GROUPS)
def groups(request, knobs):
    knobs(tile_groups=request.param)
    return request.param


class GpuCase(object):
    """tile_group_cases' env over BppVecEnv"""

    def __init__(self, bpp, pool, size, rot, E, rule, base, total):
        import torch
        self.bpp, self.size, self.rot, self.E = bpp, size, rot, E
        self.env = bpp.BppVecEnv(E, size, enable_rotation=bool(rot), pool=np.array(pool), mask_rule="space" if rule else "utils",
                                 env_id_base=base, env_id_total=total)
        self.nxt = torch.empty(E, dtype=torch.int64, device=self.env.device)

    def launch(self):
        i = self.bpp._lib.launch_info(self.E, self.size, self.rot)
        return i["kernel"], i["bins_per_wave"]

    def _out(self, r):
        out = {k: getattr(r, k).cpu().numpy() for k in tg.KEYS if k != "reward"}
        out["reward"] = r.reward.cpu().numpy()[:, 0]
        return out

    def reset(self):
        obs = self.env.reset()
        return obs.cpu().numpy(), self.env.location_masks.cpu().numpy()

    def step(self, a, seed, step):
        self.nxt.fill_(-7)
        r = self.env.step_tensors(np.asarray(a), sample=(seed, step, self.nxt))
        return self._out(r), self.nxt.cpu().numpy()

    def rollout(self, seed, step0, n):
        return self._out(self.env.rollout_uniform(seed=seed, step0=step0, nsteps=n))

    def snapshot(self):
        e = self.env
        return dict(hmap=e.hmap.cpu().numpy(), state=e.state_numpy(), ep_acc=e.ep_acc.cpu().numpy(),
                    stats=e.episode_stats().cpu().numpy(), stats_one=e.episode_stats(wide=False).cpu().numpy())


def tile_launch(bpp, E, size, rot, groups):
    i = bpp._lib.launch_info(E, size, rot)
    assert i["kernel"] == tg.BPP_KERNEL_TILE and i["bins_per_wave"] == tg.EPW[size[0]] * groups, i
    return i


@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("size", tg.SHAPES)
def test_gpu_edge_sizes_match_oracle(bpp, oracle, knobs, groups, size, rot):
    """Every tail of the 2- and 4-group forms: one bin, a wave that ends inside a group, empty waves, +-1 around a wave and a
    workgroup, a third workgroup, sixteen workgroups and a partial one with the XCD remap on and off, a mid-size launch."""
    make_env = lambda *a: GpuCase(bpp, *a)
    for E in tg.edge_sizes(size, groups, device=True):
        for xcd in ((1, 0) if E == tg.xcd_size(size, groups) else (1,)):
            knobs(xcd_remap=xcd)
            for rule in (0, 1):
                tg.lockstep(make_env, oracle, size, rot, E, groups, rule)


@pytest.mark.parametrize("size,rot", sorted(tg.TALL))
def test_gpu_tall_bins_second_histogram_word(bpp, oracle, groups, size, rot):
    tg.tall(lambda *a: GpuCase(bpp, *a), oracle, size, rot, tg.TALL_E[(size, rot)], groups)


@pytest.mark.parametrize("case", TILE_GOLDENS)
def test_gpu_golden_rollouts_under_tile_groups(bpp, groups, case):
    g = load_golden(case)
    tile_launch(bpp, g["actions"].shape[1], tuple(int(v) for v in g["size"]), int(g["rotation"]), groups)
    check_rollout(lambda pool, size, rot, E, rule: GpuEnv(bpp, pool, size, rot, E, rule), g)


OTHER_CALLERS = [((10, 10, 10), True), ((20, 20, 20), False)]


@pytest.mark.parametrize("size,rot", OTHER_CALLERS)
def test_gpu_rotating_sets_with_epsilon_under_tile_groups(bpp, oracle, groups, size, rot):
    """bpp_rollout_uniform_sets over three rotating output sets with the epsilon override == the oracle's statement of it"""
    import torch
    E = tg.MID_SIZE[size[0]]
    tile_launch(bpp, E, size, rot, groups)
    pool = np.array(tg.pool_of(size, 64, 8))      # (the shared one is read-only)
    env = bpp.BppVecEnv(E, size, enable_rotation=rot, pool=pool, env_id_base=11, env_id_total=E + 11)
    ref = oracle.OracleEnv(pool, size, rot, E, env_id_base=11, env_id_total=E + 11)
    env.reset(), ref.reset()
    actions = torch.empty(E, dtype=torch.int64, device=env.device)
    ra, r_last, t = None, None, 0
    for n in (7, 9):
        sets = env.output_sets(3)
        r = env.rollout_uniform_sets(5, t, n, actions, sets=sets, resume=t > 0, eps=0.05)
        rs, ra = oracle.rollout_uniform_sets(ref, 5, t, n, 3, resume=t > 0, actions=ra, first_mask=r_last["mask"] if r_last else None, eps=0.05)
        r_last = rs[(n - 1) % 3]
        t += n
        np.testing.assert_array_equal(actions.cpu().numpy(), ra)
        for k in tg.KEYS:
            np.testing.assert_array_equal(getattr(r, k).cpu().numpy().reshape(r_last[k].shape), r_last[k], err_msg=k)
        for j in range(3):
            np.testing.assert_array_equal(sets[j][0]["mask"].cpu().numpy(), rs[j]["mask"])
            np.testing.assert_array_equal(sets[j][0]["obs"].cpu().numpy(), rs[j]["obs"])
    np.testing.assert_array_equal(env.hmap.cpu().numpy(), ref.hmap)
    np.testing.assert_array_equal(env.ep_acc.cpu().numpy(), ref.ep_acc)
    assert ref.episode_stats()[3] >= 1


@pytest.mark.parametrize("size,rot", OTHER_CALLERS)
def test_gpu_pipelined_driver_under_tile_groups_equals_one_group(bpp, knobs, groups, monkeypatch, size, rot):
    """The pipelined driver's bin groups are launches of their own (env_id_base moved, E halved): two of them at the smallest batch
    bpp_pipeline_plan splits, byte for byte what the same rollout leaves behind with one group of bins per wave."""
    monkeypatch.setattr(bpp.vec_env, "_ENV_ROLLOUT_GROUPS", 0)
    E = 2 * bpp._lib.PIPELINE_MIN_GROUP
    plan = bpp._lib.pipeline_plan(E, 2)
    assert len(plan) == 2 and len(bpp._lib.pipeline_plan(E - 1, 2)) == 1
    for first, count in plan:
        tile_launch(bpp, count, size, rot, groups)
    pool = np.array(tg.pool_of(size, 64, 8))      # (the shared one is read-only)
    got = rollout(bpp, size, rot, E, pool, 2, "rotating_sets")
    knobs(tile_groups=1)
    tile_launch(bpp, plan[0][1], size, rot, 1)
    want = rollout(bpp, size, rot, E, pool, 2, "rotating_sets")
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert want["stats"][3] >= 1                    # episodes did finish (by the one-group form's count, itself pinned to the oracle elsewhere)


@pytest.mark.parametrize("case", ["rollout_cut2_10_rot", "rollout_cut2_20"])
def test_gpu_dropin_step_host_mirror_under_tile_groups(bpp, groups, case):
    """The reference-shaped step(): reward and done are written a second time, into page-locked host memory, by the deciding
    lane -- whose bin changes with the bins per workgroup."""
    import torch
    g = load_golden(case)
    size, rot, E = tuple(int(v) for v in g["size"]), bool(g["rotation"]), g["actions"].shape[1]
    tile_launch(bpp, E, size, rot, groups)
    env = bpp.BppVecEnv(E, size, enable_rotation=rot, pool=g["pool"], fresh_outputs=True)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), g["obs0"].astype(np.float32))
    for t in range(g["actions"].shape[0]):
        env.step_async(torch.from_numpy(g["actions"][t]))
        assert env._pending[1] is not None          # a page-locked buffer took the mirror: step_wait() copies nothing
        obs, reward, done, infos = env.step_wait()
        assert not reward.is_cuda and isinstance(done, np.ndarray)
        np.testing.assert_array_equal(reward.numpy()[:, 0], g["reward"][t], err_msg="reward t=%d" % t)
        np.testing.assert_array_equal(done, g["done"][t].astype(bool), err_msg="done t=%d" % t)
        np.testing.assert_array_equal(obs.cpu().numpy(), g["obs"][t].astype(np.float32), err_msg="obs t=%d" % t)
        ep = infos.episodes()
        d = np.flatnonzero(g["done"][t])
        np.testing.assert_array_equal(ep["bins"], d)
        np.testing.assert_array_equal(ep["ratio"], g["ratio"][t][d])
    assert g["done"].sum() >= 1


@pytest.mark.parametrize("size,gen", [((10, 10, 10), "counter"), ((20, 20, 20), "mt19937")])
def test_gpu_row_cache_kernel_under_tile_groups_matches_oracle(bpp, oracle, groups, size, gen):
    """bpp_tile_kernel_q, the row-cache twin with the same forms: a streaming env with a row cache, 40 lock-steps with refills and
    forced failures, every output of every step and the final ring against the oracle's streaming env."""
    E = 1000 + 4 * tg.EPW[size[0]] * groups // 2 + 1
    tile_launch(bpp, E, size, False, groups)

    def front(sz, n, base, spec):
        assert spec["cache"]
        env = GpuKnobEnv(sz, n, base, spec)
        assert env.env.supply.seq_cache is not None
        return env

    knob_check(front, oracle, lambda **kw: bpp._lib.set_knobs(**kw), size, E, 12, 40, lambda t: 0, refill=4, gen=gen)
    assert bpp._lib.get_knobs()["tile_groups"] == groups


@pytest.mark.parametrize("size,E,want", [((10, 10, 10), 150001, 2), ((20, 20, 20), 37501, 4)])
def test_gpu_forms_selected_by_launch_size_match_oracle(bpp, oracle, knobs, size, E, want):
    """tile_groups = 0: the first launch sizes that get the larger form without anybody asking (more than 300 MB of observation and
    mask bytes).  Four lock-steps, the second with the forced failures, every bin against the oracle."""
    knobs(tile_groups=0)
    assert bpp._lib.launch_info(E - 1, size, False)["bins_per_wave"] == tg.EPW[size[0]]
    tg.lockstep(lambda *a: GpuCase(bpp, *a), oracle, size, False, E, want, 0, steps=4, fail_at=1)
