"""The CUT-1 and RS stream kinds on the device (include/bpp_stream_kinds.h; BppVecEnv(stream=dict(kind=...))): the refill
kernels against the Python statements lock-step by lock-step (tests/stream_kind_cases.py) and whole ring by whole ring -- at
every box range and box set of that module, with rows too short and boxes that do not fit (overflow above zero), and on rings
whose rows need a second round of the refill kernels' grid-stride loop --, the rollout driver against the same lock-steps taken
one by one, HIP-stream independence, clones, checkpoints and the refusals of the stream spec."""
import numpy as np
import pytest

import stream_kind_cases as cases

pytestmark = pytest.mark.gpu
SIZE = (10, 10, 10)


class GpuKindEnv(object):
    def __init__(self, kind, size, rot, E, base, seed, depth, refill, cache, **spec):
        import bpp_amd
        self.env = bpp_amd.BppVecEnv(E, size, enable_rotation=rot, env_id_base=base, env_id_total=base + E + 3,
                                     stream=dict(spec, kind=kind, seed=seed, depth=depth, refill_every=refill, cache=cache))

    def reset(self):
        obs = self.env.reset()
        return obs.cpu().numpy(), self.env.location_masks.cpu().numpy()

    def step(self, a):
        r = self.env.step_tensors(np.asarray(a))
        out = {k: getattr(r, k).cpu().numpy() for k in ("obs", "mask", "done", "counter", "ratio")}
        out["reward"] = r.reward.cpu().numpy()[:, 0]
        return out

    def episodes(self):
        assert int(self.env.stream_overflow.item()) == 0 or self.short_rows
        return self.env.state_numpy()["episode"].copy()

    short_rows = False                                  # rows shorter than the longest sequence: overflow is expected

    def refill(self):
        self.env.refill()

    def overflow(self):
        return int(self.env.stream_overflow.item())

    def check_ring(self, kind, size, rot, seed, base, depth, box_range=cases.RANGE, box_set=None):
        """The whole ring against the statement (one device-to-host copy); returns gen_next."""
        gen_next = self.env.gen_next.cpu().numpy()
        cases.ring_check(self.env.pool.cpu().numpy(), gen_next, self.env.state_numpy()["episode"], kind, size, rot, seed, base, depth,
                         box_range, box_set)
        return gen_next


@pytest.mark.parametrize("kind", ["cut1", "rs"])
@pytest.mark.parametrize("size,rot,E,depth,refill,cache", [
    (SIZE, False, 257, 8, 4, True),                     # several workgroups and a tail
    (SIZE, False, 257, 8, 5, False),
    (SIZE, True, 257, 8, 4, True),
    ((8, 12, 9), False, 70, 8, 5, False),               # the runtime-geometry step kernel
    ((18, 8, 7), False, 70, 6, 3, False)])              # pieces of two words, 32 lanes at work per wave
def test_gpu_rows_equal_the_statement(oracle, kind, size, rot, E, depth, refill, cache):
    seed, base = 77, 1000
    env = GpuKindEnv(kind, size, rot, E, base, seed, depth, refill, cache)
    episodes = cases.lock_step_check(oracle, env, kind, size, rot, E, base, seed, 64)
    assert int(env.env.gen_next.min().item()) > depth and int(episodes.max()) >= 4


def kind_spec(kind, box_range, box_set):
    return dict(box_range=box_range) if kind == "cut1" else dict(box_set=list(box_set)) if box_set is not None else {}


@pytest.mark.parametrize("case", cases.KIND_CASES, ids=cases.case_id)
def test_gpu_ring_rows_equal_the_statement(oracle, case):
    """Every entry of every ring row against the statement, at every box range and box set of tests/stream_kind_cases.py: after
    the first refill, and again with the bins at different episodes.  420 rows: seven workgroups and a tail at 64 lanes."""
    kind, size, rot, box_range, box_set = case
    E, base, seed, depth = 70, 40, 11, 6
    env = GpuKindEnv(kind, size, rot, E, base, seed, depth, 2, False, **kind_spec(kind, box_range, box_set))
    env.check_ring(kind, size, rot, seed, base, depth, box_range, box_set)
    cases.race_bins(oracle, env, E)
    env.refill()
    gen_next = env.check_ring(kind, size, rot, seed, base, depth, box_range, box_set)
    assert len(set(gen_next.tolist())) > 2 and env.overflow() == 0


def test_gpu_short_cut1_rows_are_cut_and_counted(oracle):
    """tests/test_stream_kinds.py::test_emulated_short_cut1_rows_are_cut_and_counted on the device."""
    E, base, seed, depth, T = 20, 40, 11, 6, 36
    first = cases.expected_overflow("cut1", SIZE, False, seed, base, E, [depth] * E, pool_len_=T)
    assert 0 < first < E * depth and first == 11
    env = GpuKindEnv("cut1", SIZE, False, E, base, seed, depth, 2, False, pool_len=T)
    assert env.env.pool.shape[1] == T
    env.check_ring("cut1", SIZE, False, seed, base, depth)
    assert env.overflow() == first
    cases.race_bins(oracle, env, E)
    env.refill()
    gen_next = env.check_ring("cut1", SIZE, False, seed, base, depth)
    assert len(set(gen_next.tolist())) > 2
    assert env.overflow() == cases.expected_overflow("cut1", SIZE, False, seed, base, E, gen_next, pool_len_=T) > first
    # Uniform play puts 18 items at most into these bins: it reaches the terminator of a cut row only where rows are shorter.
    for T, deepest in ((T, None), (12, 9)):
        env, played = GpuKindEnv("cut1", SIZE, False, E, base, seed, depth, 2, False, pool_len=T), []
        env.short_rows = True
        cases.lock_step_check(oracle, env, "cut1", SIZE, False, E, base, seed, 64, fail=0, pool_len_=T, played=played)
        assert deepest is None or max(int(o["counter"].max()) for o in played) == deepest
    gen_next = env.env.gen_next.cpu().numpy()           # at 9 items a row every sequence is cut
    assert env.overflow() == cases.expected_overflow("cut1", SIZE, False, seed, base, E, gen_next, pool_len_=12) == int(gen_next.sum())


def test_gpu_bad_rs_boxes_are_played_as_the_terminator_and_counted_per_sequence():
    """BppVecEnv refuses a set with such boxes, so the refill is called on an env's bpp_stream with a device set of its own:
    every bad draw is the terminator in the ring, every other entry the statement's, and a row counts once."""
    import ctypes
    import torch
    E, base, seed, depth = 70, 40, 11, 6
    bad = cases.bad_box_set(SIZE)
    rows = [cases.ring_items("rs", SIZE, False, seed, base + e, k, box_set=bad, T=128) for e in range(E) for k in range(depth)]
    n_bad = [sum(it == SIZE for it in items) for items, over in rows]
    assert 0 < sum(n > 0 for n in n_bad) < len(rows) and max(n_bad) > 1
    env = GpuKindEnv("rs", SIZE, False, E, base, seed, depth, 2, False)
    assert env.env.pool.shape[1] == 128 and env.overflow() == 0
    env.env.gen_next.zero_()                            # every row is written again
    dev_set = torch.from_numpy(cases.box_set_array(bad)).to(env.env.device)
    assert env.env.lib.bpp_stream_refill_rs(ctypes.byref(env.env._stream), dev_set.data_ptr(), int(dev_set.shape[0]), env.env._stream_ptr()) == 0
    env.check_ring("rs", SIZE, False, seed, base, depth, box_set=bad)
    assert env.overflow() == sum(n > 0 for n in n_bad)


@pytest.mark.parametrize("kind,size,E", [("rs", SIZE, 65536), ("cut1", SIZE, 65536), ("cut1", (18, 8, 7), 32768)])
def test_gpu_second_round_of_the_grid_stride_loop(kind, size, E):
    """The smallest rings with more rows than 8 192 workgroups serve in one round (64 lanes at work per workgroup, 32 at
    18 x 8 x 7): after one refill every bin has its `depth` rows, nothing overflowed, and all rows of six bins across the
    ring -- look-ahead entries included -- are the statement's."""
    import torch
    import bpp_amd
    from bpp_amd import _lib
    base, seed, depth = 40, 11, 9
    env = bpp_amd.BppVecEnv(E, size, env_id_base=base, stream=dict(kind=kind, seed=seed, depth=depth, refill_every=2, cache=False))
    lanes = _lib.stream_kinds_info(env._stream, kind, cases.RANGE)["lanes"]
    assert lanes == (32 if size == (18, 8, 7) else 64) and 8192 * lanes < E * depth < 2 * 8192 * lanes
    gen_next = env.gen_next.cpu().numpy()
    assert (gen_next == depth).all() and int(env.stream_overflow.item()) == 0
    bins = [0, 1, 4095, E // 2, E - 2, E - 1]
    rows = env.pool[torch.from_numpy(cases.ring_rows(E, depth, bins)).to(env.pool.device)].cpu().numpy()
    cases.ring_check(rows, gen_next, np.zeros(E, np.int64), kind, size, False, seed, base, depth, bins=bins)


@pytest.mark.parametrize("kind", ["cut1", "rs"])
def test_gpu_rollout_in_one_call_equals_the_steps_taken_one_by_one(kind):
    import torch
    import bpp_amd
    E, spec = 300, dict(kind=kind, seed=5, depth=8, refill_every=4)
    one = bpp_amd.BppVecEnv(E, SIZE, enable_rotation=True, stream=spec)
    two = bpp_amd.BppVecEnv(E, SIZE, enable_rotation=True, stream=spec)
    one.reset(), two.reset()
    r = one.rollout_uniform(3, 0, 48)
    for t in range(48):
        o = two.step_tensors(two.sample_feasible(seed=3, step=t))
    for k in ("obs", "mask", "reward", "done", "counter", "ratio", "ep_ret", "ep_len"):
        assert torch.equal(getattr(r, k), getattr(o, k)), k
    two.refill()                                        # the driver ends with a refill: both rings now hold the same episodes
    assert torch.equal(one.state, two.state) and torch.equal(one.gen_next, two.gen_next) and torch.equal(one.pool, two.pool)
    assert int(one.state_numpy()["episode"].max()) >= 2 and int(one.stream_overflow.item()) == 0


@pytest.mark.parametrize("kind", ["cut1", "rs"])
def test_gpu_two_envs_on_different_hip_streams_fill_identical_rings(kind):
    import torch
    import bpp_amd
    E, spec = 1000, dict(kind=kind, seed=9, depth=8, refill_every=4)
    a = bpp_amd.BppVecEnv(E, SIZE, stream=spec)
    a.reset()
    a.rollout_uniform(1, 0, 30)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = bpp_amd.BppVecEnv(E, SIZE, stream=spec)
        b.reset()
        b.rollout_uniform(1, 0, 30)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(a.pool, b.pool) and torch.equal(a.gen_next, b.gen_next) and torch.equal(a.state, b.state)
    assert int(a.gen_next.min().item()) > 8


@pytest.mark.parametrize("kind", ["cut1", "rs"])
def test_gpu_clone_continues_the_sources_stream(kind):
    import torch
    import bpp_amd
    E, seed, base = 8, 5, 40
    env = bpp_amd.BppVecEnv(E, SIZE, env_id_base=base, stream=dict(kind=kind, seed=seed, depth=6, refill_every=1, cache=False))
    env.reset()
    for t in range(2):
        env.step_tensors(env.sample_feasible(seed=1, step=t))
    env.clone_bins([0], [1])
    NOOP = -2 ** 63
    a = torch.full((E,), NOOP, dtype=torch.int64)
    a[0] = -1
    for t in range(12):                                 # the source burns through more episodes than the ring holds
        env.step_tensors(a)
    a[0] = NOOP
    st = env.state_numpy()
    episode, cursor = int(st["episode"][1]), int(st["cursor"][1])
    o = env.step_tensors(a)
    for k in range(40):
        seq = cases.statement(kind, SIZE, False, seed, base + 0, episode)
        want = seq[cursor] if cursor < len(seq) else SIZE
        obs = o.obs[1].cpu().numpy()
        assert tuple(int(obs[(p + 1) * 100]) for p in range(3)) == tuple(want), (k, episode, cursor)
        feasible = torch.nonzero(o.mask[1]).reshape(-1)
        a[1] = int(feasible[0]) if feasible.numel() else -1
        o = env.step_tensors(a)
        episode, cursor = (episode + 1, 0) if bool(o.done[1]) else (episode, cursor + 1)
    assert episode >= 2 and int(env.stream_overflow.item()) == 0


def test_gpu_checkpoints_and_the_refusals_of_the_stream_spec():
    import torch
    import bpp_amd
    from bpp_amd import sequences
    E = 200
    for spec in (dict(kind="cut1", seed=5, depth=6, refill_every=3), dict(kind="rs", seed=5, depth=6, refill_every=3)):
        env = bpp_amd.BppVecEnv(E, SIZE, enable_rotation=True, stream=spec)
        env.reset()
        env.rollout_uniform(seed=3, step0=0, nsteps=17)
        ckpt = env.state_dict()
        assert ckpt["stream_spec"]["kind"] == spec["kind"]
        first = env.rollout_uniform(seed=3, step0=17, nsteps=23)
        want = {k: getattr(first, k).clone() for k in ("obs", "mask", "counter", "ratio", "ep_ret")}
        other = bpp_amd.BppVecEnv(E, SIZE, enable_rotation=True, stream=spec)
        other.load_state_dict(ckpt)
        again = other.rollout_uniform(seed=3, step0=17, nsteps=23)
        for k, v in want.items():
            assert torch.equal(getattr(again, k), v), k
        assert torch.equal(other.state, env.state) and torch.equal(other.gen_next, env.gen_next)
        changed = dict(spec, box_range=(2, 2, 2, 5, 5, 4)) if spec["kind"] == "cut1" else dict(spec, box_set=sequences.DEFAULT_BOX_SET[:63],
                                                                                              pool_len=ckpt["stream_spec"]["pool_len"])
        for wrong in (changed, dict(spec, kind="rs" if spec["kind"] == "cut1" else "cut1", pool_len=ckpt["stream_spec"]["pool_len"])):
            with pytest.raises(ValueError, match="stream_spec"):
                bpp_amd.BppVecEnv(E, SIZE, enable_rotation=True, stream=wrong).load_state_dict(ckpt)
    # a checkpoint without `kind` is CUT-2, and the other way round
    cut2 = bpp_amd.BppVecEnv(E, SIZE, enable_rotation=True, stream=dict(seed=5, depth=6, refill_every=3, rng="counter", pool_len=128))
    assert "kind" not in cut2.state_dict()["stream_spec"]
    with pytest.raises(ValueError, match="stream_spec"):
        cut2.load_state_dict(ckpt)
    with pytest.raises(ValueError, match="stream_spec"):
        bpp_amd.BppVecEnv(E, SIZE, enable_rotation=True, stream=dict(kind="rs", seed=5, depth=6, refill_every=3)).load_state_dict(cut2.state_dict())
    # the spec itself
    for bad in (dict(kind="cut1", rng="mt19937"), dict(kind="rs", rng="mt19937"), dict(kind="cut3"), dict(kind="cut1", box_range=(2, 2, 6, 5, 5, 5)),
                dict(kind="cut1", box_range=(3, 2, 2, 4, 5, 5)), dict(kind="rs", box_set=[]), dict(kind="rs", box_set=[(2, 2, 11)]),
                dict(kind="rs", pool_len=100)):
        with pytest.raises(ValueError):
            bpp_amd.BppVecEnv(8, SIZE, stream=bad)
    with pytest.raises(ValueError, match="BPP_CUT1_MAX_PIECES"):
        bpp_amd.BppVecEnv(8, (10, 10, 12), stream=dict(kind="cut1"))
    assert bpp_amd.BppVecEnv(8, SIZE, stream=dict(kind="cut1")).stream_spec["rng"] == "counter"
    # make_vec_envs hands the dict to the env as it is: the kind is what the dict says, whatever args.data_type is
    import types
    args = types.SimpleNamespace(container_size=SIZE, enable_rotation=False, data_type="cut2", box_size_set=None)
    envs = bpp_amd.make_vec_envs("Bpp-v0", 1, 16, 1.0, None, "cuda:0", False, args=args, stream=dict(kind="cut1", seed=4))
    obs = envs.reset().cpu().numpy()
    assert envs.stream_spec["kind"] == "cut1"
    for e in (0, 15):
        assert tuple(int(obs[e, (p + 1) * 100]) for p in range(3)) == cases.statement("cut1", SIZE, False, 4, e, 0)[0]
    assert bpp_amd.BppVecEnv(8, SIZE, stream=dict(bound=(2, 5))).stream_spec["rng"] == "mt19937"       # no kind: CUT-2 as before
