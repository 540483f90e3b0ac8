"""Native branch stepping (include/bpp_branch.h): bpp_step_subset / bpp_copy_bins and BppVecEnv.step_bins / observe_bins /
clone_bins, checked against the paths they replace -- bpp_step with BPP_ACTION_NOOP for every other bin (step_subset) and
copy_bin_records (copy_bins / clone_into) -- on twin envs over the same items.  CPU: the product's step_bins / clone_bins on an
EmuVecEnv (tests/emu_env.py) over the product kernels in the host SIMT emulator (tests/emu), and the per-n lifetime of
step_bins' results; `-m gpu`: BppVecEnv on the device at the headline sizes."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from emu_env import KEYS, EmuVecEnv, bind
from test_lookahead import NOOP, replay_branches


# ---------------------------------------------------------------------------------------------------- CPU (emulator)
def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Twins(object):
    """Two emulated envs over the same items: `full` is stepped the old way (bpp_step over all bins, BPP_ACTION_NOOP for the
    unlisted ones; copies by copy_bin_records), `sub`, an EmuVecEnv, by the product's step_bins / clone_bins."""

    def __init__(self, emu, size, rot, E, pool=None, stream=None):
        self.emu, self.E, self.size = emu, E, size
        self.full = emu.OracleEnv(pool, size, rot, E, stream=stream)
        self.sub = EmuVecEnv(emu, size, E, pool=pool, stream=stream, rotation=rot)
        self.mask = self.full.reset()[1]

    def step_full(self, ids, a, sample=None):
        full = np.full(self.E, NOOP, np.int64)
        full[ids] = a
        nxt = None
        if sample is not None:
            nxt = np.zeros(self.E, np.int64)
            o = self.full._o
            o.next_action, o.sample_seed, o.sample_step = _p(nxt).value, sample[0], sample[1]
        try:
            r = self.full.step(full)
        finally:
            self.full._o.next_action = None
        self.mask = r["mask"]
        if nxt is not None:
            r["next_action"] = nxt
        return r

    def step_sub(self, ids, a, sample=None, env=None, check=True):
        """env.step_bins as a dict of arrays (reward [n]); the cached output set of this n is filled with a sentinel byte
        first, so that a row the launch did not write cannot pass for one it wrote."""
        import torch
        env = env or self.sub
        n = len(ids)
        env._branch_out(n)[0]._flat.fill_(0xA5)
        nxt = None if sample is None else torch.full((n,), -7, dtype=torch.int64)
        res = env.step_bins(np.asarray(ids, np.int64), np.asarray(a, np.int64), check=check,
                            sample=None if sample is None else (sample[0], sample[1], nxt))
        r = {k: getattr(res, k).numpy().reshape(-1).copy() if k == "reward" else getattr(res, k).numpy().copy() for k in KEYS}
        if nxt is not None:
            r["next_action"] = nxt.numpy()
        return r

    def clone_full(self, src, dst):
        import torch
        from bpp_amd.vec_env import copy_bin_records
        env = self.full
        t = torch.from_numpy
        s, d = t(np.asarray(src, np.int64)), t(np.asarray(dst, np.int64))
        st = t(env.state.view(np.int32).reshape(self.E, 12))
        if env.stream is None:
            copy_bin_records(t(env.hmap), st, s, d)
        else:
            copy_bin_records(t(env.hmap), st, s, d, ring=t(env.pool), mt=t(env._mt.view(np.int32).reshape(self.E, -1)),
                             gen_next=t(env.gen_next), depth=env.stream.depth)
            env.reset_seq_cache()

    def clone_sub(self, src, dst):
        self.sub.clone_bins(np.asarray(src, np.int64), np.asarray(dst, np.int64))

    def assert_same_state(self, what=""):
        a, b = self.full, self.sub.oracle
        np.testing.assert_array_equal(a.hmap, b.hmap, err_msg="hmap " + what)
        np.testing.assert_array_equal(a.state.view(np.int32), b.state.view(np.int32), err_msg="state " + what)
        np.testing.assert_array_equal(a.ep_acc, b.ep_acc, err_msg="ep_acc " + what)
        if a.stream is not None:
            np.testing.assert_array_equal(a.pool, b.pool, err_msg="ring " + what)
            np.testing.assert_array_equal(a._mt, b._mt, err_msg="mt " + what)
            np.testing.assert_array_equal(a.gen_next, b.gen_next, err_msg="gen_next " + what)


def _actions(rng, emu, mask, ids, t, M):
    """Feasible draws mixed with infeasible placements, out-of-range indices and BPP_ACTION_NOOP."""
    a = emu.sample_feasible(mask, 5, t)[ids]
    u = rng.rand(len(ids))
    a[u < 0.12] = rng.randint(0, M, (u < 0.12).sum())
    a[(u >= 0.12) & (u < 0.17)] = -3
    a[(u >= 0.17) & (u < 0.3)] = NOOP
    return a


def _ids(rng, E, t):
    if t % 10 == 3:
        return rng.permutation(E)                          # n = E, unsorted
    if t % 10 == 7:
        return np.array([rng.randint(E)])                  # n = 1
    return rng.permutation(E)[:rng.randint(2, E)]


def _compare(rf, rs, ids, t):
    for k in KEYS + (("next_action",) if "next_action" in rs else ()):
        np.testing.assert_array_equal(rs[k], rf[k][ids], err_msg="%s t=%d" % (k, t))


GEOMS = [((10, 10, 10), 40), ((20, 20, 20), 20), ((7, 13, 8), 33), ((10, 10, 30), 30)]


@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("size,E", GEOMS)
def test_emulated_step_bins_equals_step_subset(emu, size, E, rot):
    """Compact row i == full row ids[i] bit for bit, and the bins' state afterwards is the same, over 40 calls (episodes
    finish and auto-reset); every 4th call also draws next_action."""
    from bpp_amd import sequences
    pool = sequences.cut2_pool(size, 17, seed=3, native=False)
    tw = Twins(emu, size, rot, E, pool=pool)
    rng = np.random.RandomState(11)
    done = 0
    for t in range(40):
        ids = _ids(rng, E, t)
        a = _actions(rng, emu, tw.mask, ids, t, tw.full.M)
        sample = (9, t) if t % 4 == 1 else None
        rf, rs = tw.step_full(ids, a, sample), tw.step_sub(ids, a, sample)
        _compare(rf, rs, ids, t)
        tw.assert_same_state("t=%d" % t)
        done += int(rs["done"].sum())
    assert done >= 5
    assert int(tw.sub.bad_ids[0]) == 0


@pytest.mark.parametrize("rng_kind", ["mt19937", "counter"])
def test_emulated_step_bins_streaming_with_row_cache(emu, rng_kind):
    """Ring pool with the row cache: the subset kernel drops the lines of the bins it steps (like every kernel but the tile
    step kernel); results and the ring stay those of the full path across refills."""
    size, E = (10, 10, 10), 24
    tw = Twins(emu, size, True, E, stream=dict(bound=(2, 5), seed=7, depth=8, rng=rng_kind))
    assert tw.sub.oracle.seq_cache is not None
    rng = np.random.RandomState(5)
    for t in range(24):
        ids = _ids(rng, E, t)
        a = _actions(rng, emu, tw.mask, ids, t, tw.full.M)
        rf, rs = tw.step_full(ids, a, (2, t)), tw.step_sub(ids, a, (2, t))
        _compare(rf, rs, ids, t)
        tw.assert_same_state("t=%d" % t)


@pytest.mark.parametrize("mode", ["static", "mt19937", "counter"])
def test_emulated_clone_bins_equals_copy_bin_records(emu, mode):
    """bpp_copy_bins == copy_bin_records (+ the row cache zero fill) byte for byte; both twins then step on, across
    refills, and stay identical."""
    from bpp_amd import sequences
    size, E = (10, 10, 10), 24
    if mode == "static":
        tw = Twins(emu, size, False, E, pool=sequences.cut2_pool(size, 9, seed=1, native=False))
    else:
        tw = Twins(emu, size, False, E, stream=dict(bound=(2, 5), seed=3, depth=8, rng=mode))
    rng = np.random.RandomState(2)
    every = np.arange(E)
    for t in range(6):                                      # some history, so that bins differ
        a = emu.sample_feasible(tw.mask, 1, t)
        _compare(tw.step_full(every, a), tw.step_sub(every, a), every, t)
    src = np.array([3, 3, 0, 17, 9, 3])                    # a root copied several times, unsorted pairs
    dst = np.array([20, 5, 11, 1, 23, 14])
    tw.clone_full(src, dst)
    tw.clone_sub(src, dst)
    tw.assert_same_state("after the clone")
    np.testing.assert_array_equal(tw.sub.oracle.hmap[dst], tw.sub.oracle.hmap[src])
    for t in range(6, 26):                                 # refill_every = 4: several refills
        ids = _ids(rng, E, t)
        a = _actions(rng, emu, tw.mask, ids, t, tw.full.M)
        _compare(tw.step_full(ids, a), tw.step_sub(ids, a), ids, t)
        tw.assert_same_state("t=%d" % t)


@pytest.mark.parametrize("size", [(10, 10, 10), (7, 13, 8)])
def test_emulated_bad_ids_are_noop_rows(emu, size):
    """Ids outside [0, E): a no-op row of an empty bin (zeros, next_action 0) and a count in bad_ids; the other slots and
    every bin are exactly what the call without them gives."""
    from bpp_amd import sequences
    E = 20
    pool = sequences.cut2_pool(size, 8, seed=2, native=False)
    tw = Twins(emu, size, True, E, pool=pool)
    ref = EmuVecEnv(emu, size, E, pool=pool, rotation=True)
    rng = np.random.RandomState(3)
    for t in range(6):
        good = rng.permutation(E)[:9]
        a = _actions(rng, emu, tw.mask, good, t, tw.full.M)
        bad_ids = np.array([-1, E, E + 100, 2 ** 40, -2 ** 62])
        ids = np.concatenate([good[:4], bad_ids[:2], good[4:], bad_ids[2:]])
        acts = np.concatenate([a[:4], [0, NOOP], a[4:], [1, 2, 3]])
        before = int(tw.sub.bad_ids[0])
        want = tw.step_sub(good, a, (4, t), env=ref)
        got = tw.step_sub(ids, acts, (4, t), check=False)
        isbad = (ids < 0) | (ids >= E)
        assert int(tw.sub.bad_ids[0]) - before == int(isbad.sum())
        for k in KEYS + ("next_action",):
            np.testing.assert_array_equal(got[k][~isbad], want[k], err_msg=k)
            assert not got[k][isbad].any(), k
        np.testing.assert_array_equal(tw.sub.oracle.hmap, ref.oracle.hmap)
        np.testing.assert_array_equal(tw.sub.oracle.state.view(np.int32), ref.oracle.state.view(np.int32))
        tw.mask = ref.oracle.step(np.full(E, NOOP, np.int64))["mask"]    # (re-emits only: ref's bins stay as they are)


def test_emulated_argument_checks(emu):
    from bpp_amd import sequences
    size, E = (10, 10, 10), 8
    tw = Twins(emu, size, False, E, pool=sequences.cut2_pool(size, 4, seed=1, native=False))
    from bpp_amd import _lib
    L, env = bind(emu), tw.sub.oracle
    ids = np.arange(2, dtype=np.int64)
    none = [np.zeros(0, np.int64) for _ in range(10)]                      # n == 0: a valid no-op
    out = _lib.StepOut(*[_p(x).value for x in none[2:]])
    assert L.bpp_step_subset(ctypes.byref(env._b), _p(none[0]), 0, _p(none[1]), ctypes.byref(out), None, None) == 0
    out = _lib.StepOut(*[_p(np.zeros((2, 400), np.float32)).value] + [None] * 7)
    assert L.bpp_step_subset(ctypes.byref(env._b), _p(ids), 2, _p(ids), ctypes.byref(out), None, None) != 0      # NULL outputs
    assert L.bpp_step_subset(ctypes.byref(env._b), None, 2, _p(ids), ctypes.byref(out), None, None) != 0
    assert L.bpp_step_subset(ctypes.byref(env._b), _p(ids), -1, _p(ids), ctypes.byref(out), None, None) != 0
    assert L.bpp_copy_bins(ctypes.byref(env._b), None, _p(ids), _p(ids), -1, None) != 0
    assert L.bpp_copy_bins(ctypes.byref(env._b), None, None, _p(ids), 1, None) != 0
    assert L.bpp_copy_bins(ctypes.byref(env._b), None, _p(ids), _p(ids), 0, None) == 0


def test_emulated_step_bins_results_live_per_n(emu):
    """step_bins' promise that mcts.py and reorder.py rely on when they keep `.done.data_ptr()` across launches: the
    compact output set of a given n is made once -- two calls with the same n hand back the same buffers -- and a call
    with another n in between neither moves nor overwrites it."""
    g = load_golden("mcts_fake_5x5x3")
    env = EmuVecEnv(emu, (5, 5, 3), 6, pool=g["pool"][:6])
    first = env.step_bins([0, 1, 2], [0, 0, 0])
    ptr, kept = first.done.data_ptr(), {k: getattr(first, k).clone() for k in KEYS}
    other = env.step_bins([3, 4], [1, 1])
    assert other.done.data_ptr() != ptr and other.obs.shape[0] == 2
    for k in KEYS:
        assert getattr(first, k).equal(kept[k]), k
    again = env.step_bins([2, 1, 0], [env.NOOP] * 3)
    assert again is first and again.done.data_ptr() == ptr
    assert again.obs[0].equal(kept["obs"][2]) and not again.done.any()


class NativeHost(object):
    """replay_branches' env interface over the native calls: compact rows scattered into full-batch arrays (an unlisted bin
    keeps its last observation and mask, reward 0, done 0)."""

    def __init__(self, tw):
        self.tw = tw
        self.last = None

    def reset(self):
        env = self.tw.sub.oracle
        self.last = {k: np.array(v) for k, v in env.out.items()}
        return self.last["obs"].copy(), self.last["mask"].copy()

    def _scatter(self, ids, r):
        o = {k: v.copy() for k, v in self.last.items()}
        o["reward"][:] = 0
        o["done"][:] = 0
        for k in KEYS:
            o[k][ids] = r[k]
        self.last = o
        return o

    def step(self, a):
        ids = np.flatnonzero(a != NOOP)
        return self._scatter(ids, self.tw.step_sub(ids, a[ids]))

    def copy(self, src, dst):
        self.tw.clone_sub(src, dst)
        return self._scatter(dst, self.tw.step_sub(dst, np.full(len(dst), NOOP, np.int64)))


@pytest.mark.parametrize("path", ["rt", "generic"])
def test_emulated_native_branches_match_reference_deepcopy(emu, path):
    """The reference-recorded deepcopy branches (tests/test_lookahead.py) replayed through bpp_copy_bins + bpp_step_subset."""
    g = load_golden("lookahead_branch_10")
    size = tuple(int(v) for v in g["size"])
    emu.set_knobs(force_generic=int(path == "generic"))
    try:
        replay_branches(lambda pool, E: NativeHost(Twins(emu, size, True, E, pool=pool)), g)
    finally:
        emu.set_knobs()


# ---------------------------------------------------------------------------------------------------- GPU (-m gpu)
def _gpu_twins(size, E, rot, mode):
    import bpp_amd
    if mode == "static":
        pool = bpp_amd.sequences.cut2_pool(size, 4096, seed=5)
        mk = lambda: bpp_amd.BppVecEnv(E, size, enable_rotation=rot, pool=pool)                 # noqa: E731
    else:
        spec = dict(bound=(2, 5), seed=13, depth=8, rng=mode, cache=True)
        mk = lambda: bpp_amd.BppVecEnv(E, size, enable_rotation=rot, stream=spec)               # noqa: E731
    envs = mk(), mk()
    for e in envs:
        e.reset()
    return envs


def _gpu_assert_same_state(a, b, what):
    import torch
    assert torch.equal(a.hmap, b.hmap), "hmap " + what
    assert torch.equal(a.state, b.state), "state " + what
    assert torch.equal(a.ep_acc, b.ep_acc), "ep_acc " + what
    if a._stream is not None:
        assert torch.equal(a.pool, b.pool), "ring " + what
        assert torch.equal(a.supply.mt, b.supply.mt), "mt " + what
        assert torch.equal(a.gen_next, b.gen_next), "gen_next " + what


def _gpu_actions(env, ids, t, g):
    """Feasible draws for bins `ids` mixed with random (mostly infeasible) indices, -3 and BPP_ACTION_NOOP."""
    import torch
    a = env.sample_feasible(seed=21, step=t)[ids]
    u = torch.rand(ids.numel(), generator=g).to(a.device)
    a = torch.where(u < 0.1, torch.randint(0, env.M, (ids.numel(),), generator=g).to(a.device), a)
    a = torch.where((u >= 0.1) & (u < 0.13), torch.full_like(a, -3), a)
    return torch.where((u >= 0.13) & (u < 0.25), torch.full_like(a, env.NOOP), a)


GPU_CASES = [((10, 10, 10), 65536, False, "static"), ((10, 10, 10), 65536, True, "static"), ((20, 20, 20), 32768, False, "static"),
             ((10, 10, 10), 65536, True, "mt19937"), ((10, 10, 10), 65536, False, "counter"), ((20, 20, 20), 32768, False, "counter"),
             ((7, 13, 8), 4096, True, "static")]


@pytest.mark.gpu
@pytest.mark.parametrize("size,E,rot,mode", GPU_CASES)
def test_gpu_step_bins_equals_step_subset(size, E, rot, mode):
    """Twin envs: step_subset (the full-batch launch) vs step_bins on the same ids and actions, over 24 calls -- unsorted
    subsets from one bin to all of them (arange(E): the tile kernel's full step), every other call with the fused draw.
    Compact row i == full row ids[i] bit for bit; heightmaps, records, accumulators (ring, generators) stay identical."""
    import torch
    a_env, b_env = _gpu_twins(size, E, rot, mode)
    dev = a_env.device
    g = torch.Generator().manual_seed(7)
    fins = 0
    for t in range(24):
        kind = t % 6
        if kind == 0:
            ids = torch.arange(E, device=dev)
        else:
            n = [1, 64, 1024, E // 3, E][kind - 1]
            ids = torch.randperm(E, generator=g)[:n].to(dev)
        a = _gpu_actions(a_env, ids, t, g)
        sample = t % 2 == 1
        nxt_a = torch.full((E,), -9, dtype=torch.int64, device=dev)
        nxt_b = torch.full((ids.numel(),), -9, dtype=torch.int64, device=dev)
        if kind == 0:
            ra = a_env.step_tensors(a, sample=(3, t, nxt_a) if sample else None)        # the tile kernel's lock-step
        else:
            ra = a_env.step_subset(ids, a, sample=(3, t, nxt_a) if sample else None)
        rb = b_env.step_bins(ids, a, sample=(3, t, nxt_b) if sample else None)
        for k in KEYS:
            assert torch.equal(getattr(rb, k), getattr(ra, k)[ids]), (k, t)
        if sample:
            assert torch.equal(nxt_b, nxt_a[ids]), ("next_action", t)
        _gpu_assert_same_state(a_env, b_env, "t=%d" % t)
        fins += int(rb.done.sum())
    assert fins > 100
    assert int(b_env.bad_ids[0]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("size,E,rot,mode", [((10, 10, 10), 65536, True, "static"), ((10, 10, 10), 65536, False, "mt19937"),
                                              ((20, 20, 20), 32768, False, "counter"), ((7, 13, 8), 4096, False, "static")])
def test_gpu_clone_bins_equals_clone_into(size, E, rot, mode):
    """clone_bins + observe_bins vs clone_into (copy_bin_records, whole-cache zero fill, full re-emit): the same bins byte
    for byte and the same observations; both twins then play on, across refills, and stay identical."""
    import torch
    a_env, b_env = _gpu_twins(size, E, rot, mode)
    dev = a_env.device
    every = torch.arange(E, device=dev)
    for t in range(5):
        a = a_env.sample_feasible(seed=1, step=t)
        a_env.step_tensors(a)
        b_env.step_bins(every, a)
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(E, generator=g)
    roots = perm[:700].to(dev)
    src = roots.repeat_interleave(4)[torch.randperm(2800, generator=g).to(dev)]
    dst = perm[700:3500].to(dev)
    ra = a_env.clone_into(src, dst)
    b_env.clone_bins(src, dst)
    rb = b_env.observe_bins(dst)
    _gpu_assert_same_state(a_env, b_env, "after the clone")
    for k in ("obs", "mask"):
        assert torch.equal(getattr(rb, k), getattr(ra, k)[dst]), k
        assert torch.equal(getattr(rb, k), getattr(ra, k)[src]), k
    for t in range(5, 20):
        ids = torch.cat([dst[:1000], torch.randperm(E, generator=g)[:2000].to(dev)]).unique()
        ids = ids[torch.randperm(ids.numel(), generator=g).to(dev)]
        a = _gpu_actions(a_env, ids, t, g)
        ra, rb = a_env.step_subset(ids, a), b_env.step_bins(ids, a)
        for k in KEYS:
            assert torch.equal(getattr(rb, k), getattr(ra, k)[ids]), (k, t)
        _gpu_assert_same_state(a_env, b_env, "t=%d" % t)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(10, 10, 10), (7, 13, 8)])
def test_gpu_bad_ids_and_checks(size):
    """check=True raises on ids out of range, duplicates and src / dst overlap (and launches nothing); check=False lets an
    out-of-range id through as a no-op row counted in bad_ids, without changing any other slot or bin."""
    import torch
    E = 4096
    a_env, b_env = _gpu_twins(size, E, True, "static")
    dev = a_env.device
    for bad in ([0, E], [-1, 3], [5, 9, 5]):
        with pytest.raises(ValueError):
            b_env.step_bins(bad, [0] * len(bad))
        with pytest.raises(ValueError):
            b_env.observe_bins(bad)
    for src, dst in (([1, 2], [3, 1]), ([1, 2], [3, 3]), ([1, E], [3, 4]), ([1, 2], [3, -4])):
        with pytest.raises(ValueError):
            b_env.clone_bins(src, dst)
    _gpu_assert_same_state(a_env, b_env, "after the refused calls")
    good = torch.tensor([7, 3, 100, 4000, 42], device=dev)
    a = a_env.sample_feasible(seed=2, step=0)[good]
    ids = torch.tensor([7, 3, -1, 100, E, 4000, 2 ** 40, 42], device=dev)
    isbad = (ids < 0) | (ids >= E)
    acts = torch.zeros(ids.numel(), dtype=torch.int64, device=dev)
    acts[~isbad] = a
    nxt_a = torch.empty(5, dtype=torch.int64, device=dev)
    nxt_b = torch.full((8,), -9, dtype=torch.int64, device=dev)
    ra = a_env.step_bins(good, a, sample=(1, 1, nxt_a))
    ra = {k: getattr(ra, k).clone() for k in KEYS}
    rb = b_env.step_bins(ids, acts, sample=(1, 1, nxt_b), check=False)
    assert int(b_env.bad_ids[0]) == 3
    for k in KEYS:
        v = getattr(rb, k)
        assert torch.equal(v[~isbad], ra[k]), k
        assert not v[isbad].any(), k
    assert torch.equal(nxt_b[~isbad], nxt_a) and not nxt_b[isbad].any()
    _gpu_assert_same_state(a_env, b_env, "after the bad slots")


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["prefix", "generic"])
def test_gpu_native_branches_match_reference_deepcopy(path):
    """lookahead_branch_10 (the reference's copy.deepcopy branches) replayed through clone_bins + step_bins / observe_bins."""
    import bpp_amd
    g = load_golden("lookahead_branch_10")
    size = tuple(int(v) for v in g["size"])

    class GpuNative(object):
        def __init__(self, pool, E):
            self.env = bpp_amd.BppVecEnv(E, size, enable_rotation=True, pool=pool)
            self.last = None

        def reset(self):
            obs = self.env.reset()
            self.last = dict(obs=obs.cpu().numpy(), mask=self.env.location_masks.cpu().numpy(), reward=np.zeros(self.env.E, np.float32),
                             done=np.zeros(self.env.E, np.uint8), counter=np.zeros(self.env.E, np.int32), ratio=np.zeros(self.env.E),
                             ep_ret=np.zeros(self.env.E), ep_len=np.zeros(self.env.E, np.int32))
            return self.last["obs"].copy(), self.last["mask"].copy()

        def _scatter(self, ids, r):
            o = {k: v.copy() for k, v in self.last.items()}
            o["reward"][:] = 0
            o["done"][:] = 0
            for k in KEYS:
                v = getattr(r, k).cpu().numpy()
                o[k][ids] = v[:, 0] if k == "reward" else v
            self.last = o
            return o

        def step(self, a):
            ids = np.flatnonzero(a != NOOP)
            return self._scatter(ids, self.env.step_bins(ids, a[ids]))

        def copy(self, src, dst):
            self.env.clone_bins(src, dst)
            return self._scatter(dst, self.env.observe_bins(dst))

    old = bpp_amd._lib.set_knobs(force_generic=int(path == "generic"))
    try:
        replay_branches(GpuNative, g)
    finally:
        bpp_amd._lib.set_knobs(**old)
