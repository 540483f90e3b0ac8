"""Cases shared by tests/test_tile_groups.py (the emulated kernels, CPU) and tests/test_gpu_tile_groups.py (the device): the tile step
kernel in its forms with 2 and 4 groups of bins per wave (bpp_knobs.tile_groups; chosen by launch size when the knob is 0) against
the oracle.  Plain numpy, no device named here: the env under test comes from a factory

    make_env(pool, size, rot, E, rule, base, total) -> env

    env.launch()                 -> (kernel, bins_per_wave) of bpp_launch_info for this env's launch under the current knobs
    env.reset()                  -> (obs, mask)
    env.step(actions, seed, t)   -> (dict over KEYS, next_action): one lock-step that also draws, inside the step kernel, the
                                    uniform-feasible action for the new observation with (seed, t)
    env.rollout(seed, step0, n)  -> dict over KEYS after n lock-steps of the native uniform driver
    env.snapshot()               -> dict(hmap, state (records with the oracle's field names), ep_acc, stats, stats_one): byte
                                    heightmaps, state records, accumulator rows and their sum in both forms of the reduction

Every comparison is bit-exact.  Every "this path really ran" condition is taken from launch_info or from the ORACLE's data (finished
episodes, NOOPs played, share of tall bins), never from what the env under test returned."""
import functools

import numpy as np

from bpp_amd import sequences

KEYS = ("obs", "mask", "reward", "done", "counter", "ratio", "ep_ret", "ep_len")
BPP_KERNEL_TILE = 2
NOOP = -2 ** 63                                     # BPP_ACTION_NOOP
GROUPS = (2, 4)
# every kTileGeo entry (csrc/bpp_kernels.hip): K = 1 / K = 2 with four bins per wave; K = 1 / K = 2 (two-phase scan) with one
SHAPES = [(10, 10, 10), (10, 10, 20), (20, 20, 10), (20, 20, 20)]
EPW = {10: 4, 20: 1}                                # bins of one group, by bin side
MID_SIZE = {10: 4099, 20: 515}
BASE, EXTRA, POOL_ROWS = 5, 4, 37                   # env_id_base = 5, env_id_total = E + 9
STEPS, FAIL_AT = 16, 5
# tall(): (size, rot) -> lock-steps.  On the oracle (pool seed 13, rollout seed 17, three chunks) 94 of 600 / 81 of 600 / 166 of 531
# bins are taller than 11 at a chunk end
TALL = {((10, 10, 20), False): 120, ((10, 10, 22), True): 120, ((20, 20, 20), False): 110}
TALL_E = {((10, 10, 20), False): 600, ((10, 10, 22), True): 600, ((20, 20, 20), False): 531}


@functools.lru_cache(maxsize=None)
def pool_of(size, rows, seed):
    p = sequences.cut2_pool(size, rows, seed=seed, native=False)
    p.flags.writeable = False
    return p


def same(got, want, msg):
    if not np.array_equal(got, want):               # (the report is only built when there is something to report)
        np.testing.assert_array_equal(got, want, err_msg=msg)
        raise AssertionError(msg)


def check_launch(env, size, groups):
    """The launch is the tile kernel with `groups` groups per wave, read from launch_info: a shape that falls through to another
    kernel or another form fails here.  Returns (EPW, NBW, NB)."""
    kernel, bpw = env.launch()
    epw = EPW[size[0]]
    assert kernel == BPP_KERNEL_TILE, "kernel %d, not the tile kernel" % kernel
    assert bpw == epw * groups, "bins per wave %d, expected %d groups of %d" % (bpw, groups, epw)
    return epw, bpw, 4 * bpw


def edge_sizes(size, groups, device=False):
    """Bin counts at the tail logic's edges, from NBW = EPW * groups bins per wave and NB = 4 * NBW per workgroup."""
    epw = EPW[size[0]]
    nbw = epw * groups
    nb = 4 * nbw
    sizes = [1,
             epw * (groups - 1) + 1,                # wave 0's last group holds one bin, waves 1-3 are empty
             nbw, nbw + 1,
             nb - 1, nb, nb + 1,
             2 * nb + nbw + epw + 1]                # a third workgroup whose wave 1 ends inside its second group
    if device:
        sizes += [xcd_size(size, groups), MID_SIZE[size[0]]]
    return sorted(set(sizes))


def xcd_size(size, groups):
    """Sixteen workgroups and a partial seventeenth: xcd_block_of permutes them"""
    nbw = EPW[size[0]] * groups
    return 16 * 4 * nbw + 3 * nbw - 1


def lockstep(make_env, oracle, size, rot, E, groups, rule, steps=STEPS, fail_at=FAIL_AT, seed=17):
    """The env under test against the oracle on EVERY bin: observation, mask, reward, done, counter, ratio, Monitor sums and the
    fused draw of the next action every lock-step; heightmaps, state records, accumulator rows and their sums at the end.  The
    actions are the fused draw with 5 % of them replaced by values from [-2, M + 2] and 5 % by BPP_ACTION_NOOP; lock-step `fail_at`
    places every third bin's item in the far corner, where it cannot fit."""
    pool = pool_of(tuple(size), POOL_ROWS, 1)
    total = BASE + E + EXTRA
    env = make_env(pool, size, rot, E, rule, BASE, total)
    epw, nbw, nb = check_launch(env, size, groups)
    ref = oracle.OracleEnv(pool, size, rot, E, env_id_base=BASE, env_id_total=total, mask_rule=rule)
    tag = "%r rot=%d E=%d groups=%d rule=%d" % (tuple(size), rot, E, groups, rule)
    obs, mask = env.reset()
    robs, rmask = ref.reset()
    same(obs, robs, tag + " reset obs")
    same(mask, rmask, tag + " reset mask")
    A, M = ref.A, ref.M
    rng = np.random.RandomState(1000 * E + 10 * groups + rule)
    a = oracle.sample_feasible(rmask, seed, 0, env_id_base=BASE)
    finished = noops = 0
    for t in range(steps):
        a = a.copy()
        bad = rng.rand(E) < 0.05
        a[bad] = rng.randint(-2, M + 3, size=int(bad.sum()))
        a[rng.rand(E) < 0.05] = NOOP
        if t == fail_at:
            a[::3] = A - 1
        if t == 2:
            a[E - 1] = NOOP                         # (so that the smallest runs play one too: the tail bin of the last wave)
        if t == 9:
            a[E // 2] = -1
        out, nxt = env.step(a, seed, t + 1)
        o = ref.step(a, copy=False)
        for k in KEYS:
            same(out[k], o[k], "%s: %s t=%d" % (tag, k, t))
        same(nxt, oracle.sample_feasible(o["mask"], seed, t + 1, env_id_base=BASE), "%s: next_action t=%d" % (tag, t))
        finished += int(o["done"].sum())
        noops += int((a == NOOP).sum())
        a = nxt
    snap = env.snapshot()
    same(snap["hmap"], ref.hmap, tag + " heightmaps")
    for f in ref.state.dtype.names:                 # hmax among them
        same(snap["state"][f], ref.state[f], "%s: state.%s" % (tag, f))
    same(snap["ep_acc"], ref.ep_acc, tag + " ep_acc")
    want = ref.episode_stats()
    same(snap["stats"], want, tag + " episode_stats")
    same(snap["stats_one"], want, tag + " episode_stats, one-workgroup form")
    # conditions on the inputs, from the oracle's side
    assert finished >= 1 and want[3] == finished, (tag, finished, want)
    assert noops >= 1, tag
    return finished, noops


def tall(make_env, oracle, size, rot, E, groups):
    """K = 2 bins grown until a good share of them is taller than the first histogram word holds (11), so that the second word
    decides masks: three chunks of the native uniform driver, every chunk's outputs, heightmaps and hmax against the oracle."""
    steps = TALL[(tuple(size), bool(rot))]
    pool = pool_of(tuple(size), 64, 13)
    env = make_env(pool, size, rot, E, 0, 0, E)
    epw, nbw, nb = check_launch(env, size, groups)
    assert E % nb != 0
    ref = oracle.OracleEnv(pool, size, rot, E)
    tag = "%r rot=%d E=%d groups=%d" % (tuple(size), rot, E, groups)
    env.reset(), ref.reset()
    tall_seen, done_steps = 0, 0
    for chunk in (steps // 3, steps // 3, steps - 2 * (steps // 3)):
        out = env.rollout(17, done_steps, chunk)
        o, _ = oracle.rollout_uniform(ref, 17, done_steps, chunk)
        done_steps += chunk
        for k in KEYS:
            same(out[k], o[k], "%s: %s after %d" % (tag, k, done_steps))
        snap = env.snapshot()
        same(snap["hmap"], ref.hmap, "%s: heightmaps after %d" % (tag, done_steps))
        same(snap["state"]["hmax"], ref.state["hmax"], "%s: hmax after %d" % (tag, done_steps))
        oracle_hmax = ref.hmap.max(1)
        same(ref.state["hmax"], oracle_hmax, tag + ": the record's hmax is the map's maximum")
        tall_seen = max(tall_seen, int((oracle_hmax > 11).sum()))
    same(snap["ep_acc"], ref.ep_acc, tag + " ep_acc")
    same(snap["stats"], ref.episode_stats(), tag + " episode_stats")
    assert 20 * tall_seen >= E, "%s: only %d of %d bins are taller than 11 at a chunk end" % (tag, tall_seen, E)
    return tall_seen
