"""Shared by tests/test_stream_kinds.py (emulator) and tests/test_gpu_stream_kinds.py (device): the statement-made pool a
streaming env of kind "cut1" / "rs" is compared against, and the lock-step comparison itself.

A streaming env plays, as episode k of global bin g, the sequence the Python statement (sequences.cut1_stream_sequence /
rs_stream_sequence) gives for (seed0, g, k).  A pool-mode env of the C restatement (oracle.OracleEnv, env_id_base 0,
env_id_total E) plays pool row (e + k E) mod P as episode k of bin e (include/bpp_abi.h: the static row rule), so a pool whose
row e + k E holds the statement's sequence for (seed0, env_id_base + e, k) must show the same observations, masks, rewards,
dones, ratios and counters under the same actions."""
import functools

import numpy as np

from bpp_amd import sequences

RANGE = (2, 2, 2, 5, 5, 5)
KEYS = ("obs", "mask", "reward", "done", "counter", "ratio")


def pool_len(kind, size, box_range=RANGE, box_set=None):
    W, L, H = size
    if kind == "cut1":
        return W * L * H // (box_range[0] * box_range[1] * box_range[2]) + 3
    return sequences.rs_stream_pool_len(size, box_set)


@functools.lru_cache(maxsize=None)
def statement(kind, size, rot, seed, sid, k, box_range=RANGE, box_set=None):
    if kind == "cut1":
        return tuple(sequences.cut1_stream_sequence(size, box_range, seed, sid, k, rot))
    return tuple(sequences.rs_stream_sequence(size, box_set, seed, sid, k, pool_len(kind, size, box_set=box_set) - 3))


def statement_pool(kind, size, rot, seed, base, E, K, box_range=RANGE, box_set=None):
    """uint8 [E K][T][4]: row e + k E = the statement's sequence for (seed, base + e, k)."""
    seqs = [statement(kind, size, rot, seed, base + e, k, box_range, box_set) for k in range(K) for e in range(E)]
    return sequences.pad_pool([list(s) for s in seqs], size, pool_len(kind, size, box_range, box_set) - 2)


def lock_step_check(oracle, stream_env, kind, size, rot, E, base, seed, steps, box_range=RANGE, box_set=None, fail=0.15):
    """stream_env: reset() -> (obs, mask), step(actions) -> dict of KEYS (numpy), episodes() -> int array [E].  Steps it with
    uniform-feasible actions and `fail` of them replaced by an infeasible one (bins race through their episodes), then replays
    the same actions on the pool-mode env and compares every step."""
    obs, mask = stream_env.reset()
    mask0 = mask
    rng = np.random.RandomState(seed)
    acts, outs = [], []
    for t in range(steps):
        a = oracle.sample_feasible(mask, 5, t)
        a[rng.rand(E) < fail] = -1
        r = stream_env.step(a)
        acts.append(a)
        outs.append(r)
        mask = r["mask"]
    episodes = np.asarray(stream_env.episodes())
    assert int(episodes.min()) >= 2, "every bin must get through several episodes"
    pool = statement_pool(kind, size, rot, seed, base, E, int(episodes.max()) + 3, box_range, box_set)
    ref = oracle.OracleEnv(pool, size, rot, E, env_id_base=0, env_id_total=E)
    robs, rmask = ref.reset()
    np.testing.assert_array_equal(obs, robs)
    np.testing.assert_array_equal(mask0, rmask)
    for t in range(steps):
        o = ref.step(acts[t])
        for k in KEYS:
            np.testing.assert_array_equal(np.asarray(outs[t][k]).reshape(o[k].shape), o[k], err_msg="%s t=%d" % (k, t))
    np.testing.assert_array_equal(episodes, ref.state["episode"])
    return episodes
