"""Shared by tests/test_stream_kinds.py (emulator) and tests/test_gpu_stream_kinds.py (device): the statement-made pool a
streaming env of kind "cut1" / "rs" is compared against, the lock-step comparison itself, and the comparison of a whole ring
(every entry of every row, the overflow count) with the statement.

A streaming env plays, as episode k of global bin g, the sequence the Python statement (sequences.cut1_stream_sequence /
rs_stream_sequence) gives for (seed0, g, k).  A pool-mode env of the C restatement (oracle.OracleEnv, env_id_base 0,
env_id_total E) plays pool row (e + k E) mod P as episode k of bin e (include/bpp_abi.h: the static row rule), so a pool whose
row e + k E holds the statement's sequence for (seed0, env_id_base + e, k) must show the same observations, masks, rewards,
dones, ratios and counters under the same actions.

A ring row of pool_len entries holds two look-ahead entries, the first pool_len - 3 items of the statement and the terminator
(include/bpp_stream_kinds.h); a CUT-1 sequence longer than that, and an RS row with a draw that does not fit the bin (played as
the terminator), count once each in *s->overflow."""
import functools

import numpy as np

from bpp_amd import sequences

RANGE = (2, 2, 2, 5, 5, 5)
KEYS = ("obs", "mask", "reward", "done", "counter", "ratio")

# (size, rotation, box_range) of the CUT-1 rings compared whole, and what each is there for
CUT1_CASES = [
    ((10, 10, 10), False, RANGE),                       # the default
    ((10, 10, 10), True, RANGE),                        # ... with rotation
    ((10, 10, 10), False, (2, 2, 3, 4, 5, 7)),          # all three axes differ
    ((10, 10, 10), True, (2, 3, 2, 3, 6, 10)),          # high_z = H: z is never cut
    ((8, 12, 9), False, (3, 2, 2, 5, 4, 9)),            # the runtime-geometry step kernel
    ((4, 4, 8), True, (1, 1, 1, 1, 1, 1)),              # 128 unit pieces: the cap of the piece list, one-word pieces
    ((16, 6, 8), True, (4, 1, 2, 300, 2, 4)),           # two-word pieces, a high clipped at 255, x is never cut
    ((18, 8, 7), False, RANGE),                         # 126 two-word pieces: 32 lanes at work per wave
    ((15, 9, 6), False, (3, 3, 1, 5, 5, 1)),            # a side of 15 in four bits, unit height
    ((10, 10, 10), False, (5, 5, 5, 9, 9, 9)),          # eight pieces
    ((10, 10, 10), False, (10, 10, 10, 19, 19, 19)),    # one piece, the bin itself: the item equals the terminator
]


def _many_boxes():
    r = np.random.RandomState(4096)
    return tuple(tuple(int(v) for v in b) for b in r.randint(2, 7, size=(4096, 3)))


# (size, box_set) of the RS rings compared whole (None: the default set of 64)
RS_CASES = [
    ((10, 10, 10), None),
    ((10, 10, 10), ((2, 2, 2),)),                                                               # n = 1
    ((10, 10, 10), ((2, 3, 4), (5, 5, 2), (3, 3, 3))),
    ((10, 10, 10), tuple(sequences.DEFAULT_BOX_SET[:63])),                                      # no power of two
    ((10, 10, 10), tuple((i, j, k) for i in range(2, 7) for j in range(2, 7) for k in range(2, 7))),
    ((10, 10, 10), _many_boxes()),                                                              # BPP_RS_MAX_SET boxes, with duplicates
    ((8, 12, 9), ((12, 8, 3), (2, 2, 2), (4, 6, 3), (8, 3, 9), (3, 12, 2))),                    # (12, 8, 3) fits with x / y swapped only
]
KIND_CASES = [("cut1", s, r, g, None) for s, r, g in CUT1_CASES] + [("rs", s, False, RANGE, b) for s, b in RS_CASES]


def case_id(case):
    kind, size, rot, box_range, box_set = case
    what = "x".join(map(str, box_range)) if kind == "cut1" else "default" if box_set is None else "%dboxes" % len(box_set)
    return "%s-%s%s-%s" % (kind, "x".join(map(str, size)), "-rot" if rot else "", what)


def pool_len(kind, size, box_range=RANGE, box_set=None):
    W, L, H = size
    if kind == "cut1":
        return W * L * H // (box_range[0] * box_range[1] * box_range[2]) + 3
    return sequences.rs_stream_pool_len(size, box_set)


@functools.lru_cache(maxsize=None)
def statement(kind, size, rot, seed, sid, k, box_range=RANGE, box_set=None, length=None):
    """The statement's sequence (box_set hashable: a tuple of tuples, or None).  An RS sequence has no end: `length` items of
    it, by default what the shortest ring row holds."""
    if kind == "cut1":
        return tuple(sequences.cut1_stream_sequence(size, box_range, seed, sid, k, rot))
    return tuple(sequences.rs_stream_sequence(size, box_set, seed, sid, k, length if length is not None else pool_len(kind, size, box_set=box_set) - 3))


def fits(size, box):
    """What the RS refill asks of a drawn box: no zero side, not higher than the bin, its footprint inside in one orientation."""
    (W, L, H), (x, y, z) = size, box
    return min(x, y, z) >= 1 and z <= H and ((x <= W and y <= L) or (x <= L and y <= W))


@functools.lru_cache(maxsize=None)
def ring_items(kind, size, rot, seed, sid, k, box_range=RANGE, box_set=None, T=None):
    """(the T - 3 items a ring row of T entries holds for episode k of stream sid, terminator padding included; whether the
    sequence counts as cut short)."""
    T = T if T is not None else pool_len(kind, size, box_range, box_set)
    seq = statement(kind, size, rot, seed, sid, k, box_range, box_set, T - 3 if kind == "rs" else None)
    if kind == "rs":
        good = [fits(size, b) for b in seq]
        return tuple(b if g else tuple(size) for b, g in zip(seq, good)), not all(good)
    return tuple(seq[:T - 3]) + (tuple(size),) * max(0, T - 3 - len(seq)), len(seq) > T - 3


def statement_pool(kind, size, rot, seed, base, E, K, box_range=RANGE, box_set=None, pool_len_=None):
    """uint8 [E K][T][4]: row e + k E = the statement's sequence for (seed, base + e, k), as a ring row of pool_len_ entries
    holds it."""
    T = pool_len_ if pool_len_ is not None else pool_len(kind, size, box_range, box_set)
    seqs = [ring_items(kind, size, rot, seed, base + e, k, box_range, box_set, T)[0] for k in range(K) for e in range(E)]
    return sequences.pad_pool([list(s) for s in seqs], size, T - 2)


def lock_step_check(oracle, stream_env, kind, size, rot, E, base, seed, steps, box_range=RANGE, box_set=None, fail=0.15, pool_len_=None,
                    played=None):
    """stream_env: reset() -> (obs, mask), step(actions) -> dict of KEYS (numpy), episodes() -> int array [E].  Steps it with
    uniform-feasible actions and `fail` of them replaced by an infeasible one (bins race through their episodes), then replays
    the same actions on the pool-mode env and compares every step.  pool_len_: the ring's, where its rows are shorter than the
    longest sequence; played: a list that receives the stream env's outputs, step by step."""
    obs, mask = stream_env.reset()
    mask0 = mask
    rng = np.random.RandomState(seed)
    acts, outs = [], played if played is not None else []
    for t in range(steps):
        a = oracle.sample_feasible(mask, 5, t)
        a[rng.rand(E) < fail] = -1
        r = stream_env.step(a)
        acts.append(a)
        outs.append(r)
        mask = r["mask"]
    episodes = np.asarray(stream_env.episodes())
    assert int(episodes.min()) >= 2, "every bin must get through several episodes"
    pool = statement_pool(kind, size, rot, seed, base, E, int(episodes.max()) + 3, box_range, box_set, pool_len_)
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


def expected_ring(kind, size, rot, seed, base, E, depth, gen_next, have, box_range=RANGE, box_set=None, pool_len_=None, bins=None):
    """{(row, entry): item} for every ring entry the statement predicts: rows of episodes have[e] .. gen_next[e] - 1 of every
    bin (`have` [E]: the bin's first episode still in the ring; `bins`: only these), their look-ahead entries where the row
    they repeat has been generated.  A row of the ring's pool_len_ entries holds the first pool_len_ - 3 items, then the
    terminator."""
    T = pool_len_ if pool_len_ is not None else pool_len(kind, size, box_range, box_set)
    want = {}
    for e in (range(E) if bins is None else bins):
        for k in range(int(have[e]), int(gen_next[e])):
            row = (k % depth) * E + e
            items = ring_items(kind, size, rot, seed, base + e, k, box_range, box_set, T)[0]
            for j in range(T - 2):
                want[(row, 2 + j)] = items[j] if j < T - 3 else tuple(size)
            for ahead, entry, item in ((1, 0, 1), (2, 1, 0)):
                if k + ahead < gen_next[e]:
                    nxt = ring_items(kind, size, rot, seed, base + e, k + ahead, box_range, box_set, T)[0]
                    want[(row, entry)] = nxt[item] if item < T - 3 else tuple(size)
    return want


def expected_overflow(kind, size, rot, seed, base, E, gen_next, box_range=RANGE, box_set=None, pool_len_=None, first=None):
    """Sequences the statement says were cut short among all generated so far: episodes first[e] (0) .. gen_next[e] - 1 of every
    bin -- the counter is cumulative, and a sequence is generated once."""
    T = pool_len_ if pool_len_ is not None else pool_len(kind, size, box_range, box_set)
    return sum(ring_items(kind, size, rot, seed, base + e, k, box_range, box_set, T)[1]
               for e in range(E) for k in range(int(first[e]) if first is not None else 0, int(gen_next[e])))


def ring_check(pool, gen_next, episode, kind, size, rot, seed, base, depth, box_range=RANGE, box_set=None, bins=None):
    """pool: the ring, uint8 [depth E][pool_len][4] (numpy); gen_next, episode: int [E].  Every entry the statement predicts
    (all pool_len - 2 behind the look-ahead entries of every row, and the look-ahead entries whose row exists), byte 3 of every
    entry is 0, gen_next == episode + depth.  `bins`: compare the rows of these bins only; `pool` is then ring[ring_rows(...)],
    the rows of those bins alone."""
    pool, gen_next, episode = np.asarray(pool), np.asarray(gen_next).astype(np.int64), np.asarray(episode).astype(np.int64)
    E, T = gen_next.shape[0], pool.shape[1]
    assert pool.shape == (depth * (E if bins is None else len(bins)), T, 4)
    np.testing.assert_array_equal(gen_next, episode + depth)
    want = expected_ring(kind, size, rot, seed, base, E, depth, gen_next, np.maximum(gen_next - depth, 0), box_range, box_set, T, bins)
    assert len(want) >= (E if bins is None else len(bins)) * depth * (T - 2)
    where = np.array(list(want.keys()), np.int64)
    items = np.array(list(want.values()), np.int64)
    if bins is not None:                                # ring row slot E + e is row slot len(bins) + (place of e in bins) of `pool`
        place = {int(r): i for i, r in enumerate(ring_rows(E, depth, bins))}
        where[:, 0] = [place[int(r)] for r in where[:, 0]]
    got = pool[where[:, 0], where[:, 1], :3].astype(np.int64)
    wrong = np.flatnonzero((got != items).any(1))
    assert wrong.size == 0, "%d of %d entries differ; the first: (row, entry) %r holds %r, the statement says %r" % (
        wrong.size, len(want), tuple(where[wrong[0]]), tuple(got[wrong[0]]), tuple(items[wrong[0]]))
    assert (pool[:, :, 3] == 0).all()
    return len(want)


def ring_rows(E, depth, bins):
    """The ring rows of `bins`, slot by slot."""
    return np.array([slot * E + e for slot in range(depth) for e in bins], np.int64)


def race_bins(oracle, env, E, steps=12, fail=0.3, seed=2):
    """`steps` lock-steps of uniform-feasible actions with `fail` of them replaced by an infeasible one: the bins end up at
    different episodes.  env as in lock_step_check."""
    obs, mask = env.reset()
    rng = np.random.RandomState(seed)
    for t in range(steps):
        a = oracle.sample_feasible(mask, 1, t)
        a[rng.rand(E) < fail] = -1
        mask = env.step(a)["mask"]


def bad_box_set(size=(10, 10, 10)):
    """About 400 boxes for a bin of `size`, three of which the RS refill must play as the terminator: a zero side, z > H, and a
    footprint too long in both orientations."""
    W, L, H = size
    r = np.random.RandomState(400)
    boxes = r.randint(2, 6, size=(400, 3))
    boxes[17] = (0, 3, 3)
    boxes[200] = (3, 3, H + 1)
    boxes[399] = (max(W, L) + 1, max(W, L) + 2, 2)
    return tuple(tuple(int(v) for v in b) for b in boxes)


def box_set_array(box_set):
    """uint8 [n][4] = (x, y, z, 0), as bpp_stream_refill_rs reads it -- without the checks of sequences.check_box_set."""
    out = np.zeros((len(box_set), 4), np.uint8)
    out[:, :3] = np.asarray(box_set, np.int64)
    return out
