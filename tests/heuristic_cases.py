"""TEST INFRASTRUCTURE ONLY -- inputs and checks of the lowest-top heuristic (include/bpp_heuristic.h), shared by
tests/test_heuristic.py (the product kernel on the SIMT emulator, host pointers) and tests/test_gpu_heuristic.py (the device).
The expected action is always oracle.policies.lowest_top_actions computed here, the comparison always assert_array_equal."""
import ctypes
import mmap
import os

import numpy as np

from bpp_amd import _lib
from oracle import policies

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BADARG = -1
RULES = ("lowest_top", "lowest_top_plain")
BIG = int(policies._BIG)
GUARD = 8
CANARY64, CANARY32 = np.int64(-0x5a5a5a5a5a5a5a5b), np.int32(-0x5a5a5a5b)

# every geometry of the edge cases: ((W, L, H), rotation)
GEOMS = [((10, 10, 10), False), ((10, 10, 10), True), ((20, 20, 20), True), ((7, 13, 8), True), ((5, 4, 6), False), ((1, 1, 3), False),
         ((4, 4, 255), False), ((32, 32, 10), False)]
# the kernel takes 16 lanes per bin up to A = 128 and a wave per bin beyond: A = 128 in four shapes (path 0), 129 and 130 (path 1);
# the largest M and LDS layout (32 x 32 with rotation); strips, where one side of the item can exceed the bin's other dimension;
# heights and z at 255 on the wave-per-bin path
GEOMS += [((8, 16, 10), True), ((16, 8, 10), False), ((128, 1, 5), True), ((1, 128, 5), True), ((3, 43, 6), True), ((43, 3, 6), False),
          ((10, 13, 9), True), ((32, 32, 10), True), ((255, 4, 12), True), ((4, 255, 12), True), ((1, 255, 4), True), ((12, 12, 255), True)]
GEOM_IDS = ["%dx%dx%d%s" % (s + ("r" if r else "",)) for s, r in GEOMS]
BATCHES = (1, 3, 63, 65, 257)
# geometries of the batch-size tests and of the carved-rows / top = NULL tests, the first three of each from the outset
BATCH_GEOMS = [((10, 10, 10), True), ((20, 20, 20), True), ((7, 13, 8), True), ((8, 16, 10), True), ((3, 43, 6), True), ((32, 32, 10), True)]
BATCH_IDS = ["10r", "20r", "7x13r", "8x16r", "3x43r", "32r"]
CARVED_GEOMS = [((10, 10, 10), True), ((20, 20, 20), False), ((5, 4, 6), False), ((8, 16, 10), True), ((255, 4, 12), True)]
CARVED_IDS = ["10r", "20", "5x4", "8x16r", "255x4r"]
# the recorded deep states: name -> (rows, then the issue's four bounds: share of rows with more than one tied entry, share of rows
# where the smooth rule picks another action than the plain one, all-ones fallback rows, most tied entries on one row)
DEEP = {"rollout_deep_cut2_10": (1920, 0.80, 0.30, 10, 81), "rollout_deep_cut2_10_rot": (1920, 0.80, 0.30, 10, 162),
        "rollout_deep_cut2_20": (1680, 0.80, 0.30, 10, 342)}
# closed loops: (size, rotation, bins, lock-steps, least episodes, a completely packed bin is asserted)
LOOPS = [((10, 10, 10), True, 64, 60, 100, True), ((20, 20, 20), False, 16, 150, 10, False), ((7, 13, 8), True, 33, 40, 40, True)]


def dims(size, rotation):
    W, L, H = (int(v) for v in size)
    return W, L, H, W * L, W * L * (1 + int(bool(rotation)))


# ------------------------------------------------------------------------------------------------------------------ the oracle
def keys(obs, mask, size, rotation):
    """int64 [n, M]: K(m) of the header -- top, BIG (on, out of range), BIG + 1 (off)."""
    top, _, _ = policies.window_tops(obs, size, rotation)
    return np.where(np.asarray(mask) > 0.5, top, BIG + 1)


def expected(obs, mask, size, rotation, rule):
    """(action int64 [n], top int32 [n]) of the oracle."""
    act = policies.lowest_top_actions(obs, mask, size, rotation, smooth=(rule == "lowest_top"))
    best = keys(obs, mask, size, rotation).min(axis=1)
    return act, np.where(best < BIG, best, -1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------- inputs
def make_obs(h, item, size):
    """One observation row: plane 0 the heights, planes 1 .. 3 the item's sides broadcast."""
    W, L, H, A, _ = dims(size, False)
    row = np.empty(4 * A, np.float32)
    row[:A] = np.asarray(h, np.float32).reshape(A)
    for k in range(3):
        row[(k + 1) * A:(k + 2) * A] = float(item[k])
    return row


def feasible_mask(obs, size, rotation):
    """The env's kind of mask for a row: on where the item lies inside the bin and its top stays within H; all ones where nothing is."""
    H = int(size[2])
    top, _, _ = policies.window_tops(obs[None], size, rotation)
    m = (top[0] <= H).astype(np.float32)
    return m if m.any() else np.ones_like(m)


def edge_rows(size, rotation, seed=0):
    """(names, obs float32 [R, 4A], mask float32 [R, M]): the edge cases of one geometry."""
    W, L, H, A, M = dims(size, rotation)
    rng = np.random.RandomState(seed + 1000 * W + L)
    rows = []

    def add(name, h, item, mask=None):
        o = make_obs(h, item, size)
        rows.append((name, o, feasible_mask(o, size, rotation) if mask is None else np.asarray(mask, np.float32)))

    ones, zeros = np.ones(M, np.float32), np.zeros(M, np.float32)
    small = (max(1, W // 3), max(1, L // 2), max(1, min(H, 255) // 4))
    add("empty bin: everything ties", np.zeros((W, L)), small)
    add("full bin, the terminator as item", np.full((W, L), H), (W, L, H), ones)
    for k in range(3):      # low heights: many ties; then the whole range of heights
        hi = (2, 3, H)[k]
        add("random heights 0..%d, random mask" % hi, rng.randint(0, hi + 1, (W, L)), (rng.randint(1, W + 1), rng.randint(1, L + 1), rng.randint(1, H + 1)),
            rng.randint(0, 2, M))
    add("random heights, feasibility mask", rng.randint(0, max(1, H // 2) + 1, (W, L)), (max(1, W // 4), max(1, L // 3), 1))
    add("mask all off", rng.randint(0, H + 1, (W, L)), small, zeros)
    item = (W, L, 1)
    inrange = policies.window_tops(make_obs(np.zeros((W, L)), item, size)[None], size, rotation)[0][0] < BIG
    if inrange.all():
        item = (W + 1, L, 1)
        inrange = np.zeros(M, bool)
    add("mask on only at out-of-range entries", rng.randint(0, H + 1, (W, L)), item, ~inrange)
    add("item wider than the bin", rng.randint(0, 3, (W, L)), (W + 1, 1, 1), ones)
    add("item longer than the bin", rng.randint(0, 3, (W, L)), (1, L + 1, 2), ones)
    add("item with a zero side", rng.randint(0, 3, (W, L)), (0, min(2, L), 1), ones)
    add("heights and z at their largest", np.full((W, L), min(H, 255)), (1, 1, min(H, 255)), ones)
    if rotation:
        s = max(1, min(W, L) // 2)
        add("x = y: the halves tie, the unrotated one wins", np.zeros((W, L)), (s, s, 1))
        add("x = y on random heights", rng.randint(0, 3, (W, L)), (s, s, 1), ones)
        h = np.full((W, L), H)      # only row 0 is free: the item (W, 1) fits as a row strip (rotated) and never as a column strip
        h[0] = 0
        add("only the rotated footprint fits", h, (W, 1, 1))
        h = np.full((W, L), max(0, H - 1))
        h[0] = 0
        add("index A on and best", h, (W, 1, 1), ones)
    names, obs, mask = zip(*rows)
    return list(names), np.stack(obs), np.stack(mask)


def random_rows(size, rotation, n, seed):
    """n rows of low random heights (many ties) under the feasibility mask."""
    W, L, H, A, M = dims(size, rotation)
    rng = np.random.RandomState(seed)
    obs = np.stack([make_obs(rng.randint(0, min(H, 3) + 1, (W, L)), (rng.randint(1, max(1, W // 2) + 1), rng.randint(1, max(1, L // 2) + 1), 1), size)
                    for _ in range(n)])
    return obs, np.stack([feasible_mask(o, size, rotation) for o in obs])


def batch_rows(size, rotation, n, seed=5):
    """n rows: the edge rows first, random rows behind them."""
    _, obs, mask = edge_rows(size, rotation)
    if n > obs.shape[0]:
        more = random_rows(size, rotation, n - obs.shape[0], seed)
        obs, mask = np.concatenate([obs, more[0]]), np.concatenate([mask, more[1]])
    return np.ascontiguousarray(obs[:n]), np.ascontiguousarray(mask[:n])


def garbage_rows(size, rotation, seed=3):
    """Rows no contract covers: NaN, infinities and 1e9 in every plane and in the mask, alone and mixed."""
    W, L, H, A, M = dims(size, rotation)
    rng = np.random.RandomState(seed)
    vals = np.array([np.nan, np.inf, -np.inf, 1e9, -1e9, 0.0, 1.0, 3.0, 255.0, 256.0, 1e-30, -0.0, 0.5], np.float32)
    obs, mask = [], []
    for v in vals[:5]:
        obs.append(np.full(4 * A, v, np.float32)), mask.append(np.full(M, v, np.float32))
        good = make_obs(rng.randint(0, 3, (W, L)), (1, 1, 1), size)
        for plane in range(4):      # one plane of garbage in an otherwise sound row, under a mask that is all on
            o = good.copy()
            o[plane * A:(plane + 1) * A] = v
            obs.append(o), mask.append(np.ones(M, np.float32))
        obs.append(good), mask.append(np.full(M, v, np.float32))
    for _ in range(12):
        obs.append(vals[rng.randint(0, len(vals), 4 * A)]), mask.append(vals[rng.randint(0, len(vals), M)])
    return np.stack(obs), np.stack(mask)


def deep_rows(g):
    """(obs [T E, 4A], mask [T E, M], recorded actions [T E]) of a rollout_deep_* recording: obs0 / mask0, then obs[:-1] / mask[:-1]."""
    obs = np.concatenate([g["obs0"][None], g["obs"][:-1]]).astype(np.float32)
    mask = np.concatenate([g["mask0"][None], g["mask"][:-1]]).astype(np.float32)
    return obs.reshape(-1, obs.shape[-1]), mask.reshape(-1, mask.shape[-1]), g["actions"].reshape(-1).astype(np.int64)


def check_deep(name, g, run):
    """Test 1 for one recording: run(obs, mask, size, rotation, rule) -> (action, top)."""
    rows, tied_share, differ_share, fallbacks, most = DEEP[name]
    size, rotation = tuple(int(v) for v in g["size"]), bool(g["rotation"])
    obs, mask, recorded = deep_rows(g)
    assert obs.shape[0] == rows
    K = keys(obs, mask, size, rotation)
    best = K.min(axis=1)
    tied = np.where(best < BIG, (K == best[:, None]).sum(axis=1), 0)
    fallback = (mask > 0.5).all(axis=1)        # nothing was feasible: the env hands out a mask that is all ones
    want = {r: expected(obs, mask, size, rotation, r) for r in RULES}
    differ = want["lowest_top"][0] != want["lowest_top_plain"][0]
    print("%s: %d rows, %.1f %% tied, %.1f %% smooth != plain, %d fallback rows, most ties %d, recorded == oracle on %.2f %%"
          % (name, rows, 100 * (tied > 1).mean(), 100 * differ.mean(), int(fallback.sum()), int(tied.max()),
             100 * (recorded == want["lowest_top"][0]).mean()))
    assert (tied > 1).mean() >= tied_share and differ.mean() >= differ_share and fallback.sum() >= fallbacks and tied.max() >= most
    assert (recorded == want["lowest_top"][0]).mean() >= 0.98       # the remainder is the recorder's p_random
    for r in RULES:
        act, top = run(obs, mask, size, rotation, r)
        np.testing.assert_array_equal(act, want[r][0], err_msg="%s %s" % (name, r))
        np.testing.assert_array_equal(top, want[r][1], err_msg="%s %s top" % (name, r))


def check_rows(run, obs, mask, size, rotation, names=None):
    """Both rules on the rows, as ONE call each, against the oracle."""
    for r in RULES:
        want = expected(obs, mask, size, rotation, r)
        act, top = run(obs, mask, size, rotation, r)
        bad = np.flatnonzero(act != want[0])
        np.testing.assert_array_equal(act, want[0], err_msg="%s %s: rows %s" % (size, r, [names[i] if names else i for i in bad[:5]]))
        np.testing.assert_array_equal(top, want[1])


def check_batches(run, size, rotation):
    """check_rows at every batch size of BATCHES.  batch_rows(n) is the first n rows of batch_rows(max): the oracle runs once, on the
    largest batch, and every smaller batch is held to its first rows."""
    obs, mask = batch_rows(size, rotation, max(BATCHES))
    want = {r: expected(obs, mask, size, rotation, r) for r in RULES}
    for n in BATCHES:
        o, m = np.ascontiguousarray(obs[:n]), np.ascontiguousarray(mask[:n])
        for r in RULES:
            act, top = run(o, m, size, rotation, r)
            np.testing.assert_array_equal(act, want[r][0][:n], err_msg="%s %s: %d rows" % (size, r, n))
            np.testing.assert_array_equal(top, want[r][1][:n])


def check_independence(run, size, rotation):
    """A row gives the same action alone, first, in the middle and last of a batch."""
    obs, mask = batch_rows(size, rotation, 70)
    whole = run(obs, mask, size, rotation, "lowest_top")[0]
    for r in (0, 11, 69):
        alone = run(obs[r:r + 1], mask[r:r + 1], size, rotation, "lowest_top")[0]
        for at in (0, 33, 69):
            o, m = obs.copy(), mask.copy()
            o[at], m[at] = obs[r], mask[r]
            moved = run(o, m, size, rotation, "lowest_top")[0]
            assert moved[at] == alone[0] == whole[r], (r, at)
            keep = np.arange(70) != at
            np.testing.assert_array_equal(moved[keep], whole[keep])


def oracle_loop(orc, size, rotation, bins, steps, act):
    """`steps` lock-steps of orc.OracleEnv under act(obs, mask) -> (actions [steps, bins], final heightmaps, episodes, full bins,
    fallback rows); pool: sequences.cut2_pool(size, 32, seed=1)."""
    from bpp_amd import sequences
    env = orc.OracleEnv(sequences.cut2_pool(size, 32, seed=1), size, rotation, bins)
    obs, mask = env.reset()
    actions, episodes, full, fallbacks = [], 0, 0, 0
    for _ in range(steps):
        a = act(obs, mask)
        fallbacks += int((mask > 0.5).all(axis=1).sum())
        out = env.step(a)
        actions.append(a)
        episodes += int(out["done"].sum())
        full += int((out["done"].astype(bool) & (out["ratio"] == 1.0)).sum())
        obs, mask = out["obs"], out["mask"]
    return np.stack(actions), env.hmap.copy(), episodes, full, fallbacks


def oracle_heuristic(size, rotation):
    return lambda obs, mask: policies.lowest_top_actions(obs, mask, size, rotation)


# ------------------------------------------------------------------------------------------------- a library with host pointers
def bind(L):
    return _lib.bind_heuristic(L)


def info(L, size, rotation, n):
    return _lib.heuristic_info(size, rotation, n, L)


def call(L, obs, stride, mask, n, W, Ln, rotation, rule, action, top):
    """bpp_heuristic_act with raw addresses (None = NULL)."""
    return L.bpp_heuristic_act(obs, stride, mask, n, W, Ln, rotation, rule, action, top, None)


def host_runner(L, want_top=True):
    """run(obs, mask, size, rotation, rule) on a library that takes host pointers (the emulator): obs may be a row view with unit
    inner stride; the outputs lie between guard words, which must be intact."""
    def run(obs, mask, size, rotation, rule):
        W, Ln, H, A, M = dims(size, rotation)
        assert obs.dtype == np.float32 and obs.strides[1] == 4 and mask.dtype == np.float32 and mask.flags.c_contiguous
        n = obs.shape[0]
        stride = obs.strides[0] // 4 if n > 1 else obs.shape[1]
        act = np.full(n + 2 * GUARD, CANARY64, np.int64)
        top = np.full(n + 2 * GUARD, CANARY32, np.int32)
        rc = call(L, obs.ctypes.data, stride, mask.ctypes.data, n, W, Ln, int(bool(rotation)), _lib.HEURISTIC_RULES[rule],
                  act[GUARD:].ctypes.data, top[GUARD:].ctypes.data if want_top else None)
        assert rc == 0, L.bpp_last_error()
        for buf, canary in ((act, CANARY64), (top, CANARY32)):
            assert (buf[:GUARD] == canary).all() and (buf[GUARD + n:] == canary).all(), "guard words overwritten"
        if not want_top:
            assert (top == CANARY32).all()
        return act[GUARD:GUARD + n].copy(), top[GUARD:GUARD + n].copy()
    return run


class Fenced(object):
    """A copy of an array (float32 unless told otherwise) that ends exactly where an inaccessible page begins: a read past its end
    is a host fault.  tests/test_ppo.py fences the gather's source and indices with it as well."""

    def __init__(self, arr, dtype=np.float32):
        arr = np.ascontiguousarray(arr, dtype)
        page = mmap.PAGESIZE
        size = (arr.nbytes + page - 1) // page * page
        self.map = mmap.mmap(-1, size + page)
        base = ctypes.addressof(ctypes.c_char.from_buffer(self.map))
        libc = ctypes.CDLL(None, use_errno=True)
        libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        if libc.mprotect(base + size, page, 0) != 0:
            raise OSError(ctypes.get_errno(), "mprotect")
        self.array = np.frombuffer(self.map, arr.dtype, arr.size, size - arr.nbytes).reshape(arr.shape)
        self.array[...] = arr


def refusals(L):
    """Every refusal of the header, with no device needed: the pointers are never followed."""
    o = np.zeros(4 * 100, np.float32).ctypes.data
    m = np.zeros(200, np.float32).ctypes.data
    a = np.zeros(1, np.int64).ctypes.data
    good = dict(obs=o, stride=400, mask=m, n=1, W=10, Ln=10, rotation=1, rule=0, action=a, top=None)
    bad = [dict(obs=None), dict(mask=None), dict(action=None), dict(n=0), dict(n=-3), dict(W=0), dict(Ln=0), dict(W=256, Ln=1, stride=4 * 256),
           dict(W=33, Ln=32, stride=4 * 33 * 32), dict(rotation=2), dict(rule=2), dict(rule=-1), dict(stride=399), dict(stride=0)]
    for change in bad:
        rc = call(L, **dict(good, **change))
        assert rc == BADARG, change
        assert L.bpp_last_error().decode().startswith("bpp_heuristic_act: "), L.bpp_last_error()
    out = (ctypes.c_int32 * 4)()
    for args in ((0, 10, 0, 1), (10, 10, 2, 1), (10, 10, 0, 0), (64, 32, 0, 1), (300, 1, 0, 1)):
        assert L.bpp_heuristic_act_info(*args, out) == BADARG, args
        assert L.bpp_last_error().decode().startswith("bpp_heuristic_act_info: ")
    assert L.bpp_heuristic_act_info(10, 10, 0, 1, None) == BADARG


def check_info(L):
    """The launch shape of every geometry: 16 lanes per bin up to A = 128, a wave per bin beyond; four waves per workgroup."""
    for size, rotation in GEOMS:
        W, Ln, H, A, M = dims(size, rotation)
        for n in (1, 3, 63, 65, 257, 65536):
            got = info(L, size, rotation, n)
            bpw = 4 if A <= 128 else 1
            per_bin = (A + 3) // 4 * 4 + (M + 3) // 4 * 4 + (2 * M + 3) // 4 * 4
            assert got == dict(bins_per_wave=bpw, lds_bytes=4 * bpw * per_bin, workgroups=(n + 4 * bpw - 1) // (4 * bpw), path=int(A > 128)), (size, n, got)
            assert got["lds_bytes"] <= 64 * 1024
    # both sides of the switch, and the largest layout, by name
    assert info(L, (8, 16, 10), True, 1)["path"] == 0 and info(L, (128, 1, 5), True, 1)["path"] == 0
    assert info(L, (3, 43, 6), True, 1)["path"] == 1 and info(L, (43, 3, 6), False, 1)["path"] == 1
    big = info(L, (32, 32, 10), True, 1)
    assert big["path"] == 1 and big["lds_bytes"] == 4 * (1024 + 2048 + 2 * 2048) <= 64 * 1024


# ------------------------------------------------------------------------------------------------------ a small bin enumerated
ENUM_SIZE = (3, 3, 4)
FOOTPRINTS = [(x, y) for x in (1, 2, 3) for y in (1, 2, 3)]


def enumerated_rows(levels):
    """Every heightmap of the 3 x 3 bin with heights below `levels`, rotation on, the mask all ones, items (x, y, 1).
    levels = 3: the 3^9 = 19 683 maps, map i with footprint number i mod 9.  levels = 2: the 2^9 maps times all nine footprints.
    -> (obs [n, 36], mask [n, 18], least share of rows on which the two rules must differ, from the oracle alone)."""
    maps = (np.arange(levels ** 9)[:, None] // levels ** np.arange(9)[None, :]) % levels
    if levels == 3:
        item = np.arange(len(maps)) % 9
    else:
        maps, item = np.repeat(maps, 9, axis=0), np.tile(np.arange(9), len(maps))
    fp = np.array(FOOTPRINTS)[item]
    obs = np.empty((len(maps), 36), np.float32)
    obs[:, :9] = maps
    obs[:, 9:18], obs[:, 18:27], obs[:, 27:] = fp[:, :1], fp[:, 1:], 1.0
    return obs, np.ones((len(maps), 18), np.float32), {3: 0.25, 2: 0.30}[levels]


def check_enumerated(run, levels):
    """Both rules on the whole enumeration, one call each; before that, from the oracle alone, that the smooth rule decides
    otherwise than the plain one on the stated share of rows (so the score R(m) - R(h) cannot go unexercised)."""
    obs, mask, share = enumerated_rows(levels)
    want = {r: expected(obs, mask, ENUM_SIZE, True, r) for r in RULES}
    differ = (want["lowest_top"][0] != want["lowest_top_plain"][0]).mean()
    print("3x3 bin, heights below %d: %d rows, smooth != plain on %.1f %%" % (levels, obs.shape[0], 100 * differ))
    assert differ >= share
    for r in RULES:
        act, top = run(obs, mask, ENUM_SIZE, True, r)
        np.testing.assert_array_equal(act, want[r][0], err_msg="enumerated, %s" % r)
        np.testing.assert_array_equal(top, want[r][1])
