"""The endless device-generated supply of the reference's other two item generators, CUT-1 and RS
(include/bpp_stream_kinds.h), on the CPU: the Python statements (sequences.cut1_stream_sequence / rs_stream_sequence) against
the exact generators' distributions, and the product's refill kernels -- compiled for the host SIMT emulator -- against the
statements: lock-step by lock-step through a pool-mode env of the C restatement (tests/stream_kind_cases.py), entry by entry
in the ring (at every box range and box set of that module; with rows too short and boxes that do not fit, where the overflow
count is the statement's), through a clone, and every refusal of the host entry points."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from bpp_amd import _lib, sequences

import stream_kind_cases as cases
from stream_kind_cases import RANGE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -1
SIZE = (10, 10, 10)


# ---- the statements ---------------------------------------------------------------------------------------------------------
class _Coin(object):
    """np.random.rand() of the exact generator, from Python's random (any fair coin serves the comparison)."""

    def __init__(self, rng):
        self.rng = rng

    def rand(self):
        return self.rng.random()


def _exact_cut1(seed, rot):
    r = random.Random(seed)
    return sequences.cut1_sequence(SIZE, RANGE, r, rot, _Coin(random.Random(seed + 7)) if rot else None)


@pytest.mark.parametrize("rot", [False, True])
def test_cut1_statement_has_the_exact_generators_distribution(rot):
    """2 000 sequences each: the counter statement, the exact generator, a second exact sample (the noise floor).  Measured:
    total variation counter / exact 0.026 against 0.027 exact / exact for all items, 0.103 against 0.089 for first items."""
    N = 2000
    a = [sequences.cut1_stream_sequence(SIZE, RANGE, 99, g, 0, rot) for g in range(N)]
    b = [_exact_cut1(1000 + g, rot) for g in range(N)]
    c = [_exact_cut1(50000 + g, rot) for g in range(N)]
    assert all(sum(x * y * z for x, y, z in s) == 1000 for s in a)                     # every sequence fills the bin exactly
    la, lb = np.array([len(s) for s in a]), np.array([len(s) for s in b])
    assert abs(la.mean() - lb.mean()) < 4 * np.sqrt(la.var() / N + lb.var() / N) + 1e-9

    def hist(seqs, first):
        h = np.zeros((6, 6, 6))
        for s in seqs:
            for x, y, z in (s[:1] if first else s):
                h[x, y, z] += 1
        return h / h.sum()
    for first in (False, True):
        tv_ab = 0.5 * np.abs(hist(a, first) - hist(b, first)).sum()
        tv_bc = 0.5 * np.abs(hist(b, first) - hist(c, first)).sum()
        print("rot=%s first=%s tv(counter, exact)=%.4f tv(exact, exact')=%.4f" % (rot, first, tv_ab, tv_bc))
        assert tv_ab < 1.5 * tv_bc + 0.003, (first, tv_ab, tv_bc)


def test_cut1_statement_swaps_as_often_as_the_exact_generator():
    """With rotation the first item is the piece with x / y swapped when the coin says so: the share of swapped first items
    (seen by cutting the same sequence without rotation -- the coin is the only draw that differs, and it comes after the
    pick) is within 4 standard errors of the exact generator's."""
    N = 2000

    def share(make):
        swapped = known = 0
        for g in range(N):
            with_rot, without = make(g, True)[0], make(g, False)[0]
            if without[0] != without[1]:                # a square footprint shows nothing
                known += 1
                assert with_rot in (without, (without[1], without[0], without[2]))
                swapped += with_rot != without
        return swapped / known, known
    pa, na = share(lambda g, rot: sequences.cut1_stream_sequence(SIZE, RANGE, 99, g, 0, rot))
    pb, nb = share(lambda g, rot: _exact_cut1(1000 + g, rot))
    print("swapped first items: counter %.4f of %d, exact %.4f of %d" % (pa, na, pb, nb))
    assert abs(pa - pb) < 4 * np.sqrt(pa * (1 - pa) / na + pb * (1 - pb) / nb)
    assert abs(pa - 0.5) < 4 * np.sqrt(0.25 / na)


def test_rs_statement_draws_the_boxes_uniformly():
    n = len(sequences.DEFAULT_BOX_SET)
    assert n == 64
    index = {b: i for i, b in enumerate(sequences.DEFAULT_BOX_SET)}
    counts = np.zeros(n)
    for g in range(500):                                # 500 rows of 128 items = 64 000 draws
        for b in sequences.rs_stream_sequence(SIZE, None, 3, g, g % 7, 128):
            counts[index[b]] += 1
    expect = counts.sum() / n
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print("chi-square over 64 boxes: %.1f" % chi2)
    assert counts.sum() == 64000 and chi2 < 63 + 5 * np.sqrt(126)


def test_statements_advance_the_draw_index_as_the_header_says():
    """choice over one axis is a draw; the coin is drawn only with rotation; an RS item is one draw."""
    rng = sequences.CounterRandom(5, 6, 7)
    seq = sequences.cut1_sequence(SIZE, RANGE, rng, False, None)
    rng2 = sequences.CounterRandom(5, 6, 7)
    seq2 = sequences.cut1_sequence(SIZE, RANGE, rng2, True, sequences._CounterCoin(rng2))
    assert rng2.n == rng.n + len(seq2) and len(seq) >= 8
    assert sequences.rs_stream_pool_len(SIZE) == 1000 // 8 + 3
    assert len(sequences.rs_stream_sequence(SIZE, None, 1, 2, 3, 125)) == 125


# ---- the emulated kernels -----------------------------------------------------------------------------------------------------
def bound_for_sizes(size):
    lo = max(1, min(size) // 2)
    return lo, 2 * lo - 1


def bind(emu):
    L = emu.lib()
    if not getattr(L, "_bpp_kinds_bound", False):
        _lib.bind_stream_kinds(L, emu.Batch, emu.StepOut, emu.Stream)
        L._bpp_kinds_bound = True
    return L


def kind_env(emu, kind, size, rot, E, base, seed, depth, refill, cache, box_range=RANGE, box_set=None, pool_len=None, **kw):
    """emu.OracleEnv over a ring whose refills are the kind's (the front-end's own refill() is CUT-2's)."""
    L = bind(emu)
    rg = _lib.box_range_arg(box_range)
    bs = sequences.check_box_set(size, box_set if kind == "rs" else [(1, 1, 1)])     # (CUT-1 hands no set to its refill)

    class KindEnv(emu.OracleEnv):
        def refill(self):
            if kind == "cut1":
                rc = L.bpp_stream_refill_cut1(ctypes.byref(self.stream), rg, int(rot), None)
            else:
                rc = L.bpp_stream_refill_rs(ctypes.byref(self.stream), bs.ctypes.data, bs.shape[0], None)
            emu._check(rc)
            self._since_refill = 0

        def episodes(self):
            return self.state["episode"].copy()

        def rollout(self, seed, step0, n):
            a = np.zeros(self.E, np.int64)
            self.refill()
            emu._check(L.bpp_rollout_uniform_stream_kind(ctypes.byref(self._b), ctypes.byref(self._o), a.ctypes.data, seed, step0, n,
                                                         ctypes.byref(self.stream), self.refill_every, _lib.STREAM_KINDS[kind], rg, int(rot),
                                                         bs.ctypes.data, bs.shape[0], None))
            return self.out, a

    spec = dict(bound=bound_for_sizes(size), seed=seed, depth=depth, refill_every=refill, rng="counter", cache=cache,
                pool_len=pool_len or cases.pool_len(kind, size, box_range, box_set))
    return KindEnv(None, size, rot, E, env_id_base=base, env_id_total=base + E + 3, stream=spec, **kw)


@pytest.mark.parametrize("kind", ["cut1", "rs"])
@pytest.mark.parametrize("size,rot,E,base,depth,refill,cache", [
    (SIZE, False, 70, 1000, 8, 4, True),
    (SIZE, False, 70, 1000, 8, 5, False),
    (SIZE, True, 33, 1000, 8, 4, True),
    (SIZE, False, 9, 2 ** 33 + 5, 8, 4, True),
    ((8, 12, 9), False, 20, 1000, 8, 5, False),         # the runtime-geometry step kernel
    (SIZE, False, 1, 1000, 8, 4, True),
    ((16, 6, 8), True, 5, 1000, 6, 3, False),           # a side of 16: pieces of two words
    ((18, 8, 7), False, 5, 1000, 6, 3, False),          # 126 pieces of two words: 32 lanes at work per wave
    ((25, 8, 5), False, 5, 1000, 6, 3, False)])        # a footprint of 200 cells
def test_emulated_rows_equal_the_statement(emu, oracle, kind, size, rot, E, base, depth, refill, cache):
    seed = 77
    env = kind_env(emu, kind, size, rot, E, base, seed, depth, refill, cache)
    episodes = cases.lock_step_check(oracle, env, kind, size, rot, E, base, seed, 64)
    assert int(env.overflow[0]) == 0
    assert int(env.gen_next.min()) > depth              # several refills generated something for every bin
    assert int(episodes.max()) >= 4


def check_ring(env, kind, size, rot, seed, base, depth, box_range=RANGE, box_set=None):
    return cases.ring_check(env.pool, env.gen_next, env.state["episode"], kind, size, rot, seed, base, depth, box_range, box_set)


@pytest.mark.parametrize("kind,rot", [("cut1", False), ("cut1", True), ("rs", False)])
def test_emulated_ring_rows_and_look_ahead_entries(emu, oracle, kind, rot):
    E, base, seed, depth = 70, 40, 11, 6
    env = kind_env(emu, kind, SIZE, rot, E, base, seed, depth, 2, False)
    check_ring(env, kind, SIZE, rot, seed, base, depth)     # the first refill: episodes 0 .. depth - 1
    cases.race_bins(oracle, env, E)                         # bins at different episodes; a refill every two lock-steps
    env.refill()
    assert len(set(env.gen_next.tolist())) > 2
    check_ring(env, kind, SIZE, rot, seed, base, depth)
    assert int(env.overflow[0]) == 0


@pytest.mark.parametrize("case", cases.KIND_CASES, ids=cases.case_id)
def test_emulated_ring_rows_equal_the_statement(emu, oracle, case):
    """Whole rows at every box range and box set of tests/stream_kind_cases.py, after the first refill and again with the bins
    at different episodes."""
    kind, size, rot, box_range, box_set = case
    E, base, seed, depth = 9 + cases.KIND_CASES.index(case) % 12, 40, 11, 6
    env = kind_env(emu, kind, size, rot, E, base, seed, depth, 2, False, box_range, box_set)
    check_ring(env, kind, size, rot, seed, base, depth, box_range, box_set)
    cases.race_bins(oracle, env, E)
    env.refill()
    assert len(set(env.gen_next.tolist())) > 2
    check_ring(env, kind, size, rot, seed, base, depth, box_range, box_set)
    assert int(env.overflow[0]) == 0


@pytest.mark.parametrize("case", [c for c in cases.KIND_CASES if c[0] == "cut1"], ids=cases.case_id)
def test_emulated_lock_steps_at_every_box_range(emu, oracle, case):
    kind, size, rot, box_range, _ = case
    E, base, seed = 9 + cases.KIND_CASES.index(case) % 12, 1000, 77
    env = kind_env(emu, kind, size, rot, E, base, seed, 6, 3, False, box_range)
    cases.lock_step_check(oracle, env, kind, size, rot, E, base, seed, 64, box_range)
    assert int(env.overflow[0]) == 0 and int(env.gen_next.min()) > 6


# ---- *s->overflow above zero ------------------------------------------------------------------------------------------------------
SHORT = 36          # a CUT-1 row of 36 entries holds 33 items; sequences at 10 x 10 x 10 under RANGE have 13 .. 39


def test_emulated_short_cut1_rows_are_cut_and_counted(emu, oracle):
    """Rows too short for some sequences: the row holds the statement's first 33 items and the terminator, the sequence
    counts once -- also after further refills (the counter is cumulative) -- and the step kernel plays the cut row to its
    terminator.  The statement alone: 11 of the first 120 sequences are longer."""
    E, base, seed, depth = 20, 40, 11, 6
    first = cases.expected_overflow("cut1", SIZE, False, seed, base, E, [depth] * E, pool_len_=SHORT)
    assert 0 < first < E * depth and first == 11
    env = kind_env(emu, "cut1", SIZE, False, E, base, seed, depth, 2, False, pool_len=SHORT)
    assert env.pool.shape[1] == SHORT
    check_ring(env, "cut1", SIZE, False, seed, base, depth)
    assert int(env.overflow[0]) == first
    cases.race_bins(oracle, env, E)
    env.refill()
    assert len(set(env.gen_next.tolist())) > 2
    check_ring(env, "cut1", SIZE, False, seed, base, depth)
    later = cases.expected_overflow("cut1", SIZE, False, seed, base, E, env.gen_next, pool_len_=SHORT)
    assert int(env.overflow[0]) == later > first
    # Uniform play puts 18 items at most into these bins, so at 33 items a row no bin reaches the terminator of a cut row.  At 9
    # items a row every sequence is cut, and bins do place all nine: the tenth is the terminator on both sides.
    for T, deepest in ((SHORT, None), (12, 9)):
        env, played = kind_env(emu, "cut1", SIZE, False, E, base, seed, depth, 2, False, pool_len=T), []
        cases.lock_step_check(oracle, env, "cut1", SIZE, False, E, base, seed, 64, fail=0, pool_len_=T, played=played)
        assert deepest is None or max(int(o["counter"].max()) for o in played) == deepest
    assert int(env.overflow[0]) == cases.expected_overflow("cut1", SIZE, False, seed, base, E, env.gen_next, pool_len_=12) == int(env.gen_next.sum())


def test_emulated_bad_rs_boxes_are_played_as_the_terminator_and_counted_per_sequence(emu):
    """BppVecEnv and check_box_set refuse such a set; the refill itself must play every bad draw as the terminator and count
    the row once, however many bad draws it has."""
    E, base, seed, depth = 20, 40, 11, 6
    bad = cases.bad_box_set(SIZE)
    rows = [cases.ring_items("rs", SIZE, False, seed, base + e, k, box_set=bad, T=128) for e in range(E) for k in range(depth)]
    n_bad = [sum(it == SIZE for it in items) for items, over in rows]
    assert 0 < sum(n > 0 for n in n_bad) < len(rows) and max(n_bad) > 1       # the statement alone: some rows, not all; per row != per item
    env = kind_env(emu, "rs", SIZE, False, E, base, seed, depth, 2, False)
    assert env.pool.shape[1] == 128 and int(env.overflow[0]) == 0
    env.gen_next[:] = 0                                     # every row is written again
    bs = cases.box_set_array(bad)
    emu._check(bind(emu).bpp_stream_refill_rs(ctypes.byref(env.stream), bs.ctypes.data, bs.shape[0], None))
    check_ring(env, "rs", SIZE, False, seed, base, depth, box_set=bad)
    assert sum(n > 0 for n in n_bad) == cases.expected_overflow("rs", SIZE, False, seed, base, E, env.gen_next, box_set=bad, pool_len_=128)
    assert int(env.overflow[0]) == sum(n > 0 for n in n_bad)


@pytest.mark.parametrize("kind", ["cut1", "rs"])
def test_emulated_clone_continues_the_sources_stream(emu, kind):
    """A cloned bin carries the source's stream id with its record: the copy plays the SOURCE's sequences."""
    import torch
    from bpp_amd.vec_env import copy_bin_records
    E, base, seed, depth = 6, 40, 5, 6
    NOOP = -2 ** 63
    env = kind_env(emu, kind, SIZE, False, E, base, seed, depth, 1, False, mask_rule=1)
    obs, mask = env.reset()
    A = 100
    for t in range(2):
        o = env.step(emu.sample_feasible(mask, 1, t, env_id_base=base))
        mask = o["mask"]
    assert not o["done"][0]
    hm, st = torch.from_numpy(env.hmap), torch.from_numpy(env.state.view(np.int32).reshape(E, 12))
    ring, mt, gn = torch.from_numpy(env.pool), torch.from_numpy(env._mt.view(np.int32).reshape(E, -1)), torch.from_numpy(env.gen_next)
    copy_bin_records(hm, st, torch.tensor([0]), torch.tensor([1]), ring=ring, mt=mt, gen_next=gn, depth=depth)
    for t in range(2 * depth):                          # the source burns through > depth episodes; everybody else waits
        a = np.full(E, NOOP, np.int64)
        a[0] = -1
        assert env.step(a)["done"][0]
    a = np.full(E, NOOP, np.int64)
    o = env.step(a)
    episode, cursor = 0, 2
    for k in range(45):
        seq = cases.statement(kind, SIZE, False, seed, base + 0, episode)
        want = seq[cursor] if cursor < len(seq) else SIZE
        assert tuple(int(o["obs"][1, (p + 1) * A]) for p in range(3)) == tuple(want), (k, episode, cursor)
        feasible = np.flatnonzero(o["mask"][1])
        a[1] = int(feasible[0]) if len(feasible) else -1
        o = env.step(a)
        episode, cursor = (episode + 1, 0) if o["done"][1] else (episode, cursor + 1)
    assert episode >= 2 and int(env.overflow[0]) == 0


@pytest.mark.parametrize("kind", ["cut1", "rs"])
def test_emulated_rollout_driver_equals_the_lock_steps_taken_one_by_one(emu, kind):
    E, base, seed = 40, 7, 3
    one = kind_env(emu, kind, SIZE, True, E, base, seed, 8, 4, True)
    two = kind_env(emu, kind, SIZE, True, E, base, seed, 8, 4, True)
    (obs, mask), _ = one.reset(), two.reset()
    r, ra = one.rollout(9, 0, 48)
    for t in range(48):
        a = emu.sample_feasible(mask, 9, t, env_id_base=base)
        o = two.step(a)
        mask = o["mask"]
    for k in cases.KEYS + ("ep_ret", "ep_len"):
        np.testing.assert_array_equal(r[k], o[k], err_msg=k)
    two.refill()                                        # the driver ends with a refill: both rings now hold the same episodes
    np.testing.assert_array_equal(one.pool, two.pool)
    np.testing.assert_array_equal(one.gen_next, two.gen_next)
    assert int(two.state["episode"].max()) >= 2


# ---- refusals, before any device is touched -------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["product", "emulated"])
def host(request):
    """(library handle, its bpp_stream / bpp_batch / bpp_step_out classes): the product library without a device, the emulated one."""
    if request.param == "product":
        _lib.build()
        return _lib.lib(), _lib.Stream, _lib.Batch, _lib.StepOut
    emu = request.getfixturevalue("emu")
    return bind(emu), emu.Stream, emu.Batch, emu.StepOut


def fake_stream(Stream, size=SIZE, E=64, depth=8, T=128, rng=_lib.STREAM_RNG_COUNTER, bound=None, ring=16):
    lo, hi = bound or bound_for_sizes(size)
    return Stream(E, depth, T, size[0], size[1], size[2], lo, hi, 0, 1, ring, 16, 16, 16, 16, None, rng, 0)


def test_every_refusal_names_its_function(host):
    lib, Stream, Batch, StepOut = host
    rg = _lib.box_range_arg

    def refused(rc, who, *words):
        msg = lib.bpp_last_error().decode()
        assert rc == BADARG and msg.startswith(who + ": "), (rc, msg)
        for w in words:
            assert w in msg, (w, msg)
        return True

    s = fake_stream(Stream)
    cut1, who = lib.bpp_stream_refill_cut1, "bpp_stream_refill_cut1"
    refused(cut1(None, rg(RANGE), 0, None), who, "NULL")
    refused(cut1(ctypes.byref(s), None, 0, None), who, "NULL")
    refused(cut1(ctypes.byref(fake_stream(Stream, ring=None)), rg(RANGE), 0, None), who, "NULL")
    refused(cut1(ctypes.byref(fake_stream(Stream, rng=_lib.STREAM_RNG_MT19937)), rg(RANGE), 0, None), who, "BPP_STREAM_RNG_COUNTER")
    refused(cut1(ctypes.byref(s), rg((2, 2, 6, 5, 5, 5)), 0, None), who, "low <= high")
    refused(cut1(ctypes.byref(s), rg((0, 2, 2, 5, 5, 5)), 0, None), who, "1 <= low")
    refused(cut1(ctypes.byref(s), rg((3, 2, 2, 4, 5, 5)), 0, None), who, "2 low - 1")
    refused(cut1(ctypes.byref(s), rg((11, 2, 2, 30, 5, 5)), 0, None), who, "below its low")
    refused(cut1(ctypes.byref(fake_stream(Stream, (10, 10, 12))), rg(RANGE), 0, None), who, "BPP_CUT1_MAX_PIECES")     # 150 pieces
    refused(cut1(ctypes.byref(fake_stream(Stream, (20, 20, 20))), rg(RANGE), 0, None), who)

    rs, who = lib.bpp_stream_refill_rs, "bpp_stream_refill_rs"
    refused(rs(None, 16, 64, None), who, "NULL")
    refused(rs(ctypes.byref(s), None, 64, None), who, "NULL")
    refused(rs(ctypes.byref(fake_stream(Stream, rng=_lib.STREAM_RNG_MT19937)), 16, 64, None), who, "BPP_STREAM_RNG_COUNTER")
    refused(rs(ctypes.byref(s), 16, 0, None), who, "box_set")
    refused(rs(ctypes.byref(s), 16, _lib.RS_MAX_SET + 1, None), who, "box_set")
    refused(rs(ctypes.byref(s), 18, 64, None), who, "misaligned")
    refused(rs(ctypes.byref(fake_stream(Stream, depth=3)), 16, 64, None), who, "depth")

    info, who = lib.bpp_stream_kinds_info, "bpp_stream_kinds_info"
    out = (ctypes.c_int32 * 4)()
    refused(info(None, 1, rg(RANGE), out), who, "NULL")
    refused(info(ctypes.byref(s), 1, rg(RANGE), None), who, "NULL")
    refused(info(ctypes.byref(s), 3, rg(RANGE), out), who, "kind")
    refused(info(ctypes.byref(fake_stream(Stream, (10, 10, 12))), 1, rg(RANGE), out), who, "BPP_CUT1_MAX_PIECES")

    roll, who = lib.bpp_rollout_uniform_stream_kind, "bpp_rollout_uniform_stream_kind"
    E = 64
    ring = Batch(E, 10, 10, 10, 0, 0, 8 * E, 128, 0, E, 16, 16, 48, None, _lib.POOL_RING, 0, None)
    static = Batch(E, 10, 10, 10, 0, 0, 64, 128, 0, E, 16, 16, 48, None, _lib.POOL_STATIC, 0, None)
    o = StepOut(16, 16)

    def call(batch=ring, out=o, actions=16, nsteps=3, stream=s, every=4, kind=1, box_range=RANGE, box_set=16, n_set=64):
        return roll(ctypes.byref(batch) if batch is not None else None, ctypes.byref(out) if out is not None else None, actions, 1, 0, nsteps,
                    ctypes.byref(stream) if stream is not None else None, every, kind, rg(box_range) if box_range else None, 0, box_set, n_set,
                    None)
    refused(call(batch=None), who, "NULL")
    refused(call(stream=None), who, "NULL")
    refused(call(actions=None), who, "NULL")
    refused(call(out=StepOut(16)), who, "NULL")
    refused(call(nsteps=-1), who, "nsteps")
    refused(call(kind=0), who, "kind")
    refused(call(batch=static), who, "ring pool")
    refused(call(every=6), who, "refill_every")
    refused(call(box_range=(2, 2, 6, 5, 5, 5)), who, "low <= high")
    refused(call(kind=2, n_set=0), who, "box_set")
    refused(call(stream=fake_stream(Stream, rng=_lib.STREAM_RNG_MT19937)), who, "BPP_STREAM_RNG_COUNTER")


def test_info_tells_the_form_of_a_refill(host):
    lib, Stream = host[0], host[1]
    info = lambda size, kind: _lib.stream_kinds_info(fake_stream(Stream, size), kind, RANGE, L=lib)      # noqa: E731
    assert info(SIZE, "cut1") == dict(lanes=64, lds_bytes=64 * (125 + 32) * 4, pieces=125, threads=64)
    assert info((8, 12, 9), "cut1") == dict(lanes=64, lds_bytes=64 * (108 + 27) * 4, pieces=108, threads=64)
    assert info((16, 6, 8), "cut1") == dict(lanes=64, lds_bytes=64 * (2 * 96 + 48) * 4, pieces=96, threads=64)
    assert info((18, 8, 7), "cut1") == dict(lanes=32, lds_bytes=32 * (2 * 126 + 63) * 4, pieces=126, threads=64)
    assert info(SIZE, "rs") == dict(lanes=64, lds_bytes=0, pieces=0, threads=64)
    # every geometry within the cap of the header fits the LDS of a workgroup, whatever its footprint
    assert info((16, 8, 8), "cut1") == dict(lanes=32, lds_bytes=32 * (2 * 128 + 64) * 4, pieces=128, threads=64)
    assert info((25, 8, 5), "cut1")["pieces"] == 125 and info((12, 12, 7), "cut1")["pieces"] == 126


def test_every_declared_symbol_is_exported():
    _lib.build()
    lib = _lib.lib()
    src = open(_lib.STREAM_KINDS_HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(bpp_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.STREAM_KIND_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    for macro, value in (("BPP_STREAM_KIND_CUT1", _lib.STREAM_KINDS["cut1"]), ("BPP_STREAM_KIND_RS", _lib.STREAM_KINDS["rs"]),
                         ("BPP_CUT1_MAX_PIECES", _lib.CUT1_MAX_PIECES),
                         ("BPP_RS_MAX_SET", _lib.RS_MAX_SET)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, src).group(1)) == value
    abi = re.sub(r"/\*.*?\*/", "", open(_lib.HDR).read(), flags=re.S)
    assert not set(names) & set(re.findall(r"\b(bpp_[a-z0-9_]+)\s*\(", abi))          # additive: nothing of it in bpp_abi.h
