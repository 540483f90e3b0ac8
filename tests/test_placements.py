"""Recorded packing plans (include/bpp_placements.h) without a GPU: the product kernels of csrc/bpp_placements.inl
compiled by g++ against the SIMT emulator, on host pointers.  The rollout fixtures replayed with note / bpp_step / commit against
the boxes the reference itself appended to space.boxes (tests/golden/placements_*.npz); the same against the live reference;
replay against the env's own heightmaps and against a numpy restatement at the edges; overflow between guard regions; subsets,
copy and gather; the refusals of the header on both libraries (the product library has no device here).  Helpers:
tests/placement_cases.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from bpp_amd import _lib
from oracle import ref_shims

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import placement_cases as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not ref_shims.available(), reason="reference tree not present")


@pytest.fixture(scope="module")
def emu_lib(emu):
    import emu_binding
    inl = os.path.join(ROOT, "online-3d-bpp-drl_amd", "csrc", "bpp_placements.inl")
    if os.path.getmtime(inl) > os.path.getmtime(emu.LIB):
        emu_binding.build(force=True)
    L = ctypes.CDLL(emu.LIB)
    _lib.bind_placements(L, batch=emu.Batch)
    _lib.bind_branch(L, batch=emu.Batch, step_out=emu.StepOut, stream=emu.Stream)
    L.bpp_last_error.restype = ctypes.c_char_p
    return L


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def passes(emu, emu_lib):
    """name -> the recorded pass over a fixture, made once and never modified: per lock-step the gathered running and finished
    plans, the replay of the running plans, and the env's heightmaps and state."""
    cache = {}

    def get(name):
        if name not in cache:
            g = pc.load_case(name)
            T, E = g["actions"].shape
            env = emu.EmuEnv(g["pool"], g["size"], g["rotation"], E)
            env.reset()
            log = pc.HostLog(emu_lib, env, pc.default_capacity(g["size"]))
            steps = []
            for t in range(T):
                out = log.step(g["actions"][t])
                assert np.array_equal(out["done"], g["done"][t]) and np.array_equal(out["counter"], g["counter"][t])
                run, fin = log.gather(False), log.gather(True)
                steps.append(dict(run=run, fin=fin, replay=pc.host_replay(emu_lib, run[0], run[1], g["size"]), hmap=env.hmap.copy(),
                                  state=env.state.copy()))
            cache[name] = (g, steps, log.overflow)
        return cache[name]
    return get


@pytest.mark.parametrize("name", pc.CASES)
def test_fixture_plans_equal_the_reference_boxes_after_every_lock_step(passes, name):
    g, steps, overflow = passes(name)
    T, E = g["actions"].shape
    exp = pc.ExpectedPlans(E, g["size"][1], pc.default_capacity(g["size"]))
    for t in range(T):
        exp.step(g["box"][t], g["done"][t])
        (run, cnt, ep), (fin, fcnt, fep) = steps[t]["run"], steps[t]["fin"]
        assert np.array_equal(cnt, exp.run_count) and np.array_equal(cnt, steps[t]["state"]["n_boxes"]), t
        assert run.tobytes() == exp.run.tobytes(), t                   # the running lists so far, zero from the count on
        assert np.array_equal(ep, exp.episode) and np.array_equal(ep, steps[t]["state"]["episode"]), t
        assert np.array_equal(fcnt, exp.fin_count) and np.array_equal(fep, exp.fin_episode), t
        assert fin.tobytes() == exp.fin.tobytes(), t                   # at every done: the list of the episode that ended
        d = g["done"][t].astype(bool)
        assert np.array_equal(fcnt[d], g["counter"][t][d])
    assert overflow == 0 and exp.dropped == 0
    rotated = {"rollout_cut2_10_rot": 1100, "rollout_deep_cut2_10_rot": 274, "rollout_wide_8x12x9_rot": 689, "rollout_short_5x4x6": 312}
    assert int((g["box"][:, :, 6] == 1).sum()) == rotated.get(name, 0)


def test_the_fixtures_hold_the_quirk_the_depth_and_the_action_out_of_range():
    g = pc.load_case("rollout_cut2_10_rot")
    assert int((g["actions"] == 100).sum()) == 41                      # a == A with rotation: not rotated, idx = A, outside the bin
    assert g["done"][g["actions"] == 100].all()
    assert pc.load_case("rollout_deep_cut2_20")["counter"].max() == 172 and pc.load_case("rollout_deep_cut2_10_rot")["counter"].max() == 31
    s = pc.load_case("rollout_short_5x4x6")
    assert s["counter"].max() == 21 and s["pool"].shape[1] == 6
    c = pc.load_case("rollout_cut2_10")
    assert int(((c["actions"] < 0) | (c["actions"] >= 100)).sum()) >= 1


@pytest.mark.parametrize("name", pc.CASES)
def test_replay_of_the_running_plans_gives_the_heightmaps_and_volumes(passes, name):
    g, steps, _ = passes(name)
    W, L, H = g["size"]
    for t, s in enumerate(steps):
        hmap, status, volume = s["replay"]
        assert (status == -1).all(), t
        assert hmap.reshape(len(status), -1).tobytes() == s["hmap"].tobytes(), t
        assert np.array_equal(volume, s["state"]["vol_sum"]), t


@needs_reference
@pytest.mark.parametrize("size,rot,seed", [((10, 10, 10), True, 5), ((6, 9, 7), False, 6)])
def test_plans_equal_the_live_reference_boxes(emu, emu_lib, size, rot, seed):
    """Recorded now: 4 bins, 60 lock-steps of uniform-feasible actions with some arbitrary ones, the reference's PackingGame beside
    the emulated step; after every lock-step every bin's plan is the reference's space.boxes / space.flags."""
    ref_shims.install()
    from envs.bpp0 import PackingGame
    from bpp_amd.placements import PackingPlans
    import torch
    rng = np.random.RandomState(seed)
    E, A = 4, size[0] * size[1]
    seqs = [[tuple(int(v) for v in rng.randint(1, 5, size=3)) for _ in range(30)] for _ in range(12)]
    pool = np.zeros((12, 31, 4), np.uint8)
    pool[:, :, :3] = size
    pool[:, :30, :3] = np.array(seqs)
    games = [PackingGame(box_creator=ref_shims.make_replay_creator([s + [size] for s in seqs], size, env_id=e, env_total=E), container_size=size,
                         enable_rotation=rot) for e in range(E)]
    for gm in games:
        gm.reset()
    env = emu.EmuEnv(pool, size, rot, E)
    _, mask = env.reset()
    log = pc.HostLog(emu_lib, env, 40)
    last = [None] * E
    for t in range(60):
        a = np.array([rng.randint(0, mask.shape[1]) if rng.rand() < 0.1 else rng.choice(np.flatnonzero(mask[e])) for e in range(E)], np.int64)
        out = log.step(a)
        mask = out["mask"].copy()
        rec, cnt, ep = log.gather(False)
        plans = PackingPlans(torch.from_numpy(rec.view(np.uint8).reshape(E, 40, 8)), torch.from_numpy(cnt), torch.from_numpy(ep), 0, size)
        frec, fcnt, fep = log.gather(True)
        fplans = PackingPlans(torch.from_numpy(frec.view(np.uint8).reshape(E, 40, 8)), torch.from_numpy(fcnt), torch.from_numpy(fep), 0, size)
        for e, gm in enumerate(games):
            _, _, done, _ = gm.step([int(a[e])])
            assert bool(done) == bool(out["done"][e])
            if done:
                last[e] = ([b.standardize() for b in gm.space.boxes], [bool(f) for f in gm.space.flags])
                gm.reset()
            assert plans.boxes(e) == [tuple(int(v) for v in b.standardize()) for b in gm.space.boxes], (t, e)
            assert plans.flags(e) == [bool(f) for f in gm.space.flags], (t, e)
            if last[e] is not None:
                assert fplans.boxes(e) == [tuple(int(v) for v in b) for b in last[e][0]] and fplans.flags(e) == last[e][1], (t, e)
            else:
                assert fcnt[e] == -1
    assert sum(l is not None for l in last) == E


@pytest.mark.parametrize("size", pc.EDGE_GEOMETRIES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("n", [1, 5, 67])
def test_replay_edges_equal_the_numpy_restatement(emu_lib, size, n):
    cap = 4 if size[0] * size[1] == 1 else 12
    records, count = pc.edge_plans(size, n, cap, seed=n + size[0])
    want = pc.replay_numpy(records, count, size)
    got = pc.host_replay(emu_lib, records, count, size)
    for w, g_ in zip(want, got):
        assert np.array_equal(w, g_)
    if n == 67:
        assert count[0] == 0 and count[1] == cap and count[2] > cap              # empty, full, more than the rows hold
        assert len(set(want[1][3:].tolist())) > 3 and (want[1][:3] == -1).all()  # first, middle and last positions are hit
        assert (want[1][3:] >= 0).sum() >= 40
        for upto in (0, 1, cap // 2, cap, cap + 9):                              # upto below, at and beyond the count
            w, g_ = pc.replay_numpy(records, count, size, upto), pc.host_replay(emu_lib, records, count, size, upto)
            assert all(np.array_equal(a, b) for a, b in zip(w, g_)), upto
        wide = np.zeros((n, cap + 3), pc.RECORD)                                 # rows further apart than the capacity
        wide[:, :cap] = records
        wide[:, cap:] = records[:, :3]
        g_ = pc.host_replay(emu_lib, wide, count, size, capacity=cap)
        assert all(np.array_equal(a, b) for a, b in zip(want, g_))
        neg = np.full(n, -1, np.int32)                                           # "no finished episode yet": an empty bin
        h, s, v = pc.host_replay(emu_lib, records, neg, size)
        assert not h.any() and (s == -1).all() and not v.any()


def test_every_kind_of_unsound_box_is_found_where_it_is(emu_lib):
    size, cap = (7, 13, 9), 12
    records, count = pc.edge_plans(size, 67, cap, seed=3)
    status = pc.host_replay(emu_lib, records, count, size)[1]
    hit = {}
    for i in range(3, 67):
        kind, where = pc.BREAKS[(i - 3) % len(pc.BREAKS)], ((i - 3) // len(pc.BREAKS)) % 3
        if status[i] >= 0:
            assert status[i] == (0, int(count[i]) // 2, int(count[i]) - 1)[where], i
            hit.setdefault(kind, set()).add(where)
    assert set(hit) == set(pc.BREAKS) and all(len(v) >= 2 for v in hit.values()), hit


def test_overflow_drops_records_keeps_counting_and_stays_inside_the_log(emu, emu_lib):
    g = pc.load_case("rollout_short_5x4x6")
    T, E = g["actions"].shape
    env = emu.EmuEnv(g["pool"], g["size"], g["rotation"], E)
    env.reset()
    log = pc.HostLog(emu_lib, env, 8, guard=4096)
    assert log.nbytes == emu_lib.bpp_placements_sizes(E, 8, 1) == E * 24 + 2 * E * 8 * 8 + 8
    exp = pc.ExpectedPlans(E, g["size"][1], 8)
    deepest = 0
    for t in range(T):
        log.step(g["actions"][t])
        exp.step(g["box"][t], g["done"][t])
        run, cnt, _ = log.gather(False)
        fin, fcnt, _ = log.gather(True)
        assert np.array_equal(cnt, env.state["n_boxes"]) and np.array_equal(cnt, exp.run_count)
        assert run.tobytes() == exp.run.tobytes() and fin.tobytes() == exp.fin.tobytes() and np.array_equal(fcnt, exp.fin_count)
        assert log.overflow == exp.dropped
        deepest = max(deepest, int(cnt.max()))
    assert deepest == 21 and exp.dropped > 0 and log.guards_intact()


def test_subset_ids_noop_copy_gather_and_clear(emu, emu_lib):
    g = pc.load_case("rollout_cut2_10_rot")
    size, E, cap = g["size"], 8, 24
    env = emu.EmuEnv(g["pool"], size, True, E)
    env.reset()
    log = pc.HostLog(emu_lib, env, cap)
    model = pc.PlanModel(np.arange(E), size, True, cap)
    rng = np.random.RandomState(0)
    n = 3
    outs = dict(obs=np.zeros((n, 400), np.float32), mask=np.zeros((n, 200), np.float32), reward=np.zeros(n, np.float32), done=np.zeros(n, np.uint8),
                counter=np.zeros(n, np.int32), ratio=np.zeros(n), ep_ret=np.zeros(n), ep_len=np.zeros(n, np.int32))
    so = emu.StepOut(*[outs[k].ctypes.data for k in ("obs", "mask", "reward", "done", "counter", "ratio", "ep_ret", "ep_len")])
    full_mask = env.out["mask"].copy()
    for t in range(40):
        if t % 2 == 0:            # all bins, a third of them left alone
            a = np.array([rng.choice(np.flatnonzero(full_mask[e])) if rng.rand() > 0.05 else 200 for e in range(E)], np.int64)
            a[rng.rand(E) < 0.33] = pc.NOOP
            model.note(env.state["item_cur"], a)
            out = log.step(a)
            full_mask = out["mask"].copy()
            model.commit(out["done"], env.hmap)
        else:                     # three scattered bins through bpp_step_subset, one of them a no-op, and an id out of range in the notes
            ids = np.ascontiguousarray(rng.permutation(E)[:n], np.int64)
            a = np.array([rng.choice(np.flatnonzero(full_mask[e])) for e in ids], np.int64)
            a[1] = pc.NOOP
            fa = np.full(E, pc.NOOP, np.int64)
            fa[ids] = a
            model.note(env.state["item_cur"], fa)
            before = log.buf.copy()
            log.note(a, ids)
            rc = emu_lib.bpp_step_subset(ctypes.byref(env._b), ids.ctypes.data, n, a.ctypes.data, ctypes.byref(so), None, None)
            assert rc == 0
            log.commit(outs["done"], ids)
            fd = np.zeros(E, np.uint8)
            fd[ids] = outs["done"]
            model.commit(fd, env.hmap)
            full_mask[ids] = outs["mask"]
            # the other bins' part of the log is untouched: count records, notes and plan rows
            other = np.setdiff1d(np.arange(E), ids)
            for lo, width, rows in ((0, 16, E), (16 * E, 8, E), (24 * E, 8 * cap, 2 * E)):
                now, was = (x[lo:lo + width * rows].reshape(rows, width) for x in (log.buf, before))
                keep = other if rows == E else np.concatenate([other, other + E])
                assert np.array_equal(now[keep], was[keep]), t
        run, cnt, ep = log.gather(False)
        fin, fcnt, fep = log.gather(True)
        assert np.array_equal(cnt, model.m.run_count) and np.array_equal(cnt, env.state["n_boxes"]), t
        assert run.tobytes() == model.m.run.tobytes() and fin.tobytes() == model.m.fin.tobytes(), t
        assert np.array_equal(fcnt, model.m.fin_count) and np.array_equal(fep, model.m.fin_episode), t
    assert (fcnt >= 0).sum() >= 2 and cnt.max() >= 4
    # an id outside the batch: skipped by note, commit and gather
    ids = np.array([E, 2, -1], np.int64)
    before = log.buf.copy()
    log.note(np.array([5, pc.NOOP, 5], np.int64), ids)
    log.commit(np.zeros(3, np.uint8), ids)
    assert np.array_equal(log.buf, before)
    r3, c3, e3 = log.gather(False, ids)
    assert c3[0] == c3[2] == -1 and e3[0] == -1 and not r3[[0, 2]].view(np.uint8).any() and r3[1].tobytes() == run[2].tobytes()
    # gather of a scattered list = the rows of the full gather, also with rows further apart
    ids = np.array([6, 0, 3, 7], np.int64)
    for finished, (full, fc, fe) in ((False, (run, cnt, ep)), (True, (fin, fcnt, fep))):
        r, c, e_ = log.gather(finished, ids, stride=cap + 5)
        assert r.tobytes() == full[ids].tobytes() and np.array_equal(c, fc[ids]) and np.array_equal(e_, fe[ids])
    # copy: dst plans = src plans, the rest alone (a pair with an id out of range is skipped)
    before = log.buf.copy()
    log.copy([1, 4, 99], [5, 2, 0])
    run2, cnt2, ep2 = log.gather(False)
    fin2, fcnt2, fep2 = log.gather(True)
    for (new, old) in ((run2, run), (cnt2, cnt), (ep2, ep), (fin2, fin), (fcnt2, fcnt), (fep2, fep)):
        assert np.array_equal(new[[5, 2]], old[[1, 4]]) and np.array_equal(new[[0, 1, 3, 4, 6, 7]], old[[0, 1, 3, 4, 6, 7]])
    # ... and the copies go on like their sources
    a = np.array([rng.choice(np.flatnonzero(full_mask[e])) for e in range(E)], np.int64)
    a[5], a[2] = a[1], a[4]
    env.hmap[[5, 2]], env.state[[5, 2]] = env.hmap[[1, 4]], env.state[[1, 4]]
    log.step(a)
    run3, cnt3, _ = log.gather(False)
    assert run3[[5, 2]].tobytes() == run3[[1, 4]].tobytes() and np.array_equal(cnt3[[5, 2]], cnt3[[1, 4]])
    log.clear()
    _, c, _ = log.gather(False)
    _, fc, fe = log.gather(True)
    assert not c.any() and (fc == -1).all() and (fe == -1).all() and log.overflow == 0
    # without keep_finished: one bank, a finished plan is dropped, asking for it is refused
    log1 = pc.HostLog(emu_lib, env, cap, keep=0)
    assert log1.nbytes == E * 24 + E * cap * 8 + 8
    for t in range(6):
        log1.step(g["actions"][t])
    _, c1, _ = log1.gather(False)
    assert np.array_equal(c1, env.state["n_boxes"])
    rec = np.zeros((E, cap), "<u8")
    assert emu_lib.bpp_placements_gather(log1.buf.ctypes.data, None, 0, 1, rec.ctypes.data, cap, c1.ctypes.data, None, E, cap, 0, None) == pc.BADARG


def test_refusals_name_their_function_on_both_libraries(lib, emu_lib, emu):
    E, cap = 4, 8
    buf = pc.aligned_bytes(E * 24 + 2 * E * cap * 8 + 8, 64)[0]
    hmap, state = np.zeros((E, 100), np.uint8), np.zeros(E * 12, np.int32)
    i64, i32, u8 = np.zeros(E + 1, np.int64), np.zeros(E + 1, np.int32), np.zeros(E * 8 * cap + 8, np.uint8)
    P = lambda a, off=0: a.ctypes.data + off      # noqa: E731

    def batch(cls, **kw):
        f = dict(num_envs=E, W=10, L=10, H=10, rotation=1, mask_rule=0, pool_size=1, pool_len=1, env_id_base=0, env_id_total=E, seq_pool=P(u8),
                 hmap=P(hmap), state=P(state), ep_acc=None, pool_mode=0, reserved0=0, seq_cache=None)
        f.update(kw)
        return ctypes.byref(cls(*[f[n] for n, _ in cls._fields_]))

    for L, B in ((lib, _lib.Batch), (emu_lib, emu.Batch)):
        def refused(name, *args):
            assert getattr(L, name)(*args) == pc.BADARG, (name, args)
            assert L.bpp_last_error().decode().startswith(name + ": "), (name, L.bpp_last_error())

        for a in ((0, cap, 1), (E, 0, 1), (E, (1 << 20) + 1, 1), (E, cap, 2), (-1, cap, 0)):
            refused("bpp_placements_sizes", *a)
        assert L.bpp_placements_sizes(E, cap, 1) == buf.size and L.bpp_placements_sizes(E, cap, 0) == E * 24 + E * cap * 8 + 8
        for a in ((None, E, cap, 1), (P(buf, 8), E, cap, 1), (P(buf), 0, cap, 1), (P(buf), E, 0, 1), (P(buf), E, cap, 3)):
            refused("bpp_placements_clear", *a, None)
        ok = dict(b=batch(B), ids=None, n=0, x=P(i64), log=P(buf), cap=cap, keep=1)
        for fn, x_bad in (("bpp_placements_note", P(i64, 4)), ("bpp_placements_commit", None)):
            for kw in (dict(b=None), dict(x=None), dict(x=x_bad), dict(log=None), dict(log=P(buf, 4)), dict(cap=0), dict(keep=-1),
                       dict(ids=P(i64, 4), n=1), dict(ids=P(i64), n=-1), dict(b=batch(B, state=None)), dict(b=batch(B, hmap=None)),
                       dict(b=batch(B, W=0)), dict(b=batch(B, W=40, L=40)), dict(b=batch(B, L=256, W=1)), dict(b=batch(B, num_envs=0))):
                c = dict(ok, **kw)
                refused(fn, c["b"], c["ids"], c["n"], c["x"], c["log"], c["cap"], c["keep"], None)
        for a in ((None, P(i64), P(i64), 1, E, cap, 1), (P(buf), None, P(i64), 1, E, cap, 1), (P(buf), P(i64), None, 1, E, cap, 1),
                  (P(buf), P(i64), P(i64), -1, E, cap, 1), (P(buf), P(i64, 4), P(i64), 1, E, cap, 1), (P(buf), P(i64), P(i64), 1, 0, cap, 1),
                  (P(buf), P(i64), P(i64), 1, E, cap, 2)):
            refused("bpp_placements_copy", *a, None)
        okg = dict(log=P(buf), ids=None, n=0, which=0, out=P(u8), stride=cap, count=P(i32), ep=P(i32), E=E, cap=cap, keep=1)
        for kw in (dict(log=None), dict(which=2), dict(which=-1), dict(which=1, keep=0), dict(out=None), dict(count=None), dict(stride=cap - 1),
                   dict(ids=P(i64), n=-2), dict(out=P(u8, 4)), dict(count=P(i32, 2)), dict(ep=P(i32, 1)), dict(ids=P(i64, 2), n=1), dict(E=0),
                   dict(cap=0)):
            c = dict(okg, **kw)
            refused("bpp_placements_gather", c["log"], c["ids"], c["n"], c["which"], c["out"], c["stride"], c["count"], c["ep"], c["E"], c["cap"],
                    c["keep"], None)
        okr = dict(rec=P(u8), stride=cap, cap=cap, count=P(i32), n=E, W=10, L=10, H=10, upto=-1, hmap=P(hmap), status=P(i32), vol=P(i32))
        for kw in (dict(rec=None), dict(count=None), dict(hmap=None), dict(n=-1), dict(cap=0), dict(stride=cap - 1), dict(W=0), dict(L=0), dict(H=0),
                   dict(H=256), dict(W=33, L=32), dict(W=1025, L=1), dict(rec=P(u8, 4)), dict(count=P(i32, 2)), dict(status=P(i32, 1)),
                   dict(vol=P(i32, 3))):
            c = dict(okr, **kw)
            refused("bpp_placements_replay", c["rec"], c["stride"], c["cap"], c["count"], c["n"], c["W"], c["L"], c["H"], c["upto"], c["hmap"],
                    c["status"], c["vol"], None)
        out = (ctypes.c_int32 * 6)()
        for a in ((0, cap, 100), (E, 0, 100), (E, cap, 0), (E, cap, 1025)):
            refused("bpp_placements_info", *a, out)
        refused("bpp_placements_info", E, cap, 100, None)
        assert _lib.placements_info(65536, 256, 100, L) == dict(step_lanes=256, step_groups=256, plan_waves=4, plan_groups=16384,
                                                                replay_cells_per_lane=2, record_bytes=8)
        assert _lib.placements_info(4099, 1, 1024, L)["step_groups"] == 17 and _lib.placements_info(1, 1, 1024, L)["replay_cells_per_lane"] == 16
    # calls that enqueue nothing are accepted without a device
    assert lib.bpp_placements_copy(P(buf), P(i64), P(i64), 0, E, cap, 1, None) == 0
    assert lib.bpp_placements_replay(P(u8), cap, cap, P(i32), 0, 10, 10, 10, -1, P(hmap), None, None, None) == 0


def test_every_declared_symbol_is_exported(lib):
    src = open(_lib.PLACEMENTS_HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(bpp_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.PLACEMENT_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.bpp_abi_version() == 16 and _lib.ABI_VERSION == 16
    assert pc.RECORD.itemsize == _lib.PLACEMENT_BYTES == 8


def test_packing_plans_host_side(tmp_path):
    """boxes / flags / write_txt / save / load of PackingPlans on host tensors: the reference's tuple order and line format."""
    import torch
    from bpp_amd.placements import PackingPlans, RECORD_DTYPE, default_capacity
    assert RECORD_DTYPE == pc.RECORD and default_capacity((10, 10, 10)) == 256 and default_capacity((5, 4, 6)) == 120
    g = pc.load_case("rollout_wide_8x12x9_rot")
    box = g["box"][:, 2]
    box = box[box[:, 0] >= 0][:5]                                     # five boxes the reference placed in bin 2
    n = len(box)
    assert n == 5 and box[:, 6].any()
    rec = np.zeros((2, 6), pc.RECORD)
    rec[1, :n] = pc.box_records(box[:n], 12)
    plans = PackingPlans(torch.from_numpy(rec.view(np.uint8).reshape(2, 6, 8)), torch.tensor([-1, n], dtype=torch.int32),
                         torch.tensor([-1, 0], dtype=torch.int32), torch.zeros(1, dtype=torch.int32), g["size"])
    assert plans.boxes(0) == [] and plans.boxes(1) == [tuple(int(v) for v in b[:6]) for b in box[:n]]
    assert plans.flags(1) == [bool(b[6]) for b in box[:n]]
    plans.write_txt(str(tmp_path / "traj.txt"), 1)
    assert open(str(tmp_path / "traj.txt")).read() == "".join("{}, {}, {}, {}, {}, {}\n".format(*b[:6]) for b in box[:n].tolist())
    plans.save(str(tmp_path / "plans.npz"))
    back = PackingPlans.load(str(tmp_path / "plans.npz"))
    assert back.size == g["size"] and back.boxes(1) == plans.boxes(1) and torch.equal(back.records, plans.records)
    assert torch.equal(back.count, plans.count) and torch.equal(back.episode, plans.episode)
