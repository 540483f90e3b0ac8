"""Batched MCTS (include/bpp_mcts.h, online-3d-bpp-drl_amd/mcts.py) against MCTS/monteCarlo.py's MCTree driven as
mcts_test.py:14-65 drives it (fixtures: tests/golden/make_mcts_golden.py).

CPU: the product kernels in the host SIMT emulator (tests/emu), the fixtures' flat policy between the launches; the sizes
bound; argument checks.  `-m gpu`: BppVecEnv + MCTSearch on the device, the same policy in torch; subsets, invalid ids,
the sync-free path, seed ranges, stream supply against pool supply, 2 048 slots against a host restatement over
oracle/ref_port.py; the toolchain's float64 sqrt against numpy.

Every claim here holds under flat_policy only: its softmax is exactly 1/c, so all priors are equal and exact and the
trajectories match bit for bit.  Under real logits the priors agree with float64 within a float32 softmax tolerance, and
what follows them (UCB choice, backup, play()) is exact given the priors' bits: tests/test_mcts_real_policy.py checks
that launch by launch."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden

NOOP = np.iinfo(np.int64).min
FILES = {"mcts_fake_10": ["default", "k2", "depth1", "depth0", "roll0", "roll2", "credit", "ep2"],
         "mcts_fake_8x12x9": ["wide"], "mcts_fake_5x5x3": ["small"], "mcts_fake_20x20x10": ["big"]}
RUNS = [(f, c) for f, cs in FILES.items() for c in cs]
MCTS_SRC = [os.path.join(ROOT, "online-3d-bpp-drl_amd", "csrc", "bpp_mcts.inl"), os.path.join(ROOT, "include", "bpp_mcts.h")]


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def case_params(g, c):
    """(S, k, search_depth, rollout_length, credit, episodes) of fixture case c, with the reference's argument types."""
    S, k, depth, rollout, credit, episodes = (float(v) for v in g[c + "_params"])
    return (int(S), int(k), None if depth < 0 else int(depth), int(rollout), 1 if credit == 1.0 else credit, int(episodes))


def expected(g, c):
    """Per trajectory, per episode: (act, n, w, nch, pos) arrays of fixture case c."""
    st = g[c + "_start"]
    episodes = case_params(g, c)[5]
    N = (len(st) - 1) // episodes
    f = [g[c + s] for s in ("_act", "_n", "_w", "_nch", "_pos")]
    return [[tuple(a[st[p * episodes + e]:st[p * episodes + e + 1]] for a in f) for e in range(episodes)] for p in range(N)]


def flat_policy_np(size):
    import torch
    from bpp_amd.mcts import flat_policy
    pol = flat_policy(size)

    def policy(obs):
        v, lg, _ = pol(torch.from_numpy(obs))
        return np.ascontiguousarray(v.numpy()), np.ascontiguousarray(lg.numpy())
    return policy


def parse_roots(raw, E, cap, ids):
    """(n, w, children, mt position) of the roots of bins ids from the raw state bytes (csrc/bpp_mcts.inl layout)."""
    raw = np.asarray(raw).view(np.uint8)
    bins = raw[:E * 192].view(np.int32).reshape(E, 48)
    pool0 = E * 192 + E * 640 * 4
    out = []
    for e in ids:
        half, pos = int(bins[e, 1]), int(bins[e, 3])
        base = pool0 + (e * 2 + half) * cap * 32
        rec = raw[base:base + 32]
        w = float(rec[:8].view(np.float64)[0])
        n, blk = (int(v) for v in rec[16:24].view(np.int32))
        ch = int(raw[base + blk * 32 + 16:base + blk * 32 + 20].view(np.int32)[0]) if blk >= 0 else 0
        out.append((n, w, ch, pos))
    return out


# ---------------------------------------------------------------------------------------------------- CPU (emulator)
def emu_mcts_lib(emu):
    """The emulated library with the MCTS entry points of the current source (tests/emu's own staleness check does not
    know bpp_mcts.inl / bpp_mcts.h): rebuilt and reloaded under a name of its own when older than them."""
    from bpp_amd import _lib
    L = emu.lib()
    stale = any(os.path.getmtime(f) > os.path.getmtime(emu.LIB) for f in MCTS_SRC)
    if stale or not all(hasattr(L, s) for s in _lib.MCTS_SYMBOLS):
        import shutil
        emu.build(force=True)
        fresh = "%s.mcts.%d" % (emu.LIB, os.getpid())
        shutil.copyfile(emu.LIB, fresh)
        emu.LIB, emu._lib = fresh, None
        L = emu.lib()
        assert all(hasattr(L, s) for s in _lib.MCTS_SYMBOLS)
    return L


class EmuMcts(object):
    """The schedule of MCTSearch.decide over the emulated library: real bins [0, n), scratch bins [n, 2n)."""

    def __init__(self, emu, pool, size, n, k, S, depth=None, rollout=-1, credit=1, zeta=1e-5):
        from bpp_amd import _lib
        self._lib = _lib
        self.emu, self.size, self.n, self.k, self.S = emu, tuple(int(v) for v in size), n, k, S
        L = emu_mcts_lib(emu)
        self.L = _lib.bind_mcts(L, emu.Batch)
        L.bpp_step_subset.argtypes = [ctypes.POINTER(emu.Batch), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                      ctypes.POINTER(emu.StepOut), ctypes.c_void_p, ctypes.c_void_p]
        L.bpp_copy_bins.argtypes = [ctypes.POINTER(emu.Batch), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                    ctypes.c_void_p]
        self.env = emu.OracleEnv(pool, self.size, False, 2 * n)
        self.env.reset()
        self.A, self.E = self.env.A, 2 * n
        self.max_depth = k - 1 if depth is None else min(depth, k - 1)
        self.rollout = 0 if rollout is None else rollout
        self.credit, self.zeta = float(credit), zeta
        sizes = (ctypes.c_int64 * 4)()
        assert self.L.bpp_mcts_sizes(self.E, k, S, self.max_depth, self.rollout, self.env.W, self.env.L, sizes) == 0
        self.nbytes, self.cap, _, self.levels = (int(v) for v in sizes)
        buf = np.zeros(self.nbytes + 16, np.uint8)
        off = (-buf.ctypes.data) % 16
        self.state = buf[off:off + self.nbytes]
        self.overflow = np.zeros(1, np.int32)
        self.policy = flat_policy_np(self.size)
        self._last = None

    def desc(self, ids, scratch):
        return self._lib.Mcts(0 if ids is None else ids.shape[0], self.k, self.S, self.max_depth, self.rollout, self.cap, self.credit,
                              self.zeta, None if ids is None else _p(ids).value, None if scratch is None else _p(scratch).value,
                              _p(self.state).value, _p(self.overflow).value, 0)

    def seed(self, ids, seeds):
        ids, seeds = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(seeds, np.int64).astype(np.uint32)
        m = self.desc(None, None)
        assert self.L.bpp_mcts_seed(ctypes.byref(self.env._b), ctypes.byref(m), _p(ids), _p(seeds), ids.shape[0], None) == 0

    def _step(self, ids, a):
        n, env = ids.shape[0], self.env
        r = dict(obs=np.zeros((n, 4 * self.A), np.float32), mask=np.zeros((n, self.A), np.float32), reward=np.zeros(n, np.float32),
                 done=np.zeros(n, np.uint8), counter=np.zeros(n, np.int32), ratio=np.zeros(n), ep_ret=np.zeros(n),
                 ep_len=np.zeros(n, np.int32))
        out = self.emu.StepOut(*[_p(r[f]).value for f in ("obs", "mask", "reward", "done", "counter", "ratio", "ep_ret", "ep_len")])
        a = np.ascontiguousarray(a, np.int64)
        assert self.L.bpp_step_subset(ctypes.byref(env._b), _p(ids), n, _p(a), ctypes.byref(out), None, None) == 0
        return r

    def decide(self, ids, scratch=None):
        ids = np.ascontiguousarray(ids, np.int64)
        scratch = ids + self.n if scratch is None else np.ascontiguousarray(scratch, np.int64)
        n, L, b = ids.shape[0], self.L, ctypes.byref(self.env._b)
        m = self.desc(ids, scratch)
        mr = ctypes.byref(m)
        obs, acts = np.zeros((n, 4 * self.A), np.float32), np.zeros(n, np.int64)
        assert L.bpp_mcts_begin(b, mr, None) == 0, L.bpp_last_error()
        for _ in range(self.S):
            assert L.bpp_copy_bins(b, None, _p(ids), _p(scratch), n, None) == 0
            done = None
            for level in range(self.max_depth):
                assert L.bpp_mcts_select(b, mr, level, _p(done), _p(acts), None) == 0, L.bpp_last_error()
                done = self._step(scratch, acts)["done"]
            assert L.bpp_mcts_emit(b, mr, 0, _p(done), _p(obs), None) == 0, L.bpp_last_error()
            value, logits = self.policy(obs)
            assert L.bpp_mcts_expand(b, mr, _p(value), _p(logits), _p(acts), None) == 0
            done = None
            for level in range(1, self.levels):
                done = self._step(scratch, acts)["done"]
                assert L.bpp_mcts_emit(b, mr, level, _p(done), _p(obs), None) == 0
                value, logits = self.policy(obs)
                assert L.bpp_mcts_rollout(b, mr, _p(value), _p(logits), _p(acts), None) == 0
            if self.levels > 0:
                done = self._step(scratch, acts)["done"]
            assert L.bpp_mcts_backup(b, mr, _p(done), None) == 0
        act, vis = np.zeros(n, np.int64), np.zeros(n, np.int32)
        assert L.bpp_mcts_finish(b, mr, _p(act), _p(vis), None) == 0
        self._last = (ids, scratch)
        return act, vis

    def advance(self, done):
        ids, scratch = self._last
        m = self.desc(ids, scratch)
        d = np.ascontiguousarray(done, np.uint8)
        assert self.L.bpp_mcts_advance(ctypes.byref(self.env._b), ctypes.byref(m), _p(d), None) == 0

    def roots(self, ids):
        return parse_roots(self.state, self.E, self.cap, ids)


def check_decisions(exp, ep, t, slots, traj, act, roots, bad):
    """Compare the decisions of live slots with the fixture; records (trajectory, slot) pairs that diverge in `bad`."""
    for j, s in enumerate(slots):
        p = traj[s]
        e = exp[p][ep[s]]
        if t[s] >= len(e[0]):
            bad.add((int(p), int(s), "longer"))
            continue
        n, w, ch, pos = roots[j]
        k = t[s]
        if not (act[j] == e[0][k] and n == e[1][k] and np.float64(w).tobytes() == np.float64(e[2][k]).tobytes()
                and ch == e[3][k] and pos == e[4][k]):
            bad.add((int(p), int(s), "decision %d of episode %d: got %r / %r, want %r" % (
                k, ep[s], (int(act[j]), n, w, ch, pos), tuple(x[k] for x in e))))


def replay_emulated(emu, g, c, N):
    size = tuple(int(v) for v in g["size"])
    S, k, depth, rollout, credit, episodes = case_params(g, c)
    exp = expected(g, c)[:N]
    em = EmuMcts(emu, g["pool"][:N], size, N, k, S, depth, rollout, credit)
    em.seed(np.arange(N), g[c + "_seeds"][:N])
    ep, t, traj = np.zeros(N, int), np.zeros(N, int), np.arange(N)
    live = np.arange(N)
    bad = set()
    ratios = np.zeros((N, episodes))
    while live.size:
        act, vis = em.decide(live)
        check_decisions(exp, ep, t, live, traj, act, em.roots(live), bad)
        assert not bad, sorted(bad)[:5]
        r = em._step(live, act)
        em.advance(r["done"])
        t[live] += 1
        for j, s in enumerate(live):
            if r["done"][j]:
                assert t[s] == len(exp[s][ep[s]][0]), "trajectory %d episode %d ends early" % (s, ep[s])
                ratios[s, ep[s]] = r["ratio"][j]
                ep[s] += 1
                t[s] = 0
        live = live[ep[live] < episodes]
    np.testing.assert_array_equal(ratios.reshape(-1), g[c + "_ratio"][:N * episodes])
    assert em.overflow[0] == 0


# the emulator runs every fixture case; the S = 100 default case on its first 3 trajectories (the device runs all of them)
EMU_TRAJ = {"default": 3}


@pytest.mark.parametrize("name,case", RUNS)
def test_emulated_mcts_matches_reference(emu, name, case):
    g = load_golden(name)
    N = len(g[case + "_seeds"])
    replay_emulated(emu, g, case, min(N, EMU_TRAJ.get(case, N)))


@pytest.mark.parametrize("name,case", RUNS)
def test_fixture_is_meaningful(name, case):
    """Every case plays whole episodes with more than one decision, its roots have children and visits, the stream is
    consumed (ties broken, rollouts sampled), and the cases differ from each other."""
    g = load_golden(name)
    S, k, depth, rollout, credit, episodes = case_params(g, case)
    st = g[case + "_start"]
    assert (np.diff(st) >= 2).all()
    assert (g[case + "_nch"] >= 1).all()
    assert (g[case + "_n"] >= S).all()
    assert len(set(g[case + "_pos"].tolist())) > 1


def test_sizes_bound(emu):
    from bpp_amd import _lib
    L = _lib.bind_mcts(emu_mcts_lib(emu), emu.Batch)
    out = (ctypes.c_int64 * 4)()
    assert L.bpp_mcts_sizes(10, 4, 100, 3, -1, 10, 10, out) == 0
    assert out[1] == 1 + 4 * 100 * 101 and out[3] == 4
    assert out[2] == 192 + 640 * 4 + 2 * out[1] * 32 and out[0] == 10 * out[2]
    assert L.bpp_mcts_sizes(1, 5, 40, 4, 2, 10, 10, out) == 0 and out[3] == 3
    assert L.bpp_mcts_sizes(1, 4, 40, 3, 0, 10, 10, out) == 0 and out[3] == 0
    assert L.bpp_mcts_sizes(1, 3, 40, 2, 5, 10, 10, out) == 0 and out[3] == 0     # k - d >= r + 1 never holds
    assert L.bpp_mcts_sizes(1, 4, 40, 0, -1, 10, 10, out) == 0 and out[1] == 1 + 40 * 101
    for args in ((1, 1, 10, 0, -1, 10, 10), (1, 17, 10, 3, -1, 10, 10), (1, 4, 0, 3, -1, 10, 10), (1, 4, 10, 4, -1, 10, 10),
                 (1, 4, 10, 3, -2, 10, 10), (1, 4, 10, 3, -1, 40, 40)):
        assert L.bpp_mcts_sizes(*args, out) != 0, args


def test_emulated_argument_checks(emu):
    from bpp_amd import _lib
    L = _lib.bind_mcts(emu_mcts_lib(emu), emu.Batch)
    pool = load_golden("mcts_fake_10")["pool"][:4]
    ids, scratch = np.arange(2, dtype=np.int64), np.arange(2, 4, dtype=np.int64)
    state, ovf = np.zeros(1 << 16, np.uint8), np.zeros(1, np.int32)
    cap = 1 + 2 * 4 * 101
    for rot, k, depth, cap_, credit, want in ((True, 3, 1, cap, 1.0, "rotation"), (False, 1, 0, cap, 1.0, "k must"),
                                              (False, 3, 3, cap, 1.0, "max_depth"), (False, 3, 1, cap + 1, 1.0, "cap"),
                                              (False, 3, 1, cap, 1.5, "credit")):
        env = emu.OracleEnv(pool, (10, 10, 10), rot, 4)
        m = _lib.Mcts(2, k, 4, depth, -1, cap_, credit, 1e-5, _p(ids).value, _p(scratch).value, _p(state).value, _p(ovf).value, 0)
        assert L.bpp_mcts_begin(ctypes.byref(env._b), ctypes.byref(m), None) != 0
        assert want in L.bpp_last_error().decode(), L.bpp_last_error()


def test_emulated_invalid_ids_touch_nothing(emu):
    """A slot whose real or scratch id lies outside [0, E) searches nothing and touches no state: the other slots decide
    what they decide without it, and it gets BPP_ACTION_NOOP with 0 visits."""
    g = load_golden("mcts_fake_10")
    S, k, depth, rollout, credit, _ = case_params(g, "k2")
    n = 4
    a = EmuMcts(emu, g["pool"][:n], (10, 10, 10), n, k, S, depth, rollout, credit)
    b = EmuMcts(emu, g["pool"][:n], (10, 10, 10), n, k, S, depth, rollout, credit)
    for em in (a, b):
        em.seed(np.arange(2 * n), np.arange(2 * n) + 5)
    want = b.decide(np.arange(n))
    ids, scratch = np.arange(n), np.arange(n) + n
    ids[1] = -2
    scratch[3] = 99
    before = a.state.copy()
    act, vis = a.decide(ids, scratch)
    for j in (0, 2):
        assert (act[j], vis[j]) == (want[0][j], want[1][j])
    for j in (1, 3):
        assert (act[j], vis[j]) == (NOOP, 0)
    # bin 3's state (its slot's scratch id is bad) is as before
    st = parse_roots(before, a.E, a.cap, [3]), parse_roots(a.state, a.E, a.cap, [3])
    assert st[0] == st[1]
    assert a.overflow[0] == 0


def test_python_argument_checks():
    from types import SimpleNamespace
    from bpp_amd.mcts import MCTSearch
    env = SimpleNamespace(can_rotate=False)
    with pytest.raises(ValueError, match="rotation"):
        MCTSearch(SimpleNamespace(can_rotate=True), 3)
    for k in (1, 17):
        with pytest.raises(ValueError, match="k must"):
            MCTSearch(env, k)
    with pytest.raises(ValueError, match="sim_times"):
        MCTSearch(env, 3, sim_times=0)
    with pytest.raises(ValueError, match="rollout_length"):
        MCTSearch(env, 3, rollout_length=-2)
    with pytest.raises(ValueError, match="credit"):
        MCTSearch(env, 3, credit=1.5)
    with pytest.raises(ValueError, match="zeta"):
        MCTSearch(env, 3, zeta=0.0)


# ---------------------------------------------------------------------------------------------------- GPU
def _gpu_env(pool, size, E):
    import torch
    from bpp_amd import BppVecEnv
    env = BppVecEnv(E, container_size=size, pool=np.ascontiguousarray(pool), device="cuda", compute_mask=True)
    env.reset()
    torch.cuda.synchronize()
    return env


def replay_gpu(g, c, N, reps=1, check=True):
    """Play the first N trajectories of case c, each replicated `reps` times, with BppVecEnv + MCTSearch (real bins [0, M),
    scratch [M, 2M), M = N * reps; bin b plays trajectory b mod N).  Returns the diverging (trajectory, bin, what) and the
    overflow counter."""
    import torch
    from bpp_amd import MCTSearch
    from bpp_amd.mcts import flat_policy
    size = tuple(int(v) for v in g["size"])
    S, k, depth, rollout, credit, episodes = case_params(g, c)
    exp = expected(g, c)[:N]
    M = N * reps
    env = _gpu_env(g["pool"][:N], size, 2 * M)
    ms = MCTSearch(env, k, sim_times=S, search_depth=depth, rollout_length=rollout, credit=credit)
    ms.seed(torch.arange(M), torch.as_tensor(np.tile(g[c + "_seeds"][:N], reps)))
    policy = flat_policy(size)
    traj = np.arange(M) % N
    ep, t = np.zeros(M, int), np.zeros(M, int)
    live = np.arange(M)
    bad = set()
    ratios = np.zeros((M, episodes))
    while live.size:
        lt = torch.as_tensor(live, device=env.device)
        act, vis = ms.decide(policy, lt, lt + M, check=check)
        check_decisions(exp, ep, t, live, traj, act.cpu().numpy(), list(zip(*ms.root_stats(lt))), bad)
        r = env.step_bins(lt, act)
        ms.advance(r.done)
        done, ratio = r.done.cpu().numpy(), r.ratio.cpu().numpy()
        t[live] += 1
        for j, s in enumerate(live):
            if done[j]:
                if t[s] != len(exp[traj[s]][ep[s]][0]):
                    bad.add((int(traj[s]), int(s), "ends early"))
                ratios[s, ep[s]] = ratio[j]
                ep[s] += 1
                t[s] = 0
        live = live[(ep[live] < episodes) & (t[live] < 200)]
    want = np.tile(g[c + "_ratio"][:N * episodes].reshape(N, episodes), (reps, 1))
    bad |= {(int(traj[s]), int(s), "ratio") for s in np.flatnonzero((ratios != want).any(1))}
    return sorted(bad), int(ms.overflow.item())


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", RUNS)
def test_gpu_mcts_matches_reference(name, case):
    g = load_golden(name)
    bad, ovf = replay_gpu(g, case, len(g[case + "_seeds"]))
    assert not bad, bad[:10]
    assert ovf == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", [("mcts_fake_10", "default"), ("mcts_fake_10", "roll2"), ("mcts_fake_10", "ep2"),
                                       ("mcts_fake_5x5x3", "small"), ("mcts_fake_8x12x9", "wide")])
def test_gpu_mcts_replicated(name, case):
    """Every trajectory 256 times (up to 2 048 slots, 4 096 bins): every replica equals the fixture."""
    g = load_golden(name)
    bad, ovf = replay_gpu(g, case, len(g[case + "_seeds"]), reps=256)
    assert not bad, bad[:10]
    assert ovf == 0


@pytest.mark.gpu
def test_gpu_check_false_is_the_same():
    g = load_golden("mcts_fake_10")
    bad, ovf = replay_gpu(g, "k2", 8, reps=4, check=False)
    assert not bad and ovf == 0


@pytest.mark.gpu
def test_gpu_subsets_and_invalid_ids():
    """A decision for a subset of the bins, in any order, equals the decision of the full batch for those bins; ids out of
    range give BPP_ACTION_NOOP and touch nothing; check=True rejects duplicates and overlapping scratch bins."""
    import torch
    from bpp_amd import MCTSearch
    from bpp_amd.mcts import flat_policy
    g = load_golden("mcts_fake_10")
    S, k, depth, rollout, credit, _ = case_params(g, "k2")
    N = 8
    pol = flat_policy((10, 10, 10))
    full_env = _gpu_env(g["pool"][:N], (10, 10, 10), 2 * N)
    full = MCTSearch(full_env, k, sim_times=S, search_depth=depth, rollout_length=rollout, credit=credit)
    ids = torch.arange(N, device="cuda")
    want_a, want_v = full.decide(pol, ids, ids + N)
    env = _gpu_env(g["pool"][:N], (10, 10, 10), 2 * N)
    ms = MCTSearch(env, k, sim_times=S, search_depth=depth, rollout_length=rollout, credit=credit)
    sub = torch.tensor([6, 1, 3], device="cuda")
    a, v = ms.decide(pol, sub, sub + N)
    assert torch.equal(a, want_a[sub]) and torch.equal(v, want_v[sub])
    bad_ids = torch.tensor([0, -1, 2, 40], device="cuda")
    a, v = ms.decide(pol, bad_ids, torch.tensor([8, 9, 10, 11], device="cuda"), check=False)
    assert int(a[1]) == NOOP and int(a[3]) == NOOP and int(v[1]) == 0 and int(v[3]) == 0
    assert int(a[0]) == int(want_a[0]) and int(a[2]) == int(want_a[2])
    with pytest.raises(ValueError):
        ms.decide(pol, torch.tensor([0, 0], device="cuda"), torch.tensor([8, 9], device="cuda"))
    with pytest.raises(ValueError):
        ms.decide(pol, torch.tensor([0, 1], device="cuda"), torch.tensor([1, 9], device="cuda"))
    assert int(ms.overflow.item()) == 0


@pytest.mark.gpu
def test_gpu_decide_does_not_synchronise():
    import torch
    from bpp_amd import MCTSearch
    from bpp_amd.mcts import flat_policy
    g = load_golden("mcts_fake_10")
    env = _gpu_env(g["pool"][:8], (10, 10, 10), 16)
    ms = MCTSearch(env, 3, sim_times=4)
    pol = flat_policy((10, 10, 10))
    ids = torch.arange(8, device=env.device)
    ms.decide(pol, ids, ids + 8)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        act, vis = ms.decide(pol, ids, ids + 8, check=False)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert act.shape == (8,)


@pytest.mark.gpu
def test_gpu_sqrt_is_correctly_rounded():
    """A check of the toolchain's float64 sqrt lowering for gfx950 only (torch's own kernel, not csrc/bpp_mcts.inl): sqrt of
    every integer 0 .. 10^6 equals numpy's.  The search kernels' own sqrt(parent.n) is covered by the fixtures, where
    every root w is compared bit for bit after u = (p * sqrt(parent.n)) / (n + 1) decided every descent."""
    import torch
    x = torch.arange(0, 10 ** 6 + 1, dtype=torch.float64, device="cuda")
    got = torch.sqrt(x).cpu().numpy()
    want = np.sqrt(np.arange(0, 10 ** 6 + 1, dtype=np.float64))
    assert got.tobytes() == want.tobytes()


@pytest.mark.gpu
def test_gpu_seed_range_is_checked():
    import torch
    from bpp_amd import MCTSearch
    g = load_golden("mcts_fake_10")
    env = _gpu_env(g["pool"][:4], (10, 10, 10), 8)
    ms = MCTSearch(env, 3, sim_times=2)
    for bad in ([-1], [1 << 32], [0.5]):
        with pytest.raises(ValueError):
            ms.seed(torch.tensor([0]), torch.tensor(bad))
    ms.seed(torch.tensor([0, 1]), torch.tensor([0, (1 << 32) - 1]))       # both ends of np.random.seed's range


@pytest.mark.gpu
def test_gpu_stream_supply_equals_pool_supply():
    """MCTSearch on a streaming env (scratch bins cloned with the source's ring, auto-reset on failed simulated steps)
    decides exactly what it decides on a pool env that holds the same items: the first episode of 256 bins, the items read
    back from the streaming env's ring."""
    import torch
    import bpp_amd
    from bpp_amd import MCTSearch
    from bpp_amd.mcts import flat_policy
    size, n = (10, 10, 10), 256
    senv = bpp_amd.BppVecEnv(2 * n, size, stream=dict(bound=(2, 5), seed=17, depth=8))
    senv.reset()
    T = senv.pool.shape[1] - 2
    items = senv.preview(T)[:n].cpu().numpy().astype(np.uint8)                 # [n, T, 3]: sequence, then the terminator
    pool = np.zeros((n, T + 1, 4), np.uint8)
    pool[:, :T, :3] = items
    pool[:, T, :3] = size
    penv = _gpu_env(pool, size, 2 * n)
    pol = flat_policy(size)
    seeds = torch.arange(n) * 31 + 7
    ids = torch.arange(n, device="cuda")
    searches = []
    for env in (senv, penv):
        ms = MCTSearch(env, 3, sim_times=12)
        ms.seed(ids, seeds)
        searches.append(ms)
    live = ids.clone()
    decisions = 0
    while live.numel():
        out = []
        for env, ms in zip((senv, penv), searches):
            act, vis = ms.decide(pol, live, live + n)
            r = env.step_bins(live, act)
            ms.advance(r.done)
            out.append((act, vis, ms.root_stats(live), r.done.clone()))
        (a0, v0, s0, d0), (a1, v1, s1, d1) = out
        assert torch.equal(a0, a1) and torch.equal(v0, v1), "decision %d" % decisions
        for x, y in zip(s0, s1):
            assert x.tobytes() == y.tobytes(), "decision %d: root records differ" % decisions
        assert torch.equal(d0, d1)
        live = live[~d0.bool()]
        decisions += 1
    assert decisions >= 5
    assert int(searches[0].overflow.item()) == 0 and int(searches[1].overflow.item()) == 0


# ---------------------------------------------------------------------------------------------------- host restatement
class HostNode(object):
    """node.py's Node / PutNode state."""
    __slots__ = ("parent", "children", "term", "value", "reward", "w", "n", "p")

    def __init__(self, parent, p):
        self.parent, self.children, self.term, self.value, self.reward, self.w, self.n, self.p = parent, {}, False, None, 0, 0, 0, p

    @property
    def q(self):
        return self.w / self.n if self.n else 0


def _clone(b):
    import copy
    c = copy.copy(b)
    c.plain = b.plain.copy()
    return c


def host_decide(root, env, k, S, max_depth, rollout, credit, rs, evaluate):
    """A restatement of MCTree.get_policy(S, zeta=1e-5) + sample_action over oracle/ref_port.PortBin, with a per-bin
    np.random.RandomState (the legacy stream np.random.seed drives).  Returns (action, root)."""
    import math
    from oracle.ref_port import place_rule
    W, L, H = env.size

    def expand(node, sim, blen):
        x, y, z = sim.item
        mask = np.zeros((W, L), np.int32)
        for i in range(W - x + 1):
            for j in range(L - y + 1):
                if place_rule(sim.plain, x, y, i, j, z, env.size) >= 0:
                    mask[i, j] = 1
        if mask.sum() == 0:
            mask[:, :] = 1
        mask = mask.reshape(-1)
        value, pvec = evaluate(sim.observation())
        valid = np.sum(mask)
        for a in range(W * L):
            if mask[a] == 1:
                node.children[a] = HostNode(node, credit * pvec[a] + (1 - credit) * (1 / valid))
        r = blen - 1 if rollout == -1 else rollout
        if r >= 1 and blen >= r + 1:
            stack = []
            for i in range(r + 1):
                value, pv = evaluate(sim.observation())
                a = rs.choice(pv.shape[0], p=pv)
                _, rew, done, _ = sim.step(a)
                if not done and i + 1 < r + 1:
                    stack.append(rew)
                if done:
                    stack.append(rew)
                    value = 0
                    break
            for rew in reversed(stack):
                value = rew + value
        node.value = value

    def choose(node):
        mx, best = -1e9 - 7, []
        for a, c in node.children.items():
            u = c.p * np.sqrt(node.n) / (c.n + 1)
            v = (c.q - node.q) + u if c.n > 0 else 0.0 + u
            if math.isclose(v, mx, rel_tol=1e-5):
                best.append((a, c))
            elif v > mx:
                mx, best = v, [(a, c)]
        return best[rs.randint(0, len(best))]

    for _ in range(S):
        node, d, sim = root, 0, _clone(env)
        while True:
            if node.term:
                value = 0
                break
            if not node.children:
                expand(node, sim, k - d)
                value = node.value
                break
            if d == max_depth:
                value = node.value
                break
            a, child = choose(node)
            _, rew, done, _ = sim.step(a)
            child.reward = rew
            if done:
                child.term, child.p = True, 0
                node, value = child, 0
                break
            node, d = child, d + 1
        while node is not None:
            value = node.reward + value
            node.n += 1
            node.w += value
            node = node.parent
    acts = list(root.children)
    visits = np.array([root.children[a].n for a in acts])
    x = 1.0 / 1e-5 * np.log(visits + 1e-10)
    p = np.exp(x - np.max(x))
    p /= np.sum(p)
    return int(rs.choice(acts, p=p)), root


@pytest.mark.gpu
def test_gpu_thousands_of_slots_match_a_host_restatement():
    """2 048 slots over the first decisions of 2 048 CUT-2 sequences (S = 6, k = 3, rollouts on) against the host
    restatement above over the oracle's Python env port: action, root n and root w bit for bit, every slot."""
    import torch
    import bpp_amd
    from bpp_amd import MCTSearch
    from bpp_amd.mcts import flat_policy
    from oracle.ref_port import PortBin
    size, n, k, S, decisions = (10, 10, 10), 2048, 3, 6, 3
    pool = bpp_amd.sequences.cut2_pool(size, n, seed=23)
    env = _gpu_env(pool, size, 2 * n)
    ms = MCTSearch(env, k, sim_times=S)
    seeds = np.arange(n) * 13 + 5
    ids = torch.arange(n, device="cuda")
    ms.seed(ids, torch.as_tensor(seeds))
    tpol = flat_policy(size)

    def evaluate(obs):
        v, lg, _ = tpol(torch.as_tensor(np.asarray(obs, np.float32))[None])
        x = lg[0].numpy()
        p = np.exp(x - np.max(x))
        p /= np.sum(p)
        return float(v[0]), p

    bins = [PortBin(pool, size, False, bin_id=b, total=2 * n) for b in range(n)]
    rss = [np.random.RandomState(int(s)) for s in seeds]
    roots = [HostNode(None, 1.0) for _ in range(n)]
    live = list(range(n))
    bad = []
    for t in range(decisions):
        lt = torch.as_tensor(live, device="cuda")
        act, vis = ms.decide(tpol, lt, lt + n)
        dn, dw, _, _ = ms.root_stats(lt)
        act = act.cpu().numpy()
        res = env.step_bins(lt, torch.as_tensor(act, device="cuda"))
        ms.advance(res.done)
        done = res.done.cpu().numpy()
        nxt = []
        for j, b in enumerate(live):
            a, root = host_decide(roots[b], bins[b], k, S, k - 1, -1, 1, rss[b], evaluate)
            if (a, root.n) != (int(act[j]), int(dn[j])) or np.float64(root.w).tobytes() != np.float64(dw[j]).tobytes():
                bad.append((b, t, (a, root.n, root.w), (int(act[j]), int(dn[j]), float(dw[j]))))
                continue
            _, _, d, _ = bins[b].step(a)
            assert bool(d) == bool(done[j]), (b, t)
            if not d:
                child = roots[b].children[a]
                child.p, child.parent = 1.0, None
                roots[b] = child
                nxt.append(b)
        assert not bad, bad[:5]
        live = nxt
    assert int(ms.overflow.item()) == 0
