"""MCTSearch -- the reference's Monte Carlo tree search (MCTS/monteCarlo.py MCTree, MCTS/node.py PutNode, driven as
MCTS/mcts_test.py:14-65 drives them) for a whole batch of bins at once.

Every bin's tree and random stream live on the device (include/bpp_mcts.h, csrc/bpp_mcts.inl); the copy.deepcopy(env)
of every simulation is a scratch bin of the same BppVecEnv, cloned and stepped with the native branch calls
(include/bpp_branch.h).  A decision is a fixed schedule of launches and the only thing between two of them is the
caller's batched forward, so `decide` enqueues a whole decision without waiting for the device.
"""
import ctypes

import torch

from . import _lib
from .reorder import check_ids, check_policy_output

# byte layout of the state buffer (csrc/bpp_mcts.inl): MBin [E] (192 bytes), MT words [E][640], pools [E][2][cap] x 32 bytes
_BIN_BYTES, _MT_WORDS, _REC_BYTES = 192, 640, 32


def flat_policy(size):
    """A stand-in for the CNN whose softmax is exact on both sides (tests/golden/make_mcts_golden.py records the reference
    under it; tools/bench_mcts.py times the search under it).  For an observation row (plane 0 heights h, item x, y, z):
      s = sum(h) + 3x + 5y + 7z;  logits[a] = 0 where (37 a + s) mod 11 < 4 or a = s mod A, else -1e4;
      value = ((7 s) mod 41 - 10) / 256.
    exp(-1e4) is 0 in float32, so the softmax is exactly 1/c on the c selected positions, feasible or not.
    Returns policy(obs) -> (value f32 [n], logits f32 [n, A], None) on obs's device."""
    W, L, H = (int(v) for v in size)
    A = W * L

    def policy(obs):
        o = obs.reshape(-1, 4, A).to(torch.int64)
        s = o[:, 0].sum(1) + 3 * o[:, 1, 0] + 5 * o[:, 2, 0] + 7 * o[:, 3, 0]
        a = torch.arange(A, dtype=torch.int64, device=obs.device)
        sel = (torch.remainder(37 * a[None] + s[:, None], 11) < 4) | (a[None] == torch.remainder(s, A)[:, None])
        logits = torch.where(sel, torch.zeros((), device=obs.device), torch.full((), -1e4, device=obs.device)).to(torch.float32)
        value = ((torch.remainder(7 * s, 41) - 10).to(torch.float64) / 256.0).to(torch.float32)
        return value, logits, None
    return policy


class MCTSearch(object):
    """Batched MCTS over a BppVecEnv (no rotation, W*L <= 1024; item pool or streaming supply).

    MCTSearch(env, k, sim_times=100, search_depth=None, rollout_length=-1, credit=1.0, zeta=1e-5): the parameters of MCTree
    and mcts_test.test -- k known items (2 .. 16), max_depth = min(search_depth, k - 1) (k - 1 for None), rollout_length -1
    (to the end of the known items), None or 0 (no rollout) or r >= 1, credit in [0, 1], play()'s temperature zeta.

    decide(policy, ids, scratch) -> (action int64 [n], root_visits int32 [n]) on the env's device: for every real bin
    ids[i], sim_times simulations of the bin's tree (MCTree.get_policy) and the sampled action (sample_action).  scratch[i]
    is a bin of the same env that the search overwrites: the scratch bins must be distinct and disjoint from ids, and their
    heightmaps, records and Monitor sums are garbage afterwards.  The real bins are only read.
    advance(done): after the caller stepped the real bins with the actions (env.step_bins(ids, action).done), the chosen
    child becomes each tree's root (MCTree.succeed); a bin whose episode ended starts its next decision with a fresh tree.
    reset(ids=None): drop the trees of bins ids (None: all).  seed(ids, seeds): np.random.seed(seeds[j]) for bin ids[j].
    The random streams continue across decisions and episodes; reset does not reseed.  Every bin starts seeded with its id.

    policy(obs) gets float32 observation rows [n, 4A] and returns (value [n] or [n, 1], logits [n, A], pred [n, A] or None):
    the CNNPro heads (reorder.check_policy_output).  The search uses nmodel.evaluate(obs, False): the float32 softmax of
    the logits; pred is ignored.  With the real network the softmax is not bit-exact against numpy's (expf, and a
    different summation order), so decisions can differ from the reference where two children tie within rounding.

    Memory: bpp_mcts_sizes gives cap = 1 + (max_depth + 1) * sim_times * (W L + 1) records of 32 bytes per pool half, for
    every bin of the env (real and scratch, since any bin may be listed in ids): 2 * cap * 32 bytes + 2.7 KB per bin, 2.6 MB
    at 10x10 and the defaults.  With the usual layout -- real bins [0, n), scratch bins [n, 2n) -- the scratch bins' half
    of that memory never holds a tree: E = 2n bins need 5.2 MB * n, so n = 16 384 slots take 85 GB of the MI355X's 288 GB,
    42 GB of it idle.
    `overflow` (int32 [1] on the device) counts slots whose pool half ran out during a decision (that slot's search stops);
    it stays 0 with the pool sizes bpp_mcts_sizes gives.  No host synchronisation: a decision is enqueued on the current
    stream (check=True spends one on validating ids and scratch).
    """

    def __init__(self, env, k, sim_times=100, search_depth=None, rollout_length=-1, credit=1.0, zeta=1e-5):
        if getattr(env, "can_rotate", False):
            raise ValueError("MCTS supports bins without rotation only (node.py masks W*L positions)")
        k = int(k)
        if not 2 <= k <= _lib.MCTS_MAX_K:
            raise ValueError("k must be in 2 .. %d, got %d" % (_lib.MCTS_MAX_K, k))
        if int(sim_times) < 1:
            raise ValueError("sim_times must be positive")
        max_depth = k - 1 if search_depth is None else min(int(search_depth), k - 1)
        if max_depth < 0:
            raise ValueError("search_depth must be non-negative")
        r = 0 if rollout_length is None else int(rollout_length)
        if r < -1:
            raise ValueError("rollout_length must be -1, None, 0 or positive")
        if not 0.0 <= float(credit) <= 1.0:
            raise ValueError("credit must be in [0, 1]")
        if not float(zeta) > 0.0:
            raise ValueError("zeta must be positive")
        self.env, self.k, self.sim_times, self.max_depth, self.rollout_length = env, k, int(sim_times), max_depth, r
        self.credit, self.zeta = float(credit), float(zeta)
        sizes = (ctypes.c_int64 * 4)()
        _lib.check(env.lib.bpp_mcts_sizes(env.E, k, self.sim_times, max_depth, r, env.W, env.L, sizes), env.lib)
        self.nbytes, self.cap, self.bin_bytes, self.rollout_levels = (int(v) for v in sizes)
        dev = env.device
        self.state = torch.zeros(((self.nbytes + 15) // 16 * 16,), dtype=torch.uint8, device=dev)
        self.overflow = torch.zeros((1,), dtype=torch.int32, device=dev)
        self._sets = {}
        self._pending = None
        all_ids = torch.arange(env.E, dtype=torch.int64, device=dev)
        self.seed(all_ids, all_ids)

    def _desc(self, n, ids=None, scratch=None):
        return _lib.Mcts(n, self.k, self.sim_times, self.max_depth, self.rollout_length, self.cap, self.credit, self.zeta,
                         None if ids is None else ids.data_ptr(), None if scratch is None else scratch.data_ptr(),
                         self.state.data_ptr(), self.overflow.data_ptr(), 0)

    def _set(self, n):
        ent = self._sets.get(n)
        if ent is None:
            dev, env = self.env.device, self.env
            ent = dict(obs=torch.zeros((n, env.obs_len), dtype=torch.float32, device=dev),
                       actions=torch.zeros((n,), dtype=torch.int64, device=dev),
                       action=torch.zeros((n,), dtype=torch.int64, device=dev),
                       visits=torch.zeros((n,), dtype=torch.int32, device=dev))
            self._sets[n] = ent
        return ent

    def seed(self, ids, seeds):
        """np.random.seed(seeds[j]) for bin ids[j]; the trees are left alone.  ValueError for a seed outside [0, 2^32), as
        np.random.seed raises (one host sync)."""
        env = self.env
        ids = env._ids(ids)
        s = torch.as_tensor(seeds, device=env.device).reshape(-1)
        if s.numel() != ids.numel():
            raise ValueError("ids and seeds must have the same length")
        if s.is_floating_point() or s.dtype == torch.bool:
            raise ValueError("seeds must be integers")
        s = s.to(torch.int64)
        if s.numel() and bool(((s < 0) | (s > 0xFFFFFFFF)).any()):
            raise ValueError("seeds must lie in [0, 2**32)")
        s = torch.where(s > 0x7FFFFFFF, s - (1 << 32), s).to(torch.int32).contiguous()     # the uint32 bit pattern
        m = self._desc(0)
        _lib.check(env.lib.bpp_mcts_seed(env._batch_ref, ctypes.byref(m), ids.data_ptr(), s.data_ptr(), ids.numel(), env._stream_ptr()), env.lib)

    def reset(self, ids=None):
        """Drop the trees of bins ids (None: every bin); the random streams continue."""
        env = self.env
        ids_t = None if ids is None else env._ids(ids)
        m = self._desc(0)
        _lib.check(env.lib.bpp_mcts_clear(env._batch_ref, ctypes.byref(m), None if ids_t is None else ids_t.data_ptr(),
                                          0 if ids_t is None else ids_t.numel(), env._stream_ptr()), env.lib)
        self._pending = None

    def decide(self, policy, ids, scratch, check=True):
        env = self.env
        if env._first_reset:
            raise RuntimeError("call env.reset() before decide()")
        ids, scratch = env._ids(ids), env._ids(scratch)
        n = ids.numel()
        if check:
            check_ids(ids, scratch, env.E)
        elif scratch.numel() != n:
            raise ValueError("ids and scratch must have the same length")
        st = self._set(n)
        m = self._desc(n, ids, scratch)
        L, b, mr = env.lib, env._batch_ref, ctypes.byref(m)
        obs, actions, A = st["obs"], st["actions"], env.A
        env._on_device()
        stream = env._stream_ptr()
        _lib.check(L.bpp_mcts_begin(b, mr, stream), L)
        for _ in range(self.sim_times):
            env.clone_bins(ids, scratch, check=False)                 # select()'s copy.deepcopy(sim_env)
            done = None
            for level in range(self.max_depth):
                _lib.check(L.bpp_mcts_select(b, mr, level, done, actions.data_ptr(), stream), L)
                done = env.step_bins(scratch, actions, check=False).done.data_ptr()
            _lib.check(L.bpp_mcts_emit(b, mr, 0, done, obs.data_ptr(), stream), L)
            value, logits, _ = check_policy_output(policy(obs), n, A)
            _lib.check(L.bpp_mcts_expand(b, mr, value.data_ptr(), logits.data_ptr(), actions.data_ptr(), stream), L)
            done = None
            for level in range(1, self.rollout_levels):
                done = env.step_bins(scratch, actions, check=False).done.data_ptr()
                _lib.check(L.bpp_mcts_emit(b, mr, level, done, obs.data_ptr(), stream), L)
                value, logits, _ = check_policy_output(policy(obs), n, A)
                _lib.check(L.bpp_mcts_rollout(b, mr, value.data_ptr(), logits.data_ptr(), actions.data_ptr(), stream), L)
            if self.rollout_levels > 0:
                done = env.step_bins(scratch, actions, check=False).done.data_ptr()
            _lib.check(L.bpp_mcts_backup(b, mr, done, stream), L)
        _lib.check(L.bpp_mcts_finish(b, mr, st["action"].data_ptr(), st["visits"].data_ptr(), stream), L)
        self._pending = (ids, scratch)
        return st["action"].clone(), st["visits"].clone()

    def advance(self, done):
        """After stepping the real bins of the last decide with its actions: MCTree.succeed, or a dropped tree where `done`."""
        if self._pending is None:
            raise RuntimeError("advance() needs a decide() before it")
        env = self.env
        ids, scratch = self._pending
        d = torch.as_tensor(done, device=env.device).reshape(-1)
        if d.numel() != ids.numel():
            raise ValueError("done must have one entry per slot of the last decide")
        d = d.to(torch.uint8).contiguous()
        m = self._desc(ids.numel(), ids, scratch)
        _lib.check(env.lib.bpp_mcts_advance(env._batch_ref, ctypes.byref(m), d.data_ptr(), env._stream_ptr()), env.lib)
        self._pending = None

    def root_stats(self, ids):
        """(n int32 [m], w float64 [m], children int32 [m], mt position int32 [m]) of the roots of bins ids, as numpy arrays:
        the bins' records and their root and header records are gathered on the device, then copied (one sync);
        children = 0 for a bin without an expanded root."""
        env = self.env
        ids = env._ids(ids)
        E, st, dev = env.E, self.state, env.device
        rec = st[:E * _BIN_BYTES].view(torch.int32).view(E, _BIN_BYTES // 4)[ids]
        half, pos = rec[:, 1].to(torch.int64), rec[:, 3]
        pool0 = E * _BIN_BYTES + E * _MT_WORDS * 4
        base = pool0 + (ids * 2 + half) * (self.cap * _REC_BYTES)
        root = st[base[:, None] + torch.arange(_REC_BYTES, device=dev)[None]]
        w = root[:, :8].contiguous().view(torch.float64)[:, 0]
        nb = root[:, 16:24].contiguous().view(torch.int32)
        n, blk = nb[:, 0], nb[:, 1]
        hb = base + blk.clamp(min=0).to(torch.int64) * _REC_BYTES + 16
        ch = st[hb[:, None] + torch.arange(4, device=dev)[None]].contiguous().view(torch.int32)[:, 0]
        ch = torch.where(blk >= 0, ch, torch.zeros_like(ch))
        return tuple(t.cpu().numpy() for t in (n, w, ch, pos))
