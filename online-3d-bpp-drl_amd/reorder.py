"""ReorderSearch -- the BPP-k lookahead of the paper (`main.py --mode test --preview k`): one acktr/reorder.py ReorderTree
per item, as unified_test.py:9-27 builds it, for a whole batch of bins at once.

Every bin's tree lives on the device (include/bpp_reorder.h, csrc/bpp_reorder.inl); its copy.deepcopy(env) branches are
scratch bins of the same BppVecEnv, cloned and stepped with the native branch calls (include/bpp_branch.h).  A decision
is a fixed schedule of launches -- k baseline levels, then `times` iterations of a copy and k levels -- and the only thing
between two levels is the caller's batched forward, so `decide` enqueues a whole decision without waiting for the device.
"""
import ctypes
import math

import torch

from . import _lib


def int_policy(size, mask_fn=None):
    """A deterministic stand-in for the CNN, exact in int64 so that numpy, the reference's post-processing and torch on the
    device agree bit for bit (tests/golden/make_reorder_golden.py records the reference under it; tools/bench_reorder.py
    times the search under it).  For an observation row (plane 0 heights h, item x, y, z):
      s = sum(h) + 3x + 5y + 7z;  logits[a] = ((37 a + s) mod A) / 8  (distinct values: gcd(37, A) = 1);
      pred[a] = feasible[a] and (h[a] + a + s) mod 7 != 0, all zero when s mod 97 == 0;  value = ((7 s) mod 41 - 10) / 256,
    feasible = get_possible_position(obs) (acktr/utils.py, batched_mask_from_obs) so that episodes run until the bin is full.
    mask_fn(obs [n, 4A] float32) -> float32 [n, A]: the feasibility mask (default: batched_mask_from_obs on the device).
    Returns policy(obs) -> (value f32 [n], logits f32 [n, A], pred f32 [n, A]) on obs's device."""
    W, L, H = (int(v) for v in size)
    A = W * L
    if math.gcd(37, A) != 1:
        raise ValueError("int_policy needs gcd(37, W*L) = 1")
    if mask_fn is None:
        from .masks import batched_mask_from_obs

        def mask_fn(obs):
            return batched_mask_from_obs(obs, (W, L, H))

    def policy(obs):
        o = obs.reshape(-1, 4, A).to(torch.int64)
        h = o[:, 0]
        s = h.sum(1) + 3 * o[:, 1, 0] + 5 * o[:, 2, 0] + 7 * o[:, 3, 0]
        a = torch.arange(A, dtype=torch.int64, device=obs.device)
        logits = torch.remainder(37 * a[None] + s[:, None], A).to(torch.float32) / 8.0
        feas = torch.as_tensor(mask_fn(obs), device=obs.device) > 0.5
        pred = (feas & (torch.remainder(h + a[None] + s[:, None], 7) != 0) & (torch.remainder(s[:, None], 97) != 0)).to(torch.float32)
        value = ((torch.remainder(7 * s, 41) - 10).to(torch.float64) / 256.0).to(torch.float32)
        return value, logits, pred
    return policy


def check_policy_output(out, n, A):
    """(value f32 [n], logits f32 [n, A], pred f32 [n, A] or None), contiguous, from what a policy returned:
    (value [n] or [n, 1], logits [n, A], pred [n, A] or None).  ValueError for any other shape."""
    if not isinstance(out, (tuple, list)) or len(out) != 3:
        raise ValueError("policy(obs) must return (value, logits, pred)")
    value, logits, pred = out
    if not (torch.is_tensor(value) and torch.is_tensor(logits)):
        raise ValueError("policy(obs): value and logits must be tensors")
    if tuple(value.shape) not in ((n,), (n, 1)):
        raise ValueError("policy(obs): value must have shape [n] or [n, 1] (n = %d), got %r" % (n, tuple(value.shape)))
    if tuple(logits.shape) != (n, A):
        raise ValueError("policy(obs): logits must have shape [n, A] = [%d, %d], got %r" % (n, A, tuple(logits.shape)))
    if pred is not None:
        if not torch.is_tensor(pred) or tuple(pred.shape) != (n, A):
            raise ValueError("policy(obs): pred must be None or have shape [n, A] = [%d, %d]" % (n, A))
        pred = pred.detach().to(torch.float32).contiguous()
    return (value.detach().reshape(n).to(torch.float32).contiguous(), logits.detach().to(torch.float32).contiguous(), pred)


def check_ids(ids, scratch, num_envs):
    """ValueError unless ids and scratch (int64 tensors) have the same length, lie in [0, num_envs), are distinct and are
    disjoint: one device-to-host copy of a few flags."""
    if ids.numel() != scratch.numel():
        raise ValueError("ids and scratch must have the same length")
    both = torch.cat([ids, scratch])
    if both.numel() == 0:
        return
    s = torch.sort(both).values
    flags = torch.stack([((both < 0) | (both >= num_envs)).any(), (s[1:] == s[:-1]).any()]).tolist()
    if flags[0]:
        raise ValueError("bin ids must lie in [0, %d)" % num_envs)
    if flags[1]:
        raise ValueError("ids and scratch must be distinct bins, and scratch must not overlap ids")


class ReorderSearch(object):
    """BPP-k reorder search over a BppVecEnv (no rotation, item-pool supply).

    ReorderSearch(env, k, times=100, v_bound=0.1): k previewed items (1 .. 8), min(times, (k-1)!) search iterations
    (acktr/reorder.py:75), the conservative rule's threshold v_bound.

    decide(policy, ids, scratch) -> (action int64 [n], value float64 [n], default bool [n]) on the env's device: for every
    real bin ids[i], ReorderTree(nmodel, env.preview(k)[ids[i]], bin, times).reorder_search() -- the action to step it
    with, max_exp, and whether the action is the greedy baseline's.  scratch[i] is a bin of the same env that the search
    overwrites: the scratch bins must be distinct and disjoint from ids.  Their heightmaps, records and Monitor sums
    (ep_acc, episode counters) are garbage afterwards.  The real bins are only read.

    policy(obs) gets float32 observation rows [n, 4A] (plane 0 mixed with the masks of the items still to come:
    reorder.py:104-110) and returns (value [n] or [n, 1], logits [n, A], pred [n, A] or None): the CNNPro heads.  The
    position of a row is model_loader.evaluate(use_mask=True): argmax of softmax(logits) * (pred >= 0.5) in float32 --
    np.argmax in the baseline, argsort(...)[-1] in the search (an all-zero row gives A - 1, what numpy sorts last for
    A <= 256; ties between equal positive maxima are left to the kernel's order).

    No host synchronisation: a decision is enqueued on the current stream (check=True spends one on validating ids and
    scratch).  `overflow` (int32 [1] on the device) counts slots whose node pool ran out; it stays 0 with the pool sizes
    bpp_reorder_sizes gives.
    """

    def __init__(self, env, k, times=100, v_bound=0.1):
        if getattr(env, "can_rotate", False):
            raise ValueError("the reorder search supports bins without rotation only (acktr/reorder.py indexes an A-sized mask)")
        k = int(k)
        if not 1 <= k <= _lib.REORDER_MAX_K:
            raise ValueError("k must be in 1 .. %d, got %d" % (_lib.REORDER_MAX_K, k))
        if int(times) < 1:
            raise ValueError("times must be positive")
        if getattr(env, "_stream", None) is not None:
            raise ValueError("the reorder search needs an env over an item pool; a streaming env's clones would have to "
                             "continue the source's ring (not supported)")
        self.env, self.k, self.v_bound = env, k, float(v_bound)
        self.times = min(int(times), math.factorial(k - 1))
        self._sets = {}
        self.overflow = None

    def _set(self, n):
        """Work buffers for n slots, made once per n."""
        ent = self._sets.get(n)
        if ent is None:
            env = self.env
            sizes = (ctypes.c_int64 * 3)()
            _lib.check(env.lib.bpp_reorder_sizes(n, self.k, self.times, env.W, env.L, sizes), env.lib)
            assert int(sizes[1]) == self.times
            dev = env.device
            if self.overflow is None:
                self.overflow = torch.zeros((1,), dtype=torch.int32, device=dev)
            ent = dict(work=torch.empty((max(int(sizes[0]), 16) + 15) // 16 * 16, dtype=torch.uint8, device=dev),
                       nodes=int(sizes[2]), obs=torch.zeros((n, env.obs_len), dtype=torch.float32, device=dev),
                       actions=torch.zeros((n,), dtype=torch.int64, device=dev), action=torch.zeros((n,), dtype=torch.int64, device=dev),
                       value=torch.zeros((n,), dtype=torch.float64, device=dev), default=torch.zeros((n,), dtype=torch.uint8, device=dev))
            self._sets[n] = ent
        return ent

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
        r = _lib.Reorder(n, self.k, self.times, st["nodes"], self.v_bound, ids.data_ptr(), scratch.data_ptr(),
                         st["work"].data_ptr(), self.overflow.data_ptr(), 0)
        L, b, rr = env.lib, env._batch_ref, ctypes.byref(r)
        obs, actions = st["obs"], st["actions"]
        env._on_device()
        stream = env._stream_ptr()
        _lib.check(L.bpp_reorder_begin(b, rr, stream), L)
        done = None
        for it in range(-1, self.times):
            env.clone_bins(ids, scratch, check=False)                 # copy.deepcopy(self.env)
            for level in range(self.k):
                _lib.check(L.bpp_reorder_emit(b, rr, it, level, done, obs.data_ptr(), stream), L)
                value, logits, pred = check_policy_output(policy(obs), n, env.A)
                _lib.check(L.bpp_reorder_choose(b, rr, value.data_ptr(), logits.data_ptr(),
                                                None if pred is None else pred.data_ptr(), actions.data_ptr(), stream), L)
                res = env.step_bins(scratch, actions, check=False)
                done = res.done.data_ptr()
        _lib.check(L.bpp_reorder_commit(b, rr, done, stream), L)
        _lib.check(L.bpp_reorder_finish(b, rr, st["action"].data_ptr(), st["value"].data_ptr(), st["default"].data_ptr(), stream), L)
        return st["action"].clone(), st["value"].clone(), st["default"].clone().to(torch.bool)
