"""MultiBinPacker -- the paper's multi-bin packing (multi_bin/multi_bin.py): a policy trained on w x w bins packs a larger
W x L pallet through sliding w x w windows, for a whole batch of pallets at once.

Per decision the pallet's heightmap is cut into K windows; the policy gives a value and a position in every window, and one
window is picked by an advantage rule that remembers, per window, the last reward and the last value (include/
bpp_multibin.h, csrc/bpp_multibin.inl).  A decision is emit -> the caller's forward -> choose, then the caller steps the
pallets and commits the step's done flags; nothing in between waits for the device.
"""
import ctypes

import torch

from . import _lib
from .reorder import check_policy_output


class MultiBinPacker(object):
    """Multi-bin packing over a BppVecEnv without rotation (item pool or stream supply; the packer never clones bins).

    MultiBinPacker(env, window=10, stride=10): windows of side `window` every `stride` cells, dx outer and dy inner
    (slipingWindow, multi_bin.py:10-20); K = ((W - w) // s + 1) * ((L - w) // s + 1) <= 256.

    decide(policy, ids=None, check=True) -> (action int64 [n], adv float64 [n], window int32 [n]) on the env's device, for
    pallets ids (None: every pallet, slot i = pallet i): multi_bin.get_action with the per-episode history of every pallet.
    policy(obs) gets float32 rows [n K, 4 w^2] -- row i K + k is window k of pallet ids[i] -- and returns (value [n K] or
    [n K, 1], logits [n K, w^2], pred) as the CNNPro heads of a w x w x H bin; pred is ignored (the reference evaluates with
    use_mask=False).  window -1: no window (action 0, adv -1e8).  check=True validates the ids (one host sync); with
    check=False a slot whose id lies outside [0, E) gets BPP_ACTION_NOOP and touches nothing.

    commit(done): after stepping the pallets with the actions -- env.step_bins(ids, action).done, or step_tensors(...).done
    when the decision covered the batch -- records the step's reward for the chosen windows and clears the history of the
    pallets whose episode ended.  reset(ids=None): clear the history of pallets ids (None: all).
    """

    def __init__(self, env, window=10, stride=10):
        if getattr(env, "can_rotate", False):
            raise ValueError("multi-bin packing supports pallets without rotation only (multi_bin.py has none)")
        if isinstance(window, (tuple, list)) or isinstance(stride, (tuple, list)):
            raise ValueError("window and stride are single integers: only square windows are defined")
        w, s = int(window), int(stride)
        if s < 1:
            raise ValueError("stride must be at least 1")
        if w < 1 or w > min(env.W, env.L):
            raise ValueError("window side must be in 1 .. min(W, L) = %d" % min(env.W, env.L))
        if w * w > 1024:
            raise ValueError("window area must be at most 1024")
        K = ((env.W - w) // s + 1) * ((env.L - w) // s + 1)
        if K > _lib.MULTIBIN_MAX_K:
            raise ValueError("%d windows: more than the %d one pallet may have" % (K, _lib.MULTIBIN_MAX_K))
        self.env, self.w, self.s, self.K = env, w, s, K
        sizes = (ctypes.c_int64 * 3)()
        _lib.check(env.lib.bpp_multibin_sizes(env.W, env.L, w, s, 0, env.E, sizes), env.lib)
        assert int(sizes[0]) == K
        self.state = torch.zeros((max(int(sizes[1]), 8) + 7) // 8, dtype=torch.float64, device=env.device)
        self._sets = {}
        self._pending = None

    @property
    def window_offsets(self):
        """(dx, dy) of every window, in window order."""
        env, w, s = self.env, self.w, self.s
        return [(dx, dy) for dx in range(0, env.W - w + 1, s) for dy in range(0, env.L - w + 1, s)]

    def _set(self, n):
        """Work buffers for n slots, made once per n."""
        ent = self._sets.get(n)
        if ent is None:
            env, dev = self.env, self.env.device
            sizes = (ctypes.c_int64 * 3)()
            _lib.check(env.lib.bpp_multibin_sizes(env.W, env.L, self.w, self.s, n, env.E, sizes), env.lib)
            ent = dict(work=torch.empty((max(int(sizes[2]), 16) + 15) // 16 * 16, dtype=torch.uint8, device=dev),
                       obs=torch.zeros((n * self.K, 4 * self.w * self.w), dtype=torch.float32, device=dev),
                       action=torch.zeros((n,), dtype=torch.int64, device=dev), adv=torch.zeros((n,), dtype=torch.float64, device=dev),
                       window=torch.zeros((n,), dtype=torch.int32, device=dev), all=None)
            self._sets[n] = ent
        return ent

    def _desc(self, ids, st):
        return _lib.MultiBin(ids.numel(), self.w, self.s, self.K, ids.data_ptr(), self.state.data_ptr(), st["work"].data_ptr())

    def _slots(self, ids):
        env = self.env
        if ids is None:
            st = self._set(env.E)
            if st["all"] is None:
                st["all"] = torch.arange(env.E, dtype=torch.int64, device=env.device)
            return st["all"], st
        ids = env._ids(ids)
        return ids, self._set(ids.numel())

    def decide(self, policy, ids=None, check=True):
        env = self.env
        if env._first_reset:
            raise RuntimeError("call env.reset() before decide()")
        ids, st = self._slots(ids)
        n = ids.numel()
        if check and ids is not st["all"]:
            env._check_ids(ids)
        m = self._desc(ids, st)
        L, b, mm = env.lib, env._batch_ref, ctypes.byref(m)
        env._on_device()
        stream = env._stream_ptr()
        obs = st["obs"]
        _lib.check(L.bpp_multibin_emit(b, mm, obs.data_ptr(), stream), L)
        value, logits, _ = check_policy_output(policy(obs), n * self.K, self.w * self.w)
        _lib.check(L.bpp_multibin_choose(b, mm, value.data_ptr(), logits.data_ptr(), st["action"].data_ptr(), st["adv"].data_ptr(),
                                         st["window"].data_ptr(), stream), L)
        self._pending = (ids, st)
        return st["action"].clone(), st["adv"].clone(), st["window"].clone()

    def commit(self, done):
        if self._pending is None:
            raise RuntimeError("commit() needs a decide() before it")
        ids, st = self._pending
        n = ids.numel()
        d = torch.as_tensor(done, device=self.env.device).reshape(-1)
        if d.numel() != n:
            raise ValueError("done must have one entry per slot of the last decide() (%d), got %d" % (n, d.numel()))
        if d.dtype != torch.uint8 or not d.is_contiguous():
            d = (d != 0).to(torch.uint8).contiguous()
        env = self.env
        m = self._desc(ids, st)
        env._on_device()
        _lib.check(env.lib.bpp_multibin_commit(env._batch_ref, ctypes.byref(m), d.data_ptr(), env._stream_ptr()), env.lib)
        self._pending = None

    def reset(self, ids=None):
        env = self.env
        ids_t = None if ids is None else env._ids(ids)
        st = self._set(0)
        m = _lib.MultiBin(0, self.w, self.s, self.K, None, self.state.data_ptr(), st["work"].data_ptr())
        env._on_device()
        _lib.check(env.lib.bpp_multibin_clear(env._batch_ref, ctypes.byref(m), None if ids_t is None else ids_t.data_ptr(),
                                              0 if ids_t is None else ids_t.numel(), env._stream_ptr()), env.lib)
