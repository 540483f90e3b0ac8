"""BranchOps -- native branch stepping (include/bpp_branch.h): step, observe and clone a subset of the bins of a batch.

The lookahead searches (reorder.py, mcts.py, multibin.py) stand on this surface and on nothing else of the env, and nothing
here cares on which device the tensors live: the class is mixed into BppVecEnv, and into the emulated env of the CPU tests.
"""
import ctypes

import torch

from . import _lib


class BranchOps(object):
    """step_bins / observe_bins / clone_bins / preview for the object it is mixed into.

    What this class and the three search modules require of that object -- stated here, once:
      device, E, W, L, A, M, obs_len, can_rotate, compute_mask
                      the device the tensors live on and the batch's geometry (A = W L, M = actions per bin, obs_len = 4 A)
      lib             the ctypes handle of the library that implements include/bpp_branch.h and the search headers
                      (_lib.bind_branch, bind_reorder, bind_multibin, bind_mcts)
      _batch_ref      ctypes.byref of the batch's bpp_batch
      _stream         the ctypes bpp_stream of a streaming env, or None
      state, pool     int32 [E, 12] bpp_env_state records; uint8 [rows, T, 4] item pool or ring
      _first_reset    True until the first reset()
      _serial         lock-steps issued so far
      _stepped()      called after every lock-step (streaming supply: the refill schedule)
      _on_device()    make the env's device the calling thread's current one
      _stream_ptr()   the stream to launch on as a c_void_p, or None for the default stream
    """
    NOOP = -2 ** 63      # BPP_ACTION_NOOP: this bin is not stepped (state untouched, reward 0, done 0, obs/mask re-emitted)

    # native branch stepping (include/bpp_branch.h): what the calls cost scales with the bins they list, not with the batch
    def _ids(self, ids):
        t = torch.as_tensor(ids, device=self.device).reshape(-1)
        if t.dtype != torch.int64 or not t.is_contiguous():
            t = t.to(torch.int64).contiguous()
        return t

    def _check_ids(self, ids, other=None):
        """ValueError unless every id (and every id of `other`) lies in [0, E), the ids are distinct and none of them is in
        `other` -- one device-to-host copy of three flags."""
        flags = torch.zeros((3,), dtype=torch.bool, device=self.device)
        both = ids if other is None else torch.cat([ids, other])
        if both.numel():
            flags[0] = ((both < 0) | (both >= self.E)).any()
        if ids.numel():
            s = torch.sort(ids).values
            flags[1] = (s[1:] == s[:-1]).any()
            if other is not None and other.numel():
                flags[2] = torch.isin(ids, other).any()
        out_of_range, dup, overlap = flags.tolist()
        if out_of_range:
            raise ValueError("bin ids must lie in [0, %d)" % self.E)
        if dup:
            raise ValueError("bin ids must be distinct")
        if overlap:
            raise ValueError("dst must be disjoint from src")

    def _branch_out(self, n):
        """The compact output set of step_bins for `n` rows (StepTensors over one allocation, bpp_step_out), made once per n."""
        sets = self.__dict__.setdefault("_branch_sets", {})
        ent = sets.get(n)
        if ent is None:
            from .vec_env import StepTensors     # (vec_env imports this module)
            regions, total = {}, 0
            fields = [("obs", torch.float32, (n, self.obs_len), 4)]
            if self.compute_mask:
                fields.append(("mask", torch.float32, (n, self.M), 4))
            fields += [("reward", torch.float32, (n, 1), 4), ("done", torch.uint8, (n,), 1), ("counter", torch.int32, (n,), 4),
                       ("ratio", torch.float64, (n,), 8), ("ep_ret", torch.float64, (n,), 8), ("ep_len", torch.int32, (n,), 4)]
            for name, dtype, shape, width in fields:
                nbytes = width
                for d in shape:
                    nbytes *= d
                regions[name] = (total, dtype, shape, nbytes)
                total += (nbytes + 255) // 256 * 256
            flat = torch.empty((max(total, 256),), dtype=torch.uint8, device=self.device)
            base = flat.data_ptr()
            out = _lib.StepOut(*[(base + regions[k][0] if k in regions else None)
                                 for k in ("obs", "mask", "reward", "done", "counter", "ratio", "ep_ret", "ep_len")])
            ent = sets[n] = (StepTensors(_flat=flat, _layout=regions), out)
        return ent

    @property
    def bad_ids(self):
        """int32 [1] device tensor: slots of step_bins / observe_bins calls whose id lay outside [0, E) (check=False lets them
        through; such a slot returns the outputs of a no-op of an empty bin and touches no bin).  Cumulative; zero it to restart."""
        t = self.__dict__.get("_bad_ids")
        if t is None:
            t = self._bad_ids = torch.zeros((1,), dtype=torch.int32, device=self.device)
        return t

    def step_bins(self, ids, actions, sample=None, check=True):
        """Step only bins `ids` (int [n]) with `actions` (int [n]; BPP_ACTION_NOOP = `NOOP` re-emits without stepping): the
        native form of step_subset (bpp_step_subset).  ONE launch over the n bins; no other bin is read or written.  Returns
        StepTensors with n rows -- obs [n,4A], mask [n,M], reward [n,1], done, counter, ratio, ep_ret, ep_len -- where row i is
        what step_subset returns in row ids[i].  The compact buffers are kept per n: the result is valid until the next
        step_bins / observe_bins call with the same n.  sample=(seed, step, out): also draw the uniform-feasible action of
        every new observation into int64 tensor `out` [n] (== step_subset's draw for bin ids[i]).
        Never synchronises, except for check=True, which raises ValueError unless the ids lie in [0, E) and are distinct
        (check=False: an id out of range yields a no-op row and counts in `bad_ids`; duplicates race).  Counts as one
        lock-step (streaming supply: a bin advances at most one episode per call).  The full-batch outputs of the last
        step / observe() (`location_masks`, its obs) are NOT updated: they are stale for the stepped bins until the next
        step or observe()."""
        if self._first_reset:
            raise RuntimeError("call reset() before step_bins()")
        ids = self._ids(ids)
        a = torch.as_tensor(actions, device=self.device).reshape(-1)
        if a.dtype != torch.int64 or not a.is_contiguous():
            a = a.to(torch.int64).contiguous()
        n = ids.numel()
        if a.numel() != n:
            raise ValueError("ids and actions must have the same length")
        if check:
            self._check_ids(ids)
        res, out = self._branch_out(n)
        if sample is not None:
            seed, step, nxt = sample
            if nxt.device != self.device or nxt.dtype != torch.int64 or nxt.numel() != n or not nxt.is_contiguous():
                raise ValueError("sample out tensor must be a contiguous int64 [n] tensor on the env's device")
            if not self.compute_mask:
                raise RuntimeError("sample= needs compute_mask=True")
            out.next_action, out.sample_seed, out.sample_step = nxt.data_ptr(), int(seed), int(step)
        else:
            out.next_action = None
        self._on_device()
        rc = self.lib.bpp_step_subset(self._batch_ref, ids.data_ptr(), n, a.data_ptr(), ctypes.byref(out), self.bad_ids.data_ptr(),
                                      self._stream_ptr())
        if rc:
            _lib.check(rc, self.lib)
        self._serial += 1
        self._stepped()
        return res

    def observe_bins(self, ids, check=True):
        """Compact observation and mask of bins `ids` without stepping them (step_bins with every action BPP_ACTION_NOOP):
        what a search reads after clone_bins / set_current_items."""
        ids = self._ids(ids)
        return self.step_bins(ids, torch.full((ids.numel(),), self.NOOP, dtype=torch.int64, device=self.device), check=check)

    def clone_bins(self, src, dst, check=True):
        """Bins `dst` become exact copies of bins `src` -- copy_bins in ONE launch (bpp_copy_bins): heightmap and record, in
        streaming mode also the bin's ring rows, generator record and progress (seq rebased to dst's ring column); only
        dst's row-cache lines are dropped.  Nothing is re-emitted: pair it with observe_bins(dst).  The pairs are copied
        concurrently, so dst must be distinct and disjoint from src; check=True raises ValueError otherwise (and for ids
        outside [0, E)), check=False skips that synchronisation (pairs with an id out of range are skipped)."""
        src, dst = self._ids(src), self._ids(dst)
        if src.numel() != dst.numel():
            raise ValueError("src and dst must have the same length")
        if check:
            self._check_ids(dst, other=src)
        self._on_device()
        rc = self.lib.bpp_copy_bins(self._batch_ref, ctypes.byref(self._stream) if self._stream is not None else None, src.data_ptr(),
                                    dst.data_ptr(), src.numel(), self._stream_ptr())
        if rc:
            _lib.check(rc, self.lib)

    def preview(self, k):
        """The next `k` items of every bin, int32 [E, k, 3] -- `box_creator.preview(k)`
        (envs/bpp0/binCreator.py:15-18) for all bins at once (the terminator repeats past the end)."""
        st = self.state
        cursor, seq = st[:, 0].long(), st[:, 7].long()
        T = self.pool.shape[1]
        hdr = 2 if self._stream is not None else 0       # ring rows start with two look-ahead entries (include/bpp_abi.h)
        idx = hdr + torch.clamp(cursor.unsqueeze(1) + torch.arange(int(k), device=self.device).unsqueeze(0), max=T - 1 - hdr)
        return self.pool[seq.unsqueeze(1), idx][:, :, :3].to(torch.int32)
