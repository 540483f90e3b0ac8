"""Packing plans (include/bpp_placements.h): where every box of every bin was placed -- the reference's `space.boxes` and
`space.flags` (envs/bpp0/space.py:23-24,176-177) for a whole batch.

PlacementLog    the device log of an env that records (BppVecEnv.record_placements): note / commit around every lock-step.
PackingPlans    what BppVecEnv.placements() returns: compact rows of records, their counts and episode indices.
replay_plans    heightmaps rebuilt from plans, every box checked (bpp_placements_replay): the verifier.
"""
import numpy as np
import torch

from . import _lib
from ._front import stream_ptr

RECORD_DTYPE = np.dtype([("x", "u1"), ("y", "u1"), ("z", "u1"), ("lz", "u1"), ("cell", "<u2"), ("rotated", "u1"), ("pad", "u1")])


def default_capacity(size):
    """Records kept per plan where nothing is asked for: an episode can hold more boxes than a pool row has entries (the
    terminator of a short pool may be a placeable item), so this follows the bin, not the pool."""
    W, L, H = (int(v) for v in size)
    return min(W * L * H, 256)


class PlacementLog(object):
    """The opaque log of bpp_placements.h for E bins as one uint8 device tensor, and the calls on it.  `owner` supplies lib,
    device, _batch_ref, _on_device() and _stream_ptr() (BppVecEnv, or the emulated env of the CPU tests)."""

    def __init__(self, owner, capacity, keep_finished=True):
        self.owner, self.lib = owner, owner.lib
        self.E, self.capacity, self.keep = int(owner.E), int(capacity), int(bool(keep_finished))
        nbytes = self.lib.bpp_placements_sizes(self.E, self.capacity, self.keep)
        if nbytes <= 0:
            _lib.check(int(nbytes), self.lib)
        self.buf = torch.zeros((int(nbytes),), dtype=torch.uint8, device=owner.device)     # (torch allocations are 16-byte aligned)
        self.ptr = self.buf.data_ptr()
        self.clear()

    @property
    def overflow(self):
        """int32 [1] view of the log's overflow counter: records dropped because a plan outgrew `capacity`."""
        return self.buf[-8:-4].view(torch.int32)

    def clear(self):
        self.owner._on_device()
        _lib.check(self.lib.bpp_placements_clear(self.ptr, self.E, self.capacity, self.keep, self.owner._stream_ptr()), self.lib)

    def note(self, ids_ptr, n, actions_ptr, stream):
        rc = self.lib.bpp_placements_note(self.owner._batch_ref, ids_ptr, n, actions_ptr, self.ptr, self.capacity, self.keep, stream)
        if rc:
            _lib.check(rc, self.lib)

    def commit(self, ids_ptr, n, done_ptr, stream):
        rc = self.lib.bpp_placements_commit(self.owner._batch_ref, ids_ptr, n, done_ptr, self.ptr, self.capacity, self.keep, stream)
        if rc:
            _lib.check(rc, self.lib)

    def copy(self, src, dst):
        """int64 device tensors src, dst [n]: the plans of bins dst become those of bins src."""
        self.owner._on_device()
        _lib.check(self.lib.bpp_placements_copy(self.ptr, src.data_ptr(), dst.data_ptr(), src.numel(), self.E, self.capacity, self.keep,
                                                self.owner._stream_ptr()), self.lib)

    def gather(self, ids=None, finished=False, size=None):
        dev = self.buf.device
        n = self.E if ids is None else ids.numel()
        records = torch.empty((n, self.capacity, _lib.PLACEMENT_BYTES), dtype=torch.uint8, device=dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        episode = torch.empty((n,), dtype=torch.int32, device=dev)
        self.owner._on_device()
        _lib.check(self.lib.bpp_placements_gather(self.ptr, ids.data_ptr() if ids is not None else None, n,
                                                  _lib.PLAN_FINISHED if finished else _lib.PLAN_RUNNING, records.data_ptr(), self.capacity,
                                                  count.data_ptr(), episode.data_ptr(), self.E, self.capacity, self.keep,
                                                  self.owner._stream_ptr()), self.lib)
        return PackingPlans(records, count, episode, self.overflow.clone(), size, ids)


class PackingPlans(object):
    """Plans of n bins.  records: uint8 [n, capacity, 8] (bpp_placement: x, y, z, lz, cell uint16, rotated, pad; zero from the
    count on); count: int32 [n] boxes of each plan (-1: no finished episode yet; beyond capacity: the rest was dropped);
    episode: int32 [n]; overflow: the log's shared counter of dropped records; size: (W, L, H); ids: the bins, or None for all."""

    def __init__(self, records, count, episode, overflow, size, ids=None):
        self.records, self.count, self.episode, self.overflow = records, count, episode, overflow
        self.size = tuple(int(v) for v in size)
        self.ids = ids
        self._np = None

    @property
    def capacity(self):
        return int(self.records.shape[1])

    def __len__(self):
        return int(self.records.shape[0])

    def numpy(self):
        """{'records': structured [n, capacity] (RECORD_DTYPE), 'count', 'episode', 'overflow', 'size'} on the host (one copy, kept)."""
        if self._np is None:
            def host(t):
                return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
            rec = np.ascontiguousarray(host(self.records)).view(RECORD_DTYPE).reshape(len(self), self.capacity)
            self._np = dict(records=rec, count=host(self.count).astype(np.int32), episode=host(self.episode).astype(np.int32),
                            overflow=np.asarray(host(self.overflow), np.int32).reshape(-1), size=np.asarray(self.size, np.int32))
        return self._np

    def _rows(self, i):
        h = self.numpy()
        n = min(max(int(h["count"][i]), 0), self.capacity)
        return h["records"][i, :n]

    def boxes(self, i):
        """Plan i as the reference's list: (x, y, z, lx, ly, lz) per box, the order of Box.standardize() (space.py:15-16)."""
        r = self._rows(i)
        L = self.size[1]
        cell = r["cell"].astype(np.int64)
        cols = (r["x"], r["y"], r["z"], cell // L, cell % L, r["lz"])
        return [tuple(int(c[k]) for c in cols) for k in range(len(r))]

    def flags(self, i):
        """space.flags of plan i: was box k placed rotated."""
        return [bool(v) for v in self._rows(i)["rotated"]]

    def write_txt(self, path, i):
        """Plan i in the line format of user_study/user_study.py:59-60: `x, y, z, lx, ly, lz` per box."""
        with open(path, "w") as f:
            for b in self.boxes(i):
                f.write("{}, {}, {}, {}, {}, {}\n".format(*b))

    def save(self, path):
        h = self.numpy()
        np.savez_compressed(path, records=h["records"].view(np.uint8).reshape(len(self), self.capacity, 8), count=h["count"],
                            episode=h["episode"], overflow=h["overflow"], size=h["size"])

    @classmethod
    def load(cls, path):
        """Plans saved by save(), on the host."""
        with np.load(path) as d:
            return cls(torch.from_numpy(d["records"].copy()), torch.from_numpy(d["count"].copy()), torch.from_numpy(d["episode"].copy()),
                       torch.from_numpy(d["overflow"].copy()), d["size"])


def replay_plans(plans, size=None, upto=None, count=None, device=None, lib=None):
    """bpp_placements_replay: (hmap uint8 [n, W, L], status int32 [n], volume int32 [n]) of `plans` -- a PackingPlans, or records
    uint8 [n, capacity, 8] with count int32 [n] -- for a bin of `size` (W, L, H; default: the plans' own).  The first
    min(count, capacity, upto) boxes of every plan are applied in order; status -1 = every box sound, else the first that is not
    (the heightmap is the one before it); volume = sum of x y z over the applied boxes.  Runs on `device` (default: where the
    records are if that is a HIP device, else the current one); `lib`: another library handle (the CPU tests' emulator, host
    memory)."""
    if isinstance(plans, PackingPlans):
        records, count, size = plans.records, plans.count, plans.size if size is None else size
    else:
        records = plans
        if count is None or size is None:
            raise ValueError("records need count= and size=")
    records, count = torch.as_tensor(records), torch.as_tensor(count)
    if records.dim() != 3 or records.shape[2] != _lib.PLACEMENT_BYTES or records.dtype != torch.uint8 or count.numel() != records.shape[0]:
        raise ValueError("records must be uint8 [n, capacity, 8] with count [n]")
    W, L, H = (int(v) for v in size)
    if lib is None:
        lib = _lib.lib()
        dev = torch.device(device) if device is not None else (records.device if records.device.type == "cuda" else torch.device("cuda"))
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("replay_plans runs on a HIP device; there is no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
    else:
        dev = torch.device("cpu")
    records = records.to(dev).contiguous()
    count = count.to(device=dev, dtype=torch.int32).contiguous()
    n, cap = int(records.shape[0]), int(records.shape[1])
    hmap = torch.zeros((n, W, L), dtype=torch.uint8, device=dev)
    status = torch.zeros((n,), dtype=torch.int32, device=dev)
    volume = torch.zeros((n,), dtype=torch.int32, device=dev)
    if n == 0:
        return hmap, status, volume
    args = (records.data_ptr(), cap, cap, count.data_ptr(), n, W, L, H, -1 if upto is None else int(upto), hmap.data_ptr(), status.data_ptr(),
            volume.data_ptr())
    if dev.type == "cuda":
        with torch.cuda.device(dev):        # (launches target the calling thread's current device)
            _lib.check(lib.bpp_placements_replay(*args, stream_ptr(dev)), lib)
    else:
        _lib.check(lib.bpp_placements_replay(*args, None), lib)
    return hmap, status, volume
