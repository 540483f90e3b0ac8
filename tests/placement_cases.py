"""Helpers of tests/test_placements.py and tests/test_gpu_placements.py (include/bpp_placements.h): the fixtures' box lists as
record arrays, numpy restatements of note / commit and of replay, the edge plans of replay, and a host driver of the entry
points for the emulated library.  Nothing here is imported by the product."""
import ctypes
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORD = np.dtype([("x", "u1"), ("y", "u1"), ("z", "u1"), ("lz", "u1"), ("cell", "<u2"), ("rotated", "u1"), ("pad", "u1")])
CASES = ["rollout_cut2_10_rot", "rollout_deep_cut2_10_rot", "rollout_deep_cut2_20", "rollout_short_5x4x6", "rollout_wide_8x12x9_rot",
         "rollout_rs_10", "rollout_cut2_10"]
NOOP = -2 ** 63
BADARG = -1


def load_case(name):
    """The rollout fixture and the reference's boxes recorded for it (tests/golden/make_placements_golden.py)."""
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    g["box"] = np.load(os.path.join(GOLDEN, "placements_%s.npz" % name))["box"]
    g["size"] = tuple(int(v) for v in g["size"])
    g["rotation"] = bool(g["rotation"])
    return g


def default_capacity(size):
    return min(size[0] * size[1] * size[2], 256)


def box_records(box, L):
    """Reference boxes [..., 7] (x, y, z, lx, ly, lz, flag) as records [...]; rows of -1 become zero records."""
    box = np.asarray(box).astype(np.int64)
    rec = np.zeros(box.shape[:-1], RECORD)
    ok = box[..., 0] >= 0
    for k, name in ((0, "x"), (1, "y"), (2, "z"), (5, "lz"), (6, "rotated")):
        rec[name][ok] = box[..., k][ok]
    rec["cell"][ok] = (box[..., 3] * L + box[..., 4])[ok]
    return rec


class ExpectedPlans(object):
    """What the log must hold after every lock-step of a fixture, from the reference's boxes alone."""

    def __init__(self, E, L, capacity):
        self.L, self.C = L, capacity
        self.run, self.fin = np.zeros((E, capacity), RECORD), np.zeros((E, capacity), RECORD)
        self.run_count, self.fin_count = np.zeros(E, np.int32), np.full(E, -1, np.int32)
        self.fin_episode, self.episode = np.full(E, -1, np.int32), np.zeros(E, np.int32)
        self.dropped = 0

    def step(self, box_t, done_t, stepped=None):
        """One lock-step: box_t [E, 7] the reference's appended boxes (-1: none), done_t [E]; stepped [E]: the bins that took part."""
        rec = box_records(box_t, self.L)
        for e in range(len(done_t)):
            if stepped is not None and not stepped[e]:
                continue
            if done_t[e]:
                assert box_t[e][0] < 0
                self.fin[e], self.fin_count[e], self.fin_episode[e] = self.run[e], self.run_count[e], self.episode[e]
                self.run[e], self.run_count[e] = 0, 0
                self.episode[e] += 1
            else:
                assert box_t[e][0] >= 0
                if self.run_count[e] < self.C:
                    self.run[e, self.run_count[e]] = rec[e]
                else:
                    self.dropped += 1
                self.run_count[e] += 1


class PlanModel(object):
    """note / commit restated in numpy for bins `ids` of a batch: fed with what the kernels read -- the bins' state records and
    the actions before the step, `done` and the byte heightmaps after it."""

    def __init__(self, ids, size, rotation, capacity):
        self.ids, (self.W, self.L, self.H), self.rot, self.C = np.asarray(ids), size, bool(rotation), capacity
        self.m = ExpectedPlans(len(self.ids), self.L, capacity)
        self._note = None

    def note(self, item_cur, actions):
        A = self.W * self.L
        notes = []
        for it, a in zip(np.asarray(item_cur)[self.ids].tolist(), np.asarray(actions)[self.ids].tolist()):
            flag = self.rot and a > A
            idx = a - A if flag else a
            if a == NOOP or not 0 <= idx < A:
                notes.append(None)
                continue
            ix, iy, iz = it & 255, (it >> 8) & 255, (it >> 16) & 255
            notes.append((iy if flag else ix, ix if flag else iy, iz, idx, int(flag)))
        self._note = notes

    def commit(self, done, hmap):
        done, hmap = np.asarray(done)[self.ids], np.asarray(hmap).reshape(len(done), -1)[self.ids]
        box = np.full((len(self.ids), 7), -1, np.int64)
        stepped = np.zeros(len(self.ids), bool)
        for k, nt in enumerate(self._note):
            stepped[k] = bool(done[k]) or nt is not None
            if nt is not None and not done[k]:
                x, y, z, idx, flag = nt
                box[k] = (x, y, z, idx // self.L, idx % self.L, int(hmap[k, idx]) - z, flag)
        self.m.step(box, done, stepped)


def replay_numpy(records, count, size, upto=None):
    """bpp_placements_replay restated: (hmap uint8 [n, W, L], status int32 [n], volume int32 [n])."""
    W, L, H = size
    records = np.asarray(records)
    if records.dtype != RECORD:
        records = np.ascontiguousarray(records).view(RECORD).reshape(records.shape[0], records.shape[1])
    n, C = records.shape
    hmap, status, volume = np.zeros((n, W, L), np.uint8), np.full(n, -1, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        nb = min(int(count[i]), C)
        if upto is not None and upto >= 0:
            nb = min(nb, upto)
        h = hmap[i]
        for k in range(nb):
            r = records[i, k]
            x, y, z, lz, cell = int(r["x"]), int(r["y"]), int(r["z"]), int(r["lz"]), int(r["cell"])
            lx, ly = cell // L, cell % L
            inside = x >= 1 and y >= 1 and z >= 1 and lx + x <= W and ly + y <= L
            if not inside or int(h[lx:lx + x, ly:ly + y].max()) != lz or lz + z > H:
                status[i] = k
                break
            h[lx:lx + x, ly:ly + y] = lz + z
            volume[i] += x * y * z
    return hmap, status, volume


# ---- replay edges: sound plans built by dropping random boxes, then one box spoilt ---------------------------------------------
EDGE_GEOMETRIES = [(1, 1, 5), (7, 13, 9), (20, 20, 12), (32, 32, 10), (1024, 1, 8)]     # A = 1, 91, 400, 1 024, and 1 024 x 1: lx > 255
BREAKS = ("zero_x", "zero_y", "zero_z", "over_x", "over_y", "floating", "sunk", "above_h")


def sound_plan(rng, size, nboxes, zmax=3):
    """Up to `nboxes` boxes dropped at random corners of an empty bin, each on the highest cell under it (records, RECORD)."""
    W, L, H = size
    h = np.zeros((W, L), np.int64)
    out = []
    for _ in range(8 * nboxes):
        if len(out) == nboxes:
            break
        x, y, z = int(rng.randint(1, min(W, 5) + 1)), int(rng.randint(1, min(L, 5) + 1)), int(rng.randint(1, min(H, zmax) + 1))
        lx, ly = int(rng.randint(0, W - x + 1)), int(rng.randint(0, L - y + 1))
        lz = int(h[lx:lx + x, ly:ly + y].max())
        if lz + z > H:
            continue
        h[lx:lx + x, ly:ly + y] = lz + z
        out.append((x, y, z, lz, lx * L + ly, int(rng.randint(0, 2)), 0))
    return np.array(out, RECORD) if out else np.zeros(0, RECORD)


def spoil(rec, size, kind):
    """Record `rec` made unsound in the way `kind` names, or None where the geometry has no such box."""
    W, L, H = size
    r = rec.copy()
    lx, ly = int(r["cell"]) // L, int(r["cell"]) % L
    if kind.startswith("zero_"):
        r[kind[-1]] = 0
    elif kind == "over_x":
        if W - lx + 1 > 255:
            return None
        r["x"] = W - lx + 1
    elif kind == "over_y":
        r["y"] = L - ly + 1
    elif kind == "floating":
        if int(r["lz"]) + int(r["z"]) + 1 > H:
            return None
        r["lz"] += 1
    elif kind == "sunk":
        if int(r["lz"]) == 0:
            return None
        r["lz"] -= 1
    elif kind == "above_h":
        r["z"] = H - int(r["lz"]) + 1
    return r


def edge_plans(size, n, capacity, seed):
    """(records [n, capacity], count [n]): plan 0 empty, plan 1 full (count = capacity where the bin takes that many boxes), a plan
    whose count exceeds the capacity, then sound plans with ONE box spoilt -- every kind of BREAKS at the first, a middle and the
    last position, as far as n reaches (each kind comes up within the first 8 + 3 plans of some position)."""
    rng = np.random.RandomState(seed)
    records, count = np.zeros((n, capacity), RECORD), np.zeros(n, np.int32)
    for i in range(n):
        p = sound_plan(rng, size, capacity, zmax=1) if i in (1, 2) else sound_plan(rng, size, int(rng.randint(1, capacity + 1)))
        if i == 0:
            p = p[:0]
        records[i, :len(p)], count[i] = p, len(p)
        if i == 2:
            count[i] = len(p) + 7
        if i >= 3 and len(p):
            kind, where = BREAKS[(i - 3) % len(BREAKS)], ((i - 3) // len(BREAKS)) % 3
            k = (0, len(p) // 2, len(p) - 1)[where]
            bad = spoil(records[i, k], size, kind)
            if bad is not None:
                records[i, k] = bad
    return records, count


# ---- the entry points on host memory (the emulated library) --------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def aligned_bytes(n, align=64, guard=0, fill=0):
    """(uint8 view of n bytes `align`-aligned, the whole array) with `guard` bytes of `fill` on both sides."""
    raw = np.full(n + 2 * guard + align, fill, np.uint8)
    off = (-(raw.ctypes.data + guard)) % align + guard
    return raw[off:off + n], raw


class HostLog(object):
    """A log in host memory and the entry points on it: L = the emulated library bound with _lib.bind_placements(batch=emu.Batch),
    env = the emulator front-end's env (batch `_b`, hmap, state, step())."""

    def __init__(self, L, env, capacity, keep=1, guard=0):
        self.L, self.env, self.C, self.keep = L, env, int(capacity), int(keep)
        self.nbytes = int(L.bpp_placements_sizes(env.E, self.C, self.keep))
        assert self.nbytes > 0
        self.buf, self.raw = aligned_bytes(self.nbytes, 64, guard, 0xA5)
        self.guard = guard
        self.clear()

    def ok(self, rc):
        assert rc == 0, (rc, self.L.bpp_last_error().decode())

    def guards_intact(self):
        lo = self.buf.ctypes.data - self.raw.ctypes.data
        return bool((self.raw[:lo] == 0xA5).all() and (self.raw[lo + self.nbytes:] == 0xA5).all()) and lo >= self.guard

    @property
    def overflow(self):
        return int(self.buf[-8:-4].view("<i4")[0])

    def clear(self):
        self.ok(self.L.bpp_placements_clear(_p(self.buf), self.env.E, self.C, self.keep, None))

    def note(self, actions, ids=None):
        self.ok(self.L.bpp_placements_note(ctypes.byref(self.env._b), _p(ids), 0 if ids is None else len(ids), _p(actions), _p(self.buf),
                                           self.C, self.keep, None))

    def commit(self, done, ids=None):
        self.ok(self.L.bpp_placements_commit(ctypes.byref(self.env._b), _p(ids), 0 if ids is None else len(ids), _p(done), _p(self.buf),
                                             self.C, self.keep, None))

    def step(self, actions):
        """One recorded lock-step of all bins: note, bpp_step, commit."""
        a = np.ascontiguousarray(actions, np.int64)
        self.note(a)
        out = self.env.step(a, copy=False)
        self.commit(out["done"])
        return out

    def copy(self, src, dst):
        src, dst = np.ascontiguousarray(src, np.int64), np.ascontiguousarray(dst, np.int64)
        self.ok(self.L.bpp_placements_copy(_p(self.buf), _p(src), _p(dst), len(src), self.env.E, self.C, self.keep, None))

    def gather(self, finished=False, ids=None, stride=None):
        """(records [n, capacity] RECORD, count, episode) of the running / finished plans."""
        ids = None if ids is None else np.ascontiguousarray(ids, np.int64)
        n = self.env.E if ids is None else len(ids)
        stride = stride or self.C
        rec = np.full((n, stride), 0x7777777777777777, "<u8")
        count, episode = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
        self.ok(self.L.bpp_placements_gather(_p(self.buf), _p(ids), n, int(finished), _p(rec), stride, _p(count), _p(episode), self.env.E,
                                             self.C, self.keep, None))
        assert (rec[:, self.C:] == 0x7777777777777777).all()           # the padding of a wider stride is left alone
        return np.ascontiguousarray(rec[:, :self.C]).view(RECORD).reshape(n, self.C), count, episode


def host_replay(L, records, count, size, upto=None, capacity=None):
    """bpp_placements_replay on host arrays: (hmap [n, W, L], status, volume)."""
    W, Ln, H = size
    records = np.ascontiguousarray(records)
    n, stride = records.shape[0], records.shape[1]
    count = np.ascontiguousarray(count, np.int32)
    hmap, status, volume = np.full((n, W, Ln), 0xEE, np.uint8), np.full(n, -9, np.int32), np.full(n, -9, np.int32)
    rc = L.bpp_placements_replay(_p(records), stride, capacity or stride, _p(count), n, W, Ln, H, -1 if upto is None else upto, _p(hmap),
                                 _p(status), _p(volume), None)
    assert rc == 0, (rc, L.bpp_last_error().decode())
    return hmap, status, volume
