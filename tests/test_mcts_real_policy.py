"""The MCTS kernels (csrc/bpp_mcts.inl) under real-valued policy outputs, launch by launch against a teacher-forced
host tree.  Trajectories cannot be compared under real logits (one flipped near tie changes all that follows), so every
launch is checked given identical inputs:
  expand   child count and child actions = the feasible cells (the oracle's "space" rule on the scratch bin) in index
           order; every prior within 2^-23 * (8 + |x_a - max x|) * p64 of p64 = credit * softmax64(x)[a] + (1 - credit) /
           valid (|p| <= 2^-126 where p64 is below that): 2 ulp for expf, |x - max| 2^-24 for the rounded difference, 1 ulp
           for the sum, half an ulp each for the division and the credit product.  The host tree then adopts the priors' bits;
  select   with adopted priors everything is float64: the chosen child and the stream position are equal, every slot;
  rollout  the host draws u from its own RandomState (position equal); the action a must satisfy cdf64[a - 1] - CDF_TOL <=
           u <= cdf64[a] + CDF_TOL, and the host adopts it;
  backup   n and w of every node on the path bit for bit;  finish: play()'s action and the root record equal.
HostTree is first pinned: on its own (its own float32 priors and draws) under flat_policy it reproduces the committed
mcts_fake_* fixtures bit for bit.  The driver below restates MCTSearch.decide's schedule launch by launch, on the buffers
of an MCTSearch over an EmuVecEnv or (`-m gpu`) over a BppVecEnv.  It is the one deliberate second statement of a
schedule under tests/: it compares a host tree between every two launches, which MCTSearch.decide cannot offer."""
import ctypes
import math

import numpy as np
import pytest

import search_inputs as si
from conftest import load_golden
from test_mcts_search import NOOP, RUNS, case_params, expected
from test_reorder_search import make_env
from test_policy_head_f64 import CDF_TOL

TINY = 2.0 ** -126


# ------------------------------------------------------------------------------------------------- the host tree
class Node(object):
    __slots__ = ("parent", "kids", "term", "value", "vol", "w", "n", "p", "action")

    def __init__(self, parent, p, action=0):
        self.parent, self.kids, self.term, self.value, self.vol, self.w, self.n, self.p, self.action = parent, None, False, 0.0, 0, 0.0, 0, p, action


class HostTree(object):
    """MCTree / PutNode (MCTS/monteCarlo.py, MCTS/node.py) for one bin, one launch of the schedule at a time.  The env is
    not modelled: every step's outcome (done, volume of the placed item) is passed in."""

    def __init__(self, k, max_depth, rollout, credit, binvol, seed, zeta=1e-5):
        self.k, self.max_depth, self.rollout_len, self.credit, self.binvol, self.zeta = k, max_depth, rollout, credit, binvol, zeta
        self.rs = np.random.RandomState(int(seed))
        self.root, self.mode, self.pend = None, "idle", None
        self.boundary = False                      # a choose_best value came within 1e-3 relative of an isclose boundary

    def pos(self):
        return int(self.rs.get_state()[2])

    def rew(self, vol):
        return (float(vol) / self.binvol) * 10.0 if vol else 0.0

    def begin(self):
        if self.root is None:
            self.root = Node(None, 1.0)

    def start(self):
        self.node, self.depth, self.mode, self.pend, self.leaf, self.stack, self.rb, self.ri = self.root, 0, "descend", None, False, [], 0, 0

    def commit(self, done, vol):
        kind, self.pend = self.pend, None
        if kind == "descend":
            c = self.next
            c.vol = 0 if done else vol
            self.node, self.depth = c, self.depth + 1
            if done:
                if not c.term:
                    c.term, c.p = True, 0.0
                self.value, self.mode = 0.0, "backup"
        elif kind == "rollout":
            if done:
                self.value, self.mode = 0.0, "backup"
            elif self.ri + 1 < self.rb:
                self.stack.append(vol)
                self.ri += 1
            else:
                self.mode = "backup"

    def classify(self):
        nd = self.node
        if nd.term:
            self.value, self.mode = 0.0, "backup"
        elif nd.kids is None:
            self.mode = "expand"
        elif self.depth == self.max_depth:
            self.value, self.mode = nd.value, "backup"
        else:
            return True
        return False

    def choose(self):
        nd = self.node
        sq = np.sqrt(np.float64(nd.n))
        pq = nd.w / nd.n if nd.n > 0 else 0.0
        p = np.array([c.p for c in nd.kids])
        n = np.array([c.n for c in nd.kids], np.float64)
        w = np.array([c.w for c in nd.kids])
        u = (p * sq) / (n + 1.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            vals = np.where(n > 0, (w / np.where(n > 0, n, 1.0) - pq) + u, 0.0 + u)
        top = vals.max()
        near = np.abs(vals - top) <= 1.2e-3 * abs(top)
        if near.sum() == 1:
            ties = [int(vals.argmax())]
        else:                                      # node.py's order-dependent scan
            if (vals[near] != top).any():
                self.boundary = True
            mx, ties = -1000000007.0, []
            for j, v in enumerate(vals.tolist()):
                if math.isclose(v, mx, rel_tol=1e-5):
                    ties.append(j)
                elif v > mx:
                    mx, ties = v, [j]
        return nd.kids[ties[int(self.rs.randint(0, len(ties)))]]

    def select(self, level, done, vol):
        """Returns the action to step the scratch bin with, or NOOP."""
        if level == 0:
            self.start()
        else:
            self.commit(done, vol)
        if self.mode == "descend" and self.classify():
            self.next, self.pend = self.choose(), "descend"
            return self.next.action
        return NOOP

    def emit(self, rlevel, done, vol):
        """Returns whether this slot's row is emitted."""
        if rlevel == 0 and self.max_depth == 0:
            self.start()
        else:
            self.commit(done, vol)
        if rlevel == 0 and self.mode == "descend":
            self.classify()
        return (rlevel == 0 and self.mode == "expand") or (rlevel > 0 and self.mode == "rollout")

    def expand(self, cells, priors, value):
        """Children `cells` with `priors`; returns the rollout's first uniform, or None without a rollout."""
        nd = self.node
        nd.kids = [Node(nd, float(p), int(a)) for a, p in zip(cells, priors)]
        nd.value = self.value = float(value)
        self.leaf = True
        blen = self.k - self.depth
        r = blen - 1 if self.rollout_len < 0 else self.rollout_len
        if r >= 1 and blen >= r + 1:
            self.rb, self.ri, self.mode, self.pend = r + 1, 0, "rollout", "rollout"
            return self.rs.random_sample()
        self.mode = "backup"
        return None

    def roll(self, value):
        self.value, self.pend = float(value), "rollout"
        return self.rs.random_sample()

    def backup(self, done, vol):
        """Returns the path (root first) whose n and w were updated, or [] when nothing was backed up."""
        self.commit(done, vol)
        path = []
        if self.mode == "backup":
            v = self.value
            if self.rb > 0:
                for vol_ in reversed(self.stack[:self.ri]):
                    v = self.rew(vol_) + v
            if self.leaf:
                self.node.value = v
            nd = self.node
            while nd is not None:
                v = self.rew(nd.vol) + v
                nd.n += 1
                nd.w += v
                path.append(nd)
                nd = nd.parent
        self.mode = "idle"
        return path[::-1]

    def finish(self):
        kids = self.root.kids
        if self.max_depth == 0:
            self.pick = kids[int(np.argmax([c.p for c in kids]))]
        else:
            x = 1.0 / self.zeta * np.log(np.array([c.n for c in kids]) + 1e-10)
            p = np.exp(x - np.max(x))
            p /= np.sum(p)
            self.pick = kids[int(self.rs.choice(len(kids), p=p))]
        return self.pick.action

    def advance(self, done):
        if done:
            self.root = None
        else:
            self.root = self.pick
            self.root.p, self.root.parent = 1.0, None


def softmax64(x):
    with np.errstate(invalid="ignore"):
        e = np.exp(x.astype(np.float64) - x.astype(np.float64).max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


# ------------------------------------------------------------------------------------------------- the two backends
class Backend(object):
    """MCTSearch.decide's launches one at a time, on the buffers of an MCTSearch over make_env's env (emu: the emulated
    library, None: the device); `done` handles stay tensors of the env's device, everything returned for checking is numpy.
    Subclasses provide `gather`: the state bytes at an array of offsets."""

    def __init__(self, emu, pool, size, n, k, S, rollout, credit, seeds, depth=None):
        import torch
        from bpp_amd import MCTSearch
        env = make_env(emu, pool, size, 2 * n)
        if emu is None:                            # the device's scratch bins are judged by the oracle's "space" rule
            from oracle import oracle as emu
        self.torch, self.mask_from_hmap = torch, emu.mask_from_hmap
        ms = MCTSearch(env, k, sim_times=S, search_depth=depth, rollout_length=rollout, credit=credit)
        self.env, self.ms, self.L, self.b = env, ms, env.lib, env._batch_ref
        self.n, self.k, self.S, self.max_depth, self.rollout, self.cap, self.credit = n, k, S, ms.max_depth, ms.rollout_length, ms.cap, ms.credit
        self.E, self.A, self.size, self.levels = env.E, env.A, tuple(int(v) for v in size), ms.rollout_levels
        self.real = np.arange(n)
        dev = env.device
        self.ids, self.scratch = torch.arange(n, device=dev), torch.arange(n, 2 * n, device=dev)
        self.state, self.overflow = ms.state, ms.overflow
        self.acts, self.act = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
        self.vis = torch.zeros(n, dtype=torch.int32, device=dev)
        self.obs = torch.zeros((n, 4 * self.A), dtype=torch.float32, device=dev)
        ms.seed(self.ids, torch.as_tensor(np.asarray(seeds)))

    ptr = staticmethod(lambda a: None if a is None else a.data_ptr())
    host = staticmethod(lambda a: a.cpu().numpy().copy())       # (a host tensor's numpy() is a view of it)

    def new(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.env.device)

    def desc(self):
        from bpp_amd import _lib
        return _lib.Mcts(self.n, self.k, self.S, self.max_depth, self.rollout, self.cap, self.credit, 1e-5, self.ptr(self.ids),
                         self.ptr(self.scratch), self.ptr(self.state), self.ptr(self.overflow), 0)

    def call(self, name, *args):
        m = self.desc()
        rc = getattr(self.L, name)(self.b, ctypes.byref(m), *(list(args) + [self.env._stream_ptr()]))
        assert rc == 0, (name, self.L.bpp_last_error())

    def launch_acts(self, name, *args):
        self.call(name, *(list(args) + [self.ptr(self.acts)]))
        return self.host(self.acts)

    def select(self, level, done):
        return self.launch_acts("bpp_mcts_select", level, None if done is None else self.ptr(done))

    def emit(self, rlevel, done):
        self.call("bpp_mcts_emit", rlevel, None if done is None else self.ptr(done), self.ptr(self.obs))

    def expand(self, value, logits, name="bpp_mcts_expand"):
        v, x = self.new(value), self.new(logits)
        return self.launch_acts(name, self.ptr(v), self.ptr(x))

    def backup(self, done):
        self.call("bpp_mcts_backup", None if done is None else self.ptr(done))

    def finish(self):
        self.call("bpp_mcts_finish", self.ptr(self.act), self.ptr(self.vis))
        return self.host(self.act), self.host(self.vis)

    def bins(self):
        """int32 [n, 48]: the MBin records of the real bins."""
        off = self.real[:, None] * 192 + np.arange(192)[None]
        return self.gather(off).view(np.int32)

    def recs(self, half, idx):
        """bytes [n, m, 32]: records idx [n, m] of the real bins' pool halves."""
        base = self.E * 192 + self.E * 640 * 4 + (self.real * 2 + half) * self.cap * 32
        off = base[:, None, None] + idx[:, :, None] * 32 + np.arange(32)[None, None]
        return self.gather(off.reshape(self.n, -1)).reshape(self.n, idx.shape[1], 32)

    def warm(self, steps):
        for t in range(steps):
            self.env.step_tensors(self.env.sample_feasible(seed=3, step=t))

    def begin(self):
        self.env._on_device()
        self.call("bpp_mcts_begin")

    def clone(self):
        self.env.clone_bins(self.ids, self.scratch, check=False)

    def scratch_bins(self):
        it = self.host(self.env.state[self.n:, 8]).view(np.uint32)                   # bpp_env_state.item_cur
        return self.host(self.env.hmap[self.n:]), np.stack([(it >> (8 * j)) & 255 for j in range(3)], 1).astype(np.int64)

    def step(self, acts):
        return self.env.step_bins(self.scratch, self.new(acts), check=False).done

    def step_real(self, act):
        return self.env.step_bins(self.ids, self.new(act)).done

    def advance(self, done):
        d = self.torch.as_tensor(done).to(device=self.env.device, dtype=self.torch.uint8).contiguous()
        self.call("bpp_mcts_advance", d.data_ptr())

    def mask(self, hmap, items):
        return self.mask_from_hmap(hmap, items, self.size, False) > 0.5


class EmuBackend(Backend):
    def gather(self, off):
        """State bytes at offsets `off`, indexed as the host array they are."""
        return self.state.numpy()[off]


class GpuBackend(Backend):
    def __init__(self, pool, size, n, k, S, rollout, credit, seeds):
        Backend.__init__(self, None, pool, size, n, k, S, rollout, credit, seeds)

    def gather(self, off):
        return self.host(self.state[self.new(off)])


# ------------------------------------------------------------------------------------------------- the checked schedule
def logits_for(be, mask, launch, seed, shift=0.0, only=None):
    """Logit rows by slot: slot j gets family labels[j mod len] (`only`: that family for every slot), placed on `mask`."""
    ls = [only] if only else si.labels(own_mask=False)
    x = np.zeros((be.n, be.A), np.float32)
    for f, label in enumerate(ls):
        rows = np.arange(f, be.n, len(ls))
        if rows.size:
            x[rows] = si.rows_of(label, mask[rows], seed + 101 * launch + f, own_mask=False)[0]
    return x + np.float32(shift), si.hashed_values(be.n, seed + launch)


def vols(items):
    return items.prod(1)


def check_children(be, trees, live, x, value, acts, mask, what, own=False):
    """After an expand launch: the block of every expanded slot against the host mask and the float64 priors; the host
    adopts the priors.  Then the rollout's first action.  Returns the worst use of the prior bound."""
    b = be.bins()
    half, depth = b[:, 1], b[:, 5]
    node = b[np.arange(be.n), 16 + depth]
    blk = be.recs(half, node[:, None])[:, 0, 20:24].copy().view(np.int32)[:, 0]
    idx = np.maximum(blk, 0)[:, None] + np.arange(be.A + 1)[None]
    rec = be.recs(half, np.minimum(idx, be.cap - 1))
    p64 = softmax64(x)
    worst = 0.0
    for j in live:
        assert blk[j] >= 0, (what, j)
        feas = mask[j] if mask[j].any() else np.ones(be.A, bool)
        cells = np.flatnonzero(feas)
        cnt = int(rec[j, 0, 16:20].copy().view(np.int32)[0])
        assert cnt == cells.size, (what, j, "child count", cnt, cells.size)
        assert rec[j, 0, :8].copy().view(np.float64)[0] == float(value[j]), (what, j, "node value")
        kids = rec[j, 1:1 + cnt]
        got_a = kids[:, 24:26].copy().view(np.uint16)[:, 0]
        np.testing.assert_array_equal(got_a, cells, err_msg="%s slot %d: child actions" % (what, j))
        p = kids[:, 8:16].copy().view(np.float64)[:, 0]
        want = be.credit * p64[j, cells] + (1.0 - be.credit) / cells.size
        with np.errstate(invalid="ignore"):
            dist = np.abs(x[j, cells].astype(np.float64) - float(x[j].max()))
        tiny = want < TINY
        assert (np.abs(p[tiny]) <= TINY).all(), (what, j, "tiny priors")
        bound = 2.0 ** -23 * (8.0 + dist[~tiny]) * want[~tiny]
        err = np.abs(p[~tiny] - want[~tiny])
        assert (err <= bound).all(), (what, j, "prior bound", float((err / bound).max()))
        if err.size:
            worst = max(worst, float((err / bound).max()))
        pv32 = None
        if own:                                    # the host's own priors: credit * pvec[a] in float32, then float64
            pv32 = si.softmax32(x[j])
            mine = (np.float32(be.credit) * pv32[cells]).astype(np.float64) + (1.0 - be.credit) * (1.0 / cells.size)
            assert mine.tobytes() == p.tobytes(), (what, j, "priors under the exact policy")
            p = mine
        u = trees[j].expand(cells, p, np.float64(value[j]))
        check_draw(trees[j], u, acts[j], p64[j], what, j, pv32)
    return worst


def check_draw(tree, u, a, p64, what, j, pv32=None):
    if u is None:
        assert a == NOOP, (what, j, "no rollout")
        return
    if pv32 is not None:                           # the host on its own: np.random.choice(A, p=pvec) at u
        cdf = np.cumsum(pv32.astype(np.float64))
        cdf /= cdf[-1]
        assert a == int(np.searchsorted(cdf, u, "right")), (what, j, "rollout draw", int(a))
        return
    cdf = np.cumsum(p64)
    cdf /= cdf[-1]
    assert 0 <= a < p64.size, (what, j, int(a))
    lo = cdf[a - 1] if a > 0 else 0.0
    assert lo - CDF_TOL <= u <= cdf[a] + CDF_TOL, (what, j, "rollout draw", int(a), u, lo, cdf[a])


def check_path(be, trees, paths, what):
    """After a backup launch: n and w of every path node of every slot, bit for bit."""
    b = be.bins()
    depth = max([len(p) for p in paths] + [1])
    idx = b[:, 16:16 + depth]
    rec = be.recs(b[:, 1], np.clip(idx, 0, be.cap - 1))
    for j, path in enumerate(paths):
        for d, nd in enumerate(path):
            w = rec[j, d, :8].copy().view(np.float64)[0]
            n = int(rec[j, d, 16:20].copy().view(np.int32)[0])
            assert n == nd.n and np.float64(w).tobytes() == np.float64(nd.w).tobytes(), (what, j, d, (n, w), (nd.n, nd.w))


def decide(be, trees, live, seed, decision, shift=0.0, only=None, policy=None):
    """One decision of every slot, every launch checked.  policy: the exact stand-in instead of the families; the host
    then computes its own priors and rollout actions (the fixture pin).  Returns (actions, worst use of the prior bound)."""
    n = be.n
    launch = [decision * 1000]
    worst = 0.0
    be.begin()
    for t in trees:
        t.begin()
    for sim in range(be.S):
        be.clone()
        done_h, done, items = None, np.zeros(n, np.uint8), np.zeros((n, 3), np.int64)
        for level in range(be.max_depth):
            acts = be.select(level, done_h)
            want = np.array([t.select(level, bool(done[j]), int(vols(items)[j])) for j, t in enumerate(trees)])
            what = "decision %d sim %d select %d" % (decision, sim, level)
            np.testing.assert_array_equal(acts, want, err_msg=what)
            np.testing.assert_array_equal(be.bins()[:, 3], [t.pos() for t in trees], err_msg=what + ": stream position")
            _, items = be.scratch_bins()
            done_h = be.step(acts)
            done = be.host(done_h)
        be.emit(0, done_h)
        rows = np.array([t.emit(0, bool(done[j]), int(vols(items)[j])) for j, t in enumerate(trees)])
        np.testing.assert_array_equal(be.bins()[:, 14] != 0, rows, err_msg="decision %d sim %d: emitted rows" % (decision, sim))
        hmap, items = be.scratch_bins()
        mask = be.mask(hmap, items)
        launch[0] += 1
        x, value = logits_for(be, mask, launch[0], seed, shift, only)
        if policy:
            value, x = policy(be.host(be.obs))
        acts = be.expand(value, x)
        what = "decision %d sim %d expand" % (decision, sim)
        assert (acts[~rows] == NOOP).all(), what
        worst = max(worst, check_children(be, trees, np.flatnonzero(rows), x, value, acts, mask, what, own=policy is not None))
        np.testing.assert_array_equal(be.bins()[:, 3], [t.pos() for t in trees], err_msg=what + ": stream position")
        done_h, done = None, np.zeros(n, np.uint8)
        for level in range(1, be.levels):
            _, items = be.scratch_bins()
            done_h = be.step(acts)
            done = be.host(done_h)
            be.emit(level, done_h)
            rows = np.array([t.emit(level, bool(done[j]), int(vols(items)[j])) for j, t in enumerate(trees)])
            np.testing.assert_array_equal(be.bins()[:, 14] != 0, rows, err_msg="rollout rows")
            hmap, _ = be.scratch_bins()
            launch[0] += 1
            x, value = logits_for(be, np.ones((n, be.A), bool) & (hmap < 255), launch[0], seed, shift, "mild" if only else None)
            if policy:
                value, x = policy(be.host(be.obs))
            acts = be.expand(value, x, "bpp_mcts_rollout")
            what = "decision %d sim %d rollout %d" % (decision, sim, level)
            p64 = softmax64(x)
            for j in range(n):
                if rows[j]:
                    check_draw(trees[j], trees[j].roll(np.float64(value[j])), acts[j], p64[j], what, j,
                               si.softmax32(x[j]) if policy else None)
                else:
                    assert acts[j] == NOOP, (what, j)
            np.testing.assert_array_equal(be.bins()[:, 3], [t.pos() for t in trees], err_msg=what + ": stream position")
        if be.levels > 0:
            _, items = be.scratch_bins()
            done_h = be.step(acts)
            done = be.host(done_h)
        be.backup(done_h)
        paths = [t.backup(bool(done[j]), int(vols(items)[j])) for j, t in enumerate(trees)]
        check_path(be, trees, paths, "decision %d sim %d backup" % (decision, sim))
    act, vis = be.finish()
    want = np.array([t.finish() for t in trees])
    np.testing.assert_array_equal(act, want, err_msg="decision %d: play()" % decision)
    np.testing.assert_array_equal(vis, [t.root.n for t in trees], err_msg="decision %d: root visits" % decision)
    np.testing.assert_array_equal(be.bins()[:, 3], [t.pos() for t in trees], err_msg="decision %d: stream position" % decision)
    check_path(be, trees, [[t.root] for t in trees], "decision %d: root record" % decision)
    return act, worst


def run(be, seeds, decisions=3, shift=0.0, only=None, seed=11):
    be.warm(2)
    binvol = float(np.prod(be.size))
    trees = [HostTree(be.k, be.max_depth, be.rollout, be.credit, binvol, s) for s in seeds]
    worst, record = 0.0, []
    for d in range(decisions):
        act, w = decide(be, trees, None, seed, d, shift, only)
        worst = max(worst, w)
        record.append((act.copy(), np.array([t.root.n for t in trees])))
        done_h = be.step_real(act)
        be.advance(done_h)
        for j, t in enumerate(trees):
            t.advance(bool(be.host(done_h)[j]))
    assert int(be.host(be.overflow)[0]) == 0
    print("prior bound used: %.3f" % worst)
    return record, trees


SIZES = {25: ("mcts_fake_5x5x3", (5, 5, 3)), 96: ("mcts_fake_8x12x9", (8, 12, 9)), 100: ("mcts_fake_10", (10, 10, 10)),
         400: ("mcts_fake_20x20x10", (20, 20, 10))}


def pool_of(A, n):
    if A == 1024:
        from bpp_amd.sequences import cut2_pool
        pool, size = cut2_pool((32, 32, 10), 8, seed=5, bound=(2, 5), native=False), (32, 32, 10)
    else:
        name, size = SIZES[A]
        pool = load_golden(name)["pool"]
    return np.ascontiguousarray(pool[np.arange(n) % len(pool)]), size


@pytest.mark.parametrize("name,case", RUNS)
def test_host_tree_reproduces_the_fixtures(emu, name, case):
    """HostTree on its own -- its own float32 priors, its own draws and choices; the emulated env only steps the bins --
    under flat_policy: action, root n, root w, child count and stream position of every decision of the fixture."""
    import torch
    from bpp_amd.mcts import flat_policy
    g = load_golden(name)
    size = tuple(int(v) for v in g["size"])
    S, k, depth, rollout, credit, episodes = case_params(g, case)
    N = min(len(g[case + "_seeds"]), 1 if case == "default" else 3)     # trajectories: bounded for the suite's wall time
    exp = expected(g, case)[:N]
    be = EmuBackend(emu, g["pool"][:N], size, N, k, S, rollout, credit, g[case + "_seeds"][:N], depth=depth)
    tpol = flat_policy(size)
    pol = lambda obs: tuple(t.numpy() for t in tpol(torch.from_numpy(obs))[:2])          # noqa: E731
    trees = [HostTree(k, be.max_depth, be.rollout, be.credit, float(np.prod(size)), s) for s in g[case + "_seeds"][:N]]
    ep, t = np.zeros(N, int), np.zeros(N, int)
    checked = 0
    for d in range(400):
        if (ep >= episodes).all():
            break
        act, _ = decide(be, trees, None, 0, d, policy=pol)
        for j, tr in enumerate(trees):
            if ep[j] >= episodes:
                continue
            e = exp[j][ep[j]]
            got = (int(act[j]), tr.root.n, np.float64(tr.root.w).tobytes(), len(tr.root.kids), tr.pos())
            want = (int(e[0][t[j]]), int(e[1][t[j]]), np.float64(e[2][t[j]]).tobytes(), int(e[3][t[j]]), int(e[4][t[j]]))
            assert got == want, (case, j, ep[j], t[j], got, want)
            checked += 1
        done = be.host(be.step_real(act))
        be.advance(done)
        for j, tr in enumerate(trees):
            tr.advance(bool(done[j]))
            t[j] += 1
            if done[j] and ep[j] < episodes:
                assert t[j] == len(exp[j][ep[j]][0]), (case, j, "episode length")
                ep[j], t[j] = ep[j] + 1, 0
    assert (ep >= episodes).all() and checked >= N
    assert int(be.overflow[0]) == 0


GRID = [(k, rollout, credit) for k in (3, 4) for rollout in (-1, 0) for credit in (1.0, 0.7)]


@pytest.mark.parametrize("k,rollout,credit", GRID)
def test_emulated_mcts_launches_against_host_tree(emu, k, rollout, credit):
    """32 slots of 10x10x10, S = 8, three decisions with advance between them, a logit family per slot."""
    n = 32
    pool, size = pool_of(100, n)
    seeds = np.arange(n) * 7 + 3
    run(EmuBackend(emu, pool, size, n, k, 8, rollout, credit, seeds), seeds)


@pytest.mark.parametrize("A", [25, 96, 400, 1024])
def test_emulated_mcts_areas(emu, A):
    """One partial wave (25), two waves with a tail (96), seven chunks with a tail (400) and the stated limit (1024)."""
    n = 18 if A < 1024 else 6
    pool, size = pool_of(A, n)
    seeds = np.arange(n) + 40
    run(EmuBackend(emu, pool, size, n, 3, 4 if A >= 400 else 8, -1, 0.7, seeds), seeds, decisions=3 if A < 400 else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("k,rollout,credit", GRID)
def test_gpu_mcts_launches_against_host_tree(k, rollout, credit):
    """2 048 slots of 10x10x10 on the MI355X, S = 8, three decisions."""
    from bpp_amd.sequences import cut2_pool
    n = 2048
    pool = cut2_pool((10, 10, 10), n, seed=23)
    seeds = np.arange(n) * 13 + 5
    run(GpuBackend(pool, (10, 10, 10), n, k, 8, rollout, credit, seeds), seeds)


@pytest.mark.gpu
@pytest.mark.parametrize("A", [25, 96, 400, 1024])
def test_gpu_mcts_areas(A):
    n = 256 if A < 1024 else 64
    pool, size = pool_of(A, n)
    seeds = np.arange(n) + 40
    run(GpuBackend(pool, size, n, 3, 4 if A >= 400 else 8, -1, 0.7, seeds), seeds, decisions=3 if A < 400 else 1)


@pytest.mark.gpu
def test_gpu_mcts_is_shift_invariant():
    """The shifted family and the same logits + 1000: identical actions and root n for every slot whose host tree met no
    isclose boundary within 1e-3 relative; at least 95 % of the slots qualify."""
    from bpp_amd.sequences import cut2_pool
    n = 2048
    pool = cut2_pool((10, 10, 10), n, seed=23)
    seeds = np.arange(n) * 13 + 5
    out = []
    for shift in (0.0, 1000.0):
        out.append(run(GpuBackend(pool, (10, 10, 10), n, 3, 8, 0, 1.0, seeds), seeds, decisions=1, shift=shift, only="shifted"))
    (r0, t0), (r1, t1) = out
    ok = np.array([not (a.boundary or b.boundary) for a, b in zip(t0, t1)])
    print("shift invariance: %.4f of the slots qualify" % ok.mean())
    assert ok.mean() >= 0.95
    np.testing.assert_array_equal(r0[0][0][ok], r1[0][0][ok])
    np.testing.assert_array_equal(r0[0][1][ok], r1[0][1][ok])
