"""reorder_choose_kernel (csrc/bpp_reorder.inl) under real-valued policy outputs: one choose launch per input family and
phase against the float64 rule of tests/search_inputs.py -- the feasible cell (pred >= 0.5) with the largest logit, the
first one in the baseline phase, the last one in the search phase, index 0 / A - 1 for a row without a feasible cell.

A decision with k = 2 is four choose launches: baseline levels 0 and 1 (first maximum), then one search iteration's
levels 0 and 1 (last maximum).  The family under test is fed to baseline level 0 of one decision and to search level 0
of a second one, whose baseline saw a benign policy (feasible positions, value 0.5) so that its search descends; every
other launch gets the benign policy.  pred is an output of the network, not something the kernel derives from the bin: the
family rows get the feasibility mask of the emitted observation (the env's own rule on real heightmaps, reached by
uniform-feasible steps) joined with 30 % random cells -- the env's masks alone leave rows with one or two feasible cells,
too few for the wide families to be decidable in float64 -- and adapted where a family needs a mask of its own.

Two tiers, one body: ReorderSearch on an EmuVecEnv over the host SIMT emulator, and `-m gpu` on a BppVecEnv on the MI355X."""
import numpy as np
import pytest

import search_inputs as si
from conftest import load_golden
from test_reorder_search import NOOP, make_env

SIZES = {25: ("reorder_fake_5x5x3", (5, 5, 3)), 96: ("reorder_fake_8x12x9", (8, 12, 9)), 100: ("reorder_fake_10", (10, 10, 10)),
         400: ("mcts_fake_20x20x10", (20, 20, 10))}
WARM_STEPS = 3
# a search row is emitted for every slot whose baseline value is positive: the benign baseline gives reward + 0.5 unless the
# first item has no feasible position at all; half of the slots is a floor far below what bins after 3 steps give
LIVE = 0.5


def pool_rows(A, n):
    name, size = SIZES[A]
    pool = load_golden(name)["pool"]
    return np.ascontiguousarray(pool[np.arange(n) % len(pool)]), size


class Recorder(object):
    """The policy of one decision: call number -> the family rows or the benign policy; keeps what the launches got."""

    def __init__(self, size, mask_fn, family_call, label, seed):
        self.size, self.mask_fn, self.family_call, self.label, self.seed = size, mask_fn, family_call, label, seed
        self.calls, self.x, self.m = 0, None, None

    def __call__(self, obs):
        """obs float32 numpy [n, 4A] -> (value, logits, pred) float32 numpy."""
        n, A = obs.shape[0], obs.shape[1] // 4
        feas = self.mask_fn(obs) > 0.5
        c = self.calls
        self.calls += 1
        if c == self.family_call:
            dense = feas | (np.random.RandomState(self.seed + 31).rand(n, A) < 0.3)
            x, m = si.rows_of(self.label, dense, self.seed, own_mask=True)
            self.x, self.m = x, m
            return si.hashed_values(n, self.seed), x, m.astype(np.float32)
        x = si.hashed(np.arange(n * A, dtype=np.uint64) + np.uint64(c * 7717)).reshape(n, A) * np.float32(2.0)
        return np.full(n, 0.5, np.float32), np.ascontiguousarray(x), feas.astype(np.float32)


class Tier(object):
    """emu: the emulated library (21 slots), or None for the device (259 slots)."""

    def __init__(self, emu=None):
        self.emu, self.rows = emu, 259 if emu is None else 21

    def mask_fn(self, size):
        import torch
        if self.emu is not None:
            return lambda obs: self.emu.mask_from_obs(obs, size, False)
        from bpp_amd.masks import batched_mask_from_obs
        return lambda obs: batched_mask_from_obs(torch.from_numpy(obs).cuda(), size).cpu().numpy()

    def run(self, A, label, family_call, seed):
        """One k = 2 decision; returns (x, m, actions of the family's launch)."""
        import torch
        from bpp_amd import ReorderSearch
        n = self.rows
        pool, size = pool_rows(A, n)
        env = make_env(self.emu, pool, size, 2 * n)
        for t in range(WARM_STEPS):
            env.step_tensors(env.sample_feasible(seed=7, step=t))
        rec = Recorder(size, self.mask_fn(size), family_call, label, seed)

        def policy(obs):
            return tuple(torch.from_numpy(np.ascontiguousarray(t)).to(env.device) for t in rec(obs.cpu().numpy()))
        acts = []
        step = env.step_bins
        env.step_bins = lambda ids, a, **kw: (acts.append(a.cpu().numpy().copy()), step(ids, a, **kw))[1]
        rs = ReorderSearch(env, 2)
        ids = torch.arange(n, device=env.device)
        rs.decide(policy, ids, ids + n)
        assert int(rs.overflow.item()) == 0 and rec.calls == 4
        return rec.x, rec.m, acts[family_call]


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def tier(request):
    if request.param == "gpu":
        import torch
        assert torch.cuda.is_available()
        return Tier()
    return Tier(request.getfixturevalue("emu"))


@pytest.mark.parametrize("A", sorted(SIZES))
def test_reorder_choose_against_float64(tier, A):
    """Every family in both phases: equal actions on decided rows, the tolerance rules of search_inputs.judge_choice on the
    others, >= 98 % of the rows decided for every family the float64 rule can decide."""
    shares = {}
    for i, label in enumerate(si.labels(own_mask=True)):
        for family_call, last in ((0, False), (2, True)):
            x, m, a = tier.run(A, label, family_call, seed=A * 131 + i)
            live = a != NOOP
            if not last:
                assert live.all(), (label, "every slot emits baseline level 0")
            assert live.mean() >= LIVE, (label, last, live.mean())
            share = si.judge_choice(x[live], m[live], a[live], last, "A=%d %s" % (A, label))
            shares.setdefault(label, []).append(share)
    si.check_cap(shares, "reorder A=%d" % A)
