"""multibin_choose_kernel (csrc/bpp_multibin.inl) under real-valued policy outputs: per decision the window and the
advantage bit for bit against a float64 scan written in plain numpy operations (no fused multiply-add), and the position
inside the chosen window against the float64 rule of tests/search_inputs.py (first feasible cell with the largest logit).

The window masks are the kernel's own (emit writes them from the pallet's heightmap; the policy closure reads them back
to place the input families on them), so the families that need a mask of their own (nothing / everything feasible) do
not exist here: the kernel skips such windows, which the scan restates.  Values are hashed full-mantissa float32, and the
geometries give bin_num = 9, 6.25, 4 and 2.25, so bin_num * reward + (v - last) rounds twice where a fused
multiply-add would round once.  Every launch feeds one family to every window of every pallet; a pallet set plays six
decide / step / commit rounds, so windows are chosen again with history.

Two tiers, one body: MultiBinPacker on an EmuVecEnv over the host SIMT emulator, and `-m gpu` on a BppVecEnv on the MI355X."""
import numpy as np
import pytest

import search_inputs as si
from test_reorder_search import make_env

# (pallet, window side, stride): w^2 = 100, 64, 25, 400
GEOMETRIES = {"30x30_w10": ((30, 30, 10), 10, 10), "20x20_w8_s4": ((20, 20, 10), 8, 4), "10x10_w5": ((10, 10, 10), 5, 5),
              "30x30_w20_s10": ((30, 30, 10), 20, 10)}
ROUNDS = 6
WARM_STEPS = 2


def small_items(size, E):
    """E CUT-2 sequences of items with sides 2 .. 3 (16 distinct ones, repeated): the usual 2 .. 5 items leave windows of
    side 5 or 8 with one to four feasible cells, too few for the wide families to be decidable in float64."""
    from bpp_amd.sequences import cut2_pool
    pool = cut2_pool(size, 16, seed=3, bound=(2, 3), native=False)
    return np.ascontiguousarray(pool[np.arange(E) % len(pool)])


def launch_labels():
    """Families in launch order, the wide ones first (on the emptiest pallets their windows keep the most feasible cells),
    in sets of ROUNDS launches that each start from fresh pallets."""
    ls = si.labels(own_mask=False)
    ls = [l for l in ls if l.startswith("wide")] + [l for l in ls if not l.startswith("wide")]
    return [ls[i:i + ROUNDS] for i in range(0, len(ls), ROUNDS)]


class Host(object):
    """multi_bin.get_action's records and its advantage scan in float64 numpy, for every pallet at once."""

    def __init__(self, size, w, s, E):
        W, L, H = size
        self.size, self.w, self.s, self.E = size, w, s, E
        self.offs = [(dx, dy) for dx in range(0, W - w + 1, s) for dy in range(0, L - w + 1, s)]
        self.K = len(self.offs)
        self.bin_num = (W * L) / (w * w)
        self.binvol = float(W * L * H)
        self.reward, self.last, self.has = np.zeros((E, self.K)), np.zeros((E, self.K)), np.zeros((E, self.K), bool)

    def scan(self, value, masks):
        """value float32 [E, K], masks bool [E, K, w2] -> (window int [E], adv float64 [E])."""
        w2 = self.w * self.w
        cnt = masks.sum(-1)
        v = value.astype(np.float64)
        max_adv, best = np.full(self.E, -1e8), np.full(self.E, -1)
        for k in range(self.K):
            prod = self.bin_num * self.reward[:, k]
            diff = v[:, k] - self.last[:, k]
            cur = np.where(self.has[:, k], prod + diff, -0.2)
            take = (cnt[:, k] > 0) & (cnt[:, k] < w2) & (cur > max_adv)
            max_adv, best = np.where(take, cur, max_adv), np.where(take, k, best)
        return best, max_adv

    def update(self, win, value, items, done):
        rows = np.arange(self.E)
        ch = win >= 0
        self.last[rows[ch], win[ch]] = value.astype(np.float64)[rows[ch], win[ch]]
        rew = (items.prod(1).astype(np.float64) / self.binvol) * 10.0
        self.reward[rows[ch], win[ch]] = rew[ch]
        self.has[rows[ch], win[ch]] = True
        nw = ~ch & self.has[:, 0]
        self.reward[nw, 0] = rew[nw]
        d = done.astype(bool)
        self.reward[d], self.last[d], self.has[d] = 0.0, 0.0, False


def masks_of(work, n, K, w2):
    """The window masks emit wrote into the work buffer (csrc/bpp_multibin.inl: MBLayout): bool [n, K, w2]."""
    off = (n * 16 + 255) // 256 * 256
    stride = (w2 + 15) // 16 * 16
    return work[off:off + n * K * stride].reshape(n, K, stride)[:, :, :w2] != 0


def check_masks(masks, obs, mask_from_obs, w, H):
    """The masks read back from the work buffer against the host's own rule on the emitted rows (which has an all-ones
    fallback the kernel's masks do not have): a wrong offset or stride in masks_of cannot go unnoticed."""
    n, K, w2 = masks.shape
    want = mask_from_obs(obs, (w, w, H), False).reshape(n, K, w2) > 0.5
    empty = ~masks.any(-1)
    assert want[empty].all()
    np.testing.assert_array_equal(masks[~empty], want[~empty])


def family_rows(label, masks, seed):
    """(value float32 [n K], logits float32 [n K, w2]) of one launch."""
    n, K, w2 = masks.shape
    x, m = si.rows_of(label, masks.reshape(n * K, w2), seed, own_mask=False)
    assert np.array_equal(m, masks.reshape(n * K, w2))
    return si.hashed_values(n * K, seed), x


def check_launch(host, label, value, x, masks, action, adv, win, items, what):
    """One choose launch against the host: window and adv bit for bit, the position by judge_choice.  Returns the decided
    rows (one per pallet that chose a window)."""
    E, K, w = host.E, host.K, host.w
    w2, L = w * w, host.size[1]
    value = value.reshape(E, K)
    want_w, want_adv = host.scan(value, masks)
    np.testing.assert_array_equal(win, want_w, err_msg="window " + what)
    np.testing.assert_array_equal(adv.view(np.int64), want_adv.view(np.int64), err_msg="adv " + what)
    none = want_w < 0
    assert (action[none] == 0).all(), what
    ch = np.flatnonzero(~none)
    share = np.zeros(0, bool)
    if ch.size:
        k = want_w[ch]
        dx, dy = np.array([o[0] for o in host.offs])[k], np.array([o[1] for o in host.offs])[k]
        px, py = action[ch] // L - dx, action[ch] % L - dy
        assert ((px >= 0) & (px < w) & (py >= 0) & (py < w)).all(), what
        cell = px * w + py
        share = si.judge_choice(x.reshape(E, K, w2)[ch, k], masks[ch, k], cell, False, what)
    return share, want_w


class Tier(object):
    """emu: the emulated library (21 pallets), or None for the device (1 024 pallets)."""

    def __init__(self, emu=None):
        self.emu, self.pallets = emu, 1024 if emu is None else 21
        if emu is None:
            from oracle import oracle as emu
        self.mask_from_obs = emu.mask_from_obs

    def start(self, geometry):
        from bpp_amd import MultiBinPacker
        size, w, s = GEOMETRIES[geometry]
        E = self.pallets
        self.env = make_env(self.emu, small_items(size, E), size, E)
        for t in range(WARM_STEPS):
            self.env.step_tensors(self.env.sample_feasible(seed=5, step=t))
        self.mb = MultiBinPacker(self.env, w, s)
        return Host(size, w, s, E)

    def round(self, host, label, seed):
        """decide under the family's rows, step, commit.  Returns what check_launch and Host.update need."""
        import torch
        env, mb, E, K, w = self.env, self.mb, host.E, host.K, host.w
        got = {}

        def policy(obs):
            masks = masks_of(mb._sets[E]["work"].cpu().numpy(), E, K, w * w)
            check_masks(masks, obs.cpu().numpy(), self.mask_from_obs, w, host.size[2])
            value, x = family_rows(label, masks, seed)
            got.update(value=value, x=x, masks=masks, items=obs.cpu().numpy().reshape(E, K, 4, w * w)[:, 0, 1:, 0].astype(np.int64))
            return torch.from_numpy(value).to(env.device), torch.from_numpy(x).to(env.device), None
        act, adv, win = mb.decide(policy)
        r = env.step_tensors(act)
        mb.commit(r.done)
        return (got["value"], got["x"], got["masks"], act.cpu().numpy(), adv.cpu().numpy(), win.cpu().numpy(), got["items"],
                r.done.cpu().numpy())


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def tier(request):
    if request.param == "gpu":
        import torch
        assert torch.cuda.is_available()
        return Tier()
    return Tier(request.getfixturevalue("emu"))


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_multibin_choose_against_float64(tier, geometry):
    shares = {}
    again = 0
    for g, group in enumerate(launch_labels()):
        host = tier.start(geometry)
        assert len(group) >= 3, "every pallet set plays at least three decide / step / commit rounds"
        for r, label in enumerate(group):
            what = "%s %s round %d" % (geometry, label, r)
            value, x, masks, act, adv, win, items, done = tier.round(host, label, seed=1000 * g + 17 * r + host.K)
            share, want_w = check_launch(host, label, value, x, masks, act, adv, win, items, what)
            shares.setdefault(label, []).append(share)
            again += int(host.has[np.arange(host.E), np.maximum(want_w, 0)][want_w >= 0].sum())
            host.update(want_w, value.reshape(host.E, host.K), items, done)
    # a window with history wins on bin_num * reward + (v - last), never on the -0.2 of a window without: at least one such
    # decision per pallet over the test, so that the two roundings of that expression decide many advantages
    print("multibin %s: %d windows chosen with history (%d pallets)" % (geometry, again, host.E))
    assert again >= host.E, (geometry, again)
    si.check_cap(shares, "multibin " + geometry)
