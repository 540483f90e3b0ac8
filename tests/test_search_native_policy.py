"""The three native searches (ReorderSearch, MCTSearch, MultiBinPacker) under bpp_policy_forward itself -- the network of the
reference inside the searches of the reference, which is what the two halves are for and what no other test runs.  Judged forward
by forward (tests/search_native_cases.py): every forward inside a decision against a reference of its own recorded input, then a
tape replay on an identically built second env, which proves that the search kernels consumed exactly the outputs the forward
wrote (and that the next emit did not overwrite an obs the forward had still to read).

Emulated half (no marker): the product kernels on the host SIMT emulator, the three search classes on an EmuVecEnv with
pc.host_runner on a packed blob as their policy, geometry (5, 32, 25), P + 1 slots so that one trunk workgroup is partial.  Side 5 with H = 32 is judged exactly only: the float32 torch yardstick is unstable on tiny networks (policy_cases).

Device half (`-m gpu`): BppVecEnv and the three search classes with NativePolicy, geometry (10, 256, 100), T + 3 slots (odd against
P = 2, a head tile of 3): the exact network (a), its tape replay (b), the live policy on a side stream, which is another workspace
key (c), real weights under the 8 x e_torch32 rule and their replay (d), and decisions of n, n // 2 and n slots in turn (e).  The
two checkpoint examples run in both forms.  Reads nothing of the reference tree."""
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_cases as pc  # noqa: E402
import search_native_cases as sn  # noqa: E402
from conftest import load_golden  # noqa: E402
from emu_env import torch_policy  # noqa: E402
from test_gpu_policy_forward import _checkpoint  # noqa: E402
from test_policy_forward import emu_lib  # noqa: E402,F401  (the module's fixture: the emulated library bound with bind_policy)
from test_reorder_search import make_env  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
G5, G10 = (5, 32, 25), (10, 256, 100)
SEARCHES = ["reorder", "mcts", "multibin"]
REAL_SEED = 11
ROUNDS = 8            # decisions of every slot in the device half

# search -> (bin, pool fixture or None for CUT-2 sequences of small items, search parameters) at the emulated and at the device
# shapes.  The device reorder game plays small items: under a network that knows nothing of feasibility a permuted placement
# order of the fixture's 2 .. 5 items is seldom completed, and the search then never leaves the greedy baseline.
EMU_SHAPES = {"reorder": ((5, 5, 3), "reorder_fake_5x5x3", dict(k=3), 1),
              "mcts": ((5, 5, 3), "mcts_fake_5x5x3", dict(k=3, sims=4), 2),
              "multibin": ((10, 10, 10), None, dict(w=5, s=5), 2)}
DEV_SHAPES = {"reorder": ((10, 10, 10), None, dict(k=4)),
              "mcts": ((10, 10, 10), "mcts_fake_10", dict(k=3, sims=16)),
              "multibin": ((20, 20, 10), "multibin_fake_20x20x10", dict(w=10, s=10))}
MULTIBIN_PALLETS = 17


def wide_item(w):
    """An item that fits the pallet and no window of side w: 12 x 8 at w = 10, 6 x 4 at w = 5."""
    d = max(1, w // 5)
    return (w + d, w - d, 2)


def pool_of(name, size, rows, wide=None):
    """`rows` item sequences: the fixture's pool (repeated where it is shorter), or `rows` distinct CUT-2 sequences of small items,
    so that no two slots of a deterministic search hold the same observation.  wide = w: every third sequence r holds
    wide_item(w) as item (r // 3) mod 3, transposed in every other one of them -- window rows whose item planes exceed the window
    side, from the first decision of pallet 0 on.  (A wide item has no window, so it goes to the pallet's corner; on every
    pallet it would leave the last window unchosen.)"""
    if name is None:
        from bpp_amd.sequences import cut2_pool
        pool = cut2_pool(size, rows, seed=3, bound=(2, 3), native=False)
    else:
        pool = load_golden(name)["pool"]
    pool = np.ascontiguousarray(pool[np.arange(rows) % len(pool)])
    if wide is not None:
        x, y, z = wide_item(wide)
        for r in range(0, rows, 3):
            pool[r, r // 3 % 3, :3] = (x, y, z) if r % 2 == 0 else (y, x, z)
    return pool


# ------------------------------------------------------------------------------------------------------------------ the games
# A game is one env with one search object; play(policy, rounds) runs the schedule of the examples -- decide, step the real bins,
# advance / commit -- and returns the decision outputs per round, the real bins' heightmaps after the last step, and what the
# conditions need.  Two games made with the same arguments are identical.
class Game(object):
    """emu: the emulated library, or None for the device."""

    def __init__(self, emu, search, size, pool, n, **kw):
        import bpp_amd
        self.search, self.n = search, n
        E = n if search == "multibin" else 2 * n
        wide = kw["w"] if search == "multibin" else None
        self.env = make_env(emu, pool_of(pool, size, n, wide), size, E)
        self.ids = torch.arange(n, device=self.env.device)
        if search == "reorder":
            self.s = bpp_amd.ReorderSearch(self.env, kw["k"])
        elif search == "mcts":
            self.s = bpp_amd.MCTSearch(self.env, kw["k"], sim_times=kw["sims"])
            self.s.seed(self.ids, self.ids + 5)
        else:
            self.s = bpp_amd.MultiBinPacker(self.env, kw["w"], kw["s"])
            self.K = self.s.K

    def play(self, policy, rounds, stats=False):
        """Enqueues everything on the current stream; stats: also read the MCTS roots (a synchronisation per round)."""
        s, env, ids, n = self.s, self.env, self.ids, self.n
        out, info = [], dict(done=[], children=[], windows=[])
        for _ in range(rounds):
            if self.search == "reorder":
                dec = s.decide(policy, ids, ids + n)
                res = env.step_bins(ids, dec[0])
            elif self.search == "mcts":
                dec = s.decide(policy, ids, ids + n)
                if stats:
                    info["children"].append(s.root_stats(ids)[2])
                res = env.step_bins(ids, dec[0])
                s.advance(res.done)
            else:
                dec = s.decide(policy, ids)
                res = env.step_bins(ids, dec[0])
                s.commit(res.done)
                info["windows"].append(dec[2])
            out.append(dec)
            info["done"].append(res.done.reshape(-1).clone())
        final = env.heightmaps()[:n].clone()
        if env.device.type == "cuda":
            torch.cuda.synchronize()
        info["done"] = [sn.to_numpy(d).astype(bool) for d in info["done"]]
        info["windows"] = [sn.to_numpy(w) for w in info["windows"]]
        info["overflow"] = int(s.overflow.item()) if getattr(s, "overflow", None) is not None else 0
        return out, final, info


def first_episode_lengths(done):
    """Decisions of every slot's first episode, cut at the rounds played (so the mean is a lower bound)."""
    done = np.stack(done)                                      # [rounds, n]
    return np.where(done.any(0), done.argmax(0) + 1, done.shape[0])


def check_wide_rows(search, game, calls):
    """Multi-bin: row 0 of call 0 -- which the exact judge (every row of call 0), the alone judge (row 0 of call 0) and the tape all
    see -- holds an item wider than the window, as do the other window rows of that pallet."""
    if search != "multibin":
        return
    w = game.s.w
    A = w * w
    wide = [np.maximum(sn.to_numpy(obs)[:, A], sn.to_numpy(obs)[:, 2 * A]) > w for obs, _ in calls]
    assert wide[0][:game.K].all(), [int(v.sum()) for v in wide]
    print("multibin: rows whose item exceeds the window, per call: %r" % [int(v.sum()) for v in wide])


def check_conditions(search, decisions, info, K=None):
    """The meaningfulness conditions of the exact run: the search had something to decide."""
    if search == "reorder":
        dflt = np.concatenate([sn.to_numpy(d[2]).astype(bool) for d in decisions])
        print("reorder: %d of %d decisions are the greedy baseline's" % (dflt.sum(), dflt.size))
        assert (~dflt).mean() >= 0.1 and dflt.mean() >= 0.1, dflt.mean()
    elif search == "mcts":
        ch = np.concatenate(info["children"])
        lens = first_episode_lengths(info["done"])
        print("mcts: %.2f of %d roots have two or more children, mean decisions per episode >= %.2f" % ((ch >= 2).mean(), ch.size, lens.mean()))
        assert (ch >= 2).mean() >= 0.5 and lens.mean() >= 5, ((ch >= 2).mean(), lens.mean())
    else:
        win = np.concatenate(info["windows"])
        count = np.bincount(win[win >= 0], minlength=K)
        print("multibin: windows chosen %r, none %d" % (count.tolist(), int((win < 0).sum())))
        assert (count >= 1).all(), count


# ------------------------------------------------------------------------------------------------------------- emulated half
def emu_game(emu, emu_lib, search):
    size, pool, kw, rounds = EMU_SHAPES[search]
    n = pc.info(emu_lib, G5, 1)["bins_per_trunk_group"] + 1
    return Game(emu, search, size, pool, n, **kw), rounds


@pytest.mark.parametrize("search", SEARCHES)
def test_emulated_search_under_the_exact_network(emu, emu_lib, search):
    """Recorder, exact judge on every row of every call, alone judge, tape replay on a second env."""
    t0 = time.perf_counter()
    i = pc.info(emu_lib, G5, 1)
    P, T = i["bins_per_trunk_group"], i["bins_per_head_tile"]
    net = sn.exact_net(G5)
    policy = torch_policy(sn.host_policy(emu_lib, G5, net.blob))
    a, rounds = emu_game(emu, emu_lib, search)
    rec = sn.Recorder(policy)
    dec_a, hmap_a, info = a.play(rec, rounds)
    assert info["overflow"] == 0
    check_wide_rows(search, a, rec.calls)
    rows = sn.judge_exact(net, sn.host_calls(rec.calls), P, T, all_rows=True)
    alone = sn.judge_alone(policy, rec.calls, P, T)
    b, _ = emu_game(emu, emu_lib, search)
    tape = sn.Tape(rec.calls)
    dec_b, hmap_b, _ = b.play(tape, rounds)
    assert not tape.mismatch()
    sn.same_decisions(dec_a, dec_b, search + " replay")
    assert torch.equal(hmap_a, hmap_b)
    print("%s: %d calls, %d rows exact, %d alone, %.1f s" % (search, len(rec.calls), rows, alone, time.perf_counter() - t0))


@pytest.mark.parametrize("search", SEARCHES)
def test_emulated_search_under_real_weights(emu, emu_lib, search):
    """pc.real_weights at side 5: recorder and alone judge (no 8 x rule at this side, see the module's docstring); the tape replay
    as well."""
    t0 = time.perf_counter()
    i = pc.info(emu_lib, G5, 1)
    P, T = i["bins_per_trunk_group"], i["bins_per_head_tile"]
    blob = pc.pol.pack_weights(pc.real_weights(*G5, REAL_SEED), *G5).numpy()
    policy = torch_policy(sn.host_policy(emu_lib, G5, blob))
    a, rounds = emu_game(emu, emu_lib, search)
    rec = sn.Recorder(policy)
    dec_a, hmap_a, info = a.play(rec, rounds)
    assert info["overflow"] == 0 and len(rec.calls) >= 2
    check_wide_rows(search, a, rec.calls)
    alone = sn.judge_alone(policy, rec.calls, P, T)
    b, _ = emu_game(emu, emu_lib, search)
    tape = sn.Tape(rec.calls)
    dec_b, hmap_b, _ = b.play(tape, rounds)
    assert not tape.mismatch()
    sn.same_decisions(dec_a, dec_b, search + " replay")
    assert torch.equal(hmap_a, hmap_b)
    print("%s: %d calls, %d alone, %.1f s" % (search, len(rec.calls), alone, time.perf_counter() - t0))


@pytest.mark.parametrize("search", SEARCHES)
def test_conditions_hold_for_the_int64_forward_alone(emu, search):
    """The seed and shifts of sn.EXACT at the device shapes with 8 slots: the emulated search kernels driven by the int64 numpy
    forward, no policy kernel involved.  What test (a) on the device then asserts of the kernels is a property of the reference."""
    size, pool, kw = DEV_SHAPES[search]
    net = sn.exact_net(G10)
    game = Game(emu, search, size, pool, 8, **kw)
    decisions, _, info = game.play(torch_policy(net.policy_np()), ROUNDS, stats=True)
    assert info["overflow"] == 0
    check_conditions(search, decisions, info, getattr(game, "K", None))


def test_recorder_and_tape_on_host_arrays():
    """The tape returns the recorded outputs in order, flags an obs that differs in one element, and refuses a call too many."""
    calls = []

    def policy(obs):
        calls.append(1)
        return obs[:, 0] + len(calls), obs[:, :3] * 2.0, None
    rec = sn.Recorder(policy)
    buf = np.arange(12, dtype=np.float32).reshape(3, 4)
    for _ in range(2):
        rec(buf)
        buf += 1.0                                             # the caller reuses its buffer: the recorder kept a copy
    assert rec.calls[0][0][0, 0] == 0.0 and rec.calls[1][0][0, 0] == 1.0
    tape = sn.Tape(rec.calls)
    buf -= 2.0
    assert np.array_equal(tape(buf)[0], rec.calls[0][1][0])
    buf += 1.0
    assert tape(buf)[2] is None and not tape.mismatch()
    again = sn.Tape(rec.calls)
    again(buf - 1.0)
    buf[2, 3] += 1.0
    again(buf)
    assert again.mismatch()
    with pytest.raises(IndexError):
        again(buf)


def test_exact_net_is_exact_and_its_shifts_are_exponent_shifts():
    """The int64 forward of ExactNet equals a float64 torch_forward of its scaled float32 weights, on rows with heights up to H and
    item extents up to 20 (every term is an integer below 2^24 times a power of two)."""
    for geom, top in ((G5, 10), (G10, 20)):
        net = sn.exact_net(geom)
        A = geom[0] ** 2
        rng = np.random.RandomState(1)
        obs = np.concatenate([rng.randint(0, 11, (6, A)), np.repeat(rng.randint(1, top + 1, (6, 3)), A, 1)], 1).astype(np.float32)
        signs = {}
        want = net.forward(obs, signs)
        with torch.no_grad():
            ref = pc.pol.torch_forward({k: v.double() for k, v in net.plain.items()}, torch.from_numpy(obs).double())
        for h, t in zip(pc.HEADS, ref):
            assert np.array_equal(want[h].astype(np.float64), t.numpy()), (geom, h)
        assert all((p and m) or name in sn.ONE_SIGN for name, (p, m) in signs.items())


# --------------------------------------------------------------------------------------------------------------- device half
@pytest.fixture(scope="module")
def bpp():
    import bpp_amd
    assert torch.cuda.is_available()
    return bpp_amd


@pytest.fixture(scope="module")
def tiles(bpp):
    i = pc.info(bpp._lib.lib(), G10, 1)
    return i["bins_per_trunk_group"], i["bins_per_head_tile"]


def gpu_game(search, tiles):
    size, pool, kw = DEV_SHAPES[search]
    n = MULTIBIN_PALLETS if search == "multibin" else tiles[1] + 3
    return Game(None, search, size, pool, n, **kw)


def native(bpp, plain):
    return bpp.NativePolicy(G10[0], G10[2], G10[1]).load_state_dict(plain).to(DEV)


def replay(search, tiles, rec, dec_a, hmap_a):
    """(b): an identically built env and search under the tape."""
    b = gpu_game(search, tiles)
    tape = sn.Tape(rec.calls)
    dec_b, hmap_b, _ = b.play(tape, ROUNDS)
    assert not tape.mismatch(), "an obs of the replay differs from the recorded one"
    sn.same_decisions(dec_a, dec_b, search + " replay")
    assert torch.equal(hmap_a, hmap_b)


@pytest.mark.gpu
@pytest.mark.parametrize("search", SEARCHES)
def test_gpu_search_under_the_exact_network(bpp, tiles, search):
    """(a) recorder, exact judge, alone judge, the conditions, overflow 0; (b) tape replay; (c) the live policy on a side stream."""
    P, T = tiles
    net = sn.exact_net(G10)
    policy = native(bpp, net.plain)
    a = gpu_game(search, tiles)
    if search != "multibin":
        assert a.n == T + 3 and a.n % P == 1 and a.n % T == 3
    else:
        assert a.n * a.K == 68
    rec = sn.Recorder(policy)
    dec_a, hmap_a, info = a.play(rec, ROUNDS, stats=True)
    assert info["overflow"] == 0
    check_wide_rows(search, a, rec.calls)
    host = sn.host_calls(rec.calls)
    rows = sn.judge_exact(net, host, P, T)
    alone = sn.judge_alone(policy, rec.calls, P, T)
    print("%s: %d calls, %d rows exact, %d alone" % (search, len(host), rows, alone))
    check_conditions(search, dec_a, info, getattr(a, "K", None))
    replay(search, tiles, rec, dec_a, hmap_a)
    c = gpu_game(search, tiles)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        key = (torch.device(DEV), side.cuda_stream, G10)
        pc.pol._WORKSPACE.pop(key, None)                       # torch hands streams out of a pool: an earlier test may have had this one
        dec_c, hmap_c, _ = c.play(policy, ROUNDS)
        assert key in pc.pol._WORKSPACE
    side.synchronize()
    pc.pol._WORKSPACE.pop(key)
    sn.same_decisions(dec_a, dec_c, search + " side stream")
    assert torch.equal(hmap_a, hmap_c)


@pytest.mark.gpu
@pytest.mark.parametrize("search", SEARCHES)
def test_gpu_search_under_real_weights(bpp, tiles, search):
    """(d) pc.real_weights(10, 256, 100, 11): real judge (e_native <= 8 e_torch32 per head, pooled over the sampled rows of every
    eighth call, printed), alone judge, tape replay."""
    P, T = tiles
    plain = pc.real_weights(*G10, REAL_SEED)
    policy = native(bpp, plain)
    a = gpu_game(search, tiles)
    rec = sn.Recorder(policy)
    dec_a, hmap_a, info = a.play(rec, ROUNDS)
    assert info["overflow"] == 0
    check_wide_rows(search, a, rec.calls)
    sn.judge_real(plain, G10, sn.host_calls(rec.calls), P, T, "device, %s" % search)
    sn.judge_alone(policy, rec.calls, P, T)
    replay(search, tiles, rec, dec_a, hmap_a)


@pytest.mark.gpu
def test_gpu_decisions_of_n_half_and_n_slots_share_one_workspace(bpp, tiles):
    """(e) ReorderSearch.decide with n, n // 2 and n slots in turn: the workspace of this stream and geometry is grown by the first
    call and serves the other two; the third decision is a fresh search's decision on the same state (and the first one's: a
    reorder decision only reads the real bins)."""
    P, T = tiles
    policy = native(bpp, sn.exact_net(G10).plain)
    a, b = gpu_game("reorder", tiles), gpu_game("reorder", tiles)
    n, ids = a.n, a.ids
    key = (torch.device(DEV), torch.cuda.current_stream(DEV).cuda_stream, G10)
    pc.pol._WORKSPACE.pop(key, None)
    half = n // 2
    first = a.s.decide(policy, ids, ids + n)
    grown = pc.pol._WORKSPACE[key].numel()
    assert grown == (int(bpp._lib.lib().bpp_policy_forward_workspace(pc.geom_arg(G10), n)) + 3) // 4
    part = a.s.decide(policy, ids[:half], ids[:half] + n)
    again = a.s.decide(policy, ids, ids + n)
    assert pc.pol._WORKSPACE[key].numel() == grown
    fresh = b.s.decide(policy, ids, ids + n)
    torch.cuda.synchronize()
    sn.same_decisions([again], [fresh], "n after n // 2")
    sn.same_decisions([first], [fresh], "the first n")
    sn.same_decisions([part], [tuple(t[:half] for t in fresh)], "n // 2")
    assert int(a.s.overflow.item()) == 0


@pytest.mark.gpu
def test_gpu_recorder_and_tape_do_not_synchronise(bpp, tiles):
    """A decision under the recorder, and its replay under the tape, enqueue without waiting for the device."""
    policy = native(bpp, sn.exact_net(G10).plain)
    a, b = gpu_game("mcts", tiles), gpu_game("mcts", tiles)
    n, ids = a.n, a.ids
    a.s.decide(policy, ids, ids + n)                           # buffers, the workspace and the LDS opt-in are made on first use
    b.s.decide(policy, ids, ids + n)
    rec = sn.Recorder(policy)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        first = a.s.decide(rec, ids, ids + n, check=False)
        tape = sn.Tape(rec.calls)
        second = b.s.decide(tape, ids, ids + n, check=False)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert not tape.mismatch()
    sn.same_decisions([first], [second], "replay without synchronisation")


# ------------------------------------------------------------------------------------------------------------- the examples
def _example(name, **kw):
    """Both forms of examples/<name>.py at --limit 32; the two means of each and the trajectories identical between them go to
    profiles/search_native_<name>.json.  No threshold on the identical ones: nobody has measured it and MCTS samples; the parity
    statement is the tests above."""
    path, _ = _checkpoint("default_cut_2.pt")
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    ex = __import__(name)
    runs = {}
    for form, flag in (("torch", False), ("native", True)):
        r = ex.evaluate(path, limit=32, native=flag, **kw)
        assert len(r["ratio"]) == 32 and np.isfinite(r["ratio"]).all() and (r["ratio"] > 0).all() and (r["counter"] > 0).all(), form
        assert r.get("overflow", 0) == 0, form
        runs[form] = r
    same = (runs["torch"]["ratio"] == runs["native"]["ratio"]) & (runs["torch"]["counter"] == runs["native"]["counter"])
    out = {"checkpoint": "pretrained_models/default_cut_2.pt", "trajectories": 32, "arguments": kw,
           "trajectories_identical_between_the_forms": int(same.sum())}
    for form, r in runs.items():
        out[form] = {"mean_space_utilisation": float(r["ratio"].mean()), "mean_items_packed": float(r["counter"].mean()),
                     "lock_steps": int(r["lock_steps"])}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "search_native_%s.json" % name), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


@pytest.mark.gpu
def test_gpu_mcts_checkpoint_example_runs_in_both_forms(bpp):
    _example("mcts_checkpoint", k=3, sims=8)


@pytest.mark.gpu
def test_gpu_multibin_checkpoint_example_runs_in_both_forms(bpp):
    _example("multibin_checkpoint")
