"""Recorded packing plans on the device (include/bpp_placements.h): BppVecEnv.record_placements() / placements() /
replay_plans against the boxes the reference appended to space.boxes (tests/golden/placements_*.npz) through step_tensors, step()
and RolloutStorage.step; self-consistency at 4 099 and 515 bins with a numpy model of note / commit on 64 scattered bins; graph
capture; cloning, the reorder search, checkpoints and the refusals; replay at its edges; the pretrained checkpoints' 2 100
trajectories as one batch.  Helpers: tests/placement_cases.py."""
import os
import sys

import numpy as np
import pytest
import torch

import bpp_amd
from bpp_amd import PackingPlans, replay_plans

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import placement_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def records_of(plans):
    return plans.numpy()["records"]


def make_env(g, **kw):
    env = bpp_amd.BppVecEnv(g["actions"].shape[1], g["size"], enable_rotation=g["rotation"], pool=g["pool"], device=DEV, **kw)
    return env


def check_step(env, exp, g, t, done):
    exp.step(g["box"][t], g["done"][t])
    assert np.array_equal(np.asarray(done).astype(np.uint8), g["done"][t]), t
    run, fin = env.placements(), env.placements(finished=True)
    r, f = run.numpy(), fin.numpy()
    st = env.state_numpy()
    assert np.array_equal(r["count"], exp.run_count) and np.array_equal(r["count"], st["n_boxes"]), t
    assert r["records"].tobytes() == exp.run.tobytes(), t
    assert np.array_equal(r["episode"], exp.episode), t
    assert np.array_equal(f["count"], exp.fin_count) and np.array_equal(f["episode"], exp.fin_episode), t
    assert f["records"].tobytes() == exp.fin.tobytes(), t
    assert int(r["overflow"][0]) == 0


@pytest.mark.parametrize("path", ["step_tensors", "step", "storage"])
@pytest.mark.parametrize("name", pc.CASES)
def test_fixture_plans_equal_the_reference_boxes(name, path):
    g = pc.load_case(name)
    T, E = g["actions"].shape
    env = make_env(g)
    exp = pc.ExpectedPlans(E, g["size"][1], pc.default_capacity(g["size"]))
    if path == "storage":
        storage = bpp_amd.RolloutStorage(5, env, (env.obs_len,), env.action_space)
        storage.reset(env)
    else:
        env.reset()
    env.record_placements()
    assert env.placements().capacity == pc.default_capacity(g["size"])
    for t in range(T):
        a = torch.from_numpy(g["actions"][t]).to(DEV)
        if path == "step_tensors":
            done = env.step_tensors(a).done.cpu().numpy()
        elif path == "step":
            done = env.step(a)[2]
        else:
            done = storage.step(env, a).done.cpu().numpy()
        check_step(env, exp, g, t, done)
    last = env.placements()
    hmap, status, volume = replay_plans(last)
    assert torch.equal(hmap.reshape(E, -1), env.hmap) and bool((status == -1).all()) and torch.equal(volume, env.state[:, 3])
    for e in range(E):                                # the reference's tuple order, through the public accessors
        n = int(exp.run_count[e])
        assert last.boxes(e) == [(int(r["x"]), int(r["y"]), int(r["z"]), int(r["cell"]) // g["size"][1], int(r["cell"]) % g["size"][1], int(r["lz"]))
                                 for r in exp.run[e, :n]]
        assert last.flags(e) == [bool(r["rotated"]) for r in exp.run[e, :n]]
    env.close()


@pytest.mark.parametrize("size,E,steps", [((10, 10, 10), 4099, 48), ((20, 20, 20), 515, 40)])
def test_self_consistency_at_scale(size, E, steps):
    pool = bpp_amd.sequences.cut2_pool(size, 32, seed=0)
    env = bpp_amd.BppVecEnv(E, size, enable_rotation=True, pool=pool, device=DEV)
    env.reset()
    env.record_placements()
    cap = pc.default_capacity(size)
    # first, last, wave (64) and workgroup (256) edges of the one-lane-per-bin kernels, and bins in between
    edges = [0, 1, 63, 64, 65, 127, 128, 255, 256, 257, 511, 512, E - 2, E - 1]
    rng = np.random.RandomState(1)
    ids = np.array(sorted(edges + [int(v) for v in rng.choice(E, 200, replace=False) if v not in edges][:64 - len(edges)]))
    assert len(ids) == 64 and len(set(ids.tolist())) == 64
    assert {0, E - 1} <= set(ids.tolist())
    model = pc.PlanModel(ids, size, True, cap)
    a = torch.empty((E,), dtype=torch.int64, device=DEV)
    finished = 0
    for t in range(steps):
        env.sample_feasible(seed=7, step=t, out=a)
        env.epsilon_override(a, seed=7, step=t, eps=0.05)
        model.note(env.state_numpy()["item_cur"], a.cpu().numpy())
        res = env.step_tensors(a)
        done = res.done.bool()
        model.commit(res.done.cpu().numpy(), env.hmap.cpu().numpy())
        fin = env.placements(finished=True)
        assert torch.equal(fin.count[done], res.counter[done]), t          # at every done: the finished plan has the step's counter
        finished += int(done.sum())
        if t % 8 == 7 or t == steps - 1:
            run = env.placements()
            assert torch.equal(run.count, env.state[:, 2]), t
            hmap, status, volume = replay_plans(run)
            assert torch.equal(hmap.reshape(E, -1), env.hmap) and bool((status == -1).all()) and torch.equal(volume, env.state[:, 3]), t
            sub, fsub = env.placements(ids).numpy(), env.placements(ids, finished=True).numpy()
            assert sub["records"].tobytes() == model.m.run.tobytes() and np.array_equal(sub["count"], model.m.run_count), t
            assert fsub["records"].tobytes() == model.m.fin.tobytes() and np.array_equal(fsub["count"], model.m.fin_count), t
            assert np.array_equal(fsub["episode"], model.m.fin_episode), t
            assert sub["records"].tobytes() == records_of(run)[ids].tobytes()
            fh, fs, fv = replay_plans(fin)                                   # every finished plan is sound, too
            assert bool((fs == -1).all())
    assert finished > E // 4 and int(env.placements().overflow[0]) == 0
    env.close()


@pytest.mark.parametrize("side", [False, True])
def test_a_captured_lock_step_replayed_gives_the_plans_of_uncaptured_lock_steps(side):
    size, E = (10, 10, 10), 257
    pool = bpp_amd.sequences.cut2_pool(size, 32, seed=3)

    def start():
        env = bpp_amd.BppVecEnv(E, size, enable_rotation=True, pool=pool, device=DEV)
        env.reset()
        env.record_placements()
        a = env.sample_feasible(seed=5, step=0)
        env.step_tensors(a, sample=(5, 1, a))          # an uncaptured lock-step first: every kernel is loaded, every buffer exists
        return env, a

    plain, a0 = start()
    for _ in range(12):
        plain.step_tensors(a0, sample=(5, 1, a0))
    env, a = start()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    if side:
        stream = torch.cuda.Stream(device=DEV)
        with torch.cuda.graph(graph, stream=stream):
            env.step_tensors(a, sample=(5, 1, a))      # note / step / commit
        with torch.cuda.stream(stream):
            for _ in range(12):
                graph.replay()
    else:
        with torch.cuda.graph(graph):
            env.step_tensors(a, sample=(5, 1, a))
        for _ in range(12):
            graph.replay()
    torch.cuda.synchronize()
    for finished in (False, True):
        p, q = plain.placements(finished=finished).numpy(), env.placements(finished=finished).numpy()
        assert p["records"].tobytes() == q["records"].tobytes()
        assert np.array_equal(p["count"], q["count"]) and np.array_equal(p["episode"], q["episode"])
    assert torch.equal(plain.hmap, env.hmap) and int(plain.state[:, 2].sum()) > 4 * E
    plain.close()
    env.close()


def test_cloning_search_checkpoints_and_refusals(tmp_path):
    size, E = (10, 10, 10), 12
    pool = bpp_amd.sequences.cut2_pool(size, 16, seed=2)

    def fresh(record=True, **kw):
        env = bpp_amd.BppVecEnv(E, size, enable_rotation=False, pool=pool, device=DEV)
        env.reset()
        return env.record_placements(**kw) if record else env

    env = fresh()
    for t in range(6):
        env.step_tensors(env.sample_feasible(seed=1, step=t))
    # clone_bins / copy_bins / clone_into carry plans
    before = env.placements().numpy()
    env.clone_bins([0, 1], [6, 7])
    env.copy_bins([2], [8])
    env.clone_into([3], [9])
    after = env.placements().numpy()
    assert after["records"][[6, 7, 8, 9]].tobytes() == before["records"][[0, 1, 2, 3]].tobytes()
    assert np.array_equal(after["count"][[6, 7, 8, 9]], before["count"][[0, 1, 2, 3]])
    assert after["records"][[0, 1, 2, 3, 4, 5, 10, 11]].tobytes() == before["records"][[0, 1, 2, 3, 4, 5, 10, 11]].tobytes()
    hmap, status, _ = replay_plans(env.placements())
    assert torch.equal(hmap.reshape(E, -1), env.hmap) and bool((status == -1).all())
    # a reorder decision, then step_bins: the plan holds the item that was actually placed
    rs = bpp_amd.ReorderSearch(env, 3, times=2)
    ids, scratch = torch.arange(4, device=DEV), torch.arange(4, device=DEV) + 6
    action, _, _ = rs.decide(bpp_amd.reorder.int_policy(size), ids, scratch)
    items = env.state_numpy()["item_cur"][:4]
    count0 = env.placements(ids).numpy()["count"].copy()
    res = env.step_bins(ids, action)
    p = env.placements(ids)
    h = p.numpy()
    for i in range(4):
        if not bool(res.done[i]):
            last = h["records"][i, count0[i]]
            assert h["count"][i] == count0[i] + 1
            assert (int(last["x"]), int(last["y"]), int(last["z"])) == (items[i] & 255, (items[i] >> 8) & 255, (items[i] >> 16) & 255)
    hmap, status, volume = replay_plans(p)
    assert torch.equal(hmap.reshape(4, -1), env.hmap[:4]) and bool((status == -1).all()) and torch.equal(volume, env.state[:4, 3])
    # step_subset and observe() go through step_tensors: recorded / nothing recorded
    c = env.placements().numpy()["count"].copy()
    env.observe()
    assert np.array_equal(env.placements().numpy()["count"], c)
    # a state_dict round trip into a fresh env continues to the same plans
    sd = env.state_dict()
    assert set(sd["placements"]) == {"log", "capacity", "keep_finished"} and sd["placements"]["capacity"] == 256
    torch.save(sd, str(tmp_path / "env.pt"))
    twin = fresh()
    twin.load_state_dict(torch.load(str(tmp_path / "env.pt"), map_location=DEV))
    for t in range(8):
        for e_ in (env, twin):
            e_.step_tensors(e_.sample_feasible(seed=9, step=t))
    for finished in (False, True):
        p, q = env.placements(finished=finished).numpy(), twin.placements(finished=finished).numpy()
        assert p["records"].tobytes() == q["records"].tobytes() and np.array_equal(p["count"], q["count"])
        assert np.array_equal(p["episode"], q["episode"])
    # save / load of plans, replayed from the file
    env.placements().save(str(tmp_path / "plans.npz"))
    back = PackingPlans.load(str(tmp_path / "plans.npz"))
    assert back.records.device.type == "cpu" and torch.equal(replay_plans(back)[0].reshape(E, -1), env.hmap)
    # reset() clears the log: an abandoned episode is no finished plan
    env.reset()
    p, q = env.placements().numpy(), env.placements(finished=True).numpy()
    assert not p["count"].any() and (q["count"] == -1).all() and not q["records"].view(np.uint8).any()
    # the ValueErrors of load_state_dict
    plain = fresh(record=False)
    assert "placements" not in plain.state_dict()
    with pytest.raises(ValueError, match="record"):
        plain.load_state_dict(sd)                                         # key present, recording off
    with pytest.raises(ValueError, match="without packing plans"):
        twin.load_state_dict(plain.state_dict())                          # key missing, recording on
    small = fresh(capacity=32)
    with pytest.raises(ValueError, match="capacity"):
        small.load_state_dict(sd)                                         # another capacity
    nofin = fresh(keep_finished=False)
    with pytest.raises(ValueError, match="keep_finished"):
        nofin.load_state_dict(sd)
    with pytest.raises(ValueError):
        nofin.placements(finished=True)
    # the RuntimeErrors: native drivers while recording, recording twice / late / before reset, placements() without recording
    acts = torch.zeros((E,), dtype=torch.int64, device=DEV)
    for call in (lambda: env.rollout_uniform(1, 0, 4), lambda: env.rollout_uniform_sets(1, 0, 4, acts)):
        with pytest.raises(RuntimeError, match="native rollout drivers"):
            call()
    with pytest.raises(RuntimeError):
        env.record_placements()
    plain.step_tensors(plain.sample_feasible(seed=1, step=0))
    with pytest.raises(RuntimeError, match="directly after reset"):
        plain.record_placements()
    with pytest.raises(RuntimeError):
        plain.placements()
    unreset = bpp_amd.BppVecEnv(E, size, pool=pool, device=DEV)
    with pytest.raises(RuntimeError):
        unreset.record_placements()
    plain.rollout_uniform(1, 0, 2)                                        # an env that does not record still rolls out natively
    for e_ in (env, twin, plain, small, nofin, unreset):
        e_.close()


@pytest.mark.parametrize("size", pc.EDGE_GEOMETRIES, ids=lambda s: "%dx%dx%d" % s)
def test_replay_edges_equal_the_numpy_restatement(size):
    cap = 4 if size[0] * size[1] == 1 else 12
    for n in (1, 5, 67):
        records, count = pc.edge_plans(size, n, cap, seed=n + size[0])
        rec8 = torch.from_numpy(records.view(np.uint8).reshape(n, cap, 8).copy())
        for upto in (None, 0, 1, cap // 2, cap + 9) if n == 67 else (None,):
            want = pc.replay_numpy(records, count, size, upto)
            got = replay_plans(rec8, size, upto=upto, count=torch.from_numpy(count), device=DEV)
            assert got[0].device.type == "cuda"
            for w, g_ in zip(want, got):
                assert np.array_equal(w, g_.cpu().numpy()), (n, upto)
    assert (want[1][3:] >= 0).sum() >= 40


@pytest.mark.parametrize("rot", [False, True])
def test_pretrained_checkpoint_plans_of_all_2100_trajectories(rot):
    name = "pretrained_eval_cut2_10" + ("_rot" if rot else "")
    g = dict(np.load(os.path.join(pc.GOLDEN, name + ".npz")))
    pool = np.load(os.path.join(pc.GOLDEN, "cut2_dataset_10.npz"))["pool"]
    E, T = g["actions"].shape
    size = tuple(int(v) for v in g["size"])
    env = bpp_amd.BppVecEnv(E, size, enable_rotation=rot, pool=pool, device=DEV)
    env.reset()
    env.record_placements(capacity=64)
    actions = g["actions"].astype(np.int64)
    actions[np.arange(T)[None, :] >= g["steps"][:, None]] = pc.NOOP       # a trajectory that has ended is left alone
    dev_actions = torch.from_numpy(actions).to(DEV)
    for t in range(T):
        env.step_tensors(dev_actions[:, t].contiguous())
    plans = env.placements(finished=True)
    hmap, status, volume = replay_plans(plans)
    h = plans.numpy()
    assert (status.cpu().numpy() == -1).all() and (h["episode"] == 0).all() and int(h["overflow"][0]) == 0
    assert np.array_equal(h["count"], g["counter"])
    assert np.array_equal(volume.cpu().numpy() / float(size[0] * size[1] * size[2]), g["ratio"])
    if rot:
        f = np.load(os.path.join(pc.GOLDEN, "placements_%s.npz" % name))
        want = pc.box_records(f["box"], size[1])                          # [n, T] records, zero where nothing was appended
        traj = f["traj"]
        assert len(traj) == 2100
        assert h["records"][traj][:, :T].tobytes() == want.tobytes() and not h["records"][:, T:].view(np.uint8).any()
        for i in (0, 1234, 2099):
            k = int(np.flatnonzero(traj == i)[0])
            assert plans.boxes(i) == [tuple(int(v) for v in b[:6]) for b in f["box"][k] if b[0] >= 0]
    env.close()
