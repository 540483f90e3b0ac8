"""Shared by tests/test_rollout_storage.py and tests/test_gpu_rollout_storage.py: the recorded cases of
tests/golden/returns_golden.npz (make_returns_golden.py) and tests/golden/returns_edges.npz (make_returns_edges.py, which
also draws its inputs from here), a numpy front-end of bpp_compute_returns_host / the emulated bpp_compute_returns, and
random inputs for the comparisons that need no recording."""
import ctypes
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "returns_golden.npz")
VARIANTS = [(0, 0), (0, 1), (1, 0), (1, 1)]          # (use_gae, use_proper_time_limits)
INPUTS = ("rewards", "value_preds", "next_value", "masks", "bad_masks", "returns0")


def load_cases():
    """[(case id, dict of inputs, T, N, gamma, gae_lambda, use_gae, proper, returns after, value_preds[T] after)]"""
    g = np.load(GOLDEN)
    out = []
    for c, (s, k, use_gae, proper) in enumerate(g["cases"].tolist()):
        T, N = (int(v) for v in g["shapes"][s])
        d = {name: g["%s_%d" % (name, s)] for name in INPUTS}
        out.append((c, d, T, N, float(g["gl"][k][0]), float(g["gl"][k][1]), use_gae, proper, g["returns_%d" % c], g["vlast_%d" % c]))
    return out


def _float64_inputs(rng, T, N, bad_ones=False):
    return {"rewards": rng.uniform(0.0, 2.0, (T, N)), "value_preds": rng.normal(0.0, 3.0, (T + 1, N)),
            "next_value": rng.normal(0.0, 3.0, (N,)), "masks": (rng.uniform(size=(T + 1, N)) >= 0.2) * 1.0,
            "bad_masks": np.ones((T + 1, N)) if bad_ones else (rng.uniform(size=(T + 1, N)) >= 0.1) * 1.0,
            "returns0": rng.normal(0.0, 100.0, (T + 1, N))}


def random_inputs(T, N, seed, bad_ones=False):
    d = _float64_inputs(np.random.RandomState(seed), T, N, bad_ones)
    return {k: v.astype(np.float32) for k, v in d.items()}


# ---------------------------------------------------------------- the edge fixture (tests/golden/returns_edges.npz)
EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "returns_edges.npz")
EDGE_T = (1, 7, 8, 9, 13, 16, 17, 33)            # kReturnsRows = 8: one partial chunk, full chunks, full + partial
EDGE_N = (1, 3, 4, 5, 252, 256, 260)             # one lane of the 16-byte form; either side of a 64-lane workgroup; 65 lanes
EDGE_LONG = ((1000, 4), (1000, 5))               # 125 chunks, both forms
FAMILIES = ("unit", "denormal", "huge")
DENORMAL_SCALE = 4e-39                           # O(1) data times this straddles FLT_MIN = 1.1755e-38: products and sums go subnormal
HUGE_SCALE = 1.2e38                              # ... times this: two or three terms overflow FLT_MAX = 3.4028e38
HUGE_BINS = 0.4                                  # share of the bins of a "huge" set that carry the large magnitudes
EDGE_TILE = 17                                   # distinct bin columns of a wide edge set (see family_inputs)
FLT_MIN = float(np.finfo(np.float32).tiny)


def family_inputs(family, T, N, seed, tile=0):
    """Inputs of one value family, float32 (returns0: the constant -7, so that rows a call must leave alone are recognisable):
      unit      the O(1) data of random_inputs;
      denormal  rewards, values and next_value scaled by DENORMAL_SCALE (in float64, then rounded): subnormal inputs, products
                and results -- a kernel that flushes them gives different bits;
      huge      HUGE_BINS of the bins scaled by HUGE_SCALE (finite inputs, clipped to +-3.3e38): sums overflow to +-inf, and the
                next zero mask multiplies inf, which is NaN from there back to t = 0.
    tile > 0: only `tile` distinct bin columns, column n holding column n mod tile -- bins are independent, so the recorded results
    repeat with that period and compress, while every lane still has to address its own bins (EDGE_TILE is prime: no lane, wave or
    workgroup stride maps a bin onto its copy)."""
    rng = np.random.RandomState(seed)
    d = _float64_inputs(rng, T, N)
    big = ("rewards", "value_preds", "next_value")
    if family == "denormal":
        for k in big:
            d[k] = d[k] * DENORMAL_SCALE
    elif family == "huge":
        hot = np.where(rng.uniform(size=N) < HUGE_BINS, HUGE_SCALE, 1.0)
        for k in big:
            d[k] = np.clip(d[k] * hot, -3.3e38, 3.3e38)
    elif family != "unit":
        raise ValueError(family)
    d["returns0"] = np.full((T + 1, N), -7.0)
    if tile:
        d = {k: v[..., np.arange(N) % tile] for k, v in d.items()}
    return {k: np.ascontiguousarray(v.astype(np.float32)) for k, v in d.items()}


def split_product_pair():
    """(gamma, gae_lambda), the first of a fixed scan of three-decimal pairs, whose double product rounds to another float32 than
    the product of the two float32s: the kernel's gl = (float)(gamma * gae_lambda) is the former, as Python and torch form it."""
    f = np.float32
    for i in range(900, 1000):
        for j in range(900, 1000):
            g, lam = i / 1000.0, j / 1000.0
            if f(g * lam) != f(f(g) * f(lam)):
                return g, lam
    raise AssertionError("no such pair in the scan")


def edge_plan():
    """[(family, T, N, tile, [indices into edge_pairs()])] of the input sets of returns_edges.npz, in file order.  The unit family
    covers EDGE_T x {1, 3, 4, 5, 260}, EDGE_N at T = 13, both sides of the workgroup boundary at T = 9 and 17, and EDGE_LONG, with
    the five (gamma, lambda) pairs dealt round robin -- (13, 260) takes them all, EDGE_LONG (0.99, 0.95) and (1, 1); the other
    families take a few shapes each."""
    plan, k = [], 0
    shapes = [(T, N) for T in EDGE_T for N in EDGE_N if N in (1, 3, 4, 5, 260) or T == 13 or (T in (9, 17) and N in (252, 256))]
    for T, N in shapes:
        tile = EDGE_TILE if N >= 252 else 0
        plan.append(("unit", T, N, tile, list(range(5)) if (T, N) == (13, 260) else [k % 5]))
        k += 1
    # 125 chunks: pairs under which the carried value matters in every variant (gamma = 0 or lambda = 0 would multiply it away)
    plan += [("unit", T, N, 0, [g]) for (T, N), g in zip(EDGE_LONG, (0, 3))]
    for family in ("denormal", "huge"):
        for T, N, g in ((13, 5, 0), (17, 260, 4), (9, 256, 0), (33, 4, 3), (13, 252, 0)):
            plan.append((family, T, N, EDGE_TILE if N >= 252 else 0, [g]))
    return plan


def edge_pairs():
    return [(0.99, 0.95), (0.0, 0.95), (0.99, 0.0), (1.0, 1.0), split_product_pair()]


def load_edge_cases():
    """load_cases() for returns_edges.npz, with the value family appended to every tuple."""
    g = np.load(EDGES)
    shapes = [(int(T), int(N)) for T, N in g["shapes"]]
    rows = {"rewards": 0, "value_preds": 1, "masks": 1, "bad_masks": 1}           # rows beyond T

    def cut(flat, sizes):
        ends = np.cumsum(sizes)
        assert ends[-1] == flat.size
        return [flat[e - n:e] for e, n in zip(ends, sizes)]

    sets = [dict(returns0=np.full((T + 1, N), -7.0, dtype=np.float32)) for T, N in shapes]
    for name, extra in rows.items():
        for d, (T, N), a in zip(sets, shapes, cut(g[name], [(T + extra) * N for T, N in shapes])):
            d[name] = a.reshape(T + extra, N)
    for d, a in zip(sets, cut(g["next_value"], [N for _, N in shapes])):
        d["next_value"] = a
    cases = g["cases"].tolist()
    returns = cut(g["returns"], [(shapes[s][0] + 1) * shapes[s][1] for s, _, _, _ in cases])
    vlast = cut(g["vlast"], [shapes[s][1] for s, _, _, _ in cases])
    out = []
    for c, (s, k, use_gae, proper) in enumerate(cases):
        T, N = shapes[s]
        out.append((c, sets[s], T, N, float(g["gl"][k][0]), float(g["gl"][k][1]), use_gae, proper, returns[c].reshape(T + 1, N), vlast[c],
                    str(g["family"][s])))
    return out


def done_of(masks):
    """u8 [T][N] done bytes that stand for masks rows 1 .. T (nonzero bytes other than 1 among them: any nonzero byte is 'done')."""
    done = (masks[1:] == 0.0).astype(np.uint8)
    done[done == 1] = np.where(np.arange(int(done.sum())) % 3 == 0, 255, 1).astype(np.uint8)
    return done


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    """got == want bit for bit wherever `want` (the reference's value) is not NaN; where it is NaN, `got` must be NaN.  NaN
    positions are compared as a class because x86 and the GPU give the default NaN different sign and payload bits (inf - inf is
    0xFFC00000 on the one and 0x7FC00000 on the other).  Nothing else is masked out."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(bits(got)[~nan], bits(want)[~nan]) and np.isnan(got[nan]).all())


def placed(a, shift=0):
    """A copy of `a` whose data starts `shift` bytes past a 16-byte boundary."""
    flat = np.ascontiguousarray(a).reshape(-1)
    buf = np.zeros(flat.nbytes + 32, dtype=np.uint8)
    off = -buf.ctypes.data % 16 + shift
    out = buf[off:off + flat.nbytes].view(flat.dtype)
    out[:] = flat
    assert out.ctypes.data % 16 == shift
    return out.reshape(np.shape(a))


def run(handle, d, T, N, gamma, lam, use_gae, proper, use_done=False, bad=True, advantages=False, kernel=False, masks_out=True):
    """One call on 16-byte aligned COPIES of the inputs (numpy, host pointers).  kernel=True: bpp_compute_returns of an emulated
    library (the device kernel on the host), else bpp_compute_returns_host.  Returns dict(returns, value_preds, masks, advantages,
    rc, form = bins per lane bpp_compute_returns_info reports for the call)."""
    a = {k: placed(v) for k, v in d.items()}
    ret = a["returns0"]
    done = placed(done_of(a["masks"])) if use_done else None
    masks = a["masks"]
    if use_done:
        masks[1:] = -7.0                  # outputs on this path: whatever was there must not be read
    adv = placed(np.full((T, N), -7.0, dtype=np.float32)) if advantages else None

    def p(x):
        return x.ctypes.data if x is not None else None

    args = [p(a["rewards"]), p(a["value_preds"]), p(a["next_value"]), p(done), p(masks) if (masks_out or not use_done) else None,
            p(a["bad_masks"]) if bad else None, p(ret), p(adv), T, N, int(use_gae), int(proper), gamma, lam]
    info = (ctypes.c_int32 * 3)()
    form = info[0] if handle.bpp_compute_returns_info(*args, info) == 0 else None
    rc = handle.bpp_compute_returns(*args, None) if kernel else handle.bpp_compute_returns_host(*args)
    return dict(returns=ret, value_preds=a["value_preds"], masks=masks, advantages=adv, rc=rc, form=form)


# ---------------------------------------------------------------- the reference's storage across updates (storage_updates_*.npz)
STORAGE_CASES = ("cut2_10", "cut2_10_rot")


def load_storage_case(name):
    """(rollout recording, storage recording of tests/golden/make_storage_golden.py) of one case."""
    golden = os.path.dirname(GOLDEN)
    return dict(np.load(os.path.join(golden, "rollout_%s.npz" % name))), dict(np.load(os.path.join(golden, "storage_updates_%s.npz" % name)))


def check_storage_update(snap, g, s, u, small_rows=None):
    """The public slabs of a bpp_amd.RolloutStorage after update u (`snap`: name -> numpy array, taken after the second
    compute_returns; snap["returns_main"]: `returns` after the first) against the reference's storage at that point: slot j holds
    lock-step u * T + j - 1 of the rollout recording `g`, everything else is the storage recording `s`, bit for bit.
    small_rows: the rows a lock-step filled, whose done / counter / ratio rows are compared with `g` too (None: all)."""
    T = int(s["T"])
    k0 = u * T
    first = (g["obs0"], g["mask0"]) if u == 0 else (g["obs"][k0 - 1], g["mask"][k0 - 1])
    assert snap["obs"].dtype == np.float32 and snap["location_masks"].dtype == np.float32
    np.testing.assert_array_equal(snap["obs"][0], first[0], err_msg="obs[0] u=%d" % u)
    np.testing.assert_array_equal(snap["location_masks"][0], first[1], err_msg="location_masks[0] u=%d" % u)
    np.testing.assert_array_equal(snap["obs"][1:], g["obs"][k0:k0 + T], err_msg="obs u=%d" % u)
    np.testing.assert_array_equal(snap["location_masks"][1:], g["mask"][k0:k0 + T], err_msg="location_masks u=%d" % u)
    np.testing.assert_array_equal(snap["actions"][:, :, 0], g["actions"][k0:k0 + T], err_msg="actions u=%d" % u)
    assert np.array_equal(bits(snap["rewards"][:, :, 0]), bits(g["reward"][k0:k0 + T])), u
    assert np.array_equal(bits(snap["action_log_probs"][:, :, 0]), bits(s["log_probs"][u])), u
    assert np.array_equal(bits(snap["returns_main"][:, :, 0]), bits(s["returns_main"][u])), u
    for name in ("returns", "value_preds", "masks", "bad_masks"):
        assert np.array_equal(bits(snap[name][:, :, 0]), bits(s[name][u])), (name, u)
    assert np.array_equal(bits(snap["value_preds"][:T, :, 0]), bits(s["values"][u])) and \
        np.array_equal(bits(snap["value_preds"][T, :, 0]), bits(s["next_value"][u]))
    for t in (range(T) if small_rows is None else small_rows):
        for name in ("done", "counter", "ratio"):
            np.testing.assert_array_equal(snap[name][t], g[name][k0 + t], err_msg="%s u=%d t=%d" % (name, u, t))
