"""Shared pieces of tests/test_search_native_policy.py: the three searches (ReorderSearch, MCTSearch, MultiBinPacker) under
bpp_policy_forward itself, judged forward by forward.  A plain helper module.

Trajectories under a real-valued network cannot be compared (one flipped near-tie changes everything after it), so every forward
inside a decision is judged given its own input, and a replay proves that the search consumed exactly those outputs:

  Recorder   a policy wrapper that keeps, per call inside decide(), a clone of obs and of the three outputs (MCTSearch and
             ReorderSearch reuse one obs buffer across levels).  It never synchronises.
  Tape       a policy that returns the recorded outputs in order and ORs (obs != recorded obs).any() into one flag, read once
             at the end.
  ExactNet   an integer network (policy_cases._sparse_layer) whose last Linear of each head is scaled by a power of two, and its
             int64 numpy forward; float32 is exact on it in any summation order (the bound is asserted on the judged rows).
  judge_exact / judge_real / judge_alone   the three judges.

Both tiers run the same code on torch tensors: the emulated one's live on the host, the device one's on the device."""
import numpy as np
import torch

import policy_cases as pc
from bpp_amd import policy as pol

HEADS = pc.HEADS
LAST = {"value": "base.critic_linear", "logits": "dist.linear", "pred": "base.mask.5"}      # the last Linear of each head
EVERY = 8            # every EVERY-th call is judged on all of its rows, and lends its sampled rows to judge_alone
ONE_SIGN = ("base.critic_linear",)   # one output per row and no ReLU after it: pc.exact_case asks no sign of it either
MIN_REAL_ROWS = 16   # judge_real pools at least this many rows (policy_cases.synthetic_states: on fewer the yardstick is luck)

# The exact networks of the tests: geometry -> (seed, {head: s}); the last Linear of head h is multiplied by 2^-s.  Unscaled, the
# values are integers of a few hundred, the logits of a row spread over several thousand (a one-hot softmax) and the positive mask
# predictions lie around 500 .. 1000: the shifts bring the logits to a spread of a few units, the values to a few rewards (a
# step's reward is at most 10) and the mask prediction to both sides of its 0.5 threshold, so that the searches have something to
# decide.  One seed per geometry serves all three searches.  The device geometry's seed is one under which the int64 forward
# alone meets the conditions of test_search_native_policy.check_conditions at the device shapes -- most seeds give a reorder
# search that never leaves the greedy baseline; test_conditions_hold_for_the_int64_forward_alone guards the choice.  The emulated
# geometry has no conditions to meet (they are asserted on the device shapes).
EXACT = {(5, 32, 25): (22, {"value": 8, "logits": 9, "pred": 10}),
         (10, 256, 100): (43, {"value": 6, "logits": 10, "pred": 11})}


def _is_t(x):
    return torch.is_tensor(x)


def _dup(x):
    if x is None:
        return None
    return x.clone() if _is_t(x) else np.array(x)


def to_numpy(x):
    return x.detach().cpu().numpy() if _is_t(x) else np.asarray(x)


# ------------------------------------------------------------------------------------------------------- recorder and tape
class Recorder(object):
    """policy -> the same policy; `calls` holds (obs clone, (value, logits, pred) clones) per call, in call order."""

    def __init__(self, policy):
        self.policy, self.calls = policy, []

    def __call__(self, obs):
        out = tuple(self.policy(obs))
        self.calls.append((_dup(obs), tuple(_dup(t) for t in out)))
        return out


class Tape(object):
    """Replays the outputs of Recorder.calls in order.  mismatch(): whether any call's obs differed from the recorded one, read
    once; a call beyond the tape, or of another shape, raises."""

    def __init__(self, calls):
        self.calls, self.at = calls, 0
        first = calls[0][0]
        self.flag = torch.zeros((), dtype=torch.bool, device=first.device) if _is_t(first) else np.zeros((), bool)

    def __call__(self, obs):
        want, out = self.calls[self.at]
        self.at += 1
        assert tuple(obs.shape) == tuple(want.shape), (self.at - 1, tuple(obs.shape), tuple(want.shape))
        self.flag |= (obs != want).any()
        return out

    def mismatch(self):
        assert self.at == len(self.calls), "the replay made %d calls, the recording %d" % (self.at, len(self.calls))
        return bool(self.flag)


def host_policy(L, geom, blob):
    """policy(obs numpy [n, 4 A]) -> (value, logits, pred) numpy through bpp_policy_forward of library L with host pointers."""
    run = pc.host_runner(L)

    def policy(obs):
        got = run(obs, geom, blob)
        return tuple(got[h] for h in HEADS)
    return policy


# ----------------------------------------------------------------------------------------------------------- the exact network
class ExactNet(object):
    """pc._sparse_layer weights for every layer of geometry (S, H, M): at most 4 integer taps of magnitudes summing to 5 per output
    channel, bias magnitudes at most 3.  For inputs bounded by m0 every partial sum through the eight layers from the observation
    to a head's output is at most 5^8 m0 + 3 (5^8 - 1) / 4: 4.2 M at m0 = 10 and 8.1 M at m0 = 20, below 2^24, so float32 is exact
    in any order on every observation of a 10 x 10 x 10 or 20 x 20 x 10 bin.  forward() does not rely on that estimate: it carries
    the bound `mag` on every partial sum of the rows it is given, as pc.exact_case does.

    The last Linear of head h (LAST) is multiplied by 2^-shifts[h], weights and bias: an exponent shift, exact in float32 as long
    as nothing underflows, and the int64 result is multiplied by the same factor."""

    def __init__(self, S, H, M, seed, shifts):
        self.geom, self.shifts = (S, H, M), dict(shifts)
        rng = np.random.RandomState(seed)
        self.w = {}
        for name, shape in pol.layer_shapes(S, H, M):
            self.w[name + ".weight"], self.w[name + ".bias"] = pc._sparse_layer(rng, shape)
        self.plain = {k: torch.from_numpy(v.astype(np.float32)) for k, v in self.w.items()}
        for h, name in LAST.items():
            for suffix in (".weight", ".bias"):
                self.plain[name + suffix] = self.plain[name + suffix] * float(2.0 ** -self.shifts[h])
        self.blob = pol.pack_weights(self.plain, S, H, M).numpy()
        # every layer as four gathers: tap t of output channel o reads flat input index gather[name][t][o, ...] with weight
        # value[name][t][o] (an int64 matrix product has no BLAS behind it in numpy, and 256 strided slices per layer are slow)
        A, PW = S * S, S + 2
        yx = (np.arange(S)[:, None] * PW + np.arange(S)[None]).reshape(1, A)              # a 3 x 3 layer reads the padded image
        self.gather, self.value = {}, {}
        for name, shape in pol.layer_shapes(S, H, M):
            w = self.w[name + ".weight"].reshape(shape[0], -1)
            k = np.argsort(w == 0, axis=1, kind="stable")[:, :4]                          # the nonzero taps first
            self.value[name] = [np.take_along_axis(w, k[:, t:t + 1], 1) for t in range(k.shape[1])]
            if len(shape) == 2:
                self.gather[name] = [k[:, t] for t in range(k.shape[1])]
            elif shape[2] == 3:                                                           # k = c * 9 + i * 3 + j
                self.gather[name] = [(k[:, t] // 9 * PW * PW + k[:, t] % 9 // 3 * PW + k[:, t] % 3)[:, None] + yx for t in range(k.shape[1])]
            else:
                self.gather[name] = [k[:, t:t + 1] * A + np.arange(A)[None] for t in range(k.shape[1])]

    def _layer(self, x, name):
        """(pre-activation, bound on every partial sum) of layer `name` on the flat input x [n, K]: [n, OC] or [n, OC, A]."""
        idx, val = self.gather[name], self.value[name]
        b = self.w[name + ".bias"]
        shape = (1, b.shape[0]) + (1,) * (idx[0].ndim - 1)
        out = np.broadcast_to(b.reshape(shape), (x.shape[0],) + idx[0].shape).copy()
        mag = np.abs(out)
        ax = np.abs(x)
        for i, v in zip(idx, val):
            v = v.reshape(shape)
            out += v * x[:, i]
            mag += np.abs(v) * ax[:, i]
        return out, mag

    def _conv3(self, x, name):
        n, S = x.shape[0], self.geom[0]
        xp = np.pad(x.reshape(n, -1, S, S), ((0, 0), (0, 0), (1, 1), (1, 1)))
        return self._layer(xp.reshape(n, -1), name)

    def forward(self, obs, signs=None):
        """obs float32 [n, >= 4 A] holding integers -> {head: float32 [n] / [n, M]} of the int64 forward.  Asserts that every
        partial sum stays below 2^24; signs: a dict that collects, per layer, whether a positive and a negative pre-activation
        were seen on these rows."""
        S, H, M = self.geom
        A = S * S
        obs = np.asarray(obs)
        n = obs.shape[0]
        img = obs[:, :4 * A].astype(np.int64)
        assert np.array_equal(img.astype(np.float32), obs[:, :4 * A]), "the observation rows must hold integers"

        def checked(pre, mag, name):
            assert mag.max() < 2 ** 24, (name, int(mag.max()))
            if signs is not None:
                s = signs.setdefault(name, [False, False])
                s[0], s[1] = s[0] or bool((pre > 0).any()), s[1] or bool((pre < 0).any())
            return pre

        x = img
        for name in pol.TRUNK:
            x = np.maximum(checked(*self._conv3(x, name), name), 0)

        def head(name):
            h = np.maximum(checked(*self._layer(x.reshape(n, -1), name + ".0"), name + ".0"), 0).reshape(n, -1)
            return np.maximum(checked(*self._layer(h, name + ".3"), name + ".3"), 0)

        value = checked(*self._layer(head("base.critic"), "base.critic_linear"), "base.critic_linear").reshape(n)
        logits = checked(*self._layer(head("base.actor"), "dist.linear"), "dist.linear")
        pred = np.maximum(checked(*self._layer(head("base.mask"), "base.mask.5"), "base.mask.5"), 0)
        out = {}
        for h, v in (("value", value), ("logits", logits), ("pred", pred)):
            scaled = v.astype(np.float64) * 2.0 ** -self.shifts[h]
            out[h] = scaled.astype(np.float32)
            assert np.array_equal(out[h].astype(np.float64), scaled), (h, "the shift underflows float32")
        return out

    def policy_np(self):
        """The int64 forward as a host policy (no policy kernel involved): what the conditions are checked under."""
        def policy(obs):
            got = self.forward(obs)
            return tuple(np.ascontiguousarray(got[h]) for h in HEADS)
        return policy


def exact_net(geom):
    seed, shifts = EXACT[tuple(geom)]
    return ExactNet(*geom, seed, shifts)


# -------------------------------------------------------------------------------------------------------------------- judges
def sample_rows(n, P, T):
    """Rows 0, P - 1, P, T - 1, T, n - 1 of a call of n rows (those that exist): both ends of the first trunk workgroup and of the
    first head tile, the first row of the next ones, and the last row."""
    return sorted({r for r in (0, P - 1, P, T - 1, T, n - 1) if 0 <= r < n})


def host_calls(calls):
    """Recorder.calls as numpy, one device-to-host copy per tensor (after one synchronisation by the first)."""
    return [(to_numpy(o), tuple(None if t is None else to_numpy(t) for t in out)) for o, out in calls]


def judged_rows(n, c, P, T, all_rows):
    return list(range(n)) if all_rows or c % EVERY == 0 else sample_rows(n, P, T)


def judge_exact(net, calls, P, T, all_rows=False):
    """Every recorded output bit-equal to the int64 forward of its recorded obs: every row of every EVERY-th call and
    sample_rows of every other (all_rows: every row of every call).  Both signs of pre-activation at every layer over the judged
    rows.  calls: host_calls().  Returns the number of rows judged."""
    signs, rows = {}, 0
    for c, (obs, out) in enumerate(calls):
        pick = judged_rows(obs.shape[0], c, P, T, all_rows)
        want = net.forward(obs[pick], signs)
        for h, got in zip(HEADS, out):
            assert got is not None, (c, h)
            got = got.reshape(obs.shape[0], -1)[pick].reshape(want[h].shape)
            assert pc.same_bits(got, want[h]), ("call %d" % c, h, pick, np.abs(got.astype(np.float64) - want[h]).max())
        rows += len(pick)
    for name, (pos, neg) in sorted(signs.items()):                 # exact_case's own assertion, which leaves the same layer out
        assert (pos and neg) or name in ONE_SIGN, "%s: pre-activations of one sign only on the recorded rows" % name
    assert len(signs) == len(pol.layer_shapes(*net.geom)), sorted(signs)
    return rows


def alone_rows(calls, P, T):
    """[(call, row)]: sample_rows of every EVERY-th call."""
    return [(c, r) for c in range(0, len(calls), EVERY) for r in sample_rows(calls[c][0].shape[0], P, T)]


def judge_alone(policy, calls, P, T):
    """Each sampled row, evaluated by `policy` as a batch of one, gives the bits it had inside its batch (include/bpp_policy.h:
    a bin's outputs are the same bits whatever batch it is evaluated in).  calls: Recorder.calls as recorded (the rows go back to
    the policy as they are).  Returns the number of rows."""
    picks = alone_rows(calls, P, T)
    pairs = []
    for c, r in picks:
        obs, out = calls[c]
        pairs.append((c, r, tuple(_dup(t) for t in policy(obs[r:r + 1])), out))
    for c, r, one, out in pairs:
        for h, a, b in zip(HEADS, one, out):
            a, b = to_numpy(a).reshape(-1), to_numpy(b).reshape(out[1].shape[0], -1)[r]
            assert pc.same_bits(a, b), ("call %d row %d alone" % (c, r), h)
    return len(picks)


def judge_real(plain, geom, calls, P, T, label):
    """pc.check_real's rule per head, e_native <= pc.FACTOR * e_torch32, both against the float64 torch_forward, pooled over
    sample_rows of every EVERY-th call (at least MIN_REAL_ROWS rows, else over more calls).  calls: host_calls().  Prints and
    returns the figures."""
    every = EVERY
    while True:
        picks = [(c, r) for c in range(0, len(calls), every) for r in sample_rows(calls[c][0].shape[0], P, T)]
        if len(picks) >= MIN_REAL_ROWS or every == 1:
            break
        every //= 2
    assert len(picks) >= MIN_REAL_ROWS, len(picks)
    S = geom[0]
    obs = np.stack([calls[c][0][r][:4 * S * S] for c, r in picks]).astype(np.float32)
    got = {h: np.stack([calls[c][1][i].reshape(calls[c][0].shape[0], -1)[r] for c, r in picks]) for i, h in enumerate(HEADS)}
    got["value"] = got["value"].reshape(-1)
    with torch.no_grad():
        ref64 = pol.torch_forward({k: v.double() for k, v in plain.items()}, torch.from_numpy(obs).double())
        ref32 = pol.torch_forward(plain, torch.from_numpy(obs))
    return pc.check_real(got, {h: t.numpy() for h, t in zip(HEADS, ref64)}, {h: t.numpy() for h, t in zip(HEADS, ref32)},
                         "%s, %d rows:" % (label, len(picks)))


def same_decisions(a, b, what):
    """Two lists of decision tuples (tensors or arrays), bit for bit."""
    assert len(a) == len(b), what
    for t, (x, y) in enumerate(zip(a, b)):
        for j, (u, v) in enumerate(zip(x, y)):
            u, v = to_numpy(u), to_numpy(v)
            assert u.dtype == v.dtype and u.tobytes() == v.tobytes(), "%s: decision %d, output %d differs" % (what, t, j)
