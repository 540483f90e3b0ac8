"""Inputs and float64 restatements shared by the real-valued-policy tests of the search kernels
(test_reorder_real_policy.py, test_multibin_real_policy.py, test_mcts_real_policy.py).  A plain helper module.

Logit rows come from the policy-head test's families (tests/test_policy_head_f64.py: family()), placed on a given
feasibility mask, plus two families of their own:
  underflow   the row maximum sits on an infeasible cell and every feasible logit lies 88 .. 104 below it, where float32
              exp(x - max) is a denormal or zero;
  minus_inf   -inf on a third of the cells (never on all of them).
Values are full 24-bit-mantissa float32 in [-1, 1) from an integer hash, the same bits in numpy and torch."""
import numpy as np

from test_policy_head_f64 import SHIFTS, family

GAP = 1e-5        # logit gap above which exp(x - max) orders two cells for certain: an expf good to 2 ulp on a difference
                  # rounded to half an ulp blurs at most (80 + 2) * 2^-23 < 1e-5 relative at |x - max| <= 80
FAR = 80.0        # beyond this distance from the row maximum float32 softmax values are judged by the float32 restatement
HEAD_FAMILIES = ["mild", "shifted", "wide30", "wide100", "tie_all", "tie_half", "near_tie", "one_feasible_80",
                 "none_feasible", "all_feasible"]
OWN_FAMILIES = ["underflow", "minus_inf"]
# families whose rows need not be decided by the float64 rule: 98 % of the rows of every other family must be
UNCAPPED = ("near_tie", "none_feasible", "wide100", "underflow")
CAP = 0.98


def hashed(s):
    """((s * 2654435761) mod 2^24) / 2^23 - 1 as float32, exact: every 24-bit mantissa in [-1, 1)."""
    s = np.asarray(s, dtype=np.uint64)
    return (((s * np.uint64(2654435761)) % np.uint64(1 << 24)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)


def hashed_values(n, seed):
    return hashed(np.arange(n, dtype=np.uint64) * np.uint64(7919) + np.uint64(seed * 104729 + 1))


def place(name, mask, seed, own_mask):
    """(logits float32 [n, A], feasible bool [n, A]) of family `name` over the feasibility rows `mask` (bool [n, A]).
    own_mask: the caller hands the returned mask to the kernel (reorder's pred), so families that need a particular mask
    get it; otherwise the kernel builds the mask itself and the family adapts to it."""
    n, A = mask.shape
    rng = np.random.RandomState(seed + 977)
    m = mask.copy()
    rows = np.arange(n)
    if name in ("mild", "shifted", "wide30", "wide100", "tie_all", "tie_half"):
        x = family(name, n, A, seed)[0]
        if name == "tie_all" and own_mask:
            m[::3] = True
    elif name == "near_tie":                   # the two largest feasible logits 1 .. 4 ulp apart
        x = (rng.randn(n, A) * 2.0).astype(np.float32)
        for e in range(n):
            cells = np.arange(A) if own_mask else np.flatnonzero(m[e])
            if cells.size < 2:
                continue
            i, j = rng.choice(cells, 2, replace=False)
            m[e, i] = m[e, j] = True
            x[e, i] = np.float32(9.0 + rng.rand())
            x[e, j] = x[e, i]
            for _ in range(rng.randint(1, 5)):
                x[e, j] = np.nextafter(x[e, j], np.float32(0.0))
    elif name == "one_feasible_80":            # one feasible cell 80 above the rest (own_mask: the only feasible one)
        x = (rng.randn(n, A) * 2.0).astype(np.float32)
        for e in range(n):
            cells = np.flatnonzero(m[e])
            j = rng.choice(cells) if cells.size else rng.randint(A)
            if own_mask:
                m[e] = False
                m[e, j] = True
            x[e, j] = 80.0
    elif name == "none_feasible":
        assert own_mask
        x, m = (rng.randn(n, A) * 2.0).astype(np.float32), np.zeros((n, A), bool)
    elif name == "all_feasible":
        assert own_mask
        x, m = (rng.randn(n, A) * 2.0).astype(np.float32), np.ones((n, A), bool)
    elif name == "underflow":
        x = (rng.randn(n, A) * 2.0).astype(np.float32)
        for e in range(n):
            if own_mask and m[e].all():
                m[e, rng.randint(A)] = False
            bad = np.flatnonzero(~m[e])
            if bad.size == 0:
                continue                       # nothing infeasible to carry the maximum: the row stays mild
            x[e, bad[rng.randint(bad.size)]] = 100.0
            f = np.flatnonzero(m[e])
            x[e, f] = (100.0 - (88.0 + 16.0 * rng.rand(f.size))).astype(np.float32)
    elif name == "minus_inf":
        x = (rng.randn(n, A) * 2.0).astype(np.float32)
        inf = (np.arange(A)[None] + rows[:, None]) % 3 == 0
        keep = (m & ~inf).any(1) | ~m.any(1)   # a row whose feasible cells would all be -inf keeps its first one finite
        inf[rows[~keep], m[~keep].argmax(1)] = False
        x[inf] = -np.inf
        if A < 2:
            x[:] = 0.0
    else:
        raise ValueError(name)
    return np.ascontiguousarray(x, np.float32), m


def labels(own_mask):
    """Family labels in launch order; the shifted family once unshifted and once per exact shift."""
    out = []
    for name in HEAD_FAMILIES + OWN_FAMILIES:
        if not own_mask and name in ("none_feasible", "all_feasible"):
            continue
        out.append(name)
        if name == "shifted":
            out += ["shifted%+d" % c for c in SHIFTS]
    return out


def rows_of(label, mask, seed, own_mask):
    """place() for a label of labels(): 'shifted+200' is the shifted family's rows + 200 (exact in float32)."""
    if label.startswith("shifted") and label != "shifted":
        x, m = place("shifted", mask, seed, own_mask)
        return x + np.float32(int(label[7:])), m
    return place(label, mask, seed, own_mask)


def base_family(label):
    return "shifted" if label.startswith("shifted") else label


# ------------------------------------------------------------------------------------------- the position choice
def softmax32(x):
    """numpy float32 softmax with denormals kept: what the reference's float32 softmax on the CPU computes."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", under="ignore"):
        e = np.exp((x - x.max(-1, keepdims=True)).astype(np.float32)).astype(np.float32)
        return (e / e.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)


def judge_choice(x, m, a, last, what):
    """The cell `a` [n] a kernel chose as argmax of softmax(x) * m against the float64 rule: the feasible cell with the
    largest logit, the first such cell (last: the last one).  Asserts on every row; returns which rows were decided.

    decided   a feasible cell exists, the best feasible logit is within FAR of the row maximum, and the two best feasible
              logits are bit-equal or more than GAP apart: the action must be equal;
    near tie  (two best feasible logits within GAP): the chosen cell is feasible, its logit within GAP of the best;
    far       (best feasible logit more than FAR below the maximum): judged by softmax32 -- where its two best masked
              probabilities differ by more than 4 ulp of the larger the action must be equal, otherwise the chosen cell
              must lie in its tied set (every cell, when every masked probability is 0);
    a row without a feasible cell gives 0 (last: A - 1)."""
    n, A = x.shape
    xd = x.astype(np.float64)
    decided = np.zeros(n, bool)
    zero_rule = A - 1 if last else 0
    for e in range(n):
        f = np.flatnonzero(m[e])
        where = "%s row %d (last=%d)" % (what, e, last)
        assert 0 <= a[e] < A, where
        if f.size == 0:
            assert a[e] == zero_rule, (where, "no feasible cell", int(a[e]))
            continue
        xf = xd[e, f]
        best = xf.max()
        if not best >= xd[e].max() - FAR:      # far rows, and rows whose feasible cells all hold -inf
            p = softmax32(x[e]) * m[e]
            top = np.sort(p)[-2:] if A > 1 else np.array([0.0, p[0]], np.float32)
            tol = 4.0 * float(np.spacing(np.float32(top[1])))
            tied = np.flatnonzero(p >= top[1] - tol)
            if float(top[1]) - float(top[0]) > tol:
                assert a[e] == tied[0], (where, "far row", int(a[e]), int(tied[0]))
            else:
                assert a[e] in tied, (where, "far row, tied set", int(a[e]), tied[:8])
            continue
        order = np.sort(xf)
        second = order[-2] if f.size > 1 else -np.inf
        eq = f[xf == best]
        want = eq[-1] if last else eq[0]
        if best == second or best - second > GAP:
            decided[e] = True
            assert a[e] == want, (where, "decided row", int(a[e]), int(want), best, second)
        else:
            assert m[e, a[e]] and xd[e, a[e]] >= best - GAP, (where, "near tie", int(a[e]), int(want))
    return decided


def check_cap(decided, what):
    """decided: {label: [bool array of one launch, ...]}.  Over the pooled rows of all its launches, every family outside
    UNCAPPED has >= CAP of its rows decided."""
    for label, v in sorted(decided.items()):
        rows = np.concatenate(v)
        s = float(rows.mean())
        print("%s: %-16s decided %.4f of %d rows" % (what, label, s, rows.size))
        if base_family(label) not in UNCAPPED:
            assert s >= CAP, (what, label, s)
