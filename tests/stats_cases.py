"""Cases and normative statements shared by tests/test_stats_kernels.py (oracle library, emulated kernels) and
tests/test_gpu_stats_kernels.py (the device): the episode statistics (bpp_episode_stats, bpp_episode_acc_reduce) and the ordered
compaction of a step's finished bins (bpp_gather_finished).  No device, no oracle, nothing of the reference: what a result has to
be is written here in plain numpy float64 from the text of include/bpp_abi.h, and every comparison is either bit-exact against
that order or the derived bound against math.fsum -- no tolerance here is a measured number."""
import functools
import math

import numpy as np

REDUCE_LANES = 1024                                   # BPP_REDUCE_LANES
SCRATCH_DOUBLES = (REDUCE_LANES * 4 * 8 + 64) // 8    # BPP_REDUCE_SCRATCH_BYTES; the arrival word is the first behind the partials
ENQUEUE_ONLY = -1                                     # BPP_GATHER_ENQUEUE_ONLY
ACC0 = (1.5, -2.0, 0.25, 7.0)
GUARD_ROWS, GUARD = 64, -12345.678                    # rows behind row E no reduction may touch
SENTINEL = 0xA5                                       # every byte of an output buffer before a gather

# 8 192 +- 1: the one-workgroup kernel's 8-row unrolled body; 65 536 +- 1: the wide kernel's outer step; 132 101 = 2 * 65 536 + 1 029:
# a third, ragged outer step
REDUCE_SIZES = [1, 15, 16, 17, 1023, 1024, 1025, 8191, 8192, 8193, 16387, 65535, 65536, 65537, 132101]
# 262 144: the last size with 64 chunks of 4 096 bins; 262 145: the first with 8 192-bin chunks (two rounds per workgroup)
GATHER_SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 8197, 65536, 65537, 262144, 262145, 300007]
DONE_SHIFTS = [0, 1, 8, 15]                           # bytes past a 16-byte boundary
DONE_PATTERNS = ["none", "all", "p10", "last", "first_of_chunk", "last_of_chunk"]
DONE_VALUES = (1, 2, 0x7f, 0x80, 0xff)                # the carry edges of counting nonzero bytes a word at a time
REDUCE_KINDS = ("awkward", "cancel")


def bits(a):
    """float64 values as their bit patterns: -0.0 is not +0.0 here"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def finished_bytes(n):
    """BPP_FINISHED_BYTES(n)"""
    return 32 + 28 * int(n) + 4


def finished_room(E):
    """bytes of a buffer for BPP_FINISHED_BYTES(E), a whole number of float64"""
    return (finished_bytes(E) + 7) // 8 * 8


# ---------------------------------------------------------------------------------------------------- normative statements
def normative_sums(rows, acc0):
    """include/bpp_abi.h, bpp_episode_acc_reduce: 1 024 partial sums, partial r = rows r, r + 1024, r + 2048, ... added in
    ascending order to +0.0; then for d = 512, 256, ..., 1: partial[r] += partial[r + d] for r < d; finally acc + partial[0]."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    part = np.zeros((REDUCE_LANES, 4), np.float64)
    for first in range(0, rows.shape[0], REDUCE_LANES):
        blk = rows[first:first + REDUCE_LANES]
        part[:blk.shape[0]] += blk
    d = REDUCE_LANES // 2
    while d >= 1:
        part[:d] += part[d:2 * d]
        d //= 2
    return np.asarray(acc0, dtype=np.float64) + part[0]


def normative_stats(done, ep_ret, ratio, ep_len, acc0):
    """include/bpp_abi.h, bpp_episode_stats: the same order over the contributions (ep_ret, ratio, float(ep_len), 1.0) of the bins
    with done != 0; a bin that is not done contributes nothing."""
    contrib = np.stack([np.asarray(ep_ret, np.float64), np.asarray(ratio, np.float64), np.asarray(ep_len).astype(np.float64),
                        np.ones(len(done), np.float64)], axis=1)
    fin = np.asarray(done) != 0
    part = np.zeros((REDUCE_LANES, 4), np.float64)
    for first in range(0, len(done), REDUCE_LANES):
        r = np.flatnonzero(fin[first:first + REDUCE_LANES])
        part[r] += contrib[first + r]
    d = REDUCE_LANES // 2
    while d >= 1:
        part[:d] += part[d:2 * d]
        d //= 2
    return np.asarray(acc0, dtype=np.float64) + part[0]


def normative_gather(done, ep_ret, ratio, ep_len, counter):
    """include/bpp_abi.h, bpp_gather_finished: the bins with done != 0 in ascending order and their four outputs."""
    idx = np.flatnonzero(np.asarray(done))
    return dict(ep_ret=ep_ret[idx], ratio=ratio[idx], ep_len=ep_len[idx], counter=counter[idx], bin=idx.astype(np.int32))


def fsum_columns(rows, acc0):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    return np.array([math.fsum(rows[:, k].tolist() + [float(acc0[k])]) for k in range(4)])


def exact_bound(rows, acc0, E):
    """Per component, the distance a sum in ANY order of this depth may have from math.fsum: L u (sum |x| + |acc0|) / (1 - L u)
    with u = 2^-53 and L = ceil(E / 1024) + 11 -- a row passes through at most ceil(E / 1024) additions of its chain, ten tree
    levels and the final one, and the textbook bound for a value that passes through L roundings is gamma_L = L u / (1 - L u).
    (A chain's first addition is to +0.0 and exact, so one of the L roundings does not happen: that one pays for fsum's own
    rounding of the exact sum, u |sum| <= u sum |x|.)  Gradual underflow costs nothing: an addition that lands in the subnormal
    range is exact.  Derived, not measured."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    u, L = 2.0 ** -53, (int(E) + REDUCE_LANES - 1) // REDUCE_LANES + 11
    mag = np.array([math.fsum(np.abs(rows[:, k]).tolist() + [abs(float(acc0[k]))]) for k in range(4)])
    return L * u * mag / (1.0 - L * u)


# ---------------------------------------------------------------------------------------------------- data, fixed seeds
def awkward_rows(E, seed, width=4):
    """rand * 10 ** randint(-6, 7) * +-1: magnitudes over thirteen decades, both signs"""
    rng = np.random.RandomState(seed)
    shape = (int(E), width) if width else (int(E),)
    return rng.rand(*shape) * 10.0 ** rng.randint(-6, 7, size=shape) * rng.choice([-1.0, 1.0], size=shape)


def cancelling_rows(E, seed):
    """x in the rows of the even blocks of 1 024, -x in the row 1 024 further on: the two meet as neighbours in one chain and the
    partial returns to what it was -- or not quite, which is what the order decides.  A few -0.0 and subnormal entries on top
    (finite values only)."""
    rows = awkward_rows(E, seed)
    odd = np.flatnonzero(np.arange(int(E)) // REDUCE_LANES % 2 == 1)
    rows[odd] = -rows[odd - REDUCE_LANES]
    rng = np.random.RandomState(seed + 1000)
    k = max(1, int(E) // 97)
    rows[rng.randint(0, E, k), rng.randint(0, 4, k)] = -0.0
    rows[rng.randint(0, E, k), rng.randint(0, 4, k)] = 5e-324 * rng.randint(1, 1 << 20, k)
    rows[rng.randint(0, E, k), rng.randint(0, 4, k)] = -2.2250738585072014e-308 * rng.rand(k)
    assert np.isfinite(rows).all()
    return rows


def done_bytes(E, pattern, seed):
    """`done` of E bins: which bins finished by `pattern`, every nonzero byte drawn from DONE_VALUES"""
    rng = np.random.RandomState(seed)
    fin = np.zeros(int(E), bool)
    if pattern == "all":
        fin[:] = True
    elif pattern == "p10":
        fin = rng.rand(int(E)) < 0.1
    elif pattern == "last":
        fin[-1] = True
    elif pattern == "first_of_chunk":
        fin[::4096] = True
    elif pattern == "last_of_chunk":
        fin[4095::4096] = True
    else:
        assert pattern == "none", pattern
    return np.where(fin, rng.choice(np.array(DONE_VALUES, np.uint8), size=int(E)), 0).astype(np.uint8)


def frozen(a):
    a.flags.writeable = False
    return a


class ReduceCase(object):
    """rows [E, 4] (read-only) and, computed once, what bpp_episode_acc_reduce has to leave in acc when it starts from ACC0"""

    def __init__(self, E, kind, seed=5):
        self.E, self.kind = int(E), kind
        self.rows = frozen(awkward_rows(E, seed) if kind == "awkward" else cancelling_rows(E, seed))
        self.acc0 = np.array(ACC0)
        self.want = frozen(normative_sums(self.rows, self.acc0))
        self.fsum = fsum_columns(self.rows, self.acc0)
        self.bound = exact_bound(self.rows, self.acc0, E)

    def check(self, label, clear, acc, rows_after, guard_after, arrival_word):
        """acc after the call, the E rows and the GUARD_ROWS rows behind them as the call left them, the scratch buffer's arrival
        word (None: a call without a scratch buffer)"""
        label = "%s E=%d %s clear=%d" % (label, self.E, self.kind, clear)
        acc = np.asarray(acc, dtype=np.float64)
        assert bits(acc).tolist() == bits(self.want).tolist(), "%s: acc %r is not the header's order %r" % (label, acc.tolist(), self.want.tolist())
        err = np.abs(acc - self.fsum)
        assert np.all(err <= self.bound), "%s: %r from fsum, bound %r" % (label, err.tolist(), self.bound.tolist())
        after = np.zeros_like(self.rows) if clear else self.rows
        assert np.array_equal(bits(rows_after).reshape(-1), bits(after).reshape(-1)), label + (": rows not zeroed" if clear else ": rows changed")
        assert np.all(np.asarray(guard_after) == GUARD), label + ": rows behind row E were written"
        assert arrival_word is None or int(arrival_word) == 0, label + ": arrival word %r" % (arrival_word,)


@functools.lru_cache(maxsize=None)
def reduce_case(E, kind="awkward", seed=5):
    return ReduceCase(E, kind, seed)


class StatsCase(object):
    """the four per-bin outputs bpp_episode_stats reads (ep_len up to 2^31 - 1), done by pattern p10, and its sums from ACC0"""

    def __init__(self, E, seed=7):
        self.E = int(E)
        rng = np.random.RandomState(seed)
        self.done = frozen(done_bytes(E, "p10", seed))
        self.ep_ret = frozen(awkward_rows(E, seed + 1, width=0))
        self.ratio = frozen(rng.rand(self.E))
        ln = rng.randint(0, 2 ** 31 - 1, size=self.E, dtype=np.int64)
        ln[rng.randint(0, self.E, max(1, self.E // 50))] = 2 ** 31 - 1
        self.ep_len = frozen(ln.astype(np.int32))
        self.acc0 = np.array(ACC0)
        self.want = frozen(normative_stats(self.done, self.ep_ret, self.ratio, self.ep_len, self.acc0))
        idx = np.flatnonzero(self.done)
        contrib = np.stack([self.ep_ret[idx], self.ratio[idx], self.ep_len[idx].astype(np.float64), np.ones(len(idx))], axis=1)
        self.fsum = fsum_columns(contrib, self.acc0)
        self.bound = exact_bound(contrib, self.acc0, E)

    def check(self, label, acc):
        label = "%s E=%d" % (label, self.E)
        acc = np.asarray(acc, dtype=np.float64)
        assert bits(acc).tolist() == bits(self.want).tolist(), "%s: acc %r is not the header's order %r" % (label, acc.tolist(), self.want.tolist())
        assert np.all(np.abs(acc - self.fsum) <= self.bound), label
        n = int(np.count_nonzero(self.done))
        total = int(self.ep_len[self.done != 0].astype(np.int64).sum())
        assert total < 2 ** 50                                  # integers and a quarter below 2^53: exact in any order
        assert acc[3] == self.acc0[3] + n and acc[2] == self.acc0[2] + total, label


@functools.lru_cache(maxsize=None)
def stats_case(E):
    return StatsCase(E)


class GatherFields(object):
    """the four per-bin arrays a gather reads, one set per size, shared by every pattern and alignment"""

    def __init__(self, E, seed=11):
        self.E = int(E)
        rng = np.random.RandomState(seed)
        self.ep_ret = frozen(awkward_rows(E, seed, width=0))
        self.ratio = frozen(rng.rand(self.E))
        self.ep_len = frozen(rng.randint(1, 2 ** 31 - 1, size=self.E, dtype=np.int64).astype(np.int32))
        self.counter = frozen(rng.randint(0, 1 << 20, size=self.E).astype(np.int32))


@functools.lru_cache(maxsize=None)
def gather_fields(E):
    return GatherFields(E)


class GatherCase(object):
    def __init__(self, E, pattern):
        self.E, self.pattern, self.f = int(E), pattern, gather_fields(E)
        self.done = frozen(done_bytes(E, pattern, 100 + DONE_PATTERNS.index(pattern)))
        self.want = normative_gather(self.done, self.f.ep_ret, self.f.ratio, self.f.ep_len, self.f.counter)
        self.n = len(self.want["bin"])

    def image(self, entries, nbytes):
        """The bytes of an output buffer of `nbytes` that held SENTINEL everywhere before the kernel wrote header and arrays into it
        itself (the direct form: entries = n; the eager form: entries = E): header = count and 28 zero bytes, the five arrays laid
        out for `entries` entries with their first n filled, every other byte untouched."""
        n = self.n
        img = np.full(nbytes, SENTINEL, np.uint8)
        img[:32] = 0
        img[:4] = np.array([n], "<i4").view(np.uint8)
        at = 32
        for name, width in (("ep_ret", 8), ("ratio", 8), ("ep_len", 4), ("counter", 4), ("bin", 4)):
            img[at:at + width * n] = np.ascontiguousarray(self.want[name]).view(np.uint8)
            at += width * entries
        return img

    def check_written(self, label, host, entries):
        """direct and eager forms: the whole buffer, byte for byte -- nothing beyond each array's first n entries has changed"""
        label = "%s E=%d %s" % (label, self.E, self.pattern)
        host = np.asarray(host)
        assert int(host[:4].view("<i4")[0]) == self.n, "%s: header count %d, finished bins %d" % (label, int(host[:4].view("<i4")[0]), self.n)
        bad = np.flatnonzero(host != self.image(entries, host.shape[0]))
        assert bad.size == 0, "%s: %d bytes differ, the first at %d (arrays start at 32, laid out for %d entries)" % (label, bad.size, bad[0], entries)

    def check_staged(self, label, host):
        """staged form: the first BPP_FINISHED_BYTES(n) bytes were copied (the last 4 of them are room, not data), nothing behind"""
        label = "%s E=%d %s" % (label, self.E, self.pattern)
        host = np.asarray(host)
        assert int(host[:4].view("<i4")[0]) == self.n, "%s: header count %d, finished bins %d" % (label, int(host[:4].view("<i4")[0]), self.n)
        used = 32 + 28 * self.n
        bad = np.flatnonzero(host[:used] != self.image(self.n, used))
        assert bad.size == 0, "%s: %d bytes differ, the first at %d" % (label, bad.size, bad[0])
        assert np.all(host[finished_bytes(self.n):] == SENTINEL), label + ": bytes behind BPP_FINISHED_BYTES(n) were copied"


@functools.lru_cache(maxsize=None)
def gather_case(E, pattern):
    return GatherCase(E, pattern)


def shifted(base_address, room, shift):
    """offset into a byte buffer at `base_address` that lies `shift` bytes past a 16-byte boundary (room: spare bytes, >= 31)"""
    off = (-int(base_address)) % 16 + shift
    assert off <= room and (int(base_address) + off) % 16 == shift
    return off
