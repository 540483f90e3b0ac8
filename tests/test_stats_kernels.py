"""bpp_episode_acc_reduce, bpp_episode_stats and bpp_gather_finished of the oracle library and of the product kernels on the host
emulator (csrc/bpp_stats.inl) against the plain numpy statements of tests/stats_cases.py, at the sizes where the kernels take
another path.  The emulator runs workgroups one after another: these tests see a wrong formula, not a wrong hand-off between
workgroups -- tests/test_gpu_stats_kernels.py runs the same cases on the device."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stats_cases as sc  # noqa: E402

VP, I32 = ctypes.c_void_p, ctypes.c_int32
FORMS = ["oracle", "emu_one", "emu_wide"]


def ptr(a):
    return VP(a.ctypes.data)


def library(form, oracle, emu):
    return oracle.lib() if form == "oracle" else emu.lib()


def aligned_rows(rows, align=32):
    """a copy of rows [E, 4] that starts on a 32-byte boundary, as the ABI asks, with GUARD_ROWS sentinel rows behind it"""
    E = rows.shape[0]
    buf = np.full((E + sc.GUARD_ROWS) * 4 + 4, sc.GUARD, np.float64)
    off = (-buf.ctypes.data % align) // 8
    all_rows = buf[off:off + 4 * (E + sc.GUARD_ROWS)].reshape(E + sc.GUARD_ROWS, 4)
    all_rows[:E] = rows
    return all_rows[:E], all_rows[E:]


def test_the_reduce_data_tells_the_headers_order_from_numpys():
    """The condition that keeps the bit-exact tests from passing vacuously: at every size from 1 023 rows on, the sums in the
    header's order differ in bits from rows.sum(0) + acc0 (numpy's pairwise order) in at least one of the four components -- a
    kernel that added in another order would be seen.  And the cancelling rows cancel: their sum is far below their magnitude."""
    for E in sc.REDUCE_SIZES:
        case = sc.reduce_case(E)
        other = case.rows.sum(0) + case.acc0
        differing = int(np.count_nonzero(sc.bits(case.want) != sc.bits(other)))
        print("E=%d: the header's order and numpy's differ in %d of 4 components" % (E, differing))
        assert np.all(np.abs(other - case.fsum) <= case.bound)          # numpy's order is a summation of this depth too
        if E >= 1023:
            assert differing >= 1, E
        if E >= 2048:
            cancel = sc.reduce_case(E, "cancel")
            assert np.all(np.abs(cancel.fsum - cancel.acc0) < 0.1 * np.abs(cancel.rows).sum(0))
            assert np.signbit(cancel.rows[cancel.rows == 0.0]).any() and (np.abs(cancel.rows[cancel.rows != 0.0]) < 2.3e-308).any()
    for pattern in sc.DONE_PATTERNS[1:]:
        if pattern in ("all", "last", "first_of_chunk"):
            assert sc.gather_case(sc.GATHER_SIZES[0], pattern).n == 1
        seen = set(np.unique(sc.gather_case(300007, pattern).done).tolist())
        assert seen <= set(sc.DONE_VALUES) | {0} and (pattern in ("last", "none") or seen >= set(sc.DONE_VALUES))
    assert sc.gather_case(262145, "first_of_chunk").n == 65 and sc.gather_case(262145, "last_of_chunk").n == 64


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("clear", [0, 1])
@pytest.mark.parametrize("E", sc.REDUCE_SIZES)
def test_acc_reduce_gives_the_headers_bits(oracle, emu, E, clear, form):
    """bpp_episode_acc_reduce from ACC0: the normative bits, within the derived bound of fsum, rows zeroed (clear) or untouched, the
    64 rows behind row E untouched, the scratch buffer's arrival word zero again -- awkward and cancelling rows, one scratch buffer
    for both calls."""
    lib = library(form, oracle, emu)
    scratch = np.zeros(sc.SCRATCH_DOUBLES, np.float64)
    for kind in sc.REDUCE_KINDS:
        case = sc.reduce_case(E, kind)
        rows, guard = aligned_rows(case.rows)
        acc = case.acc0.copy()
        rc = lib.bpp_episode_acc_reduce(ptr(rows), I32(E), ptr(acc), I32(clear), ptr(scratch) if form == "emu_wide" else None, None)
        assert rc == 0, lib.bpp_last_error()
        case.check(form, clear, acc, rows, guard, scratch[4 * sc.REDUCE_LANES:].view(np.uint32)[0])
    assert not scratch[4 * sc.REDUCE_LANES:].any()


@pytest.mark.parametrize("form", ["oracle", "emu"])
@pytest.mark.parametrize("E", sc.REDUCE_SIZES)
def test_episode_stats_gives_the_headers_bits(oracle, emu, E, form):
    """bpp_episode_stats over a tenth of the bins, done bytes of every nonzero kind, ep_len up to 2^31 - 1."""
    lib = library(form, oracle, emu)
    case = sc.stats_case(E)
    acc = case.acc0.copy()
    rc = lib.bpp_episode_stats(ptr(case.done), ptr(case.ep_ret), ptr(case.ratio), ptr(case.ep_len), I32(E), ptr(acc), None)
    assert rc == 0, lib.bpp_last_error()
    case.check(form, acc)


def gather(lib, case, done, dev, host, n):
    f = case.f
    return lib.bpp_gather_finished(ptr(done), ptr(f.ep_ret), ptr(f.ratio), ptr(f.ep_len), ptr(f.counter), I32(case.E),
                                   ptr(dev) if dev is not None else None, ptr(host), I32(n), None)


@pytest.mark.parametrize("form", ["oracle", "emu"])
@pytest.mark.parametrize("E", sc.GATHER_SIZES)
def test_gather_finished_compacts_in_bin_order(oracle, emu, E, form):
    """bpp_gather_finished at every pattern and every position of `done` past a 16-byte boundary: staged (through a second buffer),
    direct (dev = NULL) and eager (BPP_GATHER_ENQUEUE_ONLY) forms against np.flatnonzero; in the direct and eager forms no byte
    beyond each array's first n entries has changed.  A count of n +- 1 and a count beyond E are refused, and so is the eager form
    with a staging buffer."""
    lib = library(form, oracle, emu)
    lib.bpp_gather_finished.argtypes = None
    room = sc.finished_room(E)
    store = np.zeros(E + 64, np.uint8)
    dev, host = np.zeros(room // 8, np.float64).view(np.uint8), np.zeros(room // 8, np.float64).view(np.uint8)
    for pattern in sc.DONE_PATTERNS:
        case = sc.gather_case(E, pattern)
        n = case.n
        for shift in sc.DONE_SHIFTS:
            off = sc.shifted(store.ctypes.data, 63, shift)
            done = store[off:off + E]
            done[:] = case.done
            label = "%s shift %d" % (form, shift)
            dev[:], host[:] = sc.SENTINEL, sc.SENTINEL
            assert gather(lib, case, done, dev, host, n) == 0, lib.bpp_last_error()
            case.check_staged(label + " staged", host)
            host[:] = sc.SENTINEL
            assert gather(lib, case, done, None, host, n) == 0, lib.bpp_last_error()
            case.check_written(label + " direct", host, n)
            host[:] = sc.SENTINEL
            assert gather(lib, case, done, None, host, sc.ENQUEUE_ONLY) == 0, lib.bpp_last_error()
            case.check_written(label + " eager", host, E)
            assert np.array_equal(done, case.done)
        if n < E:
            assert gather(lib, case, done, dev, host, n + 1) != 0 and b"not the number of finished bins" in lib.bpp_last_error()
        if n > 0:
            assert gather(lib, case, done, None, host, n - 1) != 0 and b"not the number of finished bins" in lib.bpp_last_error()
        assert gather(lib, case, done, dev, host, E + 1) != 0 and b"bad size" in lib.bpp_last_error()
        assert gather(lib, case, done, dev, host, sc.ENQUEUE_ONLY) != 0 and b"dev must be NULL" in lib.bpp_last_error()
