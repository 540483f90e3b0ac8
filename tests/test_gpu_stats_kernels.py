"""The kernels of csrc/bpp_stats.inl on the device, through the C ABI on torch tensors: the cases and the plain numpy statements of
tests/stats_cases.py (the same that tests/test_stats_kernels.py runs on the oracle library and the host emulator).  What only the
device can show is here: the wide reduction's hand-off of partial sums between 64 workgroups (its outer loop beyond the first
step, ragged sizes, hundreds of calls on one scratch buffer, two streams, a captured graph), and the compaction's vector loads
on a `done` that starts anywhere, with several workgroups of several rounds writing into page-locked host memory.  Every
comparison is bit-exact against the order include/bpp_abi.h states, or the derived bound against math.fsum.  All inputs are valid
and the refusals are argument checks on valid launches.  Reads nothing of the reference."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stats_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def bpp():
    import bpp_amd
    assert torch.cuda.is_available()
    bpp_amd._lib.lib()
    return bpp_amd


@pytest.fixture(scope="module")
def lib(bpp):
    return bpp._lib.lib()


def new_scratch():
    """BPP_REDUCE_SCRATCH_BYTES, zero-filled once"""
    return torch.zeros(sc.SCRATCH_DOUBLES, dtype=torch.float64, device=DEV)


def arrival_word(scratch):
    torch.cuda.synchronize()
    return int(scratch[4 * sc.REDUCE_LANES:].cpu().numpy().view(np.uint32)[0])


@pytest.fixture(scope="module")
def scratch(bpp):
    """ONE scratch buffer for every single-call case of the wide reduction: each call has to leave it ready for the next"""
    return new_scratch()


def current_stream():
    return torch.cuda.current_stream().cuda_stream


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def device_rows(rows, guard_rows=sc.GUARD_ROWS):
    """rows [E, 4] on the device behind a 32-byte-aligned start (one spare row to slice into), guard rows behind them"""
    E = rows.shape[0]
    store = torch.full(((E + guard_rows + 1) * 4,), sc.GUARD, dtype=torch.float64, device=DEV)
    off = (-store.data_ptr() % 32) // 8
    both = store[off:off + 4 * (E + guard_rows)].view(E + guard_rows, 4)
    both[:E].copy_(torch.from_numpy(np.array(rows)))
    assert both.data_ptr() % 32 == 0
    return both


def reduce_call(lib, rows, E, acc_ptr, clear, scratch, stream):
    rc = lib.bpp_episode_acc_reduce(rows.data_ptr(), E, acc_ptr, clear, scratch.data_ptr() if scratch is not None else None, stream)
    assert rc == 0, lib.bpp_last_error()


# ------------------------------------------------------------------------------------------------------------ 1. reductions
@pytest.mark.parametrize("form", ["one", "wide"])
@pytest.mark.parametrize("clear", [0, 1])
@pytest.mark.parametrize("E", sc.REDUCE_SIZES)
def test_gpu_acc_reduce_gives_the_headers_bits(lib, scratch, E, clear, form):
    """bpp_episode_acc_reduce from ACC0 in its one-workgroup and its 64-workgroup form: the normative bits, within the derived bound
    of fsum, rows zeroed (clear) or untouched, the 64 rows behind row E untouched, the arrival word zero again."""
    for kind in sc.REDUCE_KINDS:
        case = sc.reduce_case(E, kind)
        both = device_rows(case.rows)
        acc = to_dev(case.acc0)
        reduce_call(lib, both, E, acc.data_ptr(), clear, scratch if form == "wide" else None, current_stream())
        word = arrival_word(scratch)
        got = both.cpu().numpy()
        case.check(form, clear, acc.cpu().numpy(), got[:E], got[E:], word)


# ------------------------------------------------------------------------------------------ 2. one scratch buffer, many calls
MANY_SIZES, MANY_SEEDS = [1025, 8193, 65537, 132101, 17], [5, 6, 7, 8, 9]


def many_cases(count):
    """call i of a sequence: size i mod 5, data set (i + i / 5) mod 5 -- all 25 pairs within 25 calls"""
    return [sc.reduce_case(MANY_SIZES[i % 5], "awkward", MANY_SEEDS[(i + i // 5) % 5]) for i in range(count)]


def uploaded(cases):
    rows = {}
    for c in cases:
        if (c.E, id(c)) not in rows:
            rows[(c.E, id(c))] = device_rows(c.rows, guard_rows=0)
    return [rows[(c.E, id(c))] for c in cases]


def check_slots(label, slots, cases):
    got = slots.cpu().numpy()
    wrong = [i for i, c in enumerate(cases) if sc.bits(got[i]).tolist() != sc.bits(c.want).tolist()]
    assert not wrong, "%s: %d of %d calls off the header's order, the first is call %d (E=%d): %r, want %r" % (
        label, len(wrong), len(cases), wrong[0], cases[wrong[0]].E, got[wrong[0]].tolist(), cases[wrong[0]].want.tolist())


def test_gpu_wide_reduce_200_calls_back_to_back_on_one_scratch_buffer(lib):
    """Every call leaves the arrival counter at zero for the next one: 200 wide calls on one stream and one scratch buffer with no
    host synchronisation in between, five sizes and five data sets in turn, each call adding into its own slot."""
    cases = many_cases(200)
    rows = uploaded(cases)
    slots = to_dev(np.tile(np.array(sc.ACC0), (200, 1)))
    scratch = new_scratch()
    torch.cuda.synchronize()
    stream = current_stream()
    for i, c in enumerate(cases):
        reduce_call(lib, rows[i], c.E, slots.data_ptr() + 32 * i, 0, scratch, stream)
    assert arrival_word(scratch) == 0
    check_slots("one stream", slots, cases)
    for r, c in list(zip(rows, cases))[:25]:
        assert np.array_equal(sc.bits(r.cpu().numpy()), sc.bits(c.rows))


# ----------------------------------------------------------------------------------------------------------- 3. two streams
def test_gpu_wide_reduce_on_two_streams_with_a_scratch_buffer_each(lib):
    """Two streams, each with its own scratch buffer, rows and slots, 50 wide calls each, enqueued alternately."""
    sides = []
    for k in range(2):
        cases = many_cases(100)[k::2]
        sides.append(dict(cases=cases, rows=uploaded(cases), slots=to_dev(np.tile(np.array(sc.ACC0), (50, 1))), scratch=new_scratch(),
                          stream=torch.cuda.Stream(device=DEV)))
    torch.cuda.synchronize()
    for i in range(50):
        for s in sides:
            reduce_call(lib, s["rows"][i], s["cases"][i].E, s["slots"].data_ptr() + 32 * i, 0, s["scratch"], s["stream"].cuda_stream)
    for k, s in enumerate(sides):
        s["stream"].synchronize()
        assert arrival_word(s["scratch"]) == 0
        check_slots("stream %d" % k, s["slots"], s["cases"])


# -------------------------------------------------------------------------------------------------------- 4. captured graph
def test_gpu_wide_reduce_replayed_from_a_captured_graph(lib):
    """The wide reduction as the one kernel node of a captured graph (a single branch), replayed 20 times; between replays the
    rows are rewritten by a stream-ordered copy.  acc carries over from replay to replay, clear = 1 zeroes the rows."""
    E = 65537
    data = [sc.reduce_case(E, "awkward", seed) for seed in MANY_SEEDS]
    sources = [to_dev(c.rows) for c in data]
    both = device_rows(data[0].rows)
    acc, scratch = to_dev(np.array(sc.ACC0)), new_scratch()
    seen = torch.zeros((20, 4), dtype=torch.float64, device=DEV)

    def call():
        reduce_call(lib, both, E, acc.data_ptr(), 1, scratch, current_stream())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                            # warm: nothing is created inside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                         # one stream, one kernel node
        call()
    want, running = [], np.array(sc.ACC0)
    acc.copy_(to_dev(running))
    for i in range(20):
        both[:E].copy_(sources[i % 5])
        graph.replay()
        seen[i].copy_(acc)
        running = sc.normative_sums(data[i % 5].rows, running)
        want.append(running)
    assert arrival_word(scratch) == 0
    got = seen.cpu().numpy()
    for i in range(20):
        assert sc.bits(got[i]).tolist() == sc.bits(want[i]).tolist(), "replay %d: %r, want %r" % (i, got[i].tolist(), want[i].tolist())
    after = both.cpu().numpy()
    assert not after[:E].any() and np.all(after[E:] == sc.GUARD)


# ---------------------------------------------------------------------------------------------------- 5. bpp_episode_stats
@pytest.mark.parametrize("E", sc.REDUCE_SIZES)
def test_gpu_episode_stats_gives_the_headers_bits(lib, E):
    """bpp_episode_stats over a tenth of the bins, done bytes of every nonzero kind, ep_len up to 2^31 - 1."""
    case = sc.stats_case(E)
    done, ret, ratio, ln, acc = (to_dev(a) for a in (case.done, case.ep_ret, case.ratio, case.ep_len, case.acc0))
    rc = lib.bpp_episode_stats(done.data_ptr(), ret.data_ptr(), ratio.data_ptr(), ln.data_ptr(), E, acc.data_ptr(), current_stream())
    assert rc == 0, lib.bpp_last_error()
    case.check("device", acc.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ 6. gather
@pytest.fixture(scope="module")
def pinned(bpp):
    """page-locked host memory for the largest case, as BppVecEnv._gather_finished allocates it"""
    t = torch.empty((sc.finished_room(max(sc.GATHER_SIZES)),), dtype=torch.uint8).pin_memory()
    return t, t.numpy()


_fields = {}


def device_fields(E):
    if E not in _fields:
        f = sc.gather_fields(E)
        _fields[E] = tuple(to_dev(a) for a in (f.ep_ret, f.ratio, f.ep_len, f.counter))
    return _fields[E]


@pytest.mark.parametrize("pattern", sc.DONE_PATTERNS)
@pytest.mark.parametrize("E", sc.GATHER_SIZES)
def test_gpu_gather_finished_compacts_in_bin_order(lib, pinned, E, pattern):
    """bpp_gather_finished with `done` a view at 0, 1, 8 and 15 bytes past a 16-byte boundary: staged through a device buffer into
    page-locked memory, direct (dev = NULL: the kernel writes into the page-locked tensor) and eager (BPP_GATHER_ENQUEUE_ONLY, then
    bpp_wait) against np.flatnonzero -- header count and all five arrays; in the direct and eager forms no byte beyond each array's
    first n entries has changed from the sentinel.  Refused: a count of n +- 1 (after a valid launch), a count beyond E, the eager
    form with a device buffer."""
    case = sc.gather_case(E, pattern)
    n, room, stream = case.n, sc.finished_room(E), current_stream()
    ret, ratio, ln, cnt = device_fields(E)
    host_t, host_np = pinned[0][:room], pinned[1][:room]
    store = torch.zeros(E + 64, dtype=torch.uint8, device=DEV)
    dev = torch.empty(room, dtype=torch.uint8, device=DEV)
    source = to_dev(case.done)

    def gather(done, dev_ptr, count):
        return lib.bpp_gather_finished(done.data_ptr(), ret.data_ptr(), ratio.data_ptr(), ln.data_ptr(), cnt.data_ptr(), E, dev_ptr,
                                       host_t.data_ptr(), count, stream)

    for shift in sc.DONE_SHIFTS:
        off = sc.shifted(store.data_ptr(), 63, shift)
        done = store[off:off + E]
        done.copy_(source)
        assert done.data_ptr() % 16 == shift
        dev.fill_(sc.SENTINEL)
        torch.cuda.synchronize()
        host_np[:] = sc.SENTINEL
        assert gather(done, dev.data_ptr(), n) == 0, lib.bpp_last_error()
        case.check_staged("shift %d staged" % shift, host_np)
        host_np[:] = sc.SENTINEL
        assert gather(done, None, n) == 0, lib.bpp_last_error()
        case.check_written("shift %d direct" % shift, host_np, n)
        host_np[:] = sc.SENTINEL
        assert gather(done, None, sc.ENQUEUE_ONLY) == 0, lib.bpp_last_error()
        assert lib.bpp_wait(stream) == 0, lib.bpp_last_error()
        case.check_written("shift %d eager" % shift, host_np, E)
    assert torch.equal(done, source)
    if n < E:
        assert gather(done, dev.data_ptr(), n + 1) != 0 and b"not the number of finished bins" in lib.bpp_last_error()
    if n > 0:
        assert gather(done, None, n - 1) != 0 and b"not the number of finished bins" in lib.bpp_last_error()
    assert gather(done, dev.data_ptr(), E + 1) != 0 and b"bad size" in lib.bpp_last_error()
    assert gather(done, dev.data_ptr(), sc.ENQUEUE_ONLY) != 0 and b"dev must be NULL" in lib.bpp_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------- 7. Python plumbing
def test_gpu_env_episode_stats_adds_into_out_and_both_forms_agree(bpp):
    """BppVecEnv.episode_stats on an env of 1 000 bins (not a multiple of 1 024) whose accumulator rows hold awkward values:
    out=acc ADDS into a non-zero acc, wide=False and wide=True give the same (normative) bits, EpisodeStats.collect clears the
    rows and a second collect adds zero."""
    E, size = 1000, (10, 10, 10)
    env = bpp.BppVecEnv(E, size, enable_rotation=False, pool=bpp.sequences.cut2_pool(size, 8, seed=1), device=DEV)
    env.reset()
    case = sc.reduce_case(E)
    env.ep_acc.copy_(to_dev(case.rows))
    for wide in (True, False):
        acc = to_dev(case.acc0)
        assert env.episode_stats(wide=wide, out=acc) is acc
        assert sc.bits(acc.cpu().numpy()).tolist() == sc.bits(case.want).tolist(), wide
        fresh = env.episode_stats(wide=wide).cpu().numpy()
        assert sc.bits(fresh).tolist() == sc.bits(sc.normative_sums(case.rows, np.zeros(4))).tolist(), wide
    assert np.array_equal(sc.bits(env.ep_acc.cpu().numpy()), sc.bits(case.rows))
    stats = bpp.EpisodeStats(env.device)
    stats.acc.copy_(to_dev(case.acc0))
    assert stats.collect(env) is stats
    first = stats.acc.cpu().numpy()
    assert sc.bits(first).tolist() == sc.bits(case.want).tolist()
    assert not env.ep_acc.cpu().numpy().any()
    stats.collect(env)
    assert sc.bits(stats.acc.cpu().numpy()).tolist() == sc.bits(first).tolist()
    assert arrival_word(env._reduce_scratch) == 0
