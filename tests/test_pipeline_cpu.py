"""CPU-side checks of the pipelined rollout driver (include/bpp_pipeline.h): the group plan is a pure host function,
arguments are validated before any device is touched, and libbpp_hip.so exports what the header declares."""
import ctypes
import os
import re

import pytest

from bpp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -1


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


def plan(lib, E, groups):
    first, count = (ctypes.c_int32 * 4)(*([-7] * 4)), (ctypes.c_int32 * 4)(*([-7] * 4))
    n = lib.bpp_pipeline_plan(E, groups, first, count)
    return n, list(first), list(count)


@pytest.mark.parametrize("E", [1, 63, 64, 1000, 2100, 32768, 65536])
@pytest.mark.parametrize("groups", [1, 2, 3, 4])
def test_plan_covers_the_bins_disjointly_with_aligned_boundaries(lib, E, groups):
    n, first, count = plan(lib, E, groups)
    assert 1 <= n <= groups
    assert first[0] == 0 and first[n - 1] + count[n - 1] == E
    for g in range(n):
        assert count[g] > 0 and first[g] % _lib.PIPELINE_ALIGN == 0
        if g + 1 < n:
            assert first[g + 1] == first[g] + count[g]          # contiguous, disjoint, in order
        if n > 1:
            assert count[g] >= _lib.PIPELINE_MIN_GROUP
    assert first[n:] == [-7] * (4 - n) and count[n:] == [-7] * (4 - n)     # nothing written past the groups made
    if groups == 1:
        assert (n, first[0], count[0]) == (1, 0, E)
    if E >= groups * (_lib.PIPELINE_MIN_GROUP + _lib.PIPELINE_ALIGN):
        assert n == groups                                      # fewer only when E is too small
    assert _lib.pipeline_plan(E, groups) == list(zip(first[:n], count[:n]))


def test_plan_sizes(lib):
    """Equal groups where the alignment allows, the remainder in the last one, no group under the minimum."""
    assert _lib.pipeline_plan(65536, 2) == [(0, 32768), (32768, 32768)]
    assert _lib.pipeline_plan(65536, 4) == [(k * 16384, 16384) for k in range(4)]
    assert _lib.pipeline_plan(33000, 2) == [(0, 16512), (16512, 16488)]
    assert _lib.pipeline_plan(33000, 4) == [(0, 8256), (8256, 8256), (16512, 8256), (24768, 8232)]
    assert _lib.pipeline_plan(2 * _lib.PIPELINE_MIN_GROUP, 4) == [(0, 8192), (8192, 8192)]
    assert _lib.pipeline_plan(2 * _lib.PIPELINE_MIN_GROUP - 1, 4) == [(0, 2 * _lib.PIPELINE_MIN_GROUP - 1)]
    assert _lib.pipeline_plan(2 * _lib.PIPELINE_MIN_GROUP + 1, 2) == [(0, 2 * _lib.PIPELINE_MIN_GROUP + 1)]   # 8256 + 8129: one group
    assert _lib.pipeline_plan(2 ** 31 - 1, 4)[-1] == (3 * 536870912, 536870911)


def test_argument_validation_happens_before_any_device_work(lib):
    first, count = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    assert lib.bpp_pipeline_plan(0, 2, first, count) == BADARG
    assert lib.bpp_pipeline_plan(-5, 2, first, count) == BADARG
    assert lib.bpp_pipeline_plan(65536, 0, first, count) == BADARG
    assert lib.bpp_pipeline_plan(65536, 5, first, count) == BADARG and b"groups" in lib.bpp_last_error()
    assert lib.bpp_pipeline_plan(65536, 2, None, count) == BADARG
    assert lib.bpp_pipeline_plan(65536, 2, first, None) == BADARG
    with pytest.raises(RuntimeError):
        _lib.pipeline_plan(65536, 9)

    assert lib.bpp_pipeline_create(None, 2) == BADARG
    pipe = ctypes.c_void_p(123)
    assert lib.bpp_pipeline_create(ctypes.byref(pipe), 0) == BADARG and not pipe.value
    assert lib.bpp_pipeline_create(ctypes.byref(pipe), 5) == BADARG and b"max_groups" in lib.bpp_last_error()
    assert lib.bpp_pipeline_destroy(None) == 0

    E = 65536
    b = _lib.Batch(E, 10, 10, 10, 0, 0, 64, 12, 0, E, 16, 16, 48, None, _lib.POOL_STATIC, 0, None)
    outs = (_lib.StepOut * 2)(_lib.StepOut(16, 16), _lib.StepOut(16, 16))
    call = lib.bpp_rollout_uniform_sets_pipelined

    def refused(batch=b, o=outs, nsets=2, first_mask=16, actions=16, nsteps=3, flags=0, pipe=None, groups=2):
        return call(ctypes.byref(batch) if batch is not None else None, o, nsets, first_mask, actions, 1, 0, nsteps, flags, pipe, groups,
                    None) == BADARG

    assert refused(batch=None) and refused(o=None) and refused(actions=None) and refused(nsets=0)
    assert refused(nsteps=-1)
    assert refused(groups=0) and refused(groups=5)
    ring = _lib.Batch(E, 10, 10, 10, 0, 0, 8 * E, 12, 0, E, 16, 16, 48, None, _lib.POOL_RING, 0, None)
    assert refused(batch=ring) and b"static pools only" in lib.bpp_last_error()
    cached = _lib.Batch(E, 10, 10, 10, 0, 0, 64, 12, 0, E, 16, 16, 48, None, _lib.POOL_STATIC, 0, 128)
    assert refused(batch=cached) and b"static pools only" in lib.bpp_last_error()
    no_mask = (_lib.StepOut * 2)(_lib.StepOut(16, 16), _lib.StepOut(16))
    assert refused(o=no_mask) and b"mask" in lib.bpp_last_error()
    host = (_lib.StepOut * 2)(_lib.StepOut(16, 16), _lib.StepOut(16, 16))
    host[1].host_reward, host[1].host_done = 16, 16
    assert refused(o=host) and b"host_reward" in lib.bpp_last_error()
    assert refused(first_mask=None) and b"first_mask" in lib.bpp_last_error()
    assert refused(pipe=None) and b"needs a pipe" in lib.bpp_last_error()        # two groups of 32 768 bins, no pipe


def test_every_declared_symbol_is_exported(lib):
    src = open(os.path.join(ROOT, "include", "bpp_pipeline.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(bpp_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.PIPELINE_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    for macro, value in (("BPP_PIPELINE_MAX_GROUPS", _lib.PIPELINE_MAX_GROUPS), ("BPP_PIPELINE_ALIGN", _lib.PIPELINE_ALIGN),
                         ("BPP_PIPELINE_MIN_GROUP", _lib.PIPELINE_MIN_GROUP)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, src).group(1)) == value
