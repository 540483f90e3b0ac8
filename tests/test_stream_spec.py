"""supply.resolve_stream_spec on the CPU: the defaults a stream=dict(...) resolves to, every refusal, and the buffer sizes -- the
host entry points it leans on (launch_info, bpp_stream_sizes, bpp_stream_kinds_info) answer without a device."""
import ctypes

import pytest

from bpp_amd import _lib, sequences
from bpp_amd.supply import resolve_stream_spec

E, CUBE = 64, (10, 10, 10)


def resolve(stream, size=CUBE, rotation=False):
    return resolve_stream_spec(E, size, rotation, dict(stream))


@pytest.mark.parametrize("size, stream, want", [
    (CUBE, dict(bound=(2, 5), seed=5), dict(rng="mt19937", depth=8, pool_len=128, cache=True, refill_every=4)),
    (CUBE, dict(depth=8, refill_every=3), dict(depth=8, cache=True)),
    (CUBE, dict(depth=8, refill_every=5), dict(depth=8, cache=False, refill_every=5)),           # 8 - 5 < 4: no row left for the cache
    (CUBE, dict(depth=8, pool_len=8192), dict(depth=8, cache=False, refill_every=5)),
    (CUBE, dict(cache=False), dict(cache=False, refill_every=5)),
    (CUBE, dict(cache=True, depth=5), dict(depth=5, cache=True, refill_every=1)),
    ((7, 13, 8), dict(bound=(2, 4), seed=5, depth=8), dict(depth=8, pool_len=94, cache=False, refill_every=5)),   # no tile step kernel
    (CUBE, dict(kind="cut1"), dict(rng="counter", pool_len=128, bound=(5, 9), box_range=(2, 2, 2, 5, 5, 5))),
    (CUBE, dict(kind="rs"), dict(rng="counter", pool_len=128, box_set=tuple(sequences.DEFAULT_BOX_SET))),
])
def test_defaults(size, stream, want):
    r = resolve(stream, size)
    assert {k: r.spec[k] for k in want} == want
    assert (r.bound, r.cache, r.refill_every, r.pool_len) == (r.spec["bound"], r.spec["cache"], r.spec["refill_every"], r.spec["pool_len"])
    assert r.behind == (4 if r.cache else 3)
    assert r.rng == {"mt19937": _lib.STREAM_RNG_MT19937, "counter": _lib.STREAM_RNG_COUNTER}[r.spec["rng"]]
    assert r.spec.get("kind") == stream.get("kind")         # a CUT-2 spec carries no `kind`
    assert r.box_range == r.spec.get("box_range")
    if stream.get("kind") == "rs":
        assert len(r.spec["box_set"]) == 64 and all(type(b) is tuple for b in r.spec["box_set"])
        assert [tuple(b) for b in r.box_set.tolist()] == [b + (0,) for b in sequences.DEFAULT_BOX_SET]
    else:
        assert r.box_set is None and "box_set" not in r.spec


@pytest.mark.parametrize("stream, message", [
    (dict(kind="cut3"), "stream kind must be"),
    (dict(kind="cut1", rng="mt19937"), "counter generator only"),
    (dict(depth=3), "depth must be >= 4"),
    (dict(cache=True, depth=4), ">= 5"),
    (dict(depth=8, cache=False, refill_every=6), "1 .. depth - 3"),
    (dict(refill_every=0), "refill_every must be in"),
    (dict(kind="cut1", box_range=(2, 2, 2, 5, 5)), "box_range must be"),
    (dict(kind="cut1", box_range=(3, 2, 2, 2, 5, 5)), "box_range must be"),
    (dict(kind="cut1", box_range=(1, 1, 1, 1, 1, 1)), "BPP_CUT1_MAX_PIECES"),
    (dict(kind="cut1", box_range=(2, 2, 2, 2, 2, 2)), "2 low - 1"),
    (dict(kind="rs", pool_len=100), "needs pool_len >= 128"),
    (dict(kind="rs", box_set=[(0, 1, 1)]), "does not fit"),
])
def test_refusals(stream, message):
    with pytest.raises(ValueError, match=message):
        resolve(stream)


@pytest.mark.parametrize("rng", ["mt19937", "counter"])
def test_sizes_are_the_library_s(rng):
    r = resolve(dict(depth=8, pool_len=128, rng=rng))
    p = r.probe
    assert (p.num_envs, p.depth, p.pool_len, p.W, p.L, p.H, p.bound_lo, p.bound_hi, p.rng) == (E, 8, 128, 10, 10, 10, 2, 5, r.rng)
    assert not (p.ring or p.mt or p.work or p.gen_next or p.state or p.overflow)
    sizes = (ctypes.c_int64 * 2)()
    _lib.check(_lib.lib().bpp_stream_sizes(ctypes.byref(p), sizes))
    assert r.sizes == (int(sizes[0]), int(sizes[1])) and min(r.sizes) > 0
