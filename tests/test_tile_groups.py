"""The tile step kernel's forms with 2 and 4 groups of bins per wave (bpp_knobs.tile_groups), CPU half: which form configure() picks
for which launch (the product library's host side: bpp_launch_info needs no device), and the cases of tests/tile_group_cases.py on
the emulated kernels -- the emulator runs these forms elsewhere too (tests/test_emulated_kernels.py: variant); here the SHARED cases
run, so that what tests/test_gpu_tile_groups.py asks of the device is known to be able to fail (DESIGN.md 6 lists the kernel
mutations these cases catch)."""
import ctypes
import mmap

import numpy as np
import pytest

import tile_group_cases as tg

# (size, rot, largest E with one group, groups above it): 300 MB of observation and mask bytes per launch (kOutputsPastL3)
SELECTION = [((10, 10, 10), False, 150000, 2), ((10, 10, 10), True, 125000, 2),
             ((20, 20, 20), False, 37500, 4), ((20, 20, 20), True, 31250, 4)]
OTHER = [((10, 10, 20), False, 150001, 2), ((20, 20, 10), False, 37501, 4), ((20, 20, 20), False, 32768, 1)]   # the last: BASELINE config 4


@pytest.fixture(scope="module")
def host_lib():
    from bpp_amd import _lib
    _lib.build()
    _lib.lib()
    return _lib


@pytest.fixture
def host_knobs(host_lib):
    saved = host_lib.get_knobs()
    yield lambda **kw: host_lib.set_knobs(**kw)
    host_lib.set_knobs(**saved)


@pytest.mark.parametrize("g", [0, 1, 2, 4])
def test_form_selected_by_knob_and_by_launch_size(host_lib, host_knobs, g):
    host_knobs(tile_groups=g, bins_per_wave=0, waves_per_group=0, force_generic=0, legacy_fast=0)
    cases = [(size, rot, E, big if E > last else 1) for size, rot, last, big in SELECTION for E in (last, last + 1)]
    cases += OTHER
    for size, rot, last, big in SELECTION:          # the table's thresholds are the 300 MB rule
        A = size[0] * size[1]
        assert last == 300 * 1000 * 1000 // (16 * A + 4 * A * (1 + int(rot)))
    for size, rot, E, by_size in cases:
        nit = g if g else by_size
        epw = tg.EPW[size[0]]
        i = host_lib.launch_info(E, size, rot)
        assert i["kernel"] == tg.BPP_KERNEL_TILE, (size, rot, E, i)
        assert i["bins_per_wave"] == epw * nit, (size, rot, E, g, i)
        assert i["waves_per_group"] == 4 and i["workgroups"] == -(-E // (4 * epw * nit)), (size, rot, E, g, i)


def guarded_bytes(n):
    """n zero bytes that END at a page nobody may touch, and the mapping that keeps them alive: a kernel that reads or writes
    past them stops the process with SIGSEGV (pytest's faulthandler names the test) instead of going unnoticed."""
    page = mmap.PAGESIZE
    size = (n + page - 1) // page * page
    m = mmap.mmap(-1, size + page)
    buf = np.frombuffer(m, np.uint8)
    libc = ctypes.CDLL(None, use_errno=True)
    if libc.mprotect(ctypes.c_void_p(buf.ctypes.data + size), ctypes.c_size_t(page), 0) != 0:
        raise OSError(ctypes.get_errno(), "mprotect")
    return buf[size - n:size], m


class EmuCase(object):
    """tile_group_cases' env over the emulated library.  The byte heightmaps end at a guard page: staging the tiles of a wave's
    NIT groups addresses rows by group, and a row past the last bin must not be touched (no result would show it)."""

    def __init__(self, emu, pool, size, rot, E, rule, base, total):
        self.emu, self.size, self.rot, self.E = emu, size, rot, E
        self.env = env = emu.EmuEnv(pool, size, rot, E, env_id_base=base, env_id_total=total, mask_rule=rule)
        flat, self._mapping = guarded_bytes(E * env.A)
        env.hmap = flat.reshape(E, env.A)
        env._b.hmap = env.hmap.ctypes.data
        self.nxt = np.zeros(E, np.int64)

    def launch(self):
        i = self.emu.launch_info(self.E, self.size, self.rot)
        return i[0], i[2]

    def reset(self):
        return self.env.reset()

    def step(self, a, seed, step):
        o = self.env._o
        o.next_action, o.sample_seed, o.sample_step = self.nxt.ctypes.data, int(seed), int(step)
        self.nxt[:] = -7
        return self.env.step(a), self.nxt.copy()

    def rollout(self, seed, step0, n):
        self.env._o.next_action = None
        out, _ = self.emu.rollout_uniform(self.env, seed, step0, n)
        return {k: v.copy() for k, v in out.items()}

    def snapshot(self):
        e = self.env
        return dict(hmap=e.hmap.copy(), state=e.state.copy(), ep_acc=e.ep_acc.copy(), stats=e.episode_stats(wide=True),
                    stats_one=e.episode_stats())


@pytest.fixture
def emu_groups(emu):
    def make(groups):
        emu.set_knobs(tile_groups=groups)
        return lambda *a: EmuCase(emu, *a)
    yield make
    emu.set_knobs()


EMU_SHAPES = [((10, 10, 10), True), ((20, 20, 20), False), ((10, 10, 20), False), ((20, 20, 10), True)]


@pytest.mark.parametrize("groups", tg.GROUPS)
@pytest.mark.parametrize("size,rot", EMU_SHAPES)
def test_emulated_edge_sizes_match_oracle(emu_groups, oracle, size, rot, groups):
    make_env = emu_groups(groups)
    for E in tg.edge_sizes(size, groups):
        for rule in (0, 1):
            tg.lockstep(make_env, oracle, size, rot, E, groups, rule)


@pytest.mark.parametrize("groups", tg.GROUPS)
def test_emulated_tall_bins_match_oracle(emu_groups, oracle, groups):
    assert tg.tall(emu_groups(groups), oracle, (10, 10, 20), False, 70, groups) >= 4
