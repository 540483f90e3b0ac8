"""The lowest-top heuristic (include/bpp_heuristic.h) without a GPU: the product kernel of csrc/bpp_heuristic.inl
compiled by g++ against the SIMT emulator and held to oracle.policies.lowest_top_actions action for action, and the host refusals
of the product library, which need no device.  Inputs and checks: tests/heuristic_cases.py; tests/test_gpu_heuristic.py runs the
same cases on the device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from bpp_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heuristic_cases as hc  # noqa: E402
from conftest import load_golden  # noqa: E402


@pytest.fixture(scope="module")
def emu_lib(emu):
    L = ctypes.CDLL(emu.LIB)
    L.bpp_last_error.restype = ctypes.c_char_p
    return hc.bind(L)


@pytest.fixture(scope="module")
def run(emu_lib):
    return hc.host_runner(emu_lib)


# ------------------------------------------------------------------------------------------------------- 1. recorded deep states
@pytest.mark.parametrize("name", list(hc.DEEP))
def test_recorded_deep_states_both_rules_one_call_each(run, name):
    hc.check_deep(name, load_golden(name), run)


# --------------------------------------------------------------------------------------------------------------------- 2. edges
@pytest.mark.parametrize("size,rotation", hc.GEOMS, ids=hc.GEOM_IDS)
def test_edge_rows_of_every_geometry(run, size, rotation):
    names, obs, mask = hc.edge_rows(size, rotation)
    hc.check_rows(run, obs, mask, size, rotation, names)
    for r in range(obs.shape[0]):       # and every row on its own: n = 1
        hc.check_rows(run, obs[r:r + 1], mask[r:r + 1], size, rotation, names[r:r + 1])


def test_the_edge_rows_are_what_their_names_say():
    size, rotation = (10, 10, 10), True
    names, obs, mask = hc.edge_rows(size, rotation)
    K = hc.keys(obs, mask, size, rotation)
    best = K.min(axis=1)
    row = {n: i for i, n in enumerate(names)}
    assert (K[row["empty bin: everything ties"]] == best[row["empty bin: everything ties"]]).sum() == 2 * 8 * 6
    assert best[row["full bin, the terminator as item"]] == 20 and best[row["mask all off"]] == hc.BIG + 1
    for n in ("mask on only at out-of-range entries", "item wider than the bin", "item with a zero side"):
        assert best[row[n]] == hc.BIG, n
    act = hc.expected(obs, mask, size, rotation, "lowest_top")[0]
    assert act[row["mask all off"]] == 0 and act[row["mask on only at out-of-range entries"]] == 1
    assert act[row["x = y: the halves tie, the unrotated one wins"]] < 100
    assert act[row["only the rotated footprint fits"]] == 100 and (mask[row["only the rotated footprint fits"]][:100] == 0).all()
    assert act[row["index A on and best"]] == 100 and K[row["index A on and best"]][:100].min() < hc.BIG


@pytest.mark.parametrize("size,rotation", hc.GEOMS, ids=hc.GEOM_IDS)
def test_the_edge_rows_are_what_their_names_say_at_every_geometry(size, rotation):
    """The same properties from the oracle alone, stated for any geometry: at a strip the rotated footprint of an item "wider than
    the bin" may fit along the other dimension, and a row strip (W, 1) has a rotated footprint only where W <= L."""
    W, L, H, A, M = hc.dims(size, rotation)
    names, obs, mask = hc.edge_rows(size, rotation)
    K = hc.keys(obs, mask, size, rotation)
    best = K.min(axis=1)
    act = hc.expected(obs, mask, size, rotation, "lowest_top")[0]
    row = {n: i for i, n in enumerate(names)}
    places = lambda fx, fy: max(0, W - fx + 1) * max(0, L - fy + 1)                     # noqa: E731
    sx, sy = max(1, W // 3), max(1, L // 2)
    r = row["empty bin: everything ties"]
    assert (K[r] == best[r]).sum() == places(sx, sy) + (places(sy, sx) if rotation else 0) and act[r] in (0, A)      # a corner
    assert best[row["full bin, the terminator as item"]] == 2 * H and best[row["mask all off"]] == hc.BIG + 1 and act[row["mask all off"]] == 0
    r = row["mask on only at out-of-range entries"]
    assert best[r] == hc.BIG and act[r] == np.flatnonzero(mask[r] > 0.5)[0]
    assert best[row["item with a zero side"]] == hc.BIG
    assert (best[row["item wider than the bin"]] == hc.BIG) == (not (rotation and W + 1 <= L))
    assert (best[row["item longer than the bin"]] == hc.BIG) == (not (rotation and L + 1 <= W))
    assert best[row["heights and z at their largest"]] == 2 * min(H, 255)
    if rotation:
        assert act[row["x = y: the halves tie, the unrotated one wins"]] < A and act[row["x = y on random heights"]] < A
        if 1 < W <= L:
            r = row["only the rotated footprint fits"]
            assert act[r] == A and (mask[r][:A] == 0).all()
            r = row["index A on and best"]
            assert act[r] == A and K[r][:A].min() < hc.BIG and K[r][A] == 1 < K[r][:A].min()


@pytest.mark.parametrize("size,rotation", hc.BATCH_GEOMS, ids=hc.BATCH_IDS)
def test_batch_sizes_with_tails_in_a_wave_a_workgroup_and_a_block_of_bins(run, size, rotation):
    hc.check_batches(run, size, rotation)


@pytest.mark.parametrize("size,rotation", hc.CARVED_GEOMS, ids=hc.CARVED_IDS)
def test_rows_carved_from_a_wider_tensor_with_nan_padding_and_top_null(emu_lib, run, size, rotation):
    W, L, H, A, M = hc.dims(size, rotation)
    obs, mask = hc.batch_rows(size, rotation, 21)
    for before, after in ((0, 9), (3, 4)):
        wide = np.full((21, before + 4 * A + after), np.nan, np.float32)
        wide[:, before:before + 4 * A] = obs
        hc.check_rows(run, wide[:, before:before + 4 * A], mask, size, rotation)
    no_top = hc.host_runner(emu_lib, want_top=False)
    hc.check_rows(lambda *a: (no_top(*a)[0], run(*a)[1]), obs, mask, size, rotation)


@pytest.mark.parametrize("levels", [2, 3], ids=["binary-times-footprints", "ternary"])
def test_a_three_by_three_bin_enumerated_completely(run, levels):
    hc.check_enumerated(run, levels)


# ------------------------------------------------------------------------------------------------------------------- 3. garbage
@pytest.mark.parametrize("size,rotation", hc.GEOMS, ids=hc.GEOM_IDS)
def test_garbage_stays_in_bounds(run, size, rotation):
    """No value is compared: the call returns, reads nothing past the end of its inputs (an inaccessible page lies there), leaves
    the guard words alone and gives actions in [0, M)."""
    W, L, H, A, M = hc.dims(size, rotation)
    obs, mask = hc.garbage_rows(size, rotation)
    fo, fm = hc.Fenced(obs), hc.Fenced(mask)
    for rule in hc.RULES:
        act, top = run(fo.array, fm.array, size, rotation, rule)
        assert ((act >= 0) & (act < M)).all()
        assert ((top >= -1) & (top <= 510)).all()


# -------------------------------------------------------------------------------------------------------------- 4. independence
@pytest.mark.parametrize("size,rotation", [((10, 10, 10), True), ((20, 20, 20), False)], ids=["10r", "20"])
def test_a_row_gives_the_same_action_wherever_it_stands(run, size, rotation):
    hc.check_independence(run, size, rotation)


# --------------------------------------------------------------------------------------------------------------- 5. closed loop
def test_closed_loop_on_the_emulated_env(emu, oracle, run):
    size, rotation, bins, steps = (10, 10, 10), True, 16, 30
    want = hc.oracle_loop(oracle, size, rotation, bins, steps, hc.oracle_heuristic(size, rotation))
    got = hc.oracle_loop(emu, size, rotation, bins, steps, lambda obs, mask: run(obs, mask, size, rotation, "lowest_top")[0])
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert got[2:] == want[2:] and want[2] >= 16, want[2:]


# ---------------------------------------------------------------------------------------------------------------------- 7. host
def test_refusals_before_any_device_on_the_product_library_and_the_emulator(emu_lib):
    _lib.build()
    hc.refusals(_lib.lib())
    hc.refusals(emu_lib)


def test_info_table_of_every_geometry(emu_lib):
    hc.check_info(_lib.lib())
    hc.check_info(emu_lib)


def test_symbols_have_a_list_of_their_own():
    assert _lib.HEURISTIC_SYMBOLS == ["bpp_heuristic_act", "bpp_heuristic_act_info"]
    assert not set(_lib.HEURISTIC_SYMBOLS) & set(_lib.SYMBOLS)
    hdr = open(_lib.HEURISTIC_HDR).read()
    for name, value in _lib.HEURISTIC_RULES.items():
        assert "#define BPP_HEUR_%s %d" % (name.upper(), value) in hdr
    assert all(s + "(" in hdr for s in _lib.HEURISTIC_SYMBOLS)
    assert all(s not in open(_lib.HDR).read() for s in _lib.HEURISTIC_SYMBOLS)


def test_cpu_tensors_and_bad_arguments_are_refused_by_the_python_call():
    import bpp_amd
    obs, mask = torch.zeros(2, 400), torch.ones(2, 100)
    with pytest.raises(RuntimeError, match="HIP device"):
        bpp_amd.heuristic_act(obs, mask, (10, 10, 10))
    with pytest.raises(ValueError, match="unknown heuristic rule"):
        bpp_amd.heuristic_act(obs, mask, (10, 10, 10), rule="highest_top")
    assert "oracle" not in open(os.path.join(_lib.HERE, "heuristic.py")).read()
