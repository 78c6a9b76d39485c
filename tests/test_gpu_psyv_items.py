"""Direct parity of the two palette-mode DCT descriptor kernels (psyv.hip) with the CPU restatement.

launch_psyv computes palette-mode DCT descriptors one wave per item (psyv_kernel) below 32,768 items and one lane per
item (psyv_dct_items_kernel: colours staged in LDS, the mirror applied as k ^ m, LUT rows through the scalar cache)
from there up.  tiler_debug_psyv_lane_items moves that threshold, so both kernels run here on the same small inputs
and are held to the same words: fp64 bit for bit, fp32 the rounded fp64 bit for bit.
"""
import contextlib
import functools

import numpy as np
import pytest

from tiler_amd import synth

pytestmark = pytest.mark.gpu

T, P = 300, 9
FLAG_SETS = [1, 1 | 8, 1 | 8 | 16, 1 | 8 | 32, 1 | 8 | 48]  # DCT, DCT + Q-weighting, and each mirror
CASES = [(f, -1) for f in FLAG_SETS] + [(1 | 8 | 48, 0), (1 | 8 | 48, 1)]
SIZES = [1, 63, 64, 65, 64 * 3 + 37]  # the valid mask of the one-wave block: one lane, one short, full, one over, ragged
LANE_PER_ITEM, WAVE_PER_ITEM = 1, 1 << 40
EXTREME0 = 8  # tiles 8..15 are the extreme ones (inside every unmapped case but n = 1, whose tile 0 is random)


@contextlib.contextmanager
def lane_items(gpu, min_items):
    lib = gpu.load()
    assert lib.tiler_debug_psyv_lane_items(min_items) == 0
    try:
        yield
    finally:
        lib.tiler_debug_psyv_lane_items(0)


@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(136)
    pp = rng.integers(0, 16, (T, 64)).astype(np.uint8)
    pals = synth.palettes(rng, P)
    # the extremes of the RGB tests as palette tiles: flat tiles of one index, black / white / primaries / grey in
    # palette 0, a single white pixel on black
    pals[0, :6] = np.array([0, 0xFFFFFF, 0xFF, 0xFF00, 0xFF0000, 0x808080], np.int32)
    for i in range(6):
        pp[EXTREME0 + i] = i
    pp[EXTREME0 + 6] = 0
    pp[EXTREME0 + 6, 17] = 1
    pp[EXTREME0 + 7] = 15
    return pp, pals


@functools.lru_cache(maxsize=None)
def _maps(n):
    rng = np.random.default_rng(1000 + n)
    tile_of = rng.integers(0, T, n).astype(np.int32)
    pal_of = rng.integers(0, P, n).astype(np.int32)
    if n >= 63:  # the extreme tiles, under the palette that holds 0 and 0xFFFFFF (n = 1 keeps its random tile)
        tile_of[-8:] = EXTREME0 + np.arange(8)
        pal_of[-8:] = 0
    return tile_of, pal_of


@functools.lru_cache(maxsize=None)
def _expected(oracle, n, flags, gamma, mapped):
    pp, pals = _inputs()
    if mapped:
        tile_of, pal_of = _maps(n)
        o = oracle.psyv_batch(n, palpix=pp[tile_of], pals=pals, pal_of=pal_of, flags=flags, gamma=gamma)
    else:  # tile_of = None: item i is tile i; pal_of = None: palette 0
        o = oracle.psyv_batch(n, palpix=pp[:n], pals=pals, flags=flags, gamma=gamma)
    o.setflags(write=False)
    return o


def _check(gpu, oracle, n, flags, gamma, mapped):
    pp, pals = _inputs()
    tile_of, pal_of = _maps(n) if mapped else (None, None)
    g64, g32 = gpu.psyv_batch(palpix=pp, tile_of=tile_of, palettes=pals, pal_of=pal_of, flags=flags, gamma=gamma, n=n,
                              want64=True, want32=True)
    o64 = _expected(oracle, n, flags, gamma, mapped)
    where = f"n={n} flags={flags} gamma={gamma} mapped={mapped}"
    assert np.array_equal(g64.view(np.uint64), o64.view(np.uint64)), where
    assert np.array_equal(g32.view(np.uint32), o64.astype(np.float32).view(np.uint32)), where


def test_extreme_tiles_are_distinct(oracle):
    """The inputs hold what they claim: the mirrors change the descriptors (so a dropped mirror shows) and the flat
    extreme tiles are there."""
    pp, pals = _inputs()
    assert np.all(pp[EXTREME0 + 1] == 1) and pals[0, 1] == 0xFFFFFF and pals[0, 0] == 0
    d = [_expected(oracle, 65, f, -1, True) for f in (1 | 8, 1 | 8 | 16, 1 | 8 | 32, 1 | 8 | 48)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert np.count_nonzero(np.any(d[i] != d[j], axis=1)) >= 50


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("min_items", [LANE_PER_ITEM, WAVE_PER_ITEM], ids=["lane_per_item", "wave_per_item"])
def test_psyv_dct_kernels_bit_exact(gpu, oracle, min_items, n):
    """Both kernels, forced by the hook, on every flag set and gamma, with tile_of / pal_of given and left None."""
    with lane_items(gpu, min_items):
        for flags, gamma in CASES:
            for mapped in (True, False):
                _check(gpu, oracle, n, flags, gamma, mapped)


def test_psyv_default_threshold_dispatch(gpu, oracle):
    """No hook: n = 32768 + 37 items (the lane-per-item kernel by the documented threshold, last block ragged) at DCT
    + Q-weighting + both mirrors, the widest flag set: the restatement's side of it takes 0.35 s on one host core."""
    _check(gpu, oracle, 32768 + 37, 1 | 8 | 48, -1, True)


def test_psyv_lane_items_hook_arguments(gpu):
    lib = gpu.load()
    try:
        assert lib.tiler_debug_psyv_lane_items(-1) == -1 and "min_items" in gpu.last_error()
        assert lib.tiler_debug_psyv_lane_items(5) == 0
    finally:
        assert lib.tiler_debug_psyv_lane_items(0) == 0


def test_prepare_dct_mode_lane_per_item(gpu, oracle):
    """Per-item mirrors (flags_per) through the lane-per-item kernel: Prepare's candidate descriptors in DCT mode,
    gamma -1, with the threshold at 1 -- the body of test_prepare_frame_tiling_dev_modes, unchanged."""
    from test_gpu_ft_modes import test_prepare_frame_tiling_dev_modes as prepare_body
    with lane_items(gpu, LANE_PER_ITEM):
        prepare_body(gpu, oracle, (False, -1))
