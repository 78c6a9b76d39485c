"""GPU parity of DLv3 palette quantisation (palette.hip, tiler_quantize_palettes[_dev]) against the reference's own
dlquant/quantizer.c: the committed vectors of tests/golden/dl3_ref_kat.npz (dl3_kat.py; generated from the
reference build of oracle/build_ref_dlquant.sh) for palette sizes 16 / 32 / 64 and lookup bpc 4..8, the same under
spilled recount lists, and flat tiles that wrap the 32-bit colour sums.  Only the fixture is read, never the reference
tree.  A palette row is CompareCMULHS-sorted (main.pas:2413), so it is compared with oracle.sort_cmulhs of the
reference's raw palette; that order is pinned by test_palette.py::test_sort_cmulhs_orders_by_luma_val_sat_hue."""
import ctypes
import functools

import numpy as np
import pytest

import dl3_kat
from tiler_amd.palette import quantize_palettes

pytestmark = pytest.mark.gpu

KF = 2  # the cases are dealt over two keyframes' pairs: pair = keyframe * pairs-per-keyframe + palette


@functools.lru_cache(maxsize=None)
def _inputs():
    """All non-wrap cases as one call's input: case c is pair c (tiles interleaved, not grouped by pair)."""
    cases, _ = dl3_kat.load()
    rgb = np.concatenate([c.tiles for c in cases])
    pal_of = np.concatenate([np.full(c.tiles.shape[0], i, np.int32) for i, c in enumerate(cases)])
    perm = np.random.default_rng(3).permutation(rgb.shape[0])  # a histogram does not depend on the tile order
    rgb, pal_of = rgb[perm], pal_of[perm]
    pairs = (len(cases) // KF + 1) * KF  # the last pairs stay empty
    for a in (rgb, pal_of):
        a.setflags(write=False)
    return cases, rgb, pal_of, pairs


def _check(oracle, q, bpc):
    cases, rgb, pal_of, pairs = _inputs()
    pal, uc, colors = quantize_palettes(rgb, pal_of, pairs, q, bpc)
    assert pal.shape == (pairs, q)
    for i, c in enumerate(cases):
        want = oracle.sort_cmulhs(c.palette(q, bpc))
        assert np.array_equal(pal[i], want), (c.name, q, bpc, pal[i], want)
        assert uc[i] == c.tiles.shape[0] and colors[i] == c.cells(bpc), (c.name, bpc)
    assert not pal[len(cases):].any() and not uc[len(cases):].any() and not colors[len(cases):].any()  # empty pairs


@pytest.mark.parametrize("bpc", dl3_kat.BPC)
@pytest.mark.parametrize("q", dl3_kat.QUANT_TO)
def test_quantize_equals_reference_fixture(gpu, oracle, q, bpc):
    """Every fixture case through one quantize_palettes call, one case per (keyframe, palette) pair: palettes
    equal the reference's, use counts are the tile counts, and the colour-table size is the plain numpy count of
    distinct b | g << bpc | r << 2 bpc cells."""
    _check(oracle, q, bpc)


@pytest.mark.parametrize("bpc", dl3_kat.BPC)
@pytest.mark.parametrize("q", dl3_kat.QUANT_TO)
def test_quantize_equals_reference_fixture_spilled_lists(gpu, oracle, q, bpc):
    """The same under tiler_debug_dl3(1): one recount entry per LDS batch, every longer list spills to the global
    overflow and runs in as many batches."""
    lib = gpu.load()
    assert lib.tiler_debug_dl3(1) == 0
    try:
        _check(oracle, q, bpc)
    finally:
        lib.tiler_debug_dl3(0)


@pytest.mark.parametrize("name", ["white_wraps", "white_wraps_then_merges", "white_wraps_among_20"])
def test_quantize_wraps_the_32_bit_sums_as_the_reference(gpu, oracle, name):
    """263,200 flat tiles of 0xFFFFFF (made on the device, the _dev entry point): each colour sum passes 2^32 and
    wraps as the reference's 32-bit ulong does -- alone, merged into a second colour after the wrap (quant_to 1),
    and as one of 21 colours reduced to 16."""
    import torch
    w = next(x for x in dl3_kat.load()[1] if x.name == name)
    n = int(w.tile_counts.sum())
    assert int(w.tile_counts[0]) * 64 * 255 > 1 << 32 and n * 64 < 1 << 31
    d_rgb = torch.repeat_interleave(torch.from_numpy(w.colours).cuda(), torch.from_numpy(w.tile_counts).cuda().long())
    d_rgb = d_rgb[:, None].expand(n, 64).contiguous()
    d_pal_of = torch.zeros(n, dtype=torch.int32, device="cuda")
    assert d_rgb.dtype == torch.int32 and d_rgb.shape == (n, 64)
    pal, uc, colors = np.zeros((1, w.quant_to), np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    vp = ctypes.c_void_p
    rc = gpu.load().tiler_quantize_palettes_dev(n, vp(d_rgb.data_ptr()), vp(d_pal_of.data_ptr()), None, 1, w.quant_to,
                                                w.bpc, *(a.ctypes.data_as(vp) for a in (pal, uc, colors)), None)
    assert rc == 0, gpu.last_error()
    want = oracle.sort_cmulhs(w.pal)
    assert np.array_equal(pal[0], want), (pal[0], want)
    assert uc[0] == n and colors[0] == w.colours.size
