"""GPU parity of the value-at-risk palette path (chkUseDL3 off, DoValueAtRiskBased main.pas:2256-2394):
tiler_quantize_palettes_var -- palettes, use counts and stats [U, CmlPct, merges, stop reason] -- byte for byte against
the CPU restatement (tests/var_palette_ref.py), then generate_palettes / load_and_dither with use_dl3=False.  The
smallest shape is one keyframe of 2 frames on a 4 x 3 tilemap (24 tiles) with 2 palettes of 16 colours."""
import ctypes

import numpy as np
import pytest

import var_palette_ref as ref
from tiler_amd import synth
from tiler_amd.palette import quantize_palettes_var

pytestmark = pytest.mark.gpu

TILES, P, PALSIZE = 2 * 4 * 3, 2, 16
# seeds of _seeded() found with the restatement on the CPU: what each must show is asserted from the stats
SEED_MERGES, SEED_COUNT_STOP, SEED_REPEAT_STOP = 0, 6, 1


def _acc0(tiles, n_pairs, pal_var):
    return np.full(n_pairs, ref.fpc_round(tiles * 64 * pal_var), np.int32)


def _check(rgb, pal_of, n_pairs, n_palettes, acc0, active=None):
    got = quantize_palettes_var(rgb, pal_of, n_pairs, n_palettes, acc0, PALSIZE, active)
    want = ref.quantize_palettes_var(rgb, pal_of, n_pairs, n_palettes, acc0, PALSIZE, active)
    for g, w, name in zip(got[::-1], want[::-1], ("stats", "use_count", "palettes")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        bad = np.flatnonzero((g != w).reshape(n_pairs, -1).any(axis=1))
        assert bad.size == 0, (name, bad[:5], g[bad[:2]], w[bad[:2]])
    return got


def _pairs(rng, n=TILES, n_pairs=P):
    pal_of = rng.integers(0, n_pairs, n).astype(np.int32)
    pal_of[:n_pairs] = np.arange(n_pairs)  # no pair is empty
    return pal_of


def test_noise_tiles(gpu):
    """Every colour occurs once (or nearly), so the order inside the list is the canonical tie order."""
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 1 << 24, (TILES, 64)).astype(np.int32)
    _, _, stats = _check(rgb, _pairs(rng), P, P, _acc0(TILES, P, 0.95))
    assert (stats[:, 0] > 64).all() and stats[:, 2].min() > 0


def test_three_level_tree(gpu):
    """One pair with more than 64^2 colours: its tree of minima has three levels, and the pick walks more than one
    item per thread."""
    rng = np.random.default_rng(12)
    n = 72
    rgb = rng.integers(0, 1 << 24, (n, 64)).astype(np.int32)
    pal_of = np.zeros(n, np.int32)
    pal_of[-2:] = 1
    _, _, stats = _check(rgb, pal_of, P, P, _acc0(n, P, 0.95))
    assert stats[0, 0] > 4096 and stats[0, 2] > 0


def test_low_colour_tiles(gpu):
    """5 distinct colours: U < palsize, the picks repeat."""
    rng = np.random.default_rng(2)
    cols = rng.integers(0, 1 << 24, 5).astype(np.int32)
    rgb = cols[rng.integers(0, 5, (TILES, 64))]
    pal, _, stats = _check(rgb, _pairs(rng), P, P, _acc0(TILES, P, 0.95))
    assert (stats[:, 0] == 5).all() and all(np.unique(row).size < PALSIZE for row in pal)


def test_flat_tiles(gpu):
    """Pair 1 holds one colour only (U = 1); pair 0 a few flat colours."""
    rng = np.random.default_rng(3)
    pal_of = _pairs(rng)
    rgb = np.repeat(rng.integers(0, 1 << 24, (TILES, 1)).astype(np.int32), 64, axis=1)
    rgb[pal_of == 1] = 0x336699
    pal, _, stats = _check(rgb, pal_of, P, P, _acc0(TILES, P, 0.95))
    assert stats[1].tolist() == [1, 1, 0, 0] and (pal[1] == 0x336699).all()


@pytest.mark.parametrize("pal_var", [0.0, 0.5, 0.95, 1.0])
def test_inactive_tiles(gpu, pal_var):
    """Inactive tiles count for acc0 (the keyframe's tile count) but not for the usage: with pal_var 1.0 the
    remainder never reaches 0 and CmlPct comes from min(U, palsize * P)."""
    rng = np.random.default_rng(4)
    cols = rng.integers(0, 1 << 24, 90).astype(np.int32)
    rgb = cols[np.minimum(rng.integers(0, 90, (TILES, 64)), rng.integers(0, 90, (TILES, 64)))]
    pal_of = _pairs(rng)
    active = np.ones(TILES, np.uint8)
    active[2::5] = 0
    _, uc, stats = _check(rgb, pal_of, P, P, _acc0(TILES, P, pal_var), active)
    assert uc.sum() == active.sum()
    if pal_var == 1.0:
        assert (stats[:, 1] == np.minimum(stats[:, 0], PALSIZE * P)).all()


def _seeded(seed):
    """24 tiles: pair 0 draws from a seed-sized set of random colours with skewed counts, pair 1 from grey ramps
    with regular steps (equal differences: the repeated-best stop)."""
    rng = np.random.default_rng(1000 + seed)
    pal_of = _pairs(rng)
    k = int(rng.integers(34, 60))
    cols = rng.integers(0, 1 << 24, k).astype(np.int32)
    rgb = cols[(rng.random((TILES, 64)) ** 2 * k).astype(np.int64)]
    step = int(rng.integers(1, 6))
    g = (np.arange(40) * step + int(rng.integers(0, 50))).astype(np.int32)
    ramp = (g | (g << 8) | (g << 16))[rng.integers(0, 40, (TILES, 64))]
    rgb[pal_of == 1] = ramp[pal_of == 1]
    return rgb, pal_of


@pytest.mark.parametrize("seed", sorted({SEED_MERGES, SEED_COUNT_STOP, SEED_REPEAT_STOP}))
def test_seeded_behaviours(gpu, seed):
    rgb, pal_of = _seeded(seed)
    acc0 = _acc0(TILES, P, 0.95)
    want = ref.quantize_palettes_var(rgb, pal_of, P, P, acc0, PALSIZE)[2]
    if seed == SEED_MERGES:
        assert want[:, 2].max() >= 8
    if seed == SEED_COUNT_STOP:
        assert ((want[:, 3] == 0) & (want[:, 2] > 1)).any()
    if seed == SEED_REPEAT_STOP:
        assert (want[:, 3] == 1).any()
    _check(rgb, pal_of, P, P, acc0)


def test_300_pairs_of_one_tile(gpu):
    """(n_pairs + 1) << 24 does not fit 32 bits from 255 pairs on."""
    rng = np.random.default_rng(6)
    rgb = rng.integers(0, 1 << 24, (300, 64)).astype(np.int32)
    rgb[::7] &= 0x0F0F0F  # some tiles with repeated colours
    _, uc, stats = _check(rgb, rng.permutation(300).astype(np.int32), 300, P, _acc0(1, 300, 0.95))
    assert (uc == 1).all() and stats[:, 0].max() == 64


def test_big_flat_counts_need_64_bit_products(gpu):
    """140,000 flat tiles of one saturated colour and one tile of another in the same pair: 255 * Count passes 2^31
    in the merge's weighted averages."""
    n = 140002
    rgb = np.full((n, 64), 0x0000FF, np.int32)
    rgb[n - 2] = 0xFF0000
    rgb[n - 1] = 0x123456
    pal_of = np.zeros(n, np.int32)
    pal_of[n - 1] = 1
    _, uc, stats = _check(rgb, pal_of, P, P, _acc0(n, P, 0.95))
    assert uc.tolist() == [n - 1, 1] and stats[0].tolist() == [2, 2, 1, 0] and 255 * (n - 2) * 64 > 1 << 31


def test_pair_without_active_tile_is_an_error(gpu):
    rng = np.random.default_rng(8)
    rgb = rng.integers(0, 1 << 24, (TILES, 64)).astype(np.int32)
    pal_of = _pairs(rng, n_pairs=3)
    active = (pal_of != 1).astype(np.uint8)
    with pytest.raises(gpu.TilerError, match="pair 1 "):
        quantize_palettes_var(rgb, pal_of, 3, 3, _acc0(TILES, 3, 0.95), PALSIZE, active)
    with pytest.raises(ValueError, match="pair 1 "):
        ref.quantize_palettes_var(rgb, pal_of, 3, 3, _acc0(TILES, 3, 0.95), PALSIZE, active)


def test_host_and_dev_forms_agree(gpu):
    """The _dev form on torch tensors and a non-default stream gives the host form's bytes."""
    import torch
    lib = gpu.load()
    rng = np.random.default_rng(9)
    n = 257
    rgb = (rng.integers(0, 1 << 24, (n, 64)) & 0xF0F0F0).astype(np.int32)
    pal_of = _pairs(rng, n, 3)
    active = (np.arange(n) % 5 != 3).astype(np.uint8)
    acc0 = _acc0(n, 3, 0.95)
    want = quantize_palettes_var(rgb, pal_of, 3, 3, acc0, PALSIZE, active)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    got = np.zeros((3, PALSIZE), np.int32), np.zeros(3, np.int32), np.zeros((3, 4), np.int32)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = [torch.from_numpy(a).cuda() for a in (rgb, pal_of, active)]
    stream.synchronize()
    rc = lib.tiler_quantize_palettes_var_dev(n, *(ctypes.c_void_p(t.data_ptr()) for t in d), 3, PALSIZE, 3, hp(acc0),
                                             *map(hp, got), ctypes.c_void_p(stream.cuda_stream))
    assert rc == 0, gpu.last_error()
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    assert np.array_equal(got[0], ref.quantize_palettes_var(rgb, pal_of, 3, 3, acc0, PALSIZE, active)[0])


def test_generate_palettes_var_chain(gpu):
    """generate_palettes(use_dl3=False) over two keyframes = the k-means labels + the restatement +
    finish_quantize_palette."""
    from tiler_amd.palette import finish_quantize_palette, generate_palettes, prepare_dither_tiles
    rng = np.random.default_rng(41)
    Q, NP = 60, 4
    frames = np.concatenate([synth.keyframe_frames(rng, 2, Q), synth.keyframe_frames(rng, 3, Q)])
    kf = np.array([0, 2, 5])
    pal, cent, dith, uc = generate_palettes(frames, kf, NP, use_dl3=False, pal_var=0.9)
    for k in range(2):
        f0, f1 = kf[k], kf[k + 1]
        rgb = frames[f0:f1].reshape(-1, 64)
        lab, c, _ = prepare_dither_tiles(rgb, NP)
        acc0 = np.full(NP, ref.fpc_round((f1 - f0) * Q * 64 * 0.9), np.int32)
        o_pal, o_uc, _ = ref.quantize_palettes_var(rgb, lab, NP, NP, acc0, PALSIZE)
        w_pal, w_dith, w_cent, lut = finish_quantize_palette(o_pal, o_uc, lab, c)
        assert np.array_equal(pal[k], w_pal) and np.array_equal(dith[f0 * Q:f1 * Q], w_dith)
        assert np.array_equal(cent[k], w_cent) and np.array_equal(uc[k][lut], o_uc)


def test_load_and_dither_var_to_gtm(gpu):
    """load_and_dither(use_dl3=False) -> Encoder.run_all -> a .gtm that verify_stream accepts; the palettes differ
    from the DLv3 ones (the keyword reaches the palette step)."""
    from tiler_amd.encoder import Encoder, load_and_dither
    from tiler_amd.frame_tiling import FT_MEDIUM
    rng = np.random.default_rng(79)
    tm_w, tm_h = 20, 15
    frames, _ = synth.shot_frames(rng, 6, tm_w, tm_h, shot_len=(3, 4))
    v = load_and_dither(frames, tm_w, tm_h, n_palettes=4, use_dl3=False, pal_var=0.95)
    assert not np.array_equal(v.palettes, load_and_dither(frames, tm_w, tm_h, n_palettes=4).palettes)
    e = Encoder(v)
    e.run_all(300, FT_MEDIUM, 0.2)
    res = e.verify_stream(e.save_stream(tm_w * 8, tm_h * 8, 24.0), width=tm_w * 8, height=tm_h * 8)
    assert res["frames"] == 6 and res["differing_frames"] == 0
