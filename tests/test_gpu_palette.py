"""GPU parity of palette generation: tiler_quantize_palettes (QuantizePalette with DLv3 for
every (keyframe, palette) pair at once, CompareCMULHS order) bit-exact against the CPU restatement
(oracle/palette.c) -- palettes, use counts and DLv3 colour-table sizes -- on textured / gradient / flat tiles,
empty pairs, pairs with fewer colours than the palette, skipped (inactive / out-of-range) tiles and lookup bpc
4..8.  The oracle's dl3quant is pinned to the reference's own quantizer.c by test_dl3_ref.py.  The k-means of the
chain is checked at its edges in test_gpu_kmeans_edges.py."""
import numpy as np
import pytest

from tiler_amd import synth
from tiler_amd.palette import quantize_palettes

pytestmark = pytest.mark.gpu


def _case(seed, kf_frames, q, P, flat_share=0.0):
    rng = np.random.default_rng(seed)
    tiles = [synth.keyframe_frames(rng, f, q).reshape(-1, 64) for f in kf_frames]
    pal_of = [rng.integers(0, P, t.shape[0]) + k * P for k, t in enumerate(tiles)]
    rgb = np.concatenate(tiles)
    if flat_share:
        flat = rng.random(rgb.shape[0]) < flat_share
        rgb[flat] = rgb[flat, :1]
    return rgb, np.concatenate(pal_of).astype(np.int32), len(kf_frames) * P


def _check(oracle, rgb, pal_of, pairs, bpc=7, active=None):
    g_pal, g_uc, g_h = quantize_palettes(rgb, pal_of, pairs, 16, bpc, active)
    o_pal, o_uc, o_h = oracle.quantize_palettes(rgb, pal_of, pairs, 16, bpc, active)
    assert np.array_equal(g_uc, o_uc)
    assert np.array_equal(g_h, o_h)
    bad = np.nonzero(np.any(g_pal != o_pal, 1))[0]
    assert bad.size == 0, (bad[:5], g_pal[bad[:2]], o_pal[bad[:2]])
    return g_h


def test_quantize_two_keyframes(gpu, oracle):
    rgb, pal_of, pairs = _case(1, (3, 2), 120, 6)
    h = _check(oracle, rgb, pal_of, pairs)
    assert h.max() > 1000  # textured tiles: the O(n^2) passes are exercised


def test_quantize_many_pairs(gpu, oracle):
    """1024 (keyframe, palette) pairs in one call, the clip-level form: the per-pair arrays of the workspace
    (use counts, segments, run count) are sized for every pair (an undersized carve once put the palette
    output past the end of the allocation at P >= 1024)."""
    rgb, pal_of, pairs = _case(11, (2, 2), 2048, 512)
    h = _check(oracle, rgb, pal_of, pairs)
    assert pairs == 1024 and (h > 0).sum() > 1000


@pytest.mark.parametrize("bpc", [4, 5, 6, 8])
def test_quantize_bpc(gpu, oracle, bpc):
    rgb, pal_of, pairs = _case(2 + bpc, (2,), 100, 4)
    _check(oracle, rgb, pal_of, pairs, bpc)


def test_quantize_edges(gpu, oracle):
    rgb, pal_of, pairs = _case(7, (2, 2), 60, 5, flat_share=0.6)
    pal_of[pal_of == 3] = 4       # pair 3 empty
    pal_of[::17] = 99             # out of range: skipped
    few = pal_of == 6             # pair 6: a handful of flat colours (fewer than 16)
    rgb[few] = np.int32(0x102030) + (np.arange(few.sum()) % 5)[:, None].astype(np.int32)
    active = (np.arange(rgb.shape[0]) % 11 != 0).astype(np.uint8)
    h = _check(oracle, rgb, pal_of, pairs, 7, active)
    assert h[3] == 0 and 0 < h[6] < 16


def test_quantize_clustered_long_recount_lists(gpu, oracle):
    """Few dominant colours with small noise: many entries share a nearest neighbour, so the merges' recount
    lists are long (the batched recount_next over many entries at once)."""
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (6, 3))
    n = 1500
    px = np.clip(base[rng.integers(0, 6, (n, 64))] + rng.integers(-10, 11, (n, 64, 3)), 0, 255).astype(np.int32)
    rgb = px[..., 0] | (px[..., 1] << 8) | (px[..., 2] << 16)
    pal_of = rng.integers(0, 3, n).astype(np.int32)
    _check(oracle, rgb, pal_of, 3)


@pytest.mark.parametrize("cap", [1, 3, 64])
def test_quantize_list_overflow(gpu, oracle, cap):
    """tiler_debug_dl3: with at most `cap` recount entries per LDS batch the merges' lists spill to the global
    overflow and run in several batches; palettes stay bit-exact."""
    from tiler_amd import load
    lib = load()
    rgb, pal_of, pairs = _case(5, (2,), 90, 3)
    assert lib.tiler_debug_dl3(cap) == 0
    try:
        _check(oracle, rgb, pal_of, pairs)
    finally:
        lib.tiler_debug_dl3(0)


@pytest.mark.parametrize("gamma", [-1, 0])
def test_lab_descriptor_bit_exact(gpu, oracle, gamma):
    """ComputeTilePsyVisFeatures(UseLAB) on the GPU (fdlibm exp / ln on device, detmath.hpp) equals the CPU
    restatement bit for bit, Haar and DCT."""
    from tiler_amd.psyv import psyv_batch
    rng = np.random.default_rng(20 + gamma)
    rgb = synth.frame_tiles(rng, 700)
    rgb[:5] = 0
    rgb[5:9] = 0xFFFFFF
    for wl in (True, False):
        g, _ = psyv_batch(rgb=rgb, flags=4 | (2 if wl else 0), gamma=gamma)
        o = oracle.psyv_lab_batch(rgb, gamma, wl)
        assert np.array_equal(g.view(np.uint64), o.view(np.uint64))


@pytest.mark.parametrize("n,k", [(3000, 8), (2500, 70), (200, 128), (50, 64)])
def test_kmeans_bit_exact(gpu, oracle, n, k):
    """Seeding, every Lloyd step, the final labels and centroids, and the iteration count equal the restatement's
    (the assignment takes the centroids 32 at a time: k = 70 runs three chunks, k = 128 four; n < k duplicates
    centres)."""
    from tiler_amd.palette import kmeans
    rng = np.random.default_rng(n + k)
    centers = rng.normal(0, 10, (max(2, k // 2), 192))
    X = centers[rng.integers(0, centers.shape[0], n)] + rng.normal(0, 3, (n, 192))
    gl, gc, gi = kmeans(X, k)
    ol, oc, oi = oracle.kmeans(X, k)
    assert gi == oi
    assert np.array_equal(gl, ol)
    assert np.array_equal(gc.view(np.uint64), oc.view(np.uint64))


def test_prepare_dither_tiles_bit_exact(gpu, oracle):
    from tiler_amd.palette import prepare_dither_tiles
    rgb = synth.keyframe_frames(np.random.default_rng(31), 3, 400).reshape(-1, 64)
    gl, gc, gi = prepare_dither_tiles(rgb, 16)
    ol, oc, oi = oracle.prepare_dither_tiles(rgb, 16)
    assert gi == oi and np.array_equal(gl, ol) and np.array_equal(gc, oc)
    zl, zc, _ = prepare_dither_tiles(rgb[:1], 16)  # fewer than two tiles: the reference's zero branch
    assert not zl.any() and not zc.any()


def test_generate_palettes_chain_bit_exact(gpu, oracle):
    """btnDitherClick's palette half over two keyframes on the GPU: DitheringPalIndex, palettes (DLv3 + CMULHS),
    centroids and the FinishQuantizePalette order equal the CPU chain's."""
    from tiler_amd.palette import generate_palettes
    rng = np.random.default_rng(41)
    frames = np.concatenate([synth.keyframe_frames(rng, 2, 300), synth.keyframe_frames(rng, 3, 300)])
    kf = np.array([0, 2, 5])
    g = generate_palettes(frames, kf, 8)
    o = oracle.generate_palettes(frames, kf, 8)
    for a, b, name in zip(g, o, ("palettes", "centroids", "dith", "use_count")):
        assert np.array_equal(a, b), name


def _degenerate_clip():
    """Three keyframes of 2 frames x 120 tiles (10 wide, 12 high): textured; all black (a fade); letterboxed -- the top
    and bottom four tile rows black, the middle four textured."""
    rng = np.random.default_rng(51)
    Q = 120
    textured = synth.keyframe_frames(rng, 2, Q)
    black = np.zeros((2, Q, 64), np.int32)
    letterbox = synth.keyframe_frames(rng, 2, Q)
    letterbox[:, :40] = 0
    letterbox[:, 80:] = 0
    return np.concatenate([textured, black, letterbox]), np.array([0, 2, 4, 6]), Q


def test_degenerate_clip_chain_bit_exact(gpu, oracle):
    """The palette half and the per-tile dither over a clip with a black keyframe and a letterboxed one: k-means on
    equal descriptors, seven palettes without a tile, palettes of one colour."""
    from tiler_amd.dither import dither_tiles
    from tiler_amd.palette import generate_palettes
    frames, kf, Q = _degenerate_clip()
    P = 8
    o = oracle.generate_palettes(frames, kf, P)
    assert (o[3][1] == 0).sum() == P - 1 and o[3][1].max() == 2 * Q  # the black keyframe: one palette has every tile
    assert (o[0][1] == 0).all()                                      # and every palette of it is black
    g = generate_palettes(frames, kf, P)
    for a, b, name in zip(g, o, ("palettes", "centroids", "dith", "use_count")):
        assert a.shape == b.shape and np.array_equal(a, b), name
    assert np.array_equal(g[1].view(np.uint64), o[1].view(np.uint64))
    pal_of = (np.repeat(np.arange(3), 2 * Q) * P + o[2]).astype(np.int32)
    rgb = frames.reshape(-1, 64)
    od = oracle.dither_tiles_tk(rgb, pal_of, o[0].reshape(3 * P, 16))
    assert not od[0][2 * Q:4 * Q].any() and not od[1][2 * Q:4 * Q].any() and not od[2][2 * Q:4 * Q].any()
    gd = dither_tiles(rgb, pal_of, g[0].reshape(3 * P, 16))
    for a, b, name in zip(gd, od, ("palpix", "hm", "vm")):
        assert np.array_equal(a, b), name


def test_degenerate_clip_chain_value_at_risk(gpu, oracle):
    """The same clip with chkUseDL3 off.  The value-at-risk path has no answer for a palette without a tile (the
    reference reads CMUsage[0] of an empty list): the black keyframe makes product and restatement fail alike, naming
    the same pair.  The textured and the letterboxed keyframe then go through, compared as test_gpu_palette_var.py
    compares them."""
    import var_palette_ref as ref
    from tiler_amd.palette import finish_quantize_palette, generate_palettes, prepare_dither_tiles
    frames, kf, Q = _degenerate_clip()
    P = 8
    lab = [prepare_dither_tiles(frames[kf[k]:kf[k + 1]].reshape(-1, 64), P)[0] for k in range(3)]
    assert [np.unique(v).size for v in lab] == [P, 1, P] and not lab[1].any()
    acc0 = np.full(3 * P, ref.fpc_round(2 * Q * 64 * 0.9), np.int32)
    pair_of = (np.repeat(np.arange(3), 2 * Q) * P + np.concatenate(lab)).astype(np.int32)
    with pytest.raises(ValueError, match="pair 9 "):  # keyframe 1, palette 1: the first without a tile
        ref.quantize_palettes_var(frames.reshape(-1, 64), pair_of, 3 * P, P, acc0, 16)
    with pytest.raises(gpu.TilerError, match="pair 9 "):
        generate_palettes(frames, kf, P, use_dl3=False, pal_var=0.9)
    two = np.concatenate([frames[0:2], frames[4:6]])
    pal, cent, dith, uc = generate_palettes(two, np.array([0, 2, 4]), P, use_dl3=False, pal_var=0.9)
    for k, src in enumerate((0, 2)):
        rgb = two[2 * k:2 * k + 2].reshape(-1, 64)
        c = prepare_dither_tiles(rgb, P)[1]
        o_pal, o_uc, _ = ref.quantize_palettes_var(rgb, lab[src], P, P, acc0[:P], 16)
        w_pal, w_dith, w_cent, lut = finish_quantize_palette(o_pal, o_uc, lab[src], c)
        assert np.array_equal(pal[k], w_pal) and np.array_equal(dith[k * 2 * Q:(k + 1) * 2 * Q], w_dith)
        assert np.array_equal(cent[k].view(np.uint64), w_cent.view(np.uint64)) and np.array_equal(uc[k][lut], o_uc)
