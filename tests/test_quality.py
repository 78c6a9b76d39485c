"""Quality readout, host side: the numpy restatement of the reference's Render selection / mirror rule
(main.pas:3305-3343, 3413-3446) and of ComputeCorrelationBGR over the raster + transposed copies
(main.pas:769-788, 3470-3489, PearsonCorrelation 1465-1492) that tests/test_gpu_quality.py compares the GPU with,
checked here against a plain Python loop and against the GTM player's renderer (tests/gtm_read.py); psnr and the
argument validation of tiler_amd.quality."""
import math

import numpy as np
import pytest

import gtm_read
from tiler_amd import quality

MULS = (2126, 7152, 722)  # cRedMul, cGreenMul, cBlueMul (main.pas:25-27)


# ---- restatement ------------------------------------------------------------------------------------------------
def ref_render(tile, pal, hm, vm, palpix, thm, tvm, palettes, pal_row0, n_palettes, sm=None):
    """Render's imgDest as [F][Q][64] int32 0x00BBGGRR (tile-major) + the skipped positions per frame.
    sm = (sm_tile, sm_pal, sm_hm, sm_vm, smoothed) or None."""
    tile, pal, hm, vm = (np.asarray(a, np.int64) for a in (tile, pal, hm, vm))
    if sm is not None:  # TMItem := TileMap; if SmoothedTileMap.Smoothed then TMItem := SmoothedTileMap
        st, sp, sh, sv, flag = (np.asarray(a, np.int64) for a in sm)
        use = flag != 0
        tile, pal, hm, vm = np.where(use, st, tile), np.where(use, sp, pal), np.where(use, sh, hm), np.where(use, sv, vm)
    palpix = np.asarray(palpix, np.uint8).reshape(-1, 8, 8)
    palettes = np.asarray(palettes, np.int64)
    F, Q = tile.shape
    out = np.zeros((F, Q, 64), np.int32)
    invalid = np.zeros(F, np.int32)
    for f in range(F):
        for q in range(Q):
            ti, pi = int(tile[f, q]), int(pal[f, q])
            if not (0 <= ti < palpix.shape[0]) or not (0 <= pi < n_palettes):  # InRange ... else skipped
                invalid[f] += 1
                continue
            t = palpix[ti]
            if bool(hm[f, q]) != bool(thm[ti]):  # (hmir and mirrored) xor tilePtr^.HMirror -> txm := 7 - txm
                t = t[:, ::-1]
            if bool(vm[f, q]) != bool(tvm[ti]):
                t = t[::-1, :]
            out[f, q] = (palettes[int(pal_row0[f]) + pi][t.ravel()] & 0xFFFFFF).astype(np.int32)
    return out, invalid


def raster(frame, tm_w, tm_h):
    """[Q][64] tile-major -> [H][W] screen raster."""
    return np.asarray(frame).reshape(tm_h, tm_w, 8, 8).transpose(0, 2, 1, 3).reshape(tm_h * 8, tm_w * 8)


def corr_operand(frame, tm_w, tm_h):
    """ya of ComputeCorrelationBGR(oriCorr): raster copy then transposed copy (main.pas:3475-3486), planar
    r * 2126, g * 7152, b * 722 (the bitmap holds SwapRB(ToRGB(r, g, b)), so (v shr 16) and $ff is red).
    Exact integers (int64)."""
    img = raster(frame, tm_w, tm_h).astype(np.int64)
    seq = np.concatenate([img.ravel(), img.T.ravel()])  # [W H + x H + y] = [y W + x]
    return np.concatenate([((seq >> (8 * c)) & 255) * MULS[c] for c in range(3)])


def chains(xi, yi):
    """mean + the three ordered sums of PearsonCorrelation; np.add.accumulate is strictly sequential."""
    mx, my = float(int(xi.sum())) / float(xi.size), float(int(yi.sum())) / float(yi.size)
    dx, dy = xi.astype(np.float64) - mx, yi.astype(np.float64) - my
    return (np.add.accumulate(dx * dy)[-1], np.add.accumulate(dx * dx)[-1], np.add.accumulate(dy * dy)[-1])


def pearson_tail(num, denx, deny):
    den = math.sqrt(denx) * math.sqrt(deny)
    return num / den if den != 0.0 else 0.0


def ref_corr(src, dst, tm_w, tm_h):
    src = np.asarray(src).reshape(-1, tm_w * tm_h, 64)
    dst = np.asarray(dst).reshape(-1, tm_w * tm_h, 64)
    return np.array([pearson_tail(*chains(corr_operand(a, tm_w, tm_h), corr_operand(b, tm_w, tm_h)))
                     for a, b in zip(src, dst)], np.float64)


def ref_sse(src, dst):
    src, dst = np.asarray(src).astype(np.int64), np.asarray(dst).astype(np.int64)
    F = src.shape[0]
    d = [(((src >> s) & 255) - ((dst >> s) & 255)).reshape(F, -1) for s in (0, 8, 16)]
    return np.stack([(c * c).sum(1) for c in d], 1).astype(np.uint64)


def random_frames(rng, F, Q):
    return (rng.integers(0, 1 << 24, (F, Q, 64))).astype(np.int32)


def random_scene(rng, F=3, Q=12, T=40, palsize=16, n_palettes=3, n_kf=2, with_sm=True):
    """Items with every hm/vm combination over a tileset with every thm/tvm combination, two keyframes with
    different palette rows, `smoothed` on a random half with different smoothed items."""
    palpix = rng.integers(0, palsize, (T, 64)).astype(np.uint8)
    thm, tvm = (np.arange(T) & 1).astype(np.uint8), ((np.arange(T) >> 1) & 1).astype(np.uint8)
    palettes = rng.integers(0, 1 << 24, (n_kf * n_palettes, palsize)).astype(np.int32)
    pal_row0 = (np.minimum(np.arange(F) * n_kf // max(F, 1), n_kf - 1) * n_palettes).astype(np.int32)

    def items():
        combo = rng.permutation(F * Q) % 4  # every (hm, vm) pair occurs
        return (rng.integers(0, T, (F, Q)).astype(np.int32), rng.integers(0, n_palettes, (F, Q)).astype(np.int32),
                (combo & 1).astype(np.uint8).reshape(F, Q), (combo >> 1).astype(np.uint8).reshape(F, Q))
    tm = items()
    sm = None
    if with_sm:
        flag = (rng.permutation(F * Q) < F * Q // 2).astype(np.uint8).reshape(F, Q)
        sm = items() + (flag,)
    return dict(tm=tm, sm=sm, palpix=palpix, thm=thm, tvm=tvm, palettes=palettes, pal_row0=pal_row0,
                n_palettes=n_palettes)


# ---- the restatement itself ---------------------------------------------------------------------------------------
def test_accumulate_is_the_sequential_float_loop():
    """At (tm_w, tm_h) = (2, 1) the three chains equal a plain Python float loop bit for bit."""
    rng = np.random.default_rng(1)
    a, b = random_frames(rng, 2, 2)
    xi, yi = corr_operand(a, 2, 1), corr_operand(b, 2, 1)
    assert xi.size == 3 * 2 * 16 * 8
    mx, my = float(int(xi.sum())) / xi.size, float(int(yi.sum())) / yi.size
    num = denx = deny = 0.0
    for x, y in zip(xi.tolist(), yi.tolist()):
        num += (float(x) - mx) * (float(y) - my)
        denx += (float(x) - mx) * (float(x) - mx)
        deny += (float(y) - my) * (float(y) - my)
    got = chains(xi, yi)
    for g, w in zip(got, (num, denx, deny)):
        assert np.float64(g).view(np.uint64) == np.float64(w).view(np.uint64)
    assert -1.0 <= pearson_tail(*got) <= 1.0


def test_corr_operand_order():
    """Second half = the transposed copy: element W H + x H + y is pixel (y, x) (main.pas:3484)."""
    tm_w, tm_h = 3, 2
    W, H = 24, 16
    img = np.arange(W * H, dtype=np.int32).reshape(H, W) & 255  # red byte only
    frame = img.reshape(tm_h, 8, tm_w, 8).transpose(0, 2, 1, 3).reshape(tm_w * tm_h, 64)
    assert np.array_equal(raster(frame, tm_w, tm_h), img)
    op = corr_operand(frame, tm_w, tm_h)
    assert op.size == 3 * 2 * W * H and not op[2 * W * H:].any()
    for (y, x) in ((0, 0), (5, 17), (15, 23), (9, 1)):
        assert op[y * W + x] == img[y, x] * 2126 and op[W * H + x * H + y] == img[y, x] * 2126


def test_render_matches_gtm_player():
    """Independent cross-check: with no smoothed flags the restated render equals the GTM player's drawing of
    the same items (tests/gtm_read.render), for both keyframes' palettes."""
    rng = np.random.default_rng(2)
    tm_w, tm_h = 4, 3
    sc = random_scene(rng, F=4, Q=tm_w * tm_h, with_sm=False)
    tile, pal, hm, vm = sc["tm"]
    got, invalid = ref_render(tile, pal, hm, vm, sc["palpix"], sc["thm"], sc["tvm"], sc["palettes"], sc["pal_row0"],
                              sc["n_palettes"])
    assert not invalid.any() and len(set(sc["pal_row0"].tolist())) == 2
    for f in range(4):
        g = gtm_read.GTM({}, [], width=tm_w, height=tm_h, tiles=sc["palpix"], palsize=16)
        t = tile[f].astype(np.int64)
        attrs = (pal[f].astype(np.int64) << 2) | ((vm[f] ^ sc["tvm"][t]).astype(np.int64) << 1) | (hm[f] ^ sc["thm"][t])
        rows = sc["palettes"][sc["pal_row0"][f]:sc["pal_row0"][f] + sc["n_palettes"]]
        pd = {j: (rows[j].astype("<u4") | np.uint32(0xFF000000)).view(np.uint8).reshape(-1, 4)
              for j in range(rows.shape[0])}  # LoadPalette bytes: R, G, B, A
        g.frames = [(np.stack([t, attrs], 1), pd, 0)]
        img = gtm_read.render(g)[0]
        mine = raster(got[f], tm_w, tm_h)
        for c in range(3):
            assert np.array_equal((mine >> (8 * c)) & 255, img[..., c])


def test_render_restatement_smoothed_selection_and_invalid():
    rng = np.random.default_rng(3)
    sc = random_scene(rng)
    tile, pal, hm, vm = sc["tm"]
    args = (sc["palpix"], sc["thm"], sc["tvm"], sc["palettes"], sc["pal_row0"], sc["n_palettes"])
    plain, _ = ref_render(tile, pal, hm, vm, *args)
    smooth, _ = ref_render(*sc["sm"][:4], *args)
    both, inv = ref_render(tile, pal, hm, vm, *args, sm=sc["sm"])
    flag = sc["sm"][4].astype(bool)
    assert np.array_equal(both[flag], smooth[flag]) and np.array_equal(both[~flag], plain[~flag])
    assert not inv.any() and flag.any() and not flag.all()
    bad = tile.copy()
    bad[0, 0], bad[1, 5] = -1, sc["palpix"].shape[0]
    out, inv = ref_render(bad, pal, hm, vm, *args)
    assert inv.tolist() == [1, 1, 0] and not out[0, 0].any() and not out[1, 5].any()
    assert np.array_equal(out[0, 1:], plain[0, 1:])


# ---- tiler_amd.quality, host side ---------------------------------------------------------------------------------
def test_psnr():
    assert np.isinf(quality.psnr(np.zeros((2, 3), np.uint64), 4, 3)).all()
    # 1 tile: peak = 255^2 * 3 * 64 = 12,484,800; Σ sse = 124,848 -> ratio 100 -> 20 dB
    v = quality.psnr(np.array([[124848, 0, 0], [100000, 24000, 848]], np.uint64), 1, 1)
    assert np.abs(v - 20.0).max() < 1e-12
    with pytest.raises(ValueError):
        quality.psnr(np.zeros((2, 2)), 1, 1)


def test_validation_raises_before_any_library_call(monkeypatch):
    def no_lib():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(quality, "load", no_lib)
    rng = np.random.default_rng(4)
    sc = random_scene(rng)
    tile, pal, hm, vm = sc["tm"]
    tail = (sc["palpix"], sc["thm"], sc["tvm"], sc["palettes"], sc["pal_row0"], sc["n_palettes"])
    with pytest.raises(ValueError):  # item shape mismatch
        quality.render_frames(tile, pal[:, :-1], hm, vm, *tail)
    with pytest.raises(ValueError):  # some smoothed arrays only
        quality.render_frames(tile, pal, hm, vm, *tail, sm_tile=tile)
    with pytest.raises(ValueError):  # one row per frame
        quality.render_frames(tile, pal, hm, vm, *tail[:4], sc["pal_row0"][:-1], 3)
    with pytest.raises(ValueError):  # flags per tile
        quality.render_frames(tile, pal, hm, vm, sc["palpix"], sc["thm"][:-1], *tail[2:])
    with pytest.raises(ValueError):  # items beyond int32
        quality.render_frames(tile.astype(np.int64) + (1 << 40), pal, hm, vm, *tail)
    with pytest.raises(ValueError):
        quality.render_frames_dev(1, 12, 0, 0, 0, 0, 40, 0, 0, 0, 6, 16, 0, 0, 3, 0)
    with pytest.raises(ValueError):  # misaligned output
        quality.render_frames_dev(1, 12, 256, 256, 256, 256, 40, 256, 256, 256, 6, 16, 256, 256, 3, 264)
    fr = random_frames(rng, 2, 12)
    with pytest.raises(ValueError):
        quality.frame_quality(fr, fr[:1], 4, 3)
    with pytest.raises(ValueError):
        quality.frame_quality(fr, fr, 5, 3)
    with pytest.raises(ValueError):
        quality.frame_quality(fr, fr, 0, 3)
    with pytest.raises(ValueError):
        quality.frame_quality_dev(256, 264, 1, 4, 3)
    with pytest.raises(ValueError):
        quality.frame_quality_dev(0, 256, 1, 4, 3)
    with pytest.raises(AssertionError):  # valid arguments do reach the library
        quality.frame_quality(fr, fr, 4, 3)
