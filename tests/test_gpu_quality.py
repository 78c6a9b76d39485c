"""GPU parity of the quality readout (tiler_amd.quality): corr bit-identical to the sequential fp64 restatement of
ComputeCorrelationBGR over the raster + transposed copies (tests/test_quality.py), sse equal to the integer sums,
rendered frames byte-exact (restated Render, and the GTM player's drawing of the written stream)."""
import dataclasses

import numpy as np
import pytest

from test_quality import random_frames, random_scene, ref_corr, ref_render, ref_sse
from tiler_amd import quality, synth

pytestmark = pytest.mark.gpu

SHAPES = [(4, 3), (7, 5), (20, 12)]
F_MAX = 31
_cache = {}


def frame_pairs(tm_w, tm_h):
    """31 random source frames, rendered frames random (even) or a noisy copy (odd), and their reference values
    (computed once per shape)."""
    key = (tm_w, tm_h)
    if key not in _cache:
        rng = np.random.default_rng(1000 * tm_w + tm_h)
        Q = tm_w * tm_h
        src, dst = random_frames(rng, F_MAX, Q), random_frames(rng, F_MAX, Q)
        noisy = np.clip(np.stack([(src >> s) & 255 for s in (0, 8, 16)]) + rng.integers(-9, 10, (3, F_MAX, Q, 64)),
                        0, 255)
        dst[1::2] = synth.rgb_pack(*noisy)[1::2]
        for a in (src, dst):
            a.setflags(write=False)
        _cache[key] = (src, dst, ref_corr(src, dst, tm_w, tm_h), ref_sse(src, dst))
    return _cache[key]


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("F", [1, 2, 15, 16, 31])
@pytest.mark.parametrize("tm_w,tm_h", SHAPES)
def test_corr_bit_exact_and_sse(gpu, tm_w, tm_h, F):
    """Both sides of the frames-per-workgroup boundary and a ragged tail; (7, 5) has W != H."""
    src, dst, rc, rs = frame_pairs(tm_w, tm_h)
    corr, sse = quality.frame_quality(src[:F], dst[:F], tm_w, tm_h)
    assert corr.shape == (F,) and sse.shape == (F, 3) and sse.dtype == np.uint64
    assert np.array_equal(bits(corr), bits(rc[:F]))
    assert np.array_equal(sse, rs[:F])


def test_edge_frames(gpu):
    """dst == src, constant dst, constant src, inverted src: all as the restatement.  A constant grey frame is not
    a constant operand (the channels carry different weights), a black one is: den = 0 -> exactly 0.0."""
    rng = np.random.default_rng(5)
    tm_w, tm_h = 4, 3
    a = random_frames(rng, 1, 12)[0]
    flat, black = np.full_like(a, synth.rgb_pack(77, 77, 77)), np.zeros_like(a)
    inv = a ^ 0xFFFFFF
    src = np.stack([a, a, flat, a, flat, a, black, black])
    dst = np.stack([a, flat, a, inv, flat, black, a, black])
    corr, sse = quality.frame_quality(src, dst, tm_w, tm_h)
    ref = ref_corr(src, dst, tm_w, tm_h)
    print("edge corr", corr.tolist(), ref.tolist())
    assert np.array_equal(bits(corr), bits(ref))
    assert not bits(corr)[5:].any() and not bits(ref)[5:].any()  # den = 0: +0.0
    assert np.array_equal(sse, ref_sse(src, dst)) and not sse[0].any()


def test_dev_form_agrees(gpu):
    import torch
    tm_w, tm_h = 7, 5
    src, dst, rc, rs = frame_pairs(tm_w, tm_h)
    F = 17
    d_src, d_dst = torch.from_numpy(src[:F].copy()).cuda(), torch.from_numpy(dst[:F].copy()).cuda()
    torch.cuda.synchronize()
    corr, sse = quality.frame_quality_dev(d_src.data_ptr(), d_dst.data_ptr(), F, tm_w, tm_h)
    assert np.array_equal(bits(corr), bits(rc[:F])) and np.array_equal(sse, rs[:F])
    assert quality.frame_quality(src[:0], dst[:0], tm_w, tm_h)[0].shape == (0,)


def _render_dev(sc, F, Q, with_sm):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tm = [dev(a) for a in sc["tm"]]
    sm = [dev(a) for a in sc["sm"]] if with_sm else []
    palpix, thm, tvm, pals, row0 = (dev(sc[k]) for k in ("palpix", "thm", "tvm", "palettes", "pal_row0"))
    out = torch.full((F, Q, 64), -1, dtype=torch.int32, device="cuda")
    invalid = torch.full((F,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    smp = [t.data_ptr() for t in sm] if with_sm else [0] * 5
    quality.render_frames_dev(F, Q, *[t.data_ptr() for t in tm], palpix.shape[0], palpix.data_ptr(), thm.data_ptr(),
                              tvm.data_ptr(), pals.shape[0], pals.shape[1], pals.data_ptr(), row0.data_ptr(),
                              sc["n_palettes"], out.data_ptr(), invalid.data_ptr(), *smp)
    torch.cuda.synchronize()
    return out.cpu().numpy(), invalid.cpu().numpy()


@pytest.mark.parametrize("with_sm", [True, False])
@pytest.mark.parametrize("palsize", [16, 4])
def test_render_matches_restatement(gpu, palsize, with_sm):
    """Q = 12, T = 40 with every thm/tvm combination, items with every hm/vm combination, smoothed on a random half
    with different items, two keyframes' palette rows; the NULL-smoothed form; host and _dev forms agree."""
    rng = np.random.default_rng(10 * palsize + with_sm)
    F, Q = 3, 12
    sc = random_scene(rng, F=F, Q=Q, T=40, palsize=palsize, with_sm=with_sm)
    tail = (sc["palpix"], sc["thm"], sc["tvm"], sc["palettes"], sc["pal_row0"], sc["n_palettes"])
    ref, ref_inv = ref_render(*sc["tm"], *tail, sm=sc["sm"])
    sm = sc["sm"] or (None,) * 5
    got, inv = quality.render_frames(*sc["tm"], *tail, *sm)
    assert got.dtype == np.int32 and np.array_equal(got, ref) and np.array_equal(inv, ref_inv) and not inv.any()
    dgot, dinv = _render_dev(sc, F, Q, with_sm)
    assert np.array_equal(dgot, ref) and np.array_equal(dinv, ref_inv)
    if with_sm:  # the smoothed items do change the picture
        assert not np.array_equal(ref, ref_render(*sc["tm"], *tail)[0])


def test_render_invalid_items(gpu):
    """tile = -1, tile = T, pal = n_palettes: counted per frame, rendered 0, neighbours untouched.  The kernel
    checks the ranges before indexing, so nothing is read out of bounds."""
    rng = np.random.default_rng(6)
    sc = random_scene(rng, F=3, Q=12, T=40, with_sm=True)
    tile, pal, hm, vm = (a.copy() for a in sc["tm"])
    sm = [a.copy() for a in sc["sm"]]
    tail = (sc["palpix"], sc["thm"], sc["tvm"], sc["palettes"], sc["pal_row0"], sc["n_palettes"])
    good, _ = quality.render_frames(tile, pal, hm, vm, *tail, *sm)
    sm[4][0, 3] = sm[4][0, 7] = sm[4][2, 0] = 0  # these positions use the unsmoothed item
    sm[4][2, 11] = 1                             # this one the smoothed item
    base, _ = quality.render_frames(tile, pal, hm, vm, *tail, *sm)
    tile[0, 3], tile[0, 7], pal[2, 0], sm[0][2, 11] = -1, 40, sc["n_palettes"], 40
    got, inv = quality.render_frames(tile, pal, hm, vm, *tail, *sm)
    ref, ref_inv = ref_render(tile, pal, hm, vm, *tail, sm=sm)
    assert inv.tolist() == [2, 0, 2] and np.array_equal(inv, ref_inv)
    assert np.array_equal(got, ref)
    bad = np.zeros((3, 12), bool)
    bad[0, 3] = bad[0, 7] = bad[2, 0] = bad[2, 11] = True
    assert not got[bad].any() and np.array_equal(got[~bad], base[~bad]) and good.shape == got.shape


def _end_to_end(oracle):
    """The smallest synthetic video of the pipeline test through run_all, once: (video, encoder, quality(), the
    GTM player's picture of the written stream as [F][Q][64] RGB words)."""
    if "e2e" not in _cache:
        import gtm_read
        from tiler_amd.encoder import Encoder
        from tiler_amd.frame_tiling import FT_MEDIUM
        v = synth.video(51 + FT_MEDIUM, 320, 240, kf_frames=(3, 3), n_palettes=8)
        e = Encoder(v)
        e.run_all(700, FT_MEDIUM, 0.2)
        q = e.quality(width=320, height=240)
        img = gtm_read.render(gtm_read.read_gtm(oracle, e.save_stream(320, 240, 24.0))).astype(np.int32)
        assert img.shape == (6, 240, 320, 4)
        word = img[..., 0] | (img[..., 1] << 8) | (img[..., 2] << 16)
        player = word.reshape(6, 30, 8, 40, 8).transpose(0, 1, 3, 2, 4).reshape(6, 1200, 64)
        _cache["e2e"] = (v, e, q, player)
    return _cache["e2e"]


def test_end_to_end_render_equals_gtm_player(gpu, oracle):
    """enc.quality()'s rendered frames (the SmoothedTileMaps after Smooth: what SaveStream writes) are the GTM
    player's picture of the written stream, RGB channels, byte for byte."""
    v, e, q, player = _end_to_end(oracle)
    diff = (q["rgb"] != player).any(2)
    print("end-to-end: positions that differ from the player", int(diff.sum()), "of", diff.size,
          "pixels", int((q["rgb"] != player).sum()))
    assert np.array_equal(q["rgb"], player)


def test_end_to_end_encoder_quality(gpu, oracle):
    """Same run: corr is finite, in [-1, 1] and equal to the restatement.  Render's on-screen rule
    (main.pas:3416-3418: the smoothed item only where Smoothed is set) differs from the written picture only at
    items DoTemporalSmoothing rewrote while leaving their flag clear (`PrevTMI^ := TMI^`, main.pas:4110)."""
    v, e, q, player = _end_to_end(oracle)
    sm = e.sm
    assert sm["smoothed"].any() and not q["invalid"].any()
    screen, _ = e.render(on_screen=True)
    rewritten = (sm["smoothed"] == 0) & ((sm["tile"] != e.tile) | (sm["pal"] != e.pal) | (sm["hm"] != e.hm)
                                         | (sm["vm"] != e.vm))
    diff = (screen != player).any(2)
    print("end-to-end: rewritten unflagged items", int(rewritten.sum()), "on-screen positions that differ",
          int(diff.sum()))
    assert not (diff & ~rewritten).any()
    corr = q["corr"]
    print("end-to-end corr", corr.tolist(), "psnr", q["psnr"].tolist())
    assert np.isfinite(corr).all() and (np.abs(corr) <= 1.0).all() and np.isfinite(q["psnr"]).all()
    assert np.array_equal(bits(corr), bits(ref_corr(v.frame_rgb, q["rgb"], 40, 30)))
    assert np.array_equal(q["sse"], ref_sse(v.frame_rgb, q["rgb"]))


def test_palette_exact_video_has_infinite_psnr(gpu):
    """A video whose tiles are already palette-exact (its source frames are the dithered tiles) scores inf."""
    from tiler_amd.encoder import Encoder
    v = synth.video(7, 64, 48, kf_frames=(2, 1), n_palettes=4)
    exact, invalid = Encoder(v).render()
    assert not invalid.any()
    e = Encoder(dataclasses.replace(v, frame_rgb=exact))
    q = e.quality(width=64, height=48)
    assert np.isinf(q["psnr"]).all() and not q["sse"].any()
    assert np.array_equal(bits(q["corr"]), bits(ref_corr(exact, exact, 8, 6)))
    with pytest.raises(ValueError):
        e.quality(width=64, height=40)


def test_1080p_frame_pair(gpu):
    """One 1080p shape (240 x 135 tiles, the reference's cap), F = 2: bit-exact.  The only large case."""
    rng = np.random.default_rng(8)
    tm_w, tm_h = 240, 135
    src, _ = synth.shot_frames(rng, 2, tm_w, tm_h, shot_len=(2, 2))
    noisy = np.clip(np.stack([(src >> s) & 255 for s in (0, 8, 16)]) + rng.integers(-20, 21, (3,) + src.shape), 0, 255)
    dst = synth.rgb_pack(*noisy).astype(np.int32)
    corr, sse = quality.frame_quality(src, dst, tm_w, tm_h)
    ref = ref_corr(src, dst, tm_w, tm_h)
    print("1080p corr", corr.tolist(), ref.tolist())
    assert np.array_equal(bits(corr), bits(ref))
    assert np.array_equal(sse, ref_sse(src, dst))
