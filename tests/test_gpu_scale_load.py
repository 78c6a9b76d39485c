"""Lanczos input scaling fused with the tile cut (scale.hip through tiler_amd.load) against the restatement
tests/resample_ref.py followed by tests/load_ref.py: the six non-unit factors in the four byte orders, scale 1, one
axis only, rows at every byte alignment with poisoned padding, the seams of the kernels' spans and strips, the
tilemap cap with poison beyond the last tap, clipping pictures, chunked host staging, the Load step in one call, and
the refusals.  Every comparison is exact."""
import numpy as np
import pytest

from load_ref import FORMATS, load_dims, load_ref, store_ref
from resample_ref import scale_dims
from scale_cases import (FACTOR_SIZES, GPU_SIZES, NON_UNIT, as_format, check_argument_errors, random_case,
                         want_frames)
from tiler_amd import synth

pytestmark = pytest.mark.gpu

FMTS = list(FORMATS)
CANARY = 0x5A5A5A5A


def _dev_scaled(buf, fmt, F, W, H, pitch, fs, out_w, out_h, phase=0, **kw):
    """tiler_load_frames_scaled_dev over the byte buffer `buf` placed `phase` bytes past an aligned device address,
    into tiles with 64 canary words on either side, which must survive."""
    import torch
    from tiler_amd.load import frames_to_tiles_dev
    tm_w, tm_h = load_dims(out_w, out_h)
    n = F * tm_w * tm_h * 64
    d_buf = torch.zeros(buf.size + 4, dtype=torch.uint8, device="cuda")
    d_buf[phase:phase + buf.size] = torch.from_numpy(buf).cuda()
    d_all = torch.full((n + 128,), CANARY, dtype=torch.int32, device="cuda")
    d_rgb = d_all[64:64 + n]
    torch.cuda.synchronize()
    kw = kw or {"size": (out_w, out_h)}
    assert frames_to_tiles_dev(d_buf.data_ptr() + phase, F, W, H, d_rgb.data_ptr(), fmt, pitch, fs, **kw) \
        == (tm_w, tm_h)
    torch.cuda.synchronize()
    got = d_all.cpu().numpy()
    assert (got[:64] == CANARY).all() and (got[64 + n:] == CANARY).all()
    return got[64:64 + n].reshape(F, tm_w * tm_h, 64)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("factor", NON_UNIT)
@pytest.mark.parametrize("W, H", FACTOR_SIZES)
def test_factors_and_formats(gpu, W, H, factor, fmt):
    """67 x 45 and 131 x 70 at cbxScaling's six non-unit factors: host form by scale=, device form by size=."""
    from tiler_amd.load import frames_to_tiles
    out_w, out_h = scale_dims(W, H, factor)
    assert (W, H, out_w, out_h) in GPU_SIZES
    rgbx, want = random_case(W, H, out_w, out_h)
    pics = as_format(rgbx, fmt)
    got, tm_w, tm_h = frames_to_tiles(pics, fmt, scale=factor)
    assert (tm_w, tm_h) == load_dims(out_w, out_h) and got.dtype == np.int32 and np.array_equal(got, want)
    F, bpp = pics.shape[0], pics.shape[3]
    dev = _dev_scaled(pics.reshape(-1), fmt, F, W, H, W * bpp, H * W * bpp, out_w, out_h)
    assert np.array_equal(dev, want)


def test_scale_one_is_the_unscaled_call(gpu):
    """scale = 1 and size = the source's size return what the unscaled call returns."""
    from tiler_amd.load import frames_to_tiles
    rng = np.random.default_rng(12)
    pics = rng.integers(0, 256, (2, 45, 67, 4), dtype=np.uint8)
    plain, tm_w, tm_h = frames_to_tiles(pics, "bgra32")
    assert np.array_equal(plain, load_ref(pics, "bgra32")[0])
    for kw in ({"scale": 1.0}, {"scale": 1}, {"size": (67, 45)}):
        got, gw, gh = frames_to_tiles(pics, "bgra32", **kw)
        assert (gw, gh) == (tm_w, tm_h) and np.array_equal(got, plain)
        dev = _dev_scaled(pics.reshape(-1), "bgra32", 2, 67, 45, 67 * 4, 45 * 67 * 4, 67, 45, **kw)
        assert np.array_equal(dev, plain)


@pytest.mark.parametrize("out_w, out_h", [(64, 24), (32, 48)])
@pytest.mark.parametrize("fmt", ["rgb24", "bgra32"])
def test_one_axis_only(gpu, out_w, out_h, fmt):
    """64 x 48 -> 64 x 24 and -> 32 x 48: the pass of the axis that keeps its size is skipped, not run with its
    near-identity taps."""
    from tiler_amd.load import frames_to_tiles
    rgbx, want = random_case(64, 48, out_w, out_h)
    pics = as_format(rgbx, fmt)
    got, _, _ = frames_to_tiles(pics, fmt, size=(out_w, out_h))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("phase", [0, 1, 2, 3])
def test_odd_pitch_phase_and_padding(gpu, fmt, phase):
    """F = 3 pictures of 41 x 29 with pitch = row + 5 (odd for RGB24: rows at every byte alignment), frames 7 bytes
    further apart, the base at each byte phase; padding bytes and X bytes hold 0xEE and must not show."""
    W, H, out_w, out_h, F = 41, 29, 20, 14, 3
    rgbx, want = random_case(W, H, out_w, out_h, F)
    bpp = FORMATS[fmt][1]
    pitch = W * bpp + 5
    fs = H * pitch + 7
    buf = np.full(F * fs, 0xEE, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, (F, H, W, bpp), (fs, pitch, bpp, 1))
    view[...] = as_format(rgbx, fmt)[..., :bpp]
    if bpp == 4:
        view[..., 3] = 0xEE
    assert np.array_equal(_dev_scaled(buf, fmt, F, W, H, pitch, fs, out_w, out_h, phase=phase), want)
    if phase == 0:
        from tiler_amd.load import frames_to_tiles
        assert np.array_equal(frames_to_tiles(view, fmt, size=(out_w, out_h))[0], want)


@pytest.mark.parametrize("W, H, factor, tiles", [(528, 24, 0.5, (33, 1)), (40, 200, 0.375, (1, 9)),
                                                 (24, 24, 2.0, (6, 6))])
def test_seams(gpu, W, H, factor, tiles):
    """33 tiles across (one past a 256-pixel span, two horizontal spans); nine tile rows whose strips share source
    rows; an upscale whose taps clamp at both borders of every row."""
    from tiler_amd.load import frames_to_tiles
    out_w, out_h = scale_dims(W, H, factor)
    rgbx, want = random_case(W, H, out_w, out_h)
    got, tm_w, tm_h = frames_to_tiles(rgbx[..., :3], "rgb24", scale=factor)
    assert (tm_w, tm_h) == tiles and np.array_equal(got, want)
    got4, _, _ = frames_to_tiles(as_format(rgbx, "bgra32"), "bgra32", scale=factor)
    assert np.array_equal(got4, want)


@pytest.mark.parametrize("W, H, tiles, reach", [(968, 16, (240, 4), (963, 16)), (16, 548, (4, 135), (16, 543))])
def test_cap_and_poison_beyond_the_last_tap(gpu, W, H, tiles, reach):
    """Scale 2 past ReframeUI's cap: 1936 wide gives tm_w = 240, 1096 high gives tm_h = 135.  The columns (rows) past
    the last kept pixel's taps hold poison on the device, and the device buffer ends with the last needed byte."""
    out_w, out_h = 2 * W, 2 * H
    assert load_dims(out_w, out_h) == tiles
    rgbx, want = random_case(W, H, out_w, out_h, F=1)
    clean = rgbx[0, :, :, :3]
    pic = clean.copy()
    pic[:, reach[0]:] = 0xEE
    pic[reach[1]:] = 0xEE
    assert not np.array_equal(pic, clean)
    buf = pic.reshape(-1)[:((reach[1] - 1) * W + reach[0]) * 3].copy()
    assert np.array_equal(_dev_scaled(buf, "rgb24", 1, W, H, W * 3, H * W * 3, out_w, out_h), want)


def _patterns(W, H):
    jj, ii = np.mgrid[0:H, 0:W]
    board = (((ii + jj) & 1) * 255).astype(np.uint8)
    board2 = ((((ii // 2) + (jj // 2)) & 1) * 255).astype(np.uint8)
    spikes = np.zeros((H, W), np.uint8)
    holes = np.full((H, W), 255, np.uint8)
    for (y, x) in ((0, 0), (H // 2, W // 2), (H - 1, W - 1), (1, W - 2)):
        spikes[y, x], holes[y, x] = 255, 0
    planes = [board, board2, spikes, holes, np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)]
    return np.stack([np.stack([p, 255 - p, p], 2) for p in planes])


@pytest.mark.parametrize("W, H, out_w, out_h", [(37, 29, 18, 14), (24, 16, 36, 24)])
def test_clipping_pictures(gpu, W, H, out_w, out_h):
    """0 / 255 checkerboards, impulses, all-0 and all-255: the overshoot clips at both ends, in the 8-bit picture
    between the passes too."""
    from tiler_amd.load import frames_to_tiles
    pics = _patterns(W, H)
    want = want_frames(pics, out_w, out_h)[0]
    assert (want & 0xFF == 0).any() and (want & 0xFF == 255).any()
    got, _, _ = frames_to_tiles(pics, "rgb24", size=(out_w, out_h))
    assert np.array_equal(got, want)
    assert np.array_equal(frames_to_tiles(pics[..., ::-1], "bgr24", size=(out_w, out_h))[0], want)


def test_chunked_host_staging(gpu):
    """The host form with one and with two frames per staging chunk gives what the default chunk gives (F = 5)."""
    from tiler_amd.load import frames_to_tiles
    rgbx, want = random_case(48, 32, 24, 16, F=5)
    pics = rgbx[..., :3]
    assert np.array_equal(frames_to_tiles(pics, "rgb24", scale=0.5)[0], want)
    lib = gpu.load()
    try:
        assert lib.tiler_debug_load_chunk(1) == 0
        one = frames_to_tiles(pics, "rgb24", scale=0.5)[0]
        assert lib.tiler_debug_load_chunk(2) == 0
        two = frames_to_tiles(pics, "rgb24", scale=0.5)[0]
    finally:
        lib.tiler_debug_load_chunk(0)
    assert np.array_equal(one, want) and np.array_equal(two, want)


def test_load_clip_scaled(gpu):
    """load_clip(scale=0.5) on six 40 x 24 pictures with one cut: the frames are the restatement's, the correlations
    and the split are those of the scaled frames."""
    import ctypes
    from tiler_amd.keyframes import interframe_correlation
    from tiler_amd.load import load_clip
    rng = np.random.default_rng(77)
    frames, starts = synth.shot_frames(rng, 6, 5, 3, shot_len=(3, 3))
    assert starts.size > 1
    images = store_ref(frames, 5, 3, "rgb24")
    assert images.shape == (6, 24, 40, 3)
    want = want_frames(images, 20, 12)[0]
    got, tm_w, tm_h, kf_of, kf_start, corr = load_clip(images, "rgb24", scale=0.5)
    assert (tm_w, tm_h) == (2, 1) and np.array_equal(got, want)
    want_corr = interframe_correlation(want, 2, 1)
    assert np.array_equal(corr.view(np.uint64), want_corr.view(np.uint64))
    want_kf = np.zeros(6, np.int32)
    n = gpu.load().tiler_find_keyframes(want_corr.ctypes.data_as(ctypes.c_void_p), 6, 2,
                                        want_kf.ctypes.data_as(ctypes.c_void_p))
    assert n >= 1 and np.array_equal(kf_of, want_kf) and kf_start[-1] == 6 and kf_start.size == n + 1
    same = load_clip(images, "rgb24", size=(40, 24))
    plain = load_clip(images, "rgb24")
    assert all(np.array_equal(a, b) for a, b in zip(same, plain))


def test_refusals_launch_nothing(gpu):
    check_argument_errors(gpu.load(), gpu.last_error)
