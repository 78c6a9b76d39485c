"""Raster ingest on the GPU (load.hip through tiler_amd.load) against the numpy oracle tests/load_ref.py: the four
byte orders, the crop and the cap, rows at every byte alignment, 64-bit frame offsets, strided numpy input, the way
back out, chunked host staging, the Load step in one call, and the ends of the chain (Dither in front, the GTM player
behind).  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

from gtm_cases import written_stream
from load_ref import FORMATS, load_ref, store_ref
from tiler_amd import gtm, synth

pytestmark = pytest.mark.gpu

FMTS = list(FORMATS)


def _strided(rng, fmt, F, W, H, row_pad, frame_pad, fill=None):
    """F random pictures of W x H in one byte buffer with padded rows and frames -> (buffer, view [F][H][W][bpp],
    pitch, frame_stride).  Padding and X bytes are random too (or `fill`)."""
    bpp = FORMATS[fmt][1]
    pitch = W * bpp + row_pad
    fs = H * pitch + frame_pad
    buf = rng.integers(0, 256, F * fs, dtype=np.uint8) if fill is None else np.full(F * fs, fill, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, (F, H, W, bpp), (fs, pitch, bpp, 1))
    return buf, view, pitch, fs


def _dev_load(buf, fmt, F, W, H, pitch, fs):
    import torch
    from tiler_amd.load import frames_to_tiles_dev, load_dims
    tm_w, tm_h = load_dims(W, H)
    d_src = torch.from_numpy(buf).cuda()
    d_rgb = torch.full((F, tm_w * tm_h, 64), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert frames_to_tiles_dev(d_src.data_ptr(), F, W, H, d_rgb.data_ptr(), fmt, pitch, fs) == (tm_w, tm_h)
    torch.cuda.synchronize()
    return d_rgb.cpu().numpy()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("W, H, row_pad, frame_pad", [(8, 8, 0, 0), (19, 13, 0, 0), (72, 40, 5, 3)])
def test_load_formats_and_sizes(gpu, fmt, W, H, row_pad, frame_pad):
    """One tile; a crop on both axes; 9 x 5 tiles with pitch = row + 5 (RGB24 rows start at every byte alignment)
    and frames 3 bytes further apart.  Host and _dev forms; X bytes are random and must not show."""
    from tiler_amd.load import frames_to_tiles
    rng = np.random.default_rng(W * 100 + H)
    buf, view, pitch, fs = _strided(rng, fmt, 3, W, H, row_pad, frame_pad)
    want, tm_w, tm_h = load_ref(view, fmt)
    got, gw, gh = frames_to_tiles(view, fmt)
    assert (gw, gh) == (tm_w, tm_h) and got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(_dev_load(buf, fmt, 3, W, H, pitch, fs), want)
    assert (got >> 24 == 0).all()


def test_load_cap(gpu):
    """1936 x 1096 is cut to ReframeUI's 240 x 135 tiles: the last column and row of tiles are pixels 1912..1919 and
    1072..1079, whatever lies beyond is ignored."""
    from tiler_amd.load import frames_to_tiles
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (1, 1096, 1936, 3), dtype=np.uint8)
    want, tm_w, tm_h = load_ref(img, "rgb24")
    got, gw, gh = frames_to_tiles(img, "rgb24")
    assert (gw, gh) == (240, 135) == (tm_w, tm_h) and np.array_equal(got, want)
    last = got[0, 240 * 135 - 1].reshape(8, 8)
    px = img[0, 1072:1080, 1912:1920].astype(np.int32)
    assert np.array_equal(last, px[..., 0] | (px[..., 1] << 8) | (px[..., 2] << 16))


def test_load_frame_offset_past_4g(gpu):
    """Two 16 x 16 BGRA32 pictures 2^32 + 4096 bytes apart in one device buffer: a frame offset kept in 32 bits would
    read picture 0 again, and the two differ in every pixel."""
    import torch
    from tiler_amd.load import frames_to_tiles_dev
    fs = (1 << 32) + 4096
    try:
        d_buf = torch.empty((1 << 32) + (1 << 20), dtype=torch.uint8, device="cuda")
    except RuntimeError as e:  # torch.cuda.OutOfMemoryError is one
        pytest.skip(f"no 4 GiB device buffer: {e}")
    rng = np.random.default_rng(9)
    p0 = rng.integers(0, 128, (16, 16, 4), dtype=np.uint8)
    p1 = p0 + 128  # every byte differs
    d_buf[:1024] = torch.from_numpy(p0.reshape(-1)).cuda()
    d_buf[fs:fs + 1024] = torch.from_numpy(p1.reshape(-1)).cuda()
    d_rgb = torch.zeros((2, 4, 64), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    frames_to_tiles_dev(d_buf.data_ptr(), 2, 16, 16, d_rgb.data_ptr(), "bgra32", 64, fs)
    torch.cuda.synchronize()
    got = d_rgb.cpu().numpy()
    del d_buf
    assert np.array_equal(got[0], load_ref(p0, "bgra32")[0][0])
    assert np.array_equal(got[1], load_ref(p1, "bgra32")[0][0])


def test_load_numpy_slice(gpu):
    """A clip sliced out of a larger array goes in by its strides (tests/test_load_host.py shows that no copy is
    made); the bytes around it are not part of the result."""
    from tiler_amd.load import frames_to_tiles
    rng = np.random.default_rng(4)
    big = rng.integers(0, 256, (4, 40, 100, 3), dtype=np.uint8)
    cut = big[:, 3:3 + 24, 5:5 + 40]
    want, tm_w, tm_h = load_ref(cut, "rgb24")
    got, gw, gh = frames_to_tiles(cut, "rgb24")
    assert (gw, gh) == (5, 3) == (tm_w, tm_h) and np.array_equal(got, want)
    one, _, _ = frames_to_tiles(big[2, 3:3 + 24, 5:5 + 40], "bgr24")
    assert np.array_equal(one, load_ref(cut[2], "bgr24")[0])


@pytest.mark.parametrize("fmt", FMTS)
def test_store_round_trip_and_padding(gpu, fmt):
    """tiles_to_frames(frames_to_tiles(x)) is the cropped x (X = 0xFF); with a pitch beyond the row -- here row + 5,
    so rows start at every byte alignment -- every padding byte of a 0xA5 buffer stays 0xA5; the _dev form with frames
    3 bytes further apart writes the same pictures and nothing else."""
    import torch
    from tiler_amd.load import frames_to_tiles, tiles_to_frames, tiles_to_frames_dev
    bpp = FORMATS[fmt][1]
    rng = np.random.default_rng(21)
    x = rng.integers(0, 256, (3, 29, 75, bpp), dtype=np.uint8)
    frames, tm_w, tm_h = frames_to_tiles(x, fmt)
    assert (tm_w, tm_h) == (9, 3)
    want = x[:, :24, :72].copy()
    if bpp == 4:
        want[..., 3] = 0xFF
    assert np.array_equal(store_ref(frames, tm_w, tm_h, fmt), want)
    back = tiles_to_frames(frames, tm_w, tm_h, fmt)
    assert back.shape == want.shape and back.dtype == np.uint8 and np.array_equal(back, want)
    # padded rows
    row, pitch = 72 * bpp, 72 * bpp + 5
    out = np.full((3, 24, pitch), 0xA5, np.uint8)
    view = tiles_to_frames(frames, tm_w, tm_h, fmt, pitch=pitch, out=out)
    assert np.shares_memory(view, out) and np.array_equal(view, want) and (out[:, :, row:] == 0xA5).all()
    # device form, padded rows and frames
    buf, dview, _, fs = _strided(rng, fmt, 3, 72, 24, 5, 3, fill=0xA5)
    d_dst = torch.from_numpy(buf).cuda()
    d_rgb = torch.from_numpy(frames | np.int32(0x7F000000)).cuda()  # the top byte of a tile pixel is ignored
    torch.cuda.synchronize()
    tiles_to_frames_dev(d_rgb.data_ptr(), 3, tm_w, tm_h, d_dst.data_ptr(), fmt, pitch, fs)
    torch.cuda.synchronize()
    buf[:] = d_dst.cpu().numpy()
    assert np.array_equal(dview, want)
    pad = np.ones(buf.shape, bool)
    for f in range(3):
        for j in range(24):
            pad[f * fs + j * pitch:f * fs + j * pitch + row] = False
    assert (buf[pad] == 0xA5).all()


def test_chunked_host_staging(gpu):
    """The host forms with one frame per staging chunk (the test hook) give what the default chunk gives."""
    from tiler_amd.load import frames_to_tiles, tiles_to_frames
    rng = np.random.default_rng(6)
    x = rng.integers(0, 256, (5, 16, 24, 3), dtype=np.uint8)
    want, tm_w, tm_h = frames_to_tiles(x, "rgb24")
    assert np.array_equal(want, load_ref(x, "rgb24")[0])
    lib = gpu.load()
    try:
        assert lib.tiler_debug_load_chunk(1) == 0
        got, _, _ = frames_to_tiles(x, "rgb24")
        back = tiles_to_frames(got, tm_w, tm_h, "rgb24")
        assert lib.tiler_debug_load_chunk(2) == 0  # 2 + 2 + 1
        got2, _, _ = frames_to_tiles(x, "rgb24")
    finally:
        lib.tiler_debug_load_chunk(0)
    assert np.array_equal(got, want) and np.array_equal(got2, want) and np.array_equal(back, x)


def test_load_clip(gpu):
    """The Load step in one call on a synthetic clip with shot transitions, handed over as RGB24 pictures: the
    frames come back, the correlations are those of keyframes.interframe_correlation bit for bit, the split is
    detect_keyframes'."""
    from tiler_amd.keyframes import detect_keyframes, interframe_correlation
    from tiler_amd.load import load_clip
    rng = np.random.default_rng(40)
    frames, starts = synth.shot_frames(rng, 40, 6, 4)
    assert starts.size > 1
    images = store_ref(frames, 6, 4, "rgb24")
    got, tm_w, tm_h, kf_of, kf_start, corr = load_clip(images, "rgb24")
    assert (tm_w, tm_h) == (6, 4) and np.array_equal(got, frames)
    want_corr = interframe_correlation(frames, 6, 4)
    assert corr.dtype == np.float64 and np.array_equal(corr.view(np.uint64), want_corr.view(np.uint64))
    want_kf, want_start, _ = detect_keyframes(frames, 6, 4)
    assert np.array_equal(kf_of, want_kf) and np.array_equal(kf_start, want_start) and kf_start[-1] == 40
    one = load_clip(images[:1], "rgb24")
    assert np.array_equal(one[0], frames[:1]) and one[3].tolist() == [0] and one[5].size == 0


def test_load_and_dither_raster(gpu):
    """Pictures in, a Video out: the same Video as load_and_dither over frames_to_tiles' frames, which are the
    oracle's; and the first pictures back out of an Encoder over it through render_raster."""
    from tiler_amd.encoder import Encoder, load_and_dither, load_and_dither_raster
    from tiler_amd.load import frames_to_tiles
    rng = np.random.default_rng(8)
    base = synth.keyframe_frames(rng, 3, 4, 0.3)
    images = store_ref(base, 2, 2, "bgr24")
    frames, tm_w, tm_h = frames_to_tiles(images, "bgr24")
    assert (tm_w, tm_h) == (2, 2) and np.array_equal(frames, load_ref(images, "bgr24")[0])
    assert np.array_equal(frames, base)
    v = load_and_dither_raster(images, "bgr24", n_palettes=2)
    w = load_and_dither(frames, tm_w, tm_h, n_palettes=2)
    for name in ("frame_rgb", "kf_start", "palettes", "centroids", "palpix", "thm", "tvm", "dith_pal"):
        a, b = np.asarray(getattr(v, name)), np.asarray(getattr(w, name))
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    enc = Encoder(v)
    rgb, invalid = enc.render()
    pics, inv2 = enc.render_raster("bgra32", width=16, height=16)
    assert np.array_equal(pics, store_ref(rgb, 2, 2, "bgra32")) and np.array_equal(inv2, invalid)
    with pytest.raises(ValueError):
        enc.render_raster(width=24, height=16)


def test_player_raster_is_ingest_input(gpu):
    """Playback meets ingest: the GTM player's raster (int32 0xAABBGGRR = RGBA32 bytes) through frames_to_tiles is
    the player's own tile-major output with the alpha byte masked off.  The stream is one gtm.save_stream writes from
    a seeded clip (tests/gtm_cases.py, as tests/test_gpu_gtm_play.py uses): the reference's demo streams named by
    tests/golden/gtm_demo.json are not in the tree."""
    from tiler_amd.load import frames_to_tiles
    W, H = 7, 5
    data, _ = written_stream(5, W * 8, H * 8, 50, 3, [0, 3, 6, 9])
    with gtm.Stream(data) as st:
        raster, _ = st.play(layout="raster")
        st.rewind()
        tiles, _ = st.play(layout="tiles")
    assert raster.shape == (9, H * 8, W * 8) and (raster >> 24).any()
    pics = np.ascontiguousarray(raster).view(np.uint8).reshape(9, H * 8, W * 8, 4)
    got, tm_w, tm_h = frames_to_tiles(pics, "rgba32")
    assert (tm_w, tm_h) == (W, H)
    assert np.array_equal(got, (tiles & 0x00FFFFFF).astype(np.int32))
