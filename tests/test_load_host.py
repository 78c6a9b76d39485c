"""Raster ingest, host side (no GPU): ReframeUI's dimensions, the argument checks of the load / store entry points --
made before anything touches a device, so they answer the same with and without one -- the numpy oracle
tests/load_ref.py against synth.screen_to_tiles, and the Python module's handling of strides."""
import ctypes

import numpy as np
import pytest

import tiler_amd
from load_ref import load_ref, store_ref
from tiler_amd import synth
from tiler_amd._lib import TilerError

RGB24, BGR24, BGRA32, RGBA32 = 0, 1, 2, 3


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("src, want", [((8, 8), (1, 1)), ((19, 13), (2, 1)), ((1920, 1080), (240, 135)),
                                       ((1936, 1096), (240, 135)), ((4096, 8), (240, 1))])
def test_load_dims(src, want):
    from tiler_amd.load import load_dims
    assert load_dims(*src) == want
    w, h = ctypes.c_int(-7), ctypes.c_int(-7)
    assert tiler_amd.load().tiler_load_dims(src[0], src[1], ctypes.byref(w), ctypes.byref(h)) == 0
    assert (w.value, h.value) == want


def test_load_dims_too_small():
    from tiler_amd.load import load_dims
    lib = tiler_amd.load()
    w, h = ctypes.c_int(-7), ctypes.c_int(-7)
    assert lib.tiler_load_dims(7, 100, ctypes.byref(w), ctypes.byref(h)) == -1
    assert "at least 8" in tiler_amd.last_error() and (w.value, h.value) == (-7, -7)
    assert lib.tiler_load_dims(100, 7, None, None) == -1
    with pytest.raises(TilerError, match="at least 8"):
        load_dims(7, 100)


def test_load_argument_errors():
    """Every refusal names its argument; the output array is untouched.  On a machine without a GPU a call that got
    past the checks would fail with the device's message instead, so the words also show the order."""
    lib = tiler_amd.load()
    W, H, F = 16, 8, 2
    src = np.zeros((F, H, W, 3), np.uint8)
    rgb = np.full((F, 2, 64), 0x5A5A5A5A, np.int32)
    pitch, fs = W * 3, H * W * 3
    cases = [
        ((_p(src), 4, F, W, H, pitch, fs, _p(rgb)), "fmt"),
        ((_p(src), -1, F, W, H, pitch, fs, _p(rgb)), "fmt"),
        ((_p(src), RGB24, -1, W, H, pitch, fs, _p(rgb)), "F is negative"),
        ((_p(src), RGB24, F, 7, H, pitch, fs, _p(rgb)), "at least 8"),
        ((_p(src), RGB24, F, W, H, pitch - 1, fs, _p(rgb)), "pitch"),
        ((_p(src), BGRA32, F, W, H, W * 4 - 1, fs, _p(rgb)), "pitch"),
        ((_p(src), RGB24, F, W, H, pitch, fs - 1, _p(rgb)), "frame_stride"),
        ((None, RGB24, F, W, H, pitch, fs, _p(rgb)), "src is null"),
        ((_p(src), RGB24, F, W, H, pitch, fs, None), "rgb is null"),
    ]
    for args, word in cases:
        assert lib.tiler_load_frames(*args) == -1, word
        assert word in tiler_amd.last_error() and "tiler_load_frames:" in tiler_amd.last_error()
        assert lib.tiler_load_frames_dev(*args, None) == -1, word
        assert word in tiler_amd.last_error() and "tiler_load_frames_dev:" in tiler_amd.last_error()
    assert (rgb == 0x5A5A5A5A).all()
    # the _dev form wants d_rgb on 16 bytes; an address is all the check reads
    base = rgb.ctypes.data
    mis = ctypes.c_void_p((base & ~15) + 4)
    assert lib.tiler_load_frames_dev(_p(src), RGB24, F, W, H, pitch, fs, mis, None) == -1
    assert "16-byte aligned" in tiler_amd.last_error()
    corr, kf = np.zeros(1), np.zeros(2, np.int32)
    assert lib.tiler_load_clip_dev(_p(src), RGB24, F, W, H, pitch, fs, mis, _p(corr), _p(kf), None) == -1
    assert "16-byte aligned" in tiler_amd.last_error()
    assert lib.tiler_load_clip_dev(_p(src), RGB24, F, W, H, pitch, fs, ctypes.c_void_p(base & ~15), _p(corr), None,
                                   None) == -1
    assert "kf_of_frame" in tiler_amd.last_error()


def test_store_argument_errors():
    lib = tiler_amd.load()
    F, tw, th = 2, 2, 1
    rgb = np.zeros((F, tw * th, 64), np.int32)
    dst = np.full((F, 8, 16, 4), 0xA5, np.uint8)
    pitch, fs = 64, 512
    cases = [
        ((_p(rgb), F, tw, th, 9, _p(dst), pitch, fs), "fmt"),
        ((_p(rgb), -2, tw, th, RGBA32, _p(dst), pitch, fs), "F is negative"),
        ((_p(rgb), F, 0, th, RGBA32, _p(dst), pitch, fs), "tm_w or tm_h"),
        ((_p(rgb), F, tw, th, RGBA32, _p(dst), pitch - 1, fs), "pitch"),
        ((_p(rgb), F, tw, th, RGBA32, _p(dst), pitch, fs - 1), "frame_stride"),
        ((None, F, tw, th, RGBA32, _p(dst), pitch, fs), "rgb is null"),
        ((_p(rgb), F, tw, th, RGBA32, None, pitch, fs), "dst is null"),
    ]
    for args, word in cases:
        assert lib.tiler_store_frames(*args) == -1, word
        assert word in tiler_amd.last_error() and "tiler_store_frames:" in tiler_amd.last_error()
        assert lib.tiler_store_frames_dev(*args, None) == -1, word
        assert word in tiler_amd.last_error()
    assert (dst == 0xA5).all()
    mis = ctypes.c_void_p((rgb.ctypes.data & ~15) + 8)
    assert lib.tiler_store_frames_dev(mis, F, tw, th, RGBA32, _p(dst), pitch, fs, None) == -1
    assert "16-byte aligned" in tiler_amd.last_error()


def test_no_frames_is_a_no_op():
    """F = 0 returns 0 from every form and needs neither arrays nor a device."""
    lib = tiler_amd.load()
    assert lib.tiler_load_frames(None, RGB24, 0, 16, 8, 48, 384, None) == 0
    assert lib.tiler_load_frames_dev(None, BGRA32, 0, 16, 8, 64, 512, None, None) == 0
    assert lib.tiler_store_frames(None, 0, 2, 1, BGR24, None, 48, 384) == 0
    assert lib.tiler_store_frames_dev(None, 0, 2, 1, RGBA32, None, 64, 512, None) == 0
    assert lib.tiler_load_clip_dev(None, RGB24, 0, 16, 8, 48, 384, None, None, None, None) == 0
    assert lib.tiler_debug_load_chunk(-1) == -1 and lib.tiler_debug_load_chunk(0) == 0


def test_load_ref_matches_screen_to_tiles():
    """The oracle, written from main.pas, against the project's own numpy helper on a picture whose sides are
    multiples of 8; and its other formats and its inverse against itself."""
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (3, 40, 72, 3), dtype=np.uint8)
    frames, tm_w, tm_h = load_ref(img, "rgb24")
    assert (tm_w, tm_h) == (9, 5)
    assert np.array_equal(frames, np.stack([synth.screen_to_tiles(p) for p in img]))
    assert np.array_equal(load_ref(img[..., ::-1], "bgr24")[0], frames)
    x = rng.integers(0, 256, (3, 40, 72, 1), dtype=np.uint8)
    assert np.array_equal(load_ref(np.concatenate([img, x], 3), "rgba32")[0], frames)
    assert np.array_equal(load_ref(np.concatenate([img[..., ::-1], x], 3), "bgra32")[0], frames)
    assert np.array_equal(store_ref(frames, tm_w, tm_h, "rgb24"), img)
    back = store_ref(frames, tm_w, tm_h, "bgra32")
    assert np.array_equal(back[..., :3], img[..., ::-1]) and (back[..., 3] == 0xFF).all()
    pic = rng.integers(0, 256, (13, 19, 3), dtype=np.uint8)  # 19 x 13: cropped to 16 x 8
    crop, cw, ch = load_ref(pic, "rgb24")
    assert (cw, ch) == (2, 1) and np.array_equal(crop[0], synth.screen_to_tiles(pic[:8, :16]))


def test_strides_are_passed_not_copied():
    """A clip sliced out of a larger array keeps its memory: pitch and frame stride are the array's strides.  Only
    pixels that are not dense (a channel slice, a column step) or rows running backwards are copied."""
    from tiler_amd.load import _pictures
    big = np.zeros((4, 40, 100, 3), np.uint8)
    a, pitch, fs = _pictures(big[:, 3:27, 5:45], "rgb24")
    assert np.shares_memory(a, big) and (pitch, fs) == (300, 12000) and a.shape == (4, 24, 40, 3)
    a, pitch, fs = _pictures(big[1, :16, :8], "rgb24")
    assert np.shares_memory(a, big) and a.shape == (1, 16, 8, 3) and pitch == 300 and fs >= 16 * 300
    a, pitch, fs = _pictures(big[:, :, ::2], "rgb24")
    assert not np.shares_memory(a, big) and (pitch, fs) == (150, 6000)
    a, pitch, fs = _pictures(big[:, ::-1], "rgb24")
    assert not np.shares_memory(a, big) and (pitch, fs) == (300, 12000)
    with pytest.raises(ValueError):
        _pictures(big, "bgra32")
    with pytest.raises(ValueError):
        _pictures(big.astype(np.int32), "rgb24")


def test_package_loader_survives_the_submodule():
    """tiler_amd.load is the library loader; importing the submodule tiler_amd.load rebinds that name, and the module
    stays callable as the loader."""
    import tiler_amd.load as mod
    assert tiler_amd.load() is tiler_amd._lib.load() and mod() is tiler_amd._lib.load()
    assert sorted(mod.__all__) == ["frames_to_tiles", "frames_to_tiles_dev", "load_clip", "load_dims",
                                   "tiles_to_frames", "tiles_to_frames_dev"]
