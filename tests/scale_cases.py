"""What the two scaling test files share: the (W, H, out_w, out_h) sizes the GPU tests run, the expected frames of a
scaled load (tests/resample_ref.py, then tests/load_ref.py), and the walk over the scaled entry points' refusals."""
import ctypes
import functools

import numpy as np

from load_ref import load_dims, load_ref
from resample_ref import FACTORS, resize_clip, scale_dims

NON_UNIT = tuple(f for f in FACTORS if f != 1.0)
FACTOR_SIZES = ((67, 45), (131, 70))

# every (W, H, out_w, out_h) of tests/test_gpu_scale_load.py
GPU_SIZES = tuple((w, h) + scale_dims(w, h, f) for (w, h) in FACTOR_SIZES for f in NON_UNIT) + (
    (64, 48, 64, 24), (64, 48, 32, 48),                         # one axis only
    (41, 29, 20, 14),                                           # strides and byte phases
    (528, 24, 264, 12), (40, 200, 15, 75), (24, 24, 48, 48),    # seams
    (968, 16, 1936, 32), (16, 548, 32, 1096),                   # the cap
    (37, 29, 18, 14), (24, 16, 36, 24),                         # checkerboards and impulses
    (48, 32, 24, 16),                                           # chunked host staging
    (40, 24, 20, 12),                                           # load_clip
)

ORDER = {"rgb24": (0, 1, 2), "bgr24": (2, 1, 0), "bgra32": (2, 1, 0, 3), "rgba32": (0, 1, 2, 3)}


def as_format(rgbx, fmt):
    """uint8 [..][4] R,G,B,X -> the same pictures in fmt's byte order."""
    return np.ascontiguousarray(rgbx[..., list(ORDER[fmt])])


def want_frames(rgb, out_w, out_h):
    """The oracle of a scaled load: uint8 [F][H][W][3] R,G,B -> (frames, tm_w, tm_h)."""
    tm_w, tm_h = load_dims(out_w, out_h)
    return load_ref(resize_clip(rgb, out_w, out_h, tm_w * 8, tm_h * 8), "rgb24")


@functools.lru_cache(maxsize=None)
def random_case(W, H, out_w, out_h, F=2):
    """(rgbx uint8 [F][H][W][4], expected frames) of a seeded random clip; computed once, read-only."""
    rng = np.random.default_rng(W * 7919 + H * 31 + out_w)
    rgbx = rng.integers(0, 256, (F, H, W, 4), dtype=np.uint8)
    want = want_frames(rgbx[..., :3], out_w, out_h)[0]
    rgbx.setflags(write=False)
    want.setflags(write=False)
    return rgbx, want


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def check_argument_errors(lib, last_error):
    """Every documented refusal of the three scaled entry points: -1, the message names the entry point and the
    argument, and the output array is untouched (the checks come before anything is launched)."""
    W, H, F = 64, 32, 2
    src = np.zeros((F, H, W, 3), np.uint8)
    rgb = np.full((F, 4 * 2, 64), 0x5A5A5A5A, np.int32)
    corr, kf = np.zeros(1), np.full(2, -7, np.int32)
    pitch, fs = W * 3, H * W * 3
    ok = dict(src=_p(src), fmt=0, F=F, w=W, h=H, pitch=pitch, fs=fs, ow=32, oh=16, rgb=_p(rgb))
    cases = [
        (dict(fmt=4), "fmt"), (dict(fmt=-1), "fmt"), (dict(F=-1), "F is negative"), (dict(w=7), "at least 8"),
        (dict(pitch=pitch - 1), "pitch"), (dict(fs=fs - 1), "frame_stride"), (dict(src=None), "src is null"),
        (dict(rgb=None), "rgb is null"),
        (dict(ow=7), "out_w"), (dict(oh=7), "out_h"), (dict(ow=16385), "out_w"), (dict(oh=16385), "out_h"),
        (dict(ow=0), "out_w"), (dict(oh=-3), "out_h"),
        (dict(w=72, pitch=72 * 3, fs=72 * 3 * H, ow=8), "out_w"),   # 72 > 8 * 8
        (dict(h=72, fs=72 * pitch, oh=8), "out_h"),
    ]
    names = ("src", "fmt", "F", "w", "h", "pitch", "fs", "ow", "oh", "rgb")
    for change, word in cases:
        a = [dict(ok, **change)[k] for k in names]
        assert lib.tiler_load_frames_scaled(*a) == -1, word
        assert word in last_error() and "tiler_load_frames_scaled:" in last_error(), (word, last_error())
        assert lib.tiler_load_frames_scaled_dev(*a, None) == -1, word
        assert word in last_error() and "tiler_load_frames_scaled_dev:" in last_error(), (word, last_error())
        assert lib.tiler_load_clip_scaled_dev(*a, _p(corr), _p(kf), None) == -1, word
        assert word in last_error() and "tiler_load_clip_scaled_dev:" in last_error(), (word, last_error())
    a = [ok[k] for k in names]
    mis = ctypes.c_void_p((rgb.ctypes.data & ~15) + 4)
    assert lib.tiler_load_frames_scaled_dev(*a[:-1], mis, None) == -1 and "16-byte aligned" in last_error()
    assert lib.tiler_load_clip_scaled_dev(*a[:-1], mis, _p(corr), _p(kf), None) == -1
    assert "16-byte aligned" in last_error()
    al = ctypes.c_void_p(rgb.ctypes.data & ~15)
    assert lib.tiler_load_clip_scaled_dev(*a[:-1], al, _p(corr), None, None) == -1 and "kf_of_frame" in last_error()
    assert lib.tiler_load_clip_scaled_dev(*a[:-1], al, None, _p(kf), None) == -1 and "corr" in last_error()
    assert (rgb == 0x5A5A5A5A).all() and (kf == -7).all()
    # F = 0 does nothing, with no arrays and no device
    z = [None, 0, 0, W, H, pitch, fs, 32, 16, None]
    assert lib.tiler_load_frames_scaled(*z) == 0 and lib.tiler_load_frames_scaled_dev(*z, None) == 0
    assert lib.tiler_load_clip_scaled_dev(*z, None, None, None) == 0
