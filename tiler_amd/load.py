"""The Load step's front door on libANN.so (LoadFrame main.pas:3211-3286, ReframeUI main.pas:1931-1938): raster
pictures as a decoder leaves them -> the tile-major frames [F][tm_h*tm_w][64] int32 0x00BBGGRR every other step takes,
and those frames back to pictures.  Decoding image files / ffmpeg stays out of scope: pictures arrive in memory, in
one of four byte orders, rows and frames at any pitch.
"""
from __future__ import annotations

import ctypes
import sys
import types

import numpy as np

from ._lib import check
from ._lib import load as _load_lib
from .keyframes import keyframe_starts

FORMATS = {"rgb24": 0, "bgr24": 1, "bgra32": 2, "rgba32": 3}  # TILER_PIX_*
_BPP = {"rgb24": 3, "bgr24": 3, "bgra32": 4, "rgba32": 4}

__all__ = ["load_dims", "frames_to_tiles", "frames_to_tiles_dev", "tiles_to_frames", "tiles_to_frames_dev",
           "load_clip"]


def _fmt(fmt: str) -> int:
    if fmt not in FORMATS:
        raise ValueError(f"fmt is one of {sorted(FORMATS)}, not {fmt!r}")
    return FORMATS[fmt]


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _dp(p):
    return ctypes.c_void_p(int(p)) if p else None


def load_dims(src_w: int, src_h: int):
    """ReframeUI: (tm_w, tm_h) = (min(src_w div 8, 240), min(src_h div 8, 135))."""
    w, h = ctypes.c_int(0), ctypes.c_int(0)
    check(_load_lib().tiler_load_dims(int(src_w), int(src_h), ctypes.byref(w), ctypes.byref(h)), "tiler_load_dims")
    return w.value, h.value


def scale_dims(src_w: int, src_h: int, scale: float):
    """cbxScaling: the size ffmpeg's scale=iw*S:ih*S leaves, (floor(src_w * S), floor(src_h * S)); exact for the
    reference's seven factors 0.25, 0.375, 0.5, 0.75, 1, 1.5, 2."""
    w, h = ctypes.c_int(0), ctypes.c_int(0)
    check(_load_lib().tiler_scale_dims(int(src_w), int(src_h), float(scale), ctypes.byref(w), ctypes.byref(h)),
          "tiler_scale_dims")
    return w.value, h.value


def _out_size(src_w: int, src_h: int, scale, size):
    """The size of the resized picture from the scale= / size= keywords; neither: the source's (no scaling)."""
    if scale is not None and size is not None:
        raise ValueError("give scale or size, not both")
    if size is not None:
        return int(size[0]), int(size[1])
    if scale is not None:
        return scale_dims(src_w, src_h, scale)
    return int(src_w), int(src_h)


def _pictures(images, fmt: str):
    """images as uint8 [F][H][W][bpp] with the pixel dimensions dense; rows and frames keep their strides (no copy of
    a clip sliced out of a larger array).  Returns (array, pitch, frame_stride)."""
    a = np.asarray(images)
    if a.dtype != np.uint8:
        raise ValueError("images must be uint8")
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4 or a.shape[3] != _BPP[fmt]:
        raise ValueError(f"images must be [F][H][W][{_BPP[fmt]}] or [H][W][{_BPP[fmt]}] for {fmt}")
    F, H, W, bpp = a.shape
    dense_px = a.strides[3] == 1 and a.strides[2] == bpp
    pitch, frame_stride = a.strides[1], a.strides[0]
    if F == 1:
        frame_stride = max(frame_stride, H * pitch)  # a single picture's frame stride means nothing
    if not dense_px or pitch < W * bpp or frame_stride < H * pitch:
        a = np.ascontiguousarray(a)
        pitch, frame_stride = W * bpp, H * W * bpp
    return a, pitch, frame_stride


def frames_to_tiles(images, fmt: str = "rgb24", scale=None, size=None):
    """Pictures uint8 [F][H][W][3|4] (or one [H][W][3|4]) -> (frames [F][Q][64] int32, tm_w, tm_h): the top-left
    tm_w*8 x tm_h*8 pixels of every picture, tiled on the GPU.  The array may be non-contiguous in the row and frame
    dimensions: pitch and frame stride are its strides.  scale= (cbxScaling's factor) or size=(out_w, out_h) resizes
    the pictures first, on the GPU, as Pillow's 8-bit Image.resize(size, LANCZOS) does (tiler_load_frames_scaled)."""
    code = _fmt(fmt)
    a, pitch, frame_stride = _pictures(images, fmt)
    F, H, W, _ = a.shape
    if scale is None and size is None:
        tm_w, tm_h = load_dims(W, H)
        frames = np.empty((F, tm_w * tm_h, 64), np.int32)
        check(_load_lib().tiler_load_frames(_vp(a), code, F, W, H, pitch, frame_stride, _vp(frames)),
              "tiler_load_frames")
        return frames, tm_w, tm_h
    out_w, out_h = _out_size(W, H, scale, size)
    tm_w, tm_h = load_dims(out_w, out_h)
    frames = np.empty((F, tm_w * tm_h, 64), np.int32)
    check(_load_lib().tiler_load_frames_scaled(_vp(a), code, F, W, H, pitch, frame_stride, out_w, out_h, _vp(frames)),
          "tiler_load_frames_scaled")
    return frames, tm_w, tm_h


def frames_to_tiles_dev(d_src: int, F: int, src_w: int, src_h: int, d_rgb: int, fmt: str = "rgb24", pitch=None,
                        frame_stride=None, stream=None, scale=None, size=None):
    """Device-pointer form (ints are HBM addresses; d_rgb 16-byte aligned), asynchronous on `stream`.  pitch defaults
    to src_w * bpp, frame_stride to src_h * pitch.  scale= / size= as in frames_to_tiles
    (tiler_load_frames_scaled_dev).  Returns (tm_w, tm_h)."""
    code = _fmt(fmt)
    pitch = src_w * _BPP[fmt] if pitch is None else int(pitch)
    frame_stride = src_h * pitch if frame_stride is None else int(frame_stride)
    if scale is None and size is None:
        check(_load_lib().tiler_load_frames_dev(_dp(d_src), code, int(F), int(src_w), int(src_h), pitch, frame_stride,
                                                _dp(d_rgb), _dp(stream)), "tiler_load_frames_dev")
        return load_dims(src_w, src_h)
    out_w, out_h = _out_size(src_w, src_h, scale, size)
    check(_load_lib().tiler_load_frames_scaled_dev(_dp(d_src), code, int(F), int(src_w), int(src_h), pitch,
                                                   frame_stride, out_w, out_h, _dp(d_rgb), _dp(stream)),
          "tiler_load_frames_scaled_dev")
    return load_dims(out_w, out_h)


def tiles_to_frames(frames, tm_w: int, tm_h: int, fmt: str = "rgb24", pitch=None, out=None) -> np.ndarray:
    """Frames [F][tm_h*tm_w][64] -> pictures uint8 [F][tm_h*8][tm_w*8][3|4] (X = 0xFF).  pitch (bytes, at least a
    row's) gives padded rows: the result is then a view into a [F][tm_h*8][pitch] buffer whose padding bytes the call
    leaves as they were (`out`, when given, is that buffer)."""
    code = _fmt(fmt)
    bpp = _BPP[fmt]
    frames = np.ascontiguousarray(frames, np.int32).reshape(-1, tm_w * tm_h, 64)
    F, H, W = frames.shape[0], tm_h * 8, tm_w * 8
    pitch = W * bpp if pitch is None else int(pitch)
    if pitch < W * bpp:
        raise ValueError("pitch is below a row's bytes")
    if out is None:
        out = np.empty((F, H, pitch), np.uint8)
    if out.dtype != np.uint8 or out.shape != (F, H, pitch) or not out.flags.c_contiguous:
        raise ValueError("out must be a contiguous uint8 [F][H][pitch] buffer")
    check(_load_lib().tiler_store_frames(_vp(frames), F, tm_w, tm_h, code, _vp(out), pitch, H * pitch),
          "tiler_store_frames")
    return out[:, :, :W * bpp].reshape(F, H, W, bpp)


def tiles_to_frames_dev(d_rgb: int, F: int, tm_w: int, tm_h: int, d_dst: int, fmt: str = "rgb24", pitch=None,
                        frame_stride=None, stream=None):
    """Device-pointer form of tiles_to_frames, asynchronous on `stream`."""
    code = _fmt(fmt)
    pitch = tm_w * 8 * _BPP[fmt] if pitch is None else int(pitch)
    frame_stride = tm_h * 8 * pitch if frame_stride is None else int(frame_stride)
    check(_load_lib().tiler_store_frames_dev(_dp(d_rgb), int(F), int(tm_w), int(tm_h), code, _dp(d_dst), pitch,
                                             frame_stride, _dp(stream)), "tiler_store_frames_dev")


def load_clip(images, fmt: str = "rgb24", scale=None, size=None):
    """The Load step in one call (tiler_load_clip_dev): the pictures go to HBM once, are tiled there, and the
    inter-frame correlations and the keyframe split come from the tiles where they lie.  Returns (frames [F][Q][64]
    int32, tm_w, tm_h, kf_of_frame [F], kf_start [KF+1], corr [F-1]).  The whole clip is resident for the call; a
    clip beyond HBM goes through frames_to_tiles and keyframes.detect_keyframes instead.  scale= / size= as in
    frames_to_tiles: the correlations and the split are then those of the resized frames
    (tiler_load_clip_scaled_dev)."""
    import torch
    code = _fmt(fmt)
    a, _, _ = _pictures(images, fmt)
    F, H, W, bpp = a.shape
    out_w, out_h = _out_size(W, H, scale, size)
    tm_w, tm_h = load_dims(out_w, out_h)
    d_src = torch.from_numpy(a).cuda()  # dense on the device whatever the host strides
    d_rgb = torch.empty((F, tm_w * tm_h, 64), dtype=torch.int32, device="cuda")
    corr = np.zeros(max(0, F - 1), np.float64)
    kf = np.zeros(F, np.int32)
    torch.cuda.current_stream().synchronize()
    if scale is None and size is None:
        check(_load_lib().tiler_load_clip_dev(_dp(d_src.data_ptr()), code, F, W, H, W * bpp, H * W * bpp,
                                              _dp(d_rgb.data_ptr()), _vp(corr), _vp(kf), None), "tiler_load_clip_dev")
    else:
        check(_load_lib().tiler_load_clip_scaled_dev(_dp(d_src.data_ptr()), code, F, W, H, W * bpp, H * W * bpp,
                                                     out_w, out_h, _dp(d_rgb.data_ptr()), _vp(corr), _vp(kf), None),
              "tiler_load_clip_scaled_dev")
    return d_rgb.cpu().numpy(), tm_w, tm_h, kf, keyframe_starts(kf), corr


class _Module(types.ModuleType):
    """Importing this submodule rebinds the package attribute `tiler_amd.load`, until then the library loader that
    callers spell tiler_amd.load().  Calling the module is that loader, so the spelling keeps working."""

    def __call__(self):
        return _load_lib()


sys.modules[__name__].__class__ = _Module
