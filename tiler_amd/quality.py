"""Quality readout on libANN.so: Render's destination frame (main.pas:3305-3493) from the tilemaps, and the figure
Render prints under it, lblCorrel = ComputeCorrelationBGR(source, destination) (main.pas:769-788, 3470-3489),
plus the exact per-channel SSE and the PSNR derived from it.

Frames are what FrameTiling and keyframe detection take: [F][tm_h*tm_w][64] int32 0x00BBGGRR tiles, so source and
rendered frames are directly comparable.  Drawing the bitmaps (the UI part of Render) stays out of scope.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import check, load


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _vp(d):
    return ctypes.c_void_p(int(d)) if d else None


def _dims(tm_w, tm_h):
    tm_w, tm_h = int(tm_w), int(tm_h)
    if tm_w <= 0 or tm_h <= 0 or tm_w * tm_h > (1 << 24):
        raise ValueError("quality: tm_w, tm_h must be positive with tm_w * tm_h <= 2^24")
    return tm_w, tm_h


def _sm_all_or_none(given):
    n = sum(bool(g) for g in given)
    if n not in (0, 5):
        raise ValueError("render: sm_tile, sm_pal, sm_hm, sm_vm and smoothed come together or not at all")
    return n == 5


def _render_scalars(F, Q, T, n_rows, palsize, n_palettes):
    if F < 0 or Q <= 0 or T < 0 or n_rows < 0 or n_palettes < 0:
        raise ValueError("render: negative size (or Q = 0)")
    if not 0 < palsize <= 256:
        raise ValueError("render: palsize must be in 1..256")


def render_frames(tile, pal, hm, vm, palpix, thm, tvm, palettes, pal_row0, n_palettes: int, sm_tile=None,
                  sm_pal=None, sm_hm=None, sm_vm=None, smoothed=None):
    """Render (main.pas:3305-3493; dithered, reduced, mirrored, palIdx < 0) of F frames, host arrays.

    tile/pal/hm/vm [F][Q] the TileMap items, sm_* / smoothed [F][Q] the SmoothedTileMap (all None: no Smooth was
    run); palpix [T][64], thm/tvm [T]; palettes [R][palsize] (0x00BBGGRR); pal_row0 [F] the row of palette 0 of each
    frame's keyframe; n_palettes per keyframe.  Returns (rgb [F][Q][64] int32 tile-major, invalid [F] int32: the
    positions whose tile or palette is out of range, rendered 0)."""
    tile = np.asarray(tile)
    if tile.ndim != 2:
        raise ValueError("render: items are [F][Q] arrays")
    F, Q = tile.shape
    has_sm = _sm_all_or_none([a is not None for a in (sm_tile, sm_pal, sm_hm, sm_vm, smoothed)])
    palettes = np.asarray(palettes)
    if palettes.ndim != 2:
        raise ValueError("render: palettes is [R][palsize]")
    palpix = np.asarray(palpix)
    if palpix.size % 64:
        raise ValueError("render: palpix is [T][64]")
    T = palpix.size // 64
    _render_scalars(F, Q, T, palettes.shape[0], palettes.shape[1], int(n_palettes))

    def items(a, dt, what):
        a = np.asarray(a)
        if a.shape != (F, Q):
            raise ValueError(f"render: {what} must have shape {(F, Q)}, not {a.shape}")
        if dt == np.int32 and a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 31)):
            raise ValueError(f"render: {what} does not fit int32")
        return np.ascontiguousarray(a, dt)

    tile, pal = items(tile, np.int32, "tile"), items(pal, np.int32, "pal")
    hm, vm = items(hm, np.uint8, "hm"), items(vm, np.uint8, "vm")
    if has_sm:
        sm_tile, sm_pal = items(sm_tile, np.int32, "sm_tile"), items(sm_pal, np.int32, "sm_pal")
        sm_hm, sm_vm = items(sm_hm, np.uint8, "sm_hm"), items(sm_vm, np.uint8, "sm_vm")
        smoothed = items(smoothed, np.uint8, "smoothed")
    thm, tvm = np.ascontiguousarray(thm, np.uint8).ravel(), np.ascontiguousarray(tvm, np.uint8).ravel()
    if thm.size != T or tvm.size != T:
        raise ValueError("render: thm / tvm must have one flag per tile")
    pal_row0 = np.ascontiguousarray(pal_row0, np.int32).ravel()
    if pal_row0.size != F:
        raise ValueError("render: pal_row0 must have one row per frame")
    palpix = np.ascontiguousarray(palpix, np.uint8).reshape(T, 64)
    palettes = np.ascontiguousarray(palettes, np.int32)
    out = np.zeros((F, Q, 64), np.int32)
    invalid = np.zeros(F, np.int32)
    check(load().tiler_render_frames(F, Q, _p(tile), _p(pal), _p(hm), _p(vm), _p(sm_tile), _p(sm_pal), _p(sm_hm),
                                     _p(sm_vm), _p(smoothed), T, _p(palpix), _p(thm), _p(tvm), palettes.shape[0],
                                     palettes.shape[1], _p(palettes), _p(pal_row0), int(n_palettes), _p(out),
                                     _p(invalid)), "tiler_render_frames")
    return out, invalid


def render_frames_dev(F: int, Q: int, d_tile: int, d_pal: int, d_hm: int, d_vm: int, T: int, d_palpix: int,
                      d_thm: int, d_tvm: int, n_rows: int, palsize: int, d_palettes: int, d_pal_row0: int,
                      n_palettes: int, d_out_rgb: int, d_invalid: int = 0, d_sm_tile: int = 0, d_sm_pal: int = 0,
                      d_sm_hm: int = 0, d_sm_vm: int = 0, d_smoothed: int = 0, stream=None) -> None:
    """Same with every array resident in HBM (device pointers; int32 items, uint8 flags); asynchronous on `stream`."""
    F, Q, T, n_rows, palsize, n_palettes = (int(x) for x in (F, Q, T, n_rows, palsize, n_palettes))
    _render_scalars(F, Q, T, n_rows, palsize, n_palettes)
    _sm_all_or_none((d_sm_tile, d_sm_pal, d_sm_hm, d_sm_vm, d_smoothed))
    if F and not (d_tile and d_pal and d_hm and d_vm and d_pal_row0 and d_out_rgb):
        raise ValueError("render: null device pointer")
    if int(d_out_rgb) % 16 or int(d_palpix or 0) % 4:
        raise ValueError("render: out_rgb must be 16-byte and palpix 4-byte aligned")
    check(load().tiler_render_frames_dev(F, Q, _vp(d_tile), _vp(d_pal), _vp(d_hm), _vp(d_vm), _vp(d_sm_tile),
                                         _vp(d_sm_pal), _vp(d_sm_hm), _vp(d_sm_vm), _vp(d_smoothed), T, _vp(d_palpix),
                                         _vp(d_thm), _vp(d_tvm), n_rows, palsize, _vp(d_palettes), _vp(d_pal_row0),
                                         n_palettes, _vp(d_out_rgb), _vp(d_invalid), _vp(stream)),
          "tiler_render_frames_dev")


def frame_quality(src, dst, tm_w: int, tm_h: int):
    """(corr [F] float64, sse [F][3] uint64) of source frames against rendered frames, host arrays
    [F][tm_h*tm_w][64] int32 0x00BBGGRR.  corr[f] is bit-identical to the reference's ComputeCorrelationBGR over
    the raster + transposed copies (main.pas:3470-3489); sse[f] the exact squared error of the R, G, B bytes."""
    tm_w, tm_h = _dims(tm_w, tm_h)
    fs = tm_w * tm_h * 64
    src, dst = np.asarray(src), np.asarray(dst)
    if src.size % fs or dst.size % fs or src.size != dst.size:
        raise ValueError("quality: src and dst must both be [F][tm_h*tm_w][64]")
    src = np.ascontiguousarray(src, np.int32).reshape(-1, fs)
    dst = np.ascontiguousarray(dst, np.int32).reshape(-1, fs)
    F = src.shape[0]
    corr = np.zeros(F, np.float64)
    sse = np.zeros((F, 3), np.uint64)
    check(load().tiler_frame_quality(_p(src), _p(dst), F, tm_w, tm_h, _p(corr), _p(sse)), "tiler_frame_quality")
    return corr, sse


def frame_quality_dev(d_src: int, d_dst: int, F: int, tm_w: int, tm_h: int, stream=None):
    """Same with the frames resident in HBM (device pointers, 16-byte aligned), synchronous on `stream`."""
    tm_w, tm_h = _dims(tm_w, tm_h)
    F = int(F)
    if F < 0 or (F and not (d_src and d_dst)):
        raise ValueError("quality: negative frame count or null device pointer")
    if int(d_src or 0) % 16 or int(d_dst or 0) % 16:
        raise ValueError("quality: frames must be 16-byte aligned")
    corr = np.zeros(F, np.float64)
    sse = np.zeros((F, 3), np.uint64)
    check(load().tiler_frame_quality_dev(_vp(d_src), _vp(d_dst), F, tm_w, tm_h, _p(corr), _p(sse), _vp(stream)),
          "tiler_frame_quality_dev")
    return corr, sse


def psnr(sse, tm_w: int, tm_h: int) -> np.ndarray:
    """10 log10(255^2 * 3 W H / Σ_c sse) per frame (host), inf where the frames are equal."""
    tm_w, tm_h = _dims(tm_w, tm_h)
    sse = np.asarray(sse)
    if sse.shape[-1:] != (3,):
        raise ValueError("psnr: sse is [F][3]")
    tot = sse.astype(np.uint64).sum(axis=-1).astype(np.float64)
    peak = 255.0 * 255.0 * 3.0 * (64 * tm_w * tm_h)
    with np.errstate(divide="ignore"):
        return np.where(tot == 0, np.inf, 10.0 * np.log10(peak / np.where(tot == 0, 1.0, tot)))
