"""Plain Python / numpy restatement of the 8-bit Lanczos resize the Load step's input scaling is pinned to (Pillow's
Image.resize(size, Image.LANCZOS); tests/test_scale_host.py holds the two together byte for byte): the oracle of the
scaling tests.  One pass per axis, the horizontal one first, a pass skipped when its axis keeps its size, the picture
between the passes 8-bit and clipped.  The taps are built in double with math.sin, the libm the library's host code
uses; nothing here comes from tiler_amd."""
import math

import numpy as np

PRECISION_BITS = 22
FACTORS = (0.25, 0.375, 0.5, 0.75, 1.0, 1.5, 2.0)  # cbxScaling (main.lfm:524-545)


def scale_dims(src_w, src_h, scale):
    """out = floor(src * scale) per axis (exact for the seven factors, multiples of 1/8)."""
    return int(math.floor(src_w * scale)), int(math.floor(src_h * scale))


def _sinc(t):
    if t == 0.0:
        return 1.0
    t = t * math.pi
    return math.sin(t) / t


def _lanczos(t):
    return _sinc(t) * _sinc(t / 3.0) if -3.0 <= t < 3.0 else 0.0


def coeffs(n_in, n_out):
    """(bounds int32 [n_out][2] = (xmin, xmax), taps int32 [n_out][ksize], ksize) of one axis; the taps past xmax
    are 0."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    taps = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_lanczos((x + xmin - center + 0.5) / fs) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            taps[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
    return bounds, taps, ksize


def _pass(img, n_out, n_keep=None):
    """Filter axis 0 of uint8 img [n_in][...] to n_out samples; only the first n_keep are computed and returned."""
    n_in = img.shape[0]
    bounds, taps, _ = coeffs(n_in, n_out)
    n_keep = n_out if n_keep is None else n_keep
    out = np.empty((n_keep,) + img.shape[1:], np.uint8)
    src = img.astype(np.int64)
    for xx in range(n_keep):
        xmin, xmax = bounds[xx]
        k = taps[xx, :xmax].astype(np.int64)
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, src[xmin:xmin + xmax], axes=(0, 0))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img, out_w, out_h, keep_w=None, keep_h=None):
    """uint8 img [H][W][C] -> [out_h][out_w][C]; with keep_w / keep_h only the top-left keep_w x keep_h pixels of
    that result (every output pixel is independent, so they are the same pixels)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    H, W, _ = img.shape
    keep_w = out_w if keep_w is None else keep_w
    keep_h = out_h if keep_h is None else keep_h
    if out_w != W:
        img = _pass(img.transpose(1, 0, 2), out_w, keep_w).transpose(1, 0, 2)
    else:
        img = img[:, :keep_w]
    if out_h != H:
        img = _pass(img, out_h, keep_h)
    else:
        img = img[:keep_h]
    return np.ascontiguousarray(img)


def resize_clip(images, out_w, out_h, keep_w=None, keep_h=None):
    """resize over uint8 [F][H][W][C]."""
    return np.stack([resize(im, out_w, out_h, keep_w, keep_h) for im in np.asarray(images)])
