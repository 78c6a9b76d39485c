"""numpy restatement of LoadFrame + ReframeUI (main.pas:3211-3286, 1931-1938), written from main.pas: the oracle of
the raster-ingest tests.  A plain per-format byte pick, the crop, the cap and the tile index formula; nothing here
comes from tiler_amd (one test pins it against synth.screen_to_tiles)."""
import numpy as np

# byte position of R, G, B inside a pixel, and bytes per pixel
FORMATS = {"rgb24": ((0, 1, 2), 3), "bgr24": ((2, 1, 0), 3), "bgra32": ((2, 1, 0), 4), "rgba32": ((0, 1, 2), 4)}


def load_dims(src_w, src_h):
    """ReframeUI: FTileMapWidth = min(AWidth, 1920 div 8) over AWidth = width div 8, likewise the height."""
    if src_w < 8 or src_h < 8:
        raise ValueError("picture smaller than one tile")
    return min(src_w // 8, 1920 // 8), min(src_h // 8, 1080 // 8)


def load_ref(images, fmt="rgb24"):
    """images uint8 [F][H][W][bpp] (or [H][W][bpp]) -> (frames [F][tm_h * tm_w][64] int32 0x00BBGGRR, tm_w, tm_h).
    Pixel (i, j) of the top-left tm_w*8 x tm_h*8 rectangle goes to tile tm_w * (j div 8) + (i div 8), element
    (j and 7) * 8 + (i and 7) (main.pas:3252-3258) as ToRGB(r, g, b) = b shl 16 or g shl 8 or r."""
    (ri, gi, bi), bpp = FORMATS[fmt]
    images = np.asarray(images)
    if images.ndim == 3:
        images = images[None]
    F, H, W, C = images.shape
    assert C == bpp and images.dtype == np.uint8
    tm_w, tm_h = load_dims(W, H)
    frames = np.zeros((F, tm_w * tm_h, 64), np.int32)
    jj, ii = np.mgrid[0:tm_h * 8, 0:tm_w * 8]
    ti = tm_w * (jj // 8) + (ii // 8)
    el = (jj & 7) * 8 + (ii & 7)
    px = images[:, :tm_h * 8, :tm_w * 8].astype(np.int32)
    frames[:, ti, el] = (px[..., bi] << 16) | (px[..., gi] << 8) | px[..., ri]
    return frames, tm_w, tm_h


def store_ref(frames, tm_w, tm_h, fmt="rgb24"):
    """The inverse: pictures uint8 [F][tm_h*8][tm_w*8][bpp] of tile-major frames, X = 0xFF."""
    (ri, gi, bi), bpp = FORMATS[fmt]
    frames = np.asarray(frames).reshape(-1, tm_w * tm_h, 64).astype(np.int64)
    jj, ii = np.mgrid[0:tm_h * 8, 0:tm_w * 8]
    c = frames[:, tm_w * (jj // 8) + (ii // 8), (jj & 7) * 8 + (ii & 7)]
    out = np.full(c.shape + (bpp,), 0xFF, np.uint8)
    out[..., ri] = c & 255
    out[..., gi] = (c >> 8) & 255
    out[..., bi] = (c >> 16) & 255
    return out
