"""Input scaling, host side (no GPU): the restatement tests/resample_ref.py against Pillow's 8-bit
Image.resize(size, Image.LANCZOS) byte for byte; the library's tap tables (tiler_scale_coeffs, host code) against the
restatement's, exactly; tiler_scale_dims and its refusals; the scaled entry points' refusals, which are made before
anything touches a device."""
import ctypes

import numpy as np
import pytest

import tiler_amd
from resample_ref import FACTORS, coeffs, resize, scale_dims
from scale_cases import GPU_SIZES, check_argument_errors
from tiler_amd._lib import TilerError

PIL_SHAPES = [(64, 48, 32, 24), (37, 29, 16, 8), (50, 40, 75, 60), (33, 17, 8, 8), (100, 9, 24, 8), (41, 41, 40, 40),
              (16, 16, 16, 8), (30, 20, 45, 20), (3, 3, 8, 8), (200, 120, 17, 9)]


def _pil(img, out_w, out_h):
    Image = pytest.importorskip("PIL.Image")
    mode = {3: "RGB", 4: "RGBX"}[img.shape[2]]  # RGBX: four plain channels (RGBA would be premultiplied)
    pic = Image.frombytes(mode, (img.shape[1], img.shape[0]), np.ascontiguousarray(img).tobytes())
    return np.asarray(pic.resize((out_w, out_h), Image.LANCZOS))


@pytest.mark.parametrize("W, H, out_w, out_h", PIL_SHAPES)
def test_restatement_is_pillow(W, H, out_w, out_h):
    rng = np.random.default_rng(W * 1000 + H)
    for C in (3, 4):
        img = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
        got = resize(img, out_w, out_h)
        assert got.shape == (out_h, out_w, C) and np.array_equal(got, _pil(img, out_w, out_h))


def _patterns(W, H):
    """0 / 255 checkerboards (1- and 2-pixel squares), and single-pixel impulses on black and on white: the
    overshoot clips at both ends, and the 8-bit picture between the passes matters."""
    jj, ii = np.mgrid[0:H, 0:W]
    out = []
    for cell in (1, 2):
        board = ((((ii // cell) + (jj // cell)) & 1) * 255).astype(np.uint8)
        out.append(np.stack([board, 255 - board, board], 2))
    for bg, fg in ((0, 255), (255, 0)):
        img = np.full((H, W, 3), bg, np.uint8)
        for (y, x) in ((0, 0), (H // 2, W // 2), (H - 1, W - 1), (1, W - 2)):
            img[y, x] = fg
        out.append(img)
    return out


@pytest.mark.parametrize("W, H, out_w, out_h", [(37, 29, 18, 14), (24, 16, 36, 24), (32, 32, 12, 20)])
def test_restatement_is_pillow_on_patterns(W, H, out_w, out_h):
    clipped_low = clipped_high = False
    for img in _patterns(W, H):
        got = resize(img, out_w, out_h)
        assert np.array_equal(got, _pil(img, out_w, out_h))
        clipped_low |= bool((got == 0).any())
        clipped_high |= bool((got == 255).any())
    assert clipped_low and clipped_high


def test_kept_rectangle_is_the_whole_resize():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (45, 67, 3), dtype=np.uint8)
    assert np.array_equal(resize(img, 33, 22, 32, 16), resize(img, 33, 22)[:16, :32])
    assert np.array_equal(resize(img, 67, 22, 64, 16), resize(img, 67, 22)[:16, :64])


def _lib_coeffs(n_in, n_out):
    lib = tiler_amd.load()
    ksize = lib.tiler_scale_coeffs(n_in, n_out, None, None, 0)
    assert ksize > 0, tiler_amd.last_error()
    bounds = np.full((n_out, 2), -1, np.int32)
    taps = np.full((n_out, ksize), -1, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.tiler_scale_coeffs(n_in, n_out, p(bounds), p(taps), taps.size) == ksize
    return bounds, taps, ksize


def _axis_pairs():
    pairs = set()
    for (W, H, ow, oh) in GPU_SIZES:
        pairs |= {(W, ow), (H, oh)}
    for n in (8, 9, 67, 968, 3840):
        for f in FACTORS:
            pairs.add((n, int(np.floor(n * f))))
    return sorted(pairs)


@pytest.mark.parametrize("n_in, n_out", _axis_pairs())
def test_library_taps_are_the_restatement(n_in, n_out):
    bounds, taps, ksize = _lib_coeffs(n_in, n_out)
    wb, wt, wk = coeffs(n_in, n_out)
    assert ksize == wk and np.array_equal(bounds, wb) and np.array_equal(taps, wt)
    assert (taps.sum(1) > (1 << 22) - ksize).all() and (taps.sum(1) < (1 << 22) + ksize).all()


def test_scale_coeffs_refusals():
    lib = tiler_amd.load()
    b, t = np.zeros((8, 2), np.int32), np.full((8, 13), -1, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.tiler_scale_coeffs(16, 8, p(b), p(t), 8 * 13) == 13
    for args, word in [((0, 8, p(b), p(t), 104), "in is"), ((16, 0, p(b), p(t), 104), "out is"),
                       ((16, 8, p(b), p(t), 103), "cap"), ((16, 8, p(b), None, 104), "together"),
                       ((1 << 25, 8, None, None, 0), "in is")]:
        assert lib.tiler_scale_coeffs(*args) == -1
        assert word in tiler_amd.last_error() and "tiler_scale_coeffs:" in tiler_amd.last_error()


@pytest.mark.parametrize("f", FACTORS)
def test_scale_dims(f):
    from tiler_amd.load import scale_dims as lib_dims
    for (w, h) in ((3840, 2160), (1920, 1080), (67, 45), (131, 70), (968, 16), (40, 200)):
        want = scale_dims(w, h, f)
        if min(want) < 8:
            with pytest.raises(TilerError, match="below 8"):
                lib_dims(w, h, f)
        else:
            assert lib_dims(w, h, f) == want == (int(w * f), int(h * f))
    assert lib_dims(3840, 2160, 0.5) == (1920, 1080) and lib_dims(67, 45, 0.375) == (25, 16)


def test_scale_dims_refusals():
    lib = tiler_amd.load()
    w, h = ctypes.c_int(-7), ctypes.c_int(-7)
    for scale, word in [(0.0, "finite and positive"), (-0.5, "finite and positive"),
                        (float("nan"), "finite and positive"), (float("inf"), "finite and positive"),
                        (-float("inf"), "finite and positive"), (0.1, "below 8"), (9.0, "above 16384")]:
        assert lib.tiler_scale_dims(1920, 40, scale, ctypes.byref(w), ctypes.byref(h)) == -1, scale
        assert word in tiler_amd.last_error() and "tiler_scale_dims:" in tiler_amd.last_error()
    assert (w.value, h.value) == (-7, -7)
    assert lib.tiler_scale_dims(8192, 8192, 2.0, None, None) == 0  # 16384 is the maximum itself
    assert lib.tiler_scale_dims(8193, 64, 2.0, None, None) == -1


def test_scaled_entry_points_refuse_before_the_device():
    check_argument_errors(tiler_amd.load(), tiler_amd.last_error)


def test_scale_keywords():
    from tiler_amd.load import _out_size
    assert _out_size(67, 45, None, None) == (67, 45) and _out_size(67, 45, 0.5, None) == (33, 22)
    assert _out_size(67, 45, None, (40, 30)) == (40, 30)
    with pytest.raises(ValueError):
        _out_size(67, 45, 0.5, (33, 22))
