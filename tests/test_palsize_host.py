"""CPU tests for palette sizes 32 and 64: the stride-16 view of the restatement (palsize_ref.py) against per-tile
or_psyv, which takes the palette's own pointer; the Encoder's palette-size check; the new C ABI names."""
import subprocess

import numpy as np
import pytest

import palsize_ref
from tiler_amd import _lib, synth
from tiler_amd.encoder import Encoder
from tiler_amd.psyv import palette_rows

PS_SYMBOLS = ["tiler_psyv_batch_ps", "tiler_psyv_batch_ps_dev", "tiler_prepare_frame_tiling_ps_dev",
              "tiler_smooth_keyframe_ps", "tiler_smooth_keyframe_ps_dev"]


@pytest.mark.parametrize("size", [32, 64])
@pytest.mark.parametrize("flags,gamma", [(1 | 2, -1), (1, 0), (1 | 8 | 16, -1), (1 | 2 | 32, 0)])
def test_stride_trick_equals_per_tile_psyv(oracle, size, flags, gamma):
    """or_psyv_batch over the [k P][16] view with palette indices times k equals or_psyv tile by tile with the
    palette's own 32 / 64 entries, bit for bit; the last entry of the first and the last palette are read."""
    rng = np.random.default_rng(size + flags)
    n, P = 24, 3
    pals = synth.palettes(rng, P, size).astype(np.int32)
    pp = rng.integers(0, size, (n, 64)).astype(np.uint8)
    pal_of = rng.integers(0, P, n).astype(np.int32)
    pp[0], pal_of[0] = size - 1, 0
    pp[1], pal_of[1] = size - 1, P - 1
    got = palsize_ref.psyv_batch(oracle, n, pp, pals, pal_of, flags=flags, gamma=gamma)
    for i in range(n):
        one = oracle.psyv(palpix=pp[i], pal=pals[pal_of[i]], flags=flags, gamma=gamma)
        assert np.array_equal(got[i].view(np.uint64), one.view(np.uint64)), i
    assert not np.array_equal(got[0], got[1])  # the two palettes' last colours differ


def test_palette_rows_takes_the_last_dimension():
    assert palette_rows(np.zeros((3, 64), np.int32)).shape == (3, 64)
    assert palette_rows(np.zeros((2, 3, 32), np.int32)).shape == (6, 32)
    assert palette_rows(np.zeros(48, np.int32)).shape == (3, 16)
    assert palette_rows(np.zeros(64, np.int32), 32).shape == (2, 32)
    with pytest.raises(ValueError):
        palette_rows(np.zeros((3, 64), np.int32), 16)


def test_palette_centroids_any_size():
    rng = np.random.default_rng(5)
    for size in (16, 32, 64):
        c = synth.palette_centroids(synth.palettes(rng, 4, size))
        assert c.shape == (4, 192) and np.isfinite(c).all()
    p16 = synth.palettes(rng, 2, 16)
    assert np.array_equal(synth.palette_centroids(p16), synth.palette_centroids(p16.reshape(-1)))


def test_encoder_palsize_must_match_the_palettes():
    v = synth.video(3, 32, 24, kf_frames=(2, 2), n_palettes=2)
    assert Encoder(v).palsize == 16 and Encoder(v, palsize=16).palsize == 16
    with pytest.raises(ValueError, match="palsize"):
        Encoder(v, palsize=64)


def test_ps_entry_points_declared_and_exported():
    syms = _lib.header_symbols()
    for s in PS_SYMBOLS:
        assert s in syms and s in _lib._SIGS, s
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    assert not [s for s in PS_SYMBOLS if s not in exported]
