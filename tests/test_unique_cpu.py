"""CPU tests around the GPU MakeTilesUnique (tiler_make_tiles_unique): the entry point refuses without a device instead
of computing on the host, and an Encoder without gpu_unique keeps the host path."""
import ctypes

import numpy as np
import pytest

import tiler_amd
from tiler_amd import global_tiling as gt
from tiler_amd import synth


def test_make_tiles_unique_needs_a_gpu():
    from conftest import gpu_available
    if gpu_available():
        pytest.skip("a GPU is present: this checks the no-GPU behaviour")
    lib = tiler_amd.load()
    pp = np.zeros((4, 64), np.uint8)
    act, uc, mi = np.ones(4, np.uint8), np.ones(4, np.int64), np.zeros(4, np.int64)
    seg = np.array([0, 4], np.int64)
    v = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.tiler_make_tiles_unique(v(pp), v(act), v(uc), v(mi), 4, v(seg), 1) == -1
    assert "HIP device" in tiler_amd.last_error() or "gfx950" in tiler_amd.last_error()
    assert lib.tiler_make_tiles_unique_dev(None, None, None, None, 0, v(seg), 1, None) == -1
    assert act.all() and (uc == 1).all()  # nothing was computed on the host
    with pytest.raises(tiler_amd._lib.TilerError):
        gt.make_tiles_unique_gpu(pp, act, uc)


def test_encoder_without_flag_stays_on_the_host():
    from tiler_amd.encoder import Encoder
    v = synth.video(51, 64, 48, kf_frames=(30,), n_palettes=2)
    a, b = Encoder(v), Encoder(v, gpu_unique=False)
    assert a.gpu_unique is False and a.palpix.shape[0] > a.tiles_per_frame * 25  # the default; two chunks
    a.do_make_unique()
    b.do_make_unique()
    assert (a.active == 0).any()
    for n in ("palpix", "active", "use_count", "tile"):
        assert np.array_equal(getattr(a, n), getattr(b, n)), n
    # the step is the host function chunk by chunk
    T, chunk = v.palpix.shape[0], a.tiles_per_frame * 25
    for first in range(0, T, chunk):
        s = slice(first, min(T, first + chunk))
        pp, act, uc, _ = gt.make_tiles_unique(v.palpix[s], np.ones(s.stop - s.start, np.uint8),
                                              np.ones(s.stop - s.start, np.int64))
        assert np.array_equal(a.palpix[s], pp) and np.array_equal(a.active[s], act)
        assert np.array_equal(a.use_count[s], uc)
