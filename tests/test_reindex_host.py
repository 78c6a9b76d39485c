"""CPU tests of the Reindex entry points (tiler_amd/csrc/reindex.hip): libANN.so exports them, include/tiler_ann.h
declares them, and the numpy wrappers refuse mismatched shapes before they reach the library."""
import ctypes

import numpy as np
import pytest

from tiler_amd import _lib
from tiler_amd import global_tiling as gt

SYMBOLS = ["tiler_tile_use_count", "tiler_tile_use_count_dev", "tiler_reindex_tiles", "tiler_reindex_tiles_dev",
           "tiler_gather_tiles", "tiler_gather_tiles_dev", "tiler_remap_items", "tiler_remap_items_dev",
           "tiler_debug_reindex"]


def test_library_exports_the_symbols():
    lib = ctypes.CDLL(_lib.LIB_PATH)  # a lookup needs no device
    for s in SYMBOLS:
        assert getattr(lib, s) is not None, s


def test_header_declares_them():
    declared = _lib.header_symbols()
    for s in SYMBOLS:
        assert s in declared and s in _lib._SIGS, s
    # the _dev form of a call: the same arguments and a stream
    for s in SYMBOLS:
        if s + "_dev" in SYMBOLS:
            assert _lib._SIGS[s + "_dev"][1][:-1] == _lib._SIGS[s][1] and _lib._SIGS[s + "_dev"][1][-1] is _lib.c_void_p


def test_encoder_flag_defaults_off():
    import inspect
    from tiler_amd.encoder import DistributedEncoder, Encoder
    for cls in (Encoder, DistributedEncoder):
        assert inspect.signature(cls.__init__).parameters["gpu_reindex"].default is False


@pytest.fixture
def no_library(monkeypatch):
    """Any call into the library fails the test: the wrappers must refuse first."""
    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(gt, "load", boom)


def test_wrappers_refuse_mismatched_shapes(no_library):
    tile = np.zeros((3, 5), np.int64)
    with pytest.raises(ValueError):
        gt.use_count_gpu(tile, -1)
    with pytest.raises(ValueError):
        gt.use_count_gpu(tile, 4, use_count=np.zeros(5, np.int64))
    with pytest.raises(ValueError):
        gt.use_count_gpu(tile.astype(np.float32), 4)
    with pytest.raises(ValueError):
        gt.use_count_gpu(np.array([0, 1 << 31], np.int64), 4)  # does not fit the library's int32 items
    with pytest.raises(ValueError):
        gt.reindex_tiles_gpu(np.ones(4, np.uint8), np.ones(5, np.int64))
    with pytest.raises(ValueError):
        gt.reindex_tiles_gpu(np.ones((2, 2), np.uint8), np.ones((2, 2), np.int64))
    with pytest.raises(ValueError):
        gt.remap_items_gpu(tile, np.zeros((2, 2), np.int64))
    with pytest.raises(ValueError):
        gt.remap_items_gpu(tile, np.zeros(4, np.float64))
    with pytest.raises(ValueError):
        gt.gather_tiles_gpu(np.zeros(2, np.int64))
    with pytest.raises(ValueError):
        gt.gather_tiles_gpu(np.zeros(2, np.int64), palpix=np.zeros((4, 64), np.uint8), thm=np.zeros(5, np.uint8))
    with pytest.raises(ValueError):
        gt.gather_tiles_gpu(np.zeros(2, np.int64), palpix=np.zeros((4, 32), np.uint8))
    with pytest.raises(ValueError):
        gt.gather_tiles_gpu(np.zeros((2, 1), np.int64), thm=np.zeros(5, np.uint8))
