"""CPU tests of the GlobalTiling entry points (tiler_amd/csrc/global_tiling.hip): libANN.so exports them,
include/tiler_ann.h declares them, tiler_global_tiling_counts (host code) equals plan_global_tiling's k_per_bin / run,
the argument refusals need no device, and the numpy wrappers refuse wrong shapes and dtypes before they reach the
library."""
import ctypes
import math

import numpy as np
import pytest

from tiler_amd import _lib
from tiler_amd import global_tiling as gt

SYMBOLS = ["tiler_global_tiling", "tiler_global_tiling_dev", "tiler_global_tiling_counts", "tiler_tile_dataset_lines",
           "tiler_tile_dataset_lines_dev", "tiler_kmodes_medoids_batch", "tiler_kmodes_medoids_batch_dev"]
DESIRED = [1, 64, 65536, 10 ** 7]


def test_library_exports_the_symbols():
    lib = ctypes.CDLL(_lib.LIB_PATH)  # a lookup needs no device
    for s in SYMBOLS:
        assert getattr(lib, s) is not None, s


def test_header_declares_them():
    declared = _lib.header_symbols()
    for s in SYMBOLS:
        assert s in declared and s in _lib._SIGS, s
    for s in SYMBOLS:
        if s + "_dev" in SYMBOLS:
            assert _lib._SIGS[s + "_dev"][1][:-1] == _lib._SIGS[s][1] and _lib._SIGS[s + "_dev"][1][-1] is _lib.c_void_p


def test_encoder_flag_defaults_off():
    import inspect
    from tiler_amd.encoder import Encoder
    assert inspect.signature(Encoder.__init__).parameters["gpu_global_tiling"].default is False


def _plan_counts(sizes, desired):
    """k_per_bin and run exactly as plan_global_tiling computes them (global_tiling.py), from the bin sizes alone."""
    eq = [gt.equal_quality_tile_count(int(n)) for n in sizes]
    share = desired / sum(eq)
    k = np.zeros(len(sizes), np.int64)
    run = np.zeros(len(sizes), bool)
    for p, n in enumerate(sizes):
        kc = math.ceil(eq[p] * share)
        k[p] = int(round(kc))
        run[p] = n > kc
    return k, run


def _check(sizes, desired):
    k, run = gt.global_tiling_counts(np.asarray(sizes), desired)
    ek, erun = _plan_counts(sizes, desired)
    assert k.dtype == np.int64 and run.dtype == bool
    assert np.array_equal(k, ek) and np.array_equal(run, erun), (list(sizes)[:8], desired)


def test_plan_counts_helper_is_plan_global_tiling():
    """The helper above against plan_global_tiling itself on real bins (so the vectors below test the right thing)."""
    rng = np.random.default_rng(5)
    tiles = rng.integers(0, 16, (3000, 64)).astype(np.uint8)
    dith = rng.integers(0, 6, 3000).astype(np.int32)
    for desired in (1, 64, 700):
        plan = gt.plan_global_tiling(tiles, dith, 7, desired)
        k, run = _plan_counts([b.size for b in plan.bins], desired)
        assert np.array_equal(k, plan.k_per_bin) and list(np.nonzero(run)[0]) == plan.run


@pytest.mark.parametrize("desired", DESIRED)
def test_every_size_as_a_single_bin(desired):
    for n in range(1, 4097):
        _check([n], desired)


def test_a_single_empty_bin():
    for desired in DESIRED:  # plan_global_tiling divides by zero here; the library plans nothing
        k, run = gt.global_tiling_counts(np.zeros(1, np.int32), desired)
        assert k.tolist() == [0] and run.tolist() == [False]


@pytest.mark.parametrize("desired", DESIRED)
def test_random_bins(desired):
    rng = np.random.default_rng(11)
    for _ in range(8):
        _check(rng.integers(0, 1 << 18, 128), desired)
    _check((rng.integers(0, 1 << 18, 128) * (rng.random(128) < 0.2)).clip(0) + (np.arange(128) == 5), desired)


@pytest.mark.parametrize("desired", DESIRED)
def test_bins_of_size_kc_and_kc_plus_one(desired):
    """A bin of exactly ClusterCount tiles stays, one of ClusterCount + 1 runs.  The fixed point is searched for: the
    other bins are fixed, and the probed bin's size moves until size == kc (or kc + 1) holds for it."""
    rng = np.random.default_rng(13)
    eq = [gt.equal_quality_tile_count(n) for n in range(40000)]
    found = {0: 0, 1: 0}
    for _ in range(50):
        others = rng.integers(1, 1 << 18, 127)
        s_others = sum(gt.equal_quality_tile_count(int(n)) for n in others)
        for extra in (0, 1):
            for n in range(1, len(eq)):
                if n == math.ceil(eq[n] * (desired / (s_others + eq[n]))) + extra:
                    sizes = np.append(others, n)
                    _check(sizes, desired)
                    k, run = gt.global_tiling_counts(sizes, desired)
                    assert k[-1] == n - extra and bool(run[-1]) == bool(extra)
                    found[extra] += 1
                    break
        if min(found.values()) >= 3:
            break
    assert min(found.values()) >= 1, found


@pytest.mark.parametrize("desired", DESIRED)
def test_all_bins_empty_but_one(desired):
    for n in (1, 2, 63, 4096, 1 << 18, (1 << 31) - 1):
        for p in (0, 77, 127):
            sizes = np.zeros(128, np.int64)
            sizes[p] = n
            _check(sizes, desired)


def _counts_raw(sizes, n_pal, desired, with_out=True):
    lib = _lib.load()
    b = np.ascontiguousarray(sizes, np.int32)
    k = np.zeros(max(n_pal, 1), np.int32)
    run = np.zeros(max(n_pal, 1), np.uint8)
    v = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    return lib.tiler_global_tiling_counts(v(b), n_pal, desired, v(k) if with_out else None, v(run) if with_out else None)


def test_counts_refusals():
    assert _counts_raw([5, 6], 2, 10) == 0
    assert _counts_raw([5, 6], 2, 10, with_out=False) == 0  # both outputs are optional
    assert _counts_raw([5, 6], 0, 10) == -1
    assert "n_palettes" in _lib.last_error()
    assert _counts_raw([5, 6], -1, 10) == -1
    assert _counts_raw(np.zeros(4097), 4097, 10) == -1
    assert _counts_raw([5, 6], 2, 0) == -1
    assert "desired" in _lib.last_error()
    assert _counts_raw([5, 6], 2, -3) == -1
    assert _counts_raw([5, -1], 2, 10) == -1
    assert "bin_size[1]" in _lib.last_error()
    assert _lib.load().tiler_global_tiling_counts(None, 2, 10, None, None) == -1


def test_step_refusals_need_no_device():
    """desired < 1, n_palettes < 1 or above the header's limit (4096): -1 before the device is touched -- this test
    runs on a machine without one -- and the caller's arrays stay as they were."""
    lib = _lib.load()
    v = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rng = np.random.default_rng(3)
    pp = rng.integers(0, 16, (10, 64)).astype(np.uint8)
    dp, act = np.zeros(10, np.int32), np.ones(10, np.uint8)
    uc, mi = np.ones(10, np.int64), np.full(10, 5, np.int64)
    keep = [a.copy() for a in (pp, dp, act, uc, mi)]
    for n_pal, palsize, desired, word in ((0, 16, 5, "n_palettes"), (-2, 16, 5, "n_palettes"),
                                          (4097, 16, 5, "n_palettes"), (4, 16, 0, "desired"), (4, 16, -1, "desired"),
                                          (4, 0, 5, "palsize"), (4, 257, 5, "palsize")):
        for dev in (False, True):
            args = [v(pp), v(dp), v(act), v(uc), v(mi), 10, n_pal, palsize, desired, 7, None, None, None]
            rc = lib.tiler_global_tiling_dev(*args, None) if dev else lib.tiler_global_tiling(*args)
            assert rc == -1 and word in _lib.last_error(), (n_pal, palsize, desired, dev, _lib.last_error())
    rc = lib.tiler_global_tiling(v(pp), v(dp), v(act), v(uc), v(mi), -1, 4, 16, 5, 7, None, None, None)
    assert rc == -1 and "nt" in _lib.last_error()
    for a, b in zip((pp, dp, act, uc, mi), keep):
        assert np.array_equal(a, b)


@pytest.fixture
def no_library(monkeypatch):
    """Any call into the library fails the test: the wrappers must refuse first."""
    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(gt, "load", boom)


def test_wrappers_refuse_wrong_shapes_and_dtypes(no_library):
    pp = np.zeros((4, 64), np.uint8)
    dp = np.zeros(4, np.int32)
    with pytest.raises(ValueError):
        gt.do_global_tiling_gpu(pp, np.zeros(5, np.int32), 2, 3)
    with pytest.raises(ValueError):
        gt.do_global_tiling_gpu(pp, dp.astype(np.float32), 2, 3)
    with pytest.raises(ValueError):
        gt.do_global_tiling_gpu(pp, np.array([0, 1, 1 << 31, 0], np.int64), 2, 3)
    with pytest.raises(ValueError):
        gt.do_global_tiling_gpu(pp, dp, 2, 3, active=np.ones(3, np.uint8))
    with pytest.raises(ValueError):
        gt.do_global_tiling_gpu(pp, dp, 2, 3, use_count=np.ones((4, 1), np.int64))
    with pytest.raises(ValueError):
        gt.do_global_tiling_gpu(pp, dp, 0, 3)
    with pytest.raises(ValueError):
        gt.do_global_tiling_gpu(np.zeros((4, 63), np.uint8), dp, 2, 3)
    with pytest.raises(ValueError):
        gt.tile_dataset_lines_gpu(np.zeros((4, 64), np.int32))
    with pytest.raises(ValueError):
        gt.tile_dataset_lines_gpu(np.zeros((4, 63), np.uint8))
    with pytest.raises(ValueError):
        gt.tile_dataset_lines_gpu(np.zeros(65, np.uint8))
    with pytest.raises(ValueError):
        gt.global_tiling_counts(np.zeros((2, 2), np.int32), 5)
    with pytest.raises(ValueError):
        gt.global_tiling_counts(np.zeros(0, np.int32), 5)
    with pytest.raises(ValueError):
        gt.global_tiling_counts(np.array([1.5, 2.0]), 5)
    with pytest.raises(ValueError):
        gt.global_tiling_counts(np.array([3, -1]), 5)
    with pytest.raises(ValueError):
        gt.global_tiling_counts(np.array([3, 1 << 31], np.int64), 5)
