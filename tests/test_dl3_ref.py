"""CPU tests that pin DLv3 palette quantisation to the reference's own source: dlquant/quantizer.c compiled by
oracle/build_ref_dlquant.sh (32-bit ulong as the DLL's LLP64, strict SSE float) is the ground truth, through its
committed vectors (tests/golden/dl3_ref_kat.npz, read by dl3_kat.py) everywhere and through the live build where the
reference tree is present.  Checked against it: the oracle's restatement (oracle/palette.c or_dl3quant) and the
pure-Python restatement of tests/test_palette.py, which until now only vouched for each other.  The GPU side is
tests/test_gpu_dl3_ref.py."""
import numpy as np
import pytest

import dl3_kat
from test_palette import _py_dl3quant


@pytest.mark.parametrize("bpc", dl3_kat.BPC)
def test_oracle_dl3quant_equals_reference_fixture(oracle, bpc):
    """or_dl3quant byte for byte: one colour, exactly quant_to and quant_to + 1 colours, fewer, two equal counts,
    one-pixel-per-cell gradients (calc_err ties), dominant colours with counts in the tens of thousands, textured
    tiles, noise; quant_to 16 / 32 / 64.  The histogram size is the plain count of distinct cells."""
    cases, _ = dl3_kat.load()
    assert len(cases) >= 19
    for case in cases:
        for q in dl3_kat.QUANT_TO:
            got, hist = oracle.dl3quant(case.pixels, q, bpc)
            assert np.array_equal(got, case.palette(q, bpc)), (case.name, q, bpc)
            assert hist == case.cells(bpc), (case.name, bpc)


def test_fixture_cases_are_what_they_say():
    """The edge cases hold at every bpc (a regenerated fixture that lost one would still pass the byte compare)."""
    by = {c.name: c for c in dl3_kat.load()[0]}
    for bpc in dl3_kat.BPC:
        assert by["one_colour"].cells(bpc) == 1 and by["two_equal_counts"].cells(bpc) == 2
        assert by["fewer_5"].cells(bpc) == 5
        for q in dl3_kat.QUANT_TO:
            assert by[f"exact_{q}"].cells(bpc) == q and by[f"exact_{q}_plus_1"].cells(bpc) == q + 1
        g = by["grad_1px_cells_all_bpc"]
        assert g.cells(bpc) == g.counts.sum() == 256
    g = by["grad_1px_cells_bpc7"]
    assert g.cells(7) == g.counts.sum() == 1024
    assert np.array_equal(by["two_equal_counts"].counts, [96, 96])
    assert (by["dominant_exact_plus_noise"].counts > 20000).sum() == 4
    p = by["dominant_peaked_noise"]
    assert p.counts.sum() > 90000 and p.cells(5) < 64 and p.cells(8) > 2000  # cells of thousands at low bpc
    assert all(c.counts.sum() % 64 == 0 for c in by.values())
    assert max(c.cells(8) for c in by.values()) > 2000  # long tables too


def _wrap_pixels(w):
    c = np.repeat(w.colours, w.tile_counts.astype(np.int64) * 64)
    return np.stack([c & 255, (c >> 8) & 255, (c >> 16) & 255], 1).astype(np.uint8)


def test_oracle_dl3quant_wraps_the_32_bit_sums_as_the_reference(oracle):
    """263,200 flat tiles of 0xFFFFFF carry each colour sum past 2^32 (16,844,800 * 255): the reference's 32-bit
    ulong wraps, so the cell mean is no longer white; alone, merged into a second colour, and among 20 others."""
    _, wraps = dl3_kat.load()
    assert [w.name for w in wraps] == ["white_wraps", "white_wraps_then_merges", "white_wraps_among_20"]
    for w in wraps:
        assert int(w.tile_counts[0]) * 64 * 255 > 1 << 32 and int(w.tile_counts.sum()) * 64 < 1 << 31
        got, hist = oracle.dl3quant(_wrap_pixels(w), w.quant_to, w.bpc)
        assert np.array_equal(got, w.pal), w.name
        assert hist == w.colours.size
    assert wraps[0].pal[0] != 0xFFFFFF and wraps[1].colours.size > wraps[1].quant_to  # wrapped; a merge happens


def _sweep_pixels(rng, kind, n):
    if kind == "random":
        return rng.integers(0, 256, (n, 3)).astype(np.uint8)
    if kind == "clustered":
        base = rng.integers(0, 256, (int(rng.integers(2, 20)), 3))
        px = base[rng.integers(0, base.shape[0], n)] + rng.integers(-10, 11, (n, 3))
    elif kind == "near_flat":
        px = rng.integers(0, 256, (1, 3)) + rng.integers(-2, 3, (n, 3))
    else:  # gradient between two colours with a little noise
        c0, c1 = rng.integers(0, 256, (2, 1, 3)).astype(np.float64)
        px = np.rint(c0 + (c1 - c0) * rng.random((n, 1))) + rng.integers(-1, 2, (n, 3))
    return np.clip(px, 0, 255).astype(np.uint8)


def test_oracle_dl3quant_matches_live_reference_build(oracle):
    """A seeded sweep against the reference build itself: random, clustered, near-flat and gradient pixel sets of 1 to
    4,000 pixels (sizes log-uniform, both ends included), quant_to 16 / 32 / 64, lookup_bpc 4 / 7 / 8 (15 sets each:
    540 cases) and bpc 5 / 6 (5 each).  The calls run on a few threads (both libraries are re-entrant)."""
    from concurrent.futures import ThreadPoolExecutor
    ref = oracle.ref_dlquant_lib()
    if ref is None:
        pytest.skip("reference DLv3 quantizer not built here (no reference tree): the committed fixture pins it")
    rng = np.random.default_rng(540)
    jobs = []
    for kind in ("random", "clustered", "near_flat", "gradient"):
        for q in dl3_kat.QUANT_TO:
            for bpc in dl3_kat.BPC:
                for rep in range(15 if bpc in (4, 7, 8) else 5):
                    n = (1, 4000)[rep] if rep < 2 else int(np.exp(rng.uniform(0, np.log(4000))))
                    jobs.append((kind, q, bpc, n, _sweep_pixels(rng, kind, n)))
    assert len(jobs) == 660 and {j[3] for j in jobs} >= {1, 4000}

    def run(job):
        kind, q, bpc, n, px = job
        return np.array_equal(oracle.dl3quant(px, q, bpc)[0], oracle.ref_dl3quant(ref, px, q, bpc))

    with ThreadPoolExecutor(min(8, oracle._threads())) as pool:
        bad = [j[:4] for j, same in zip(jobs, pool.map(run, jobs)) if not same]
    assert not bad, bad[:10]


PY_MAX_CELLS = 260  # the Python restatement is O(cells^2) in numpy scalars


@pytest.mark.parametrize("q,bpc", [(16, 4), (16, 5), (16, 6), (16, 7), (16, 8), (32, 7), (64, 7), (32, 4), (64, 8)])
def test_python_restatement_equals_reference_fixture(q, bpc):
    """tests/test_palette.py's _py_dl3quant (the oracle's other cross-check) on the small cases."""
    small = [c for c in dl3_kat.load()[0] if c.cells(bpc) <= PY_MAX_CELLS]
    assert len(small) >= 12 and any(c.cells(bpc) > q for c in small)
    for case in small:
        assert np.array_equal(_py_dl3quant(case.pixels, q, bpc), case.palette(q, bpc)), (case.name, q, bpc)
