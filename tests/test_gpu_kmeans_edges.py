"""GPU parity of the Dither step's k-means (kmeans.hip) with the CPU restatement (oracle/kmeans.c, itself pinned to
tests/kmeans_ref.py by test_kmeans_restatement.py) on the inputs that real clips produce and random clouds never do --
identical points (a keyframe of equal tiles), fewer distinct points than centres, exact distance ties -- and at the
kernels' own edges: max_iter, d != 192, n around 256 and 1024, k around the 32-centroid chunk, member runs of 256 | 257.
Labels, centroid words and the iteration count bit for bit; every case asserts from the ORACLE's output that the branch
it is named for was reached."""
import numpy as np
import pytest

import kmeans_ref as ref
from tiler_amd import synth

pytestmark = pytest.mark.gpu

TIE_SEED = 8  # tie_points(100, 192, seed): found on the CPU; what it must show is asserted in the test


def _check(oracle, X, k, max_iter=0):
    from tiler_amd.palette import kmeans
    o = oracle.kmeans(X, k, max_iter or ref.MAX_ITER)
    g = kmeans(X, k, max_iter)
    assert g[2] == o[2], (g[2], o[2])
    assert np.array_equal(g[0], o[0]), np.flatnonzero(g[0] != o[0])[:8]
    assert np.array_equal(g[1].view(np.uint64), o[1].view(np.uint64))
    return o


@pytest.mark.parametrize("k", [40, 70])
def test_identical_points(gpu, oracle, k):
    """300 equal rows: every seeding sum is 0 (the pick is floor(u n)), every distance ties over all k centroids --
    over one (k = 40) or two (k = 70) boundaries of the 32-centroid chunk -- and all clusters but one are empty in
    every update.  The mean of 300 equal doubles is not that double, so the labels walk for about k iterations."""
    X = ref.identical_points(300, 192, seed=k)
    seeds = oracle.kmeans(X, k, 1)[1]
    assert (seeds == X[0]).all()
    lab, _, it = _check(oracle, X, k)
    assert it > 2 and (np.bincount(lab, minlength=k) == 0).sum() >= 1
    _check(oracle, X, k, max_iter=1)


def test_fewer_distinct_points_than_centres(gpu, oracle):
    """5 distinct rows repeated to n = 1030 (L = 2), k = 12: after five draws the D^2 sum is 0."""
    X = ref.few_distinct(1030, 192, 5, seed=3)
    seeds = _check(oracle, X, 12, max_iter=1)[1]
    assert np.unique(seeds, axis=0).shape[0] == 5  # every distinct row found; the other seven seeds repeat them
    _check(oracle, X, 12)


def test_exact_ties(gpu, oracle):
    """Integer points c +- v_j with orthogonal v_j: with c + v_a and c - v_a both seeds, every other point of that
    centre is at exactly the same distance from the two.  The tie goes to the lower centroid."""
    X = ref.tie_points(100, 192, seed=TIE_SEED)
    k = 6
    lab, seeds, _ = oracle.kmeans(X, k, 1)
    tied = ref.tied_points_of(X, seeds)
    assert len(tied) >= 4
    for i in tied[:4]:  # the two distances once more, and the winner is the lower index
        ds = [ref.dist2(X[i].tolist(), c.tolist()) for c in seeds]
        at = [j for j, v in enumerate(ds) if v == min(ds)]
        assert len(at) >= 2 and lab[i] == at[0]
    _check(oracle, X, k, max_iter=1)
    _check(oracle, X, k)


@pytest.mark.parametrize("max_iter", [1, 2, 3])
def test_max_iter_cut(gpu, oracle, max_iter):
    X = ref.cloud(700, 192, 9, seed=1)
    assert oracle.kmeans(X, 9)[2] > 3
    assert _check(oracle, X, 9, max_iter)[2] == max_iter


@pytest.mark.parametrize("d", [1, 31, 32, 33, 191])
def test_dimensions(gpu, oracle, d):
    """d != 192: the transpose's partial 32 x 32 tiles and the assignment's [d][32] centroid staging."""
    _check(oracle, ref.cloud(700, d, 9, seed=d), 9)


@pytest.mark.parametrize("n,k", [(1, 1), (255, 4), (256, 4), (257, 4), (1023, 3), (1024, 3), (1025, 3)])
def test_point_count_edges(gpu, oracle, n, k):
    """One point; one workgroup of the assignment | two; L = ceil(n / 1024) = 1 | 2."""
    _check(oracle, ref.cloud(n, 192, k, seed=n), k)


@pytest.mark.parametrize("k", [32, 33, 64, 65])
def test_centroid_chunk_edges(gpu, oracle, k):
    _check(oracle, ref.cloud(600, 192, k, seed=k), k)


def test_member_runs_of_256_and_257(gpu, oracle):
    """Blobs of 256, 257 and 90 points, shuffled: after the first assignment one cluster has exactly one full run of
    256 members and another one run more."""
    X = ref.blobs((256, 257, 90), 192, seed=0)
    lab = oracle.kmeans(X, 3, 1)[0]
    assert sorted(np.bincount(lab, minlength=3).tolist()) == [90, 256, 257]
    assert _check(oracle, X, 3)[2] >= 2  # at least one update ran


def _flat(colours, n):
    c = np.asarray(colours, np.int32)
    return np.repeat(c[np.arange(n) % c.size][:, None], 64, 1)


@pytest.mark.parametrize("case", ["black", "flat3", "textured_then_black"])
def test_prepare_dither_tiles_degenerate(gpu, oracle, case):
    """PrepareDitherTiles over tiles a fade, a title card or a letterbox gives: the LAB descriptors are equal rows."""
    from tiler_amd.palette import prepare_dither_tiles
    if case == "black":
        rgb = _flat([0], 200)
    elif case == "flat3":
        rgb = _flat([0x000000, 0x2040F0, 0xFFFFFF], 200)
    else:
        rgb = np.concatenate([synth.frame_tiles(np.random.default_rng(5), 100), _flat([0], 100)])
    P = 8
    ol, oc, oi = oracle.prepare_dither_tiles(rgb, P)
    if case != "textured_then_black":
        assert np.unique(oracle.psyv_lab_batch(rgb), axis=0).shape[0] < P  # fewer distinct descriptors than palettes
    gl, gc, gi = prepare_dither_tiles(rgb, P)
    assert gi == oi
    assert np.array_equal(gl, ol)
    assert np.array_equal(gc.view(np.uint64), oc.view(np.uint64))
