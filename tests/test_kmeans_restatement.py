"""Host test: oracle/kmeans.c (the checker of the GPU k-means) against an independent plain-Python restatement of
the same text (tests/kmeans_ref.py), bit for bit -- labels, centroid words, iteration count -- on every input family
of test_gpu_kmeans_edges.py at sizes a pure-Python run affords (n <= 300, d <= 12, k <= 40), plus one two-dimensional
case at n = 1030 so that the seeding's runs of L = 2 points are pinned too."""
import numpy as np
import pytest

import kmeans_ref as ref

TIE_SEED_HOST = 4  # found on the CPU; what it must show is asserted below


def _both(oracle, X, k, max_iter=ref.MAX_ITER, seed=0):
    o = oracle.kmeans(X, k, max_iter, seed)
    r = ref.kmeans(X, k, max_iter, seed)
    assert o[2] == r[2], (o[2], r[2])
    assert np.array_equal(o[0], r[0]), np.flatnonzero(o[0] != r[0])[:8]
    assert np.array_equal(o[1].view(np.uint64), r[1].view(np.uint64))
    return o


def test_mt19937_uniforms(oracle):
    """Known answers of mt19937ar.c: the first output for the default seed 5489 is 3499211612 and the 10000th is
    4123659995 (the C++ standard's check value for mt19937); the C side's first draw agrees for several seeds."""
    out = ref.mt19937_uint32(5489, 10000)
    assert out[0] == 3499211612 and out[9999] == 4123659995
    for seed in (0, 1, 5489, 0xFFFFFFFF):
        assert oracle.lib().or_mt19937_first(seed) & 0xFFFFFFFF == ref.mt19937_uint32(seed, 1)[0]
    u = ref.uniforms(0, 700)  # past one regeneration of the 624-word state
    assert all(0.0 <= v < 1.0 for v in u) and len(set(u)) == 700


@pytest.mark.parametrize("n,k", [(300, 40), (300, 7), (2, 5)])
def test_identical_points(oracle, n, k):
    X = ref.identical_points(n, 12, seed=n + k)
    lab, cent, it = _both(oracle, X, k)
    if n == 300:
        assert it > 2 and np.bincount(lab, minlength=k).min() == 0
    seeds = _both(oracle, X, k, max_iter=1)[1]
    assert (seeds == X[0]).all()  # every pick is floor(u * n) of equal rows


def test_fewer_distinct_points_than_centres(oracle):
    X = ref.few_distinct(300, 12, 5, seed=3)
    _both(oracle, X, 12)
    seeds = _both(oracle, X, 12, max_iter=1)[1]
    assert np.unique(seeds, axis=0).shape[0] == 5  # all five rows found, then the S == 0 picks repeat them


def test_fewer_distinct_points_runs_of_two(oracle):
    """n = 1030: L = ceil(n / 1024) = 2, the last runs empty."""
    X = ref.few_distinct(1030, 2, 5, seed=4)
    _both(oracle, X, 12)
    _both(oracle, ref.cloud(1030, 2, 6, seed=5), 6)


def test_exact_ties(oracle):
    X = ref.tie_points(12, 12, seed=TIE_SEED_HOST)
    k = 6
    seeds = oracle.kmeans(X, k, 1)[1]
    assert len(ref.tied_points_of(X, seeds)) >= 4
    _both(oracle, X, k)
    _both(oracle, X, 40)


@pytest.mark.parametrize("max_iter", [1, 2, 3])
def test_max_iter_cut(oracle, max_iter):
    X = ref.cloud(300, 12, 9, seed=9)
    assert oracle.kmeans(X, 9)[2] > 3
    assert _both(oracle, X, 9, max_iter)[2] == max_iter


@pytest.mark.parametrize("d", [1, 2, 7, 12])
def test_dimensions(oracle, d):
    _both(oracle, ref.cloud(300, d, 9, seed=d), 9)


@pytest.mark.parametrize("n,k", [(1, 1), (1, 3), (255, 4), (256, 4), (257, 4), (300, 1), (300, 32), (300, 33),
                                 (30, 40)])
def test_size_edges(oracle, n, k):
    _both(oracle, ref.cloud(n, 6, k, seed=n * 41 + k), k)


def test_runs_of_256_and_257_members(oracle):
    """Host-sized stand-in for the 256 | 257 member runs is not possible below n = 513; the run boundary itself is
    reached with one blob of 280 members (runs of 256 + 24)."""
    X = ref.blobs((280, 20), 5, seed=1)
    lab = _both(oracle, X, 2, max_iter=1)[0]
    assert sorted(np.bincount(lab, minlength=2).tolist()) == [20, 280]
    _both(oracle, X, 2)


def test_seeds_differ(oracle):
    X = ref.cloud(200, 4, 5, seed=2)
    a = _both(oracle, X, 5, seed=1)
    b = _both(oracle, X, 5, seed=2)
    assert not np.array_equal(a[1], b[1])
