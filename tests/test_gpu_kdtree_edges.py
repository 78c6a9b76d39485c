"""GPU parity of the kd-tree build (tiler_amd/csrc/kdtree.hip) with the restated ANN 1.1.2 build (oracle/ann_kdtree.c)
on the inputs of tests/kd_edge_cases.py: sizes and dimensions on either side of every constant at which the build hands
over to another kernel, all-zero and exactly equal spreads, signed zeros, subnormal keys, bucket sizes around n, and a
small build right after a large one on the same pooled scratch.  Every case compares the leaf position of every point;
where the case has queries, also the indices and the distance bits of annkSearch (k = 1 and 8) and annkPriSearch
(eps = 0), whose ties resolve in the tree's order.  Everything is exact.  test_kdtree_edge_inputs.py holds, on the CPU,
that the inputs are what they claim."""
import kd_edge_cases as kc
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(gpu, oracle, rows, bs, q):
    with gpu.KDTree(rows, bs=bs) as kdt:
        pos = kdt.positions()
        got = None if q is None else (kdt.search_batch(q), kdt.search_batch(q, k=8), kdt.pri_search_batch(q, 0.0))
    okd = oracle.KDTree(rows, bs=bs)
    opos = okd.positions()
    want = None if q is None else (okd.search_batch(q), okd.search_batch(q, k=8), okd.pri_search_batch(q, 0.0))
    okd.close()
    assert np.array_equal(pos, opos), f"leaf order differs at {np.count_nonzero(pos != opos)} of {pos.size} points"
    if q is not None:
        for what, (gi, ge), (oi, oe) in zip(("search", "search k=8", "pri_search"), got, want):
            assert np.array_equal(gi, oi), f"{what}: {np.count_nonzero(gi != oi)} of {oi.size} indices differ"
            assert np.array_equal(_bits(ge), _bits(oe)), f"{what}: distance bits differ"
    return pos


def _family(family):
    return pytest.mark.parametrize("name", kc.names(family))


@_family("size")
def test_size_seams(gpu, oracle, name):
    _check(gpu, oracle, *kc.make(name))


@_family("dim")
def test_dimension_seams(gpu, oracle, name):
    _check(gpu, oracle, *kc.make(name))


@_family("spread")
def test_zero_and_equal_spreads(gpu, oracle, name):
    _check(gpu, oracle, *kc.make(name))


@_family("zero")
def test_signed_zeros(gpu, oracle, name):
    _check(gpu, oracle, *kc.make(name))


@_family("scale")
def test_subnormals_and_large_magnitudes(gpu, oracle, name):
    _check(gpu, oracle, *kc.make(name))


@_family("bucket")
def test_bucket_sizes(gpu, oracle, name):
    _check(gpu, oracle, *kc.make(name))


def test_scratch_reuse(gpu, oracle):
    """A large build, a small one and a large narrow one in a row on one device: the pooled scratch (omin / omax, chunk
    and node lists, keys) of each is the one before's, so a stale fold would show; then the first again, unchanged."""
    sets = [kc.make(name) for name in kc.names("reuse")]
    first = _check(gpu, oracle, *sets[0])
    for rows, bs, q in sets[1:]:
        _check(gpu, oracle, rows, bs, q)
    with gpu.KDTree(sets[0][0], bs=sets[0][1]) as kdt:
        again = kdt.positions()
    assert np.array_equal(again, first)
