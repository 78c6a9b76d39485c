"""ann_kdtree_pri_search_batch where tests/test_gpu_pri_search.py checks answers only: the three ways
kd_pri_resolve_kernel answers a query at eps = 0 -- flag 0 (decided from the exact tie set), flag 2 (the heap order
alone simulated up to the first tied leaf) and flag 1 (the priority search replayed in full: more than KD_PRI_CAP = 64
points within the annkSearch distance, or no entry key below the minimum distance D, as when D = 0) -- each shown to
have run by tiler_debug_pri_outcomes, and the chunk loop that keeps the heap scratch within 1 GiB taken more than once.
Every answer is oracle.KDTree.pri_search_batch's (annkPriSearch restated): index and fp32 distance bits."""
import numpy as np
import pytest

import knn_cases as kc

pytestmark = pytest.mark.gpu

PRI_ENTRY_BYTES = 12  # kdtree.hip PriEntry {float key; int s, e;}: n + 1 of them per query (ANN's pr_queue(n_pts))
HEAP_BUDGET = 1 << 30  # ann_api.hip, ann_kdtree_pri_search_batch: queries per chunk = budget / a query's heap bytes


def _pri(gpu, oracle, data, qs, eps, bs, kdt=None):
    """one batch against the oracle; returns the outcome counts (flag 0, flag 1, flag 2)"""
    data = np.ascontiguousarray(data, np.float32)
    qs = np.ascontiguousarray(qs, np.float32)
    own = kdt is None
    if own:
        kdt = gpu.KDTree(data, bs=bs)
    try:
        gi, ge = kdt.pri_search_batch(qs, eps)
        out = kdt.pri_outcomes()
    finally:
        if own:
            kdt.close()
    okd = oracle.KDTree(data, bs=bs)
    oi, oe = okd.pri_search_batch(qs, eps)
    okd.close()
    assert np.array_equal(ge.view(np.uint32), oe.view(np.uint32)), "pri search: distance mismatch"
    bad = np.nonzero(gi != oi)[0]
    assert bad.size == 0, f"pri search: {bad.size} of {len(qs)} indices differ (first {bad[:8]})"
    if eps == 0.0:
        assert sum(out) == len(qs) and min(out) >= 0, out
    else:
        assert out == (0, 0, 0), out  # every query replayed without the resolve step
    return out


@pytest.mark.parametrize("bs", [1, 4])
def test_more_than_cap_ties_replays(gpu, oracle, bs):
    """100 identical rows: a query on them or near them has more than 64 points within its annkSearch distance"""
    rng = np.random.default_rng(60 + bs)
    rows = rng.normal(0, 1, (500, 12)).astype(np.float32)
    one = rng.normal(0, 1, 12).astype(np.float32)
    data = np.concatenate([rows[:250], np.tile(one, (100, 1)), rows[250:]])
    near = np.concatenate([one + rng.normal(0, 0.01, (30, 12)).astype(np.float32), np.tile(one, (2, 1))])
    assert _pri(gpu, oracle, data, near, 0.0, bs) == (0, len(near), 0)
    others = rng.normal(0, 1, (64, 12)).astype(np.float32)
    mixed = np.concatenate([others, near])[rng.permutation(64 + len(near))]
    out = _pri(gpu, oracle, data, mixed, 0.0, bs)
    assert out[1] >= len(near) and out[0] >= 1, out
    _pri(gpu, oracle, data, mixed, 0.5, bs)
    with gpu.KDTree(data, bs=bs) as kdt:  # before the first call, and after a call on a handle without a tree
        assert kdt.pri_outcomes() == (0, 0, 0)
    from nncheck import INDEX_ORDER
    with gpu.KDTree(data, split=INDEX_ORDER) as kdt:
        kdt.pri_search_batch(mixed)
        assert kdt.pri_outcomes() == (0, 0, 0)


@pytest.mark.parametrize("bs", [1, 4])
def test_zero_distance_replays(gpu, oracle, bs):
    """queries equal to dataset rows (each present 2 or 3 times): D = 0, so no leaf entry key lies below D"""
    data, _ = kc.make("dups")
    rng = np.random.default_rng(62)
    qs = data[rng.integers(0, data.shape[0], 150)]
    assert _pri(gpu, oracle, data, qs, 0.0, bs) == (0, len(qs), 0)
    _pri(gpu, oracle, data, qs, 0.5, bs)


def test_heap_ties_simulated(gpu, oracle):
    """an integer grid with duplicates, bucket size 1: equal rows sit in different leaves with equal entry keys, so
    queries between grid points meet the heap's own tie order (flag 2) beside plainly decided ones (flag 0)"""
    rng = np.random.default_rng(50)
    data = rng.integers(0, 3, (3000, 8)).astype(np.float32)
    on = data[rng.integers(0, 3000, 40)]
    half = data[rng.integers(0, 3000, 80)] + rng.integers(0, 2, (80, 8)) * np.float32(0.5)
    between = rng.integers(0, 5, (80, 8)).astype(np.float32) * np.float32(0.5)
    qs = np.concatenate([on, half, between])[rng.permutation(200)]
    out = _pri(gpu, oracle, data, qs, 0.0, 1)
    print("outcomes (tie set, replay, heap order):", out)
    assert out[2] >= 1 and out[0] >= 1, out
    assert out[1] >= len(on), out  # D = 0 on the grid points
    _pri(gpu, oracle, data, qs, 0.5, 1)


@pytest.mark.parametrize("bs", [1, 4])
def test_chunked_batches(gpu, oracle, bs):
    """100,000 rows: a query's heap is 1.2 MB, so 2,000 queries run in 3 chunks; the answers land at their own
    offsets whatever the chunk, at eps = 0 (resolve + flagged replays) and eps = 0.5 (every query replayed)"""
    n, d, nq = 100000, 4, 2000
    chunk = max(1, min(nq, HEAP_BUDGET // ((n + 1) * PRI_ENTRY_BYTES)))
    assert (nq + chunk - 1) // chunk == 3 and nq % chunk != 0  # more than one chunk, and a ragged last one
    rng = np.random.default_rng(70 + bs)
    data = rng.integers(0, 51, (n, d)).astype(np.float32)
    qs = np.concatenate([data[rng.integers(0, n, 600)],
                         data[rng.integers(0, n, 700)] + rng.integers(-1, 2, (700, d)) * np.float32(0.5),
                         rng.integers(0, 101, (700, d)) * np.float32(0.5)]).astype(np.float32)
    qs = qs[rng.permutation(nq)]
    with gpu.KDTree(data, bs=bs) as kdt:
        out = _pri(gpu, oracle, data, qs, 0.0, bs, kdt)
        assert sum(out) == nq
        _pri(gpu, oracle, data, qs, 0.5, bs, kdt)  # the same handle: the outcome counts go back to 0
        # a batch of one chunk after a chunked one: nothing stale from the larger call
        assert sum(_pri(gpu, oracle, data, qs[:100], 0.0, bs, kdt)) == 100
