"""The inputs of tests/knn_cases.py hold what they claim, shown on the oracle alone (no GPU): at every k the GPU sweep
uses, enough queries have a tie across the last returned slot (the k-th and the (k+1)-th distance are equal, so which
candidate fills slot k is the tie order's decision), and ANN's visit order differs from index order often enough that a
lowest-index answer cannot pass as kd order."""
import numpy as np
import pytest

import knn_cases as kc


def _next_dist32(data, qs):
    """[nq] the 33rd smallest squared distance and [nq, 32] the 32 smallest, fp32 summed in dimension order (the
    oracle's own sum: one rounding per product and per add)"""
    out = np.zeros((qs.shape[0], 33), np.float32)
    for j, q in enumerate(qs):
        acc = np.zeros(data.shape[0], np.float32)
        for d in range(data.shape[1]):
            t = q[d] - data[:, d]
            acc = acc + t * t
        out[j] = np.sort(acc)[:33]
    return out[:, 32], out[:, :32]


def _tied_queries(oracle, data, qs, bs, k):
    """queries whose k-th and (k+1)-th nearest distances are equal"""
    okd = oracle.KDTree(data, bs=bs)
    try:
        if k < 32:
            _, err = okd.search_batch(qs, k=k + 1)
            return int(np.count_nonzero(err[:, k - 1] == err[:, k]))
        _, err = okd.search_batch(qs, k=32)
    finally:
        okd.close()
    nxt, first = _next_dist32(data, qs)
    assert np.array_equal(first.view(np.uint32), err.view(np.uint32))  # the numpy sum is the oracle's, bit for bit
    return int(np.count_nonzero(err[:, 31] == nxt))


@pytest.mark.parametrize("bs", kc.BS)
@pytest.mark.parametrize("name", kc.TIE_CASES)
def test_ties_across_the_last_slot(oracle, name, bs):
    data, qs = kc.make(name)
    assert qs.shape[0] <= 250 and data.shape[0] > 33
    for k in kc.K_SWEEP + kc.K_ORDER:
        tied = _tied_queries(oracle, data, qs, bs, k)
        assert tied >= kc.MIN_TIED, f"{name} bs={bs} k={k}: only {tied} queries tie across slot k"


@pytest.mark.parametrize("name", ("odd17", "odd300"))
def test_odd_d_cases_have_ties(oracle, name):
    """integer rows in 0..3: equal distances exist at every k (not a counted condition of the sweep, a sanity check)"""
    data, qs = kc.make(name)
    assert data.shape[1] % 4 != 0 or data.shape[1] > 256
    assert all(_tied_queries(oracle, data, qs, 1, k) >= 1 for k in kc.K_SWEEP)


@pytest.mark.parametrize("bs", kc.BS)
@pytest.mark.parametrize("name", kc.ORDER_CASES)
def test_kd_order_is_not_index_order(oracle, name, bs):
    data, qs = kc.make(name)
    okd = oracle.KDTree(data, bs=bs)
    try:
        for k in kc.K_ORDER:
            ki, ke = okd.search_batch(qs, k=k)
            res = [oracle.knn(data, q, k) for q in qs]
            ii = np.stack([r[0] for r in res])
            ie = np.stack([r[1] for r in res])
            assert np.array_equal(ke.view(np.uint32), ie.view(np.uint32))  # the same distances, whatever the order
            differ = int(np.count_nonzero(np.any(ki != ii, axis=1)))
            assert differ >= kc.MIN_ORDER, f"{name} bs={bs} k={k}: kd and index order differ for {differ} queries only"
    finally:
        okd.close()


def test_integer_cases_are_exact_and_tiny_sizes():
    """the integer cases hold small integers only (every fp32 distance is exact whatever the summation order), and
    the tiny cases sit on either side of k = 8, 9 and 32"""
    for name in kc.INTEGER_CASES:
        data, qs = kc.make(name)
        for a in (data, qs):
            assert np.array_equal(a, np.rint(a)) and 0 <= a.min() and a.max() <= 3
    assert [kc.make(n)[0].shape[0] for n in kc.TINY_CASES] == list(kc.TINY_N)
    assert min(kc.TINY_N) < min(kc.K_TINY) and max(kc.TINY_N) > max(kc.K_TINY)
