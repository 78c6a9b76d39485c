"""k-nearest searches at the k the rest of the suite never runs (it holds k = 1 and k = 8): include/tiler_ann.h promises
exact answers in ANN's own tie order for every k in 1..32, at ann_kdtree_search_multi, ann_kdtree_search_multi_batch
and ann_kdtree_search_batch_dev.  k in 2..7 runs the K = 8 kernel instances with a.k < K (the small-batch scan and its
merge, both shortlists' lane lists, the rescore's "settled" test against the k-th key, tier 2, nn_exact_kernel<8>,
kd_replay_kernel<8>); k in 9..32 skips the MFMA path and runs nn_exact_kernel<32> for the whole batch, then
kd_verify_kernel over a.k results and kd_replay_kernel<32>.  Inputs: tests/knn_cases.py, whose ties across the last
slot tests/test_knn_case_inputs.py proves on the oracle.  Every answer is compared with the restated ANN search
(oracle.KDTree) and, on an index-order handle, with the exhaustive lowest-index scan: indices and fp32 bits."""
import ctypes

import numpy as np
import pytest
from nncheck import INDEX_ORDER, check_nn

import knn_cases as kc

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
SCAN_D_MAX, SCAN_MAX8 = 256, 16  # nn_search.hip: the small-batch scan's widest row and its default k <= 8 batch limit
MFMA_D_MAX = 256                 # pick_S: wider rows have no shortlist fragments (the exact kernel answers every k)


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _scan_takes(d, nq, k):  # scan_small_takes for k > 1
    return d <= SCAN_D_MAX and d % 4 == 0 and k <= 8 and nq <= SCAN_MAX8


def _assert_path(st, d, nq, k):
    """what search_core reports for a batch that is not a small-batch scan: the MFMA shortlist (splits > 0, the tiers
    counted on the device) for k <= 8 on rows it has fragments for, else the exact kernel for the whole batch"""
    assert st["queries"] == nq and st["tie_order"] == 0
    if d <= MFMA_D_MAX and k <= 8:
        assert st["splits"] > 0, st
        assert 0 <= st["exhaustive_queries"] <= nq and 0 <= st["fallback_queries"] <= nq, st
    else:
        assert st["splits"] == 0 and st["exhaustive_queries"] == nq and st["fallback_queries"] == 0, st


@pytest.mark.parametrize("k", kc.K_SWEEP)
@pytest.mark.parametrize("bs", kc.BS)
@pytest.mark.parametrize("name", kc.SWEEP_CASES)
def test_batched_k_sweep(gpu, oracle, name, bs, k):
    """the full query set (MFMA path for k <= 8, exact kernel above), then 3 and 16 queries (the small-batch scan and,
    with it switched off, the tiers -- check_nn runs both), under both tie rules"""
    data, qs = kc.make(name)
    d = data.shape[1]
    st = check_nn(gpu, oracle, data, qs, k=k, bs=bs)
    _assert_path(st, d, qs.shape[0], k)
    if name == "orbit":  # a mirror-orbit index: the orbit search is k = 1 only, every other k takes the generic path
        assert st["orbit_groups"] > 0 and st["orbit_search"] == 0, st
    for nq in (3, 16):
        st = check_nn(gpu, oracle, data, qs[:nq], k=k, bs=bs)  # scan off in the run whose stats come back
        _assert_path(st, d, nq, k)
        assert st["orbit_search"] == 0
        if _scan_takes(d, nq, k):  # and the scan is what a batch of this size takes by default
            with gpu.KDTree(data, bs=bs) as kdt:
                kdt.search_batch(qs[:nq], k=k)
                st = kdt.stats()
            assert st["splits"] == 0 and st["exhaustive_queries"] == 0 and st["fallback_queries"] == 0, st


@pytest.mark.parametrize("k", kc.K_TINY)
@pytest.mark.parametrize("bs", kc.BS)
@pytest.mark.parametrize("name", kc.TINY_CASES)
def test_k_at_least_n(gpu, oracle, name, bs, k):
    """fewer rows than k: the first min(n, k) results are the oracle's under both tie rules, the rest -1 / FLT_MAX;
    through the batch entry and, one query per call, through ann_kdtree_search_multi"""
    data, qs = kc.make(name)
    n = data.shape[0]
    check_nn(gpu, oracle, data, qs, k=k, bs=bs)
    okd = oracle.KDTree(data, bs=bs)
    oi, oe = okd.search_batch(qs, k=k)
    okd.close()
    m = min(n, k)
    assert (oi[:, :m] >= 0).all() and (oi[:, m:] == -1).all() and (oe[:, m:] == FLT_MAX).all()
    for split in (0, INDEX_ORDER):
        with gpu.KDTree(data, bs=bs, split=split) as kdt:
            gi, ge = kdt.search_batch(qs, k=k)
            assert (gi[:, m:] == -1).all() and (ge[:, m:] == FLT_MAX).all() and (gi[:, :m] >= 0).all()
            for j, q in enumerate(qs):
                si, se = kdt.search_multi(q, k)
                if split == 0:
                    wi, we = oi[j], oe[j]
                else:
                    wi, we = oracle.knn(data, q, k)
                assert np.array_equal(si, wi) and np.array_equal(se.view(np.uint32), we.view(np.uint32)), (split, j)
                assert np.array_equal(si, gi[j]) and np.array_equal(se.view(np.uint32), ge[j].view(np.uint32))


@pytest.mark.parametrize("k", kc.K_ORDER)
@pytest.mark.parametrize("bs", kc.BS)
@pytest.mark.parametrize("name", kc.ORDER_CASES)
def test_forced_replay_other_k(gpu, oracle, name, bs, k):
    """tiler_debug_force_replay: every query of a batch past the scan's size takes kd_replay_kernel<8> (k = 3) or
    <32> (k = 20); the answers are the oracle's and the ones given without the hook"""
    lib = gpu.load()
    data, qs = kc.make(name)
    nq = qs.shape[0]
    assert nq > 64 and data.shape[0] > bs  # past every scan limit; a tree of more than one bucket
    with gpu.KDTree(data, bs=bs) as kdt:
        fi, fe = kdt.search_batch(qs, k=k)
    assert lib.tiler_debug_force_replay(1) == 0
    try:
        st = check_nn(gpu, oracle, data, qs, k=k, bs=bs)
        assert st["kd_replayed"] == nq, st
        check_nn(gpu, oracle, data, qs[:10], k=k, bs=bs)  # k = 3: the scan's merge replays each query itself
        with gpu.KDTree(data, bs=bs) as kdt:
            gi, ge = kdt.search_batch(qs, k=k)
    finally:
        lib.tiler_debug_force_replay(0)
    assert np.array_equal(gi, fi) and np.array_equal(ge.view(np.uint32), fe.view(np.uint32))


GUARD = 64  # words on either side of a device result buffer


@pytest.mark.parametrize("nq", [1, 33, 257])
@pytest.mark.parametrize("k", [5, 20])
def test_device_entry_layout(gpu, oracle, k, nq):
    """ann_kdtree_search_batch_dev on torch buffers: [nq][k] exactly as the host entry returns it and as the oracle
    has it, and not a word written before the buffers or past nq * k"""
    import torch
    data, qs = kc.make("ints2")
    q = np.ascontiguousarray(qs[np.arange(nq) % qs.shape[0]])
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(q).to(dev)
    di = torch.full((GUARD + nq * k + GUARD,), -77, dtype=torch.int32, device=dev)
    de = torch.full((GUARD + nq * k + GUARD,), -77.0, dtype=torch.float32, device=dev)
    with gpu.KDTree(data) as kdt:
        hi, he = kdt.search_batch(q, k=k)
        kdt.search_batch_dev(dq.data_ptr(), nq, k, di.data_ptr() + 4 * GUARD, de.data_ptr() + 4 * GUARD)
        torch.cuda.synchronize(dev)
    gi, ge = di.cpu().numpy(), de.cpu().numpy()
    for g, h, fill in ((gi, hi, -77), (ge, he, np.float32(-77.0))):
        assert (g[:GUARD] == fill).all() and (g[GUARD + nq * k:] == fill).all(), "a guard word was overwritten"
        assert np.array_equal(g[GUARD:GUARD + nq * k].view(np.uint32), h.reshape(-1).view(np.uint32))
    okd = oracle.KDTree(data)
    oi, oe = okd.search_batch(q, k=k)
    okd.close()
    assert np.array_equal(hi, oi) and np.array_equal(he.view(np.uint32), oe.view(np.uint32))


@pytest.mark.parametrize("k", [0, -1, 33])
def test_k_out_of_range(gpu, k):
    """k outside 1..32 at the three entry points: -1, the message names the range, no output word is touched"""
    import torch
    lib = gpu.load()
    data, qs = kc.make("dups")
    q = qs[:4].copy()
    with gpu.KDTree(data) as kdt:
        idx, err = np.full(4 * 40, -77, np.int32), np.full(4 * 40, -77.0, np.float32)
        lib.ann_kdtree_search_multi(kdt.handle, _vp(idx), _vp(err), 1, _vp(q[0]), 0.0)  # a good call first
        assert idx[0] >= 0 and (idx[1:] == -77).all()
        idx[0], err[0] = -77, -77.0
        assert lib.ann_kdtree_search_multi(kdt.handle, _vp(idx), _vp(err), k, _vp(q[0]), 0.0) == -1
        assert "1..32" in gpu.last_error()
        assert lib.ann_kdtree_search_multi_batch(kdt.handle, _vp(q), 4, k, 0.0, _vp(idx), _vp(err)) == -1
        assert "1..32" in gpu.last_error()
        assert (idx == -77).all() and (err == -77.0).all()
        dev = torch.device("cuda", 0)
        dq = torch.from_numpy(q).to(dev)
        di = torch.full((4 * 40,), -77, dtype=torch.int32, device=dev)
        de = torch.full((4 * 40,), -77.0, dtype=torch.float32, device=dev)
        vp = ctypes.c_void_p
        assert lib.ann_kdtree_search_batch_dev(kdt.handle, vp(dq.data_ptr()), 4, k, vp(di.data_ptr()),
                                               vp(de.data_ptr()), vp(0)) == -1
        assert "1..32" in gpu.last_error()
        torch.cuda.synchronize(dev)
        assert bool((di == -77).all()) and bool((de == -77.0).all())
        gi, _ = kdt.search_batch(q, k=3)  # the handle still answers
        assert (gi >= 0).all()


def test_mixed_k_coalescing(gpu, oracle):
    """16 threads on one handle, thread i calling ann_kdtree_search_multi with k = (1, 3, 8, 20)[i % 4]: the combiner
    batches callers of equal k only (ann_api.hip, combined_search), so every answer is the oracle's for its own k"""
    from test_gpu_concurrent import THREADS, _run_threads
    ks = (1, 3, 8, 20)
    assert THREADS % len(ks) == 0  # item i runs on thread i % THREADS: k = ks[i % 4] is a property of the thread
    data, qs = kc.make("ints2")
    nq = 400
    q = np.ascontiguousarray(qs[np.arange(nq) % qs.shape[0]])
    got = [None] * nq
    with gpu.KDTree(data) as kdt:
        def one(i):
            got[i] = kdt.search_multi(q[i], ks[i % 4])
        _run_threads(one, nq)
        cs = kdt.combine_stats()
    okd = oracle.KDTree(data)
    want = {k: okd.search_batch(q, k=k) for k in ks}
    okd.close()
    for i in range(nq):
        k = ks[i % 4]
        oi, oe = want[k]
        oi, oe = oi.reshape(nq, k)[i], oe.reshape(nq, k)[i]
        assert got[i][0].shape == (k,)
        assert np.array_equal(got[i][0], oi) and np.array_equal(got[i][1].view(np.uint32), oe.view(np.uint32)), (i, k)
    assert cs["calls"] == nq
    assert cs["batches"] >= len(ks)  # batches never mix k
