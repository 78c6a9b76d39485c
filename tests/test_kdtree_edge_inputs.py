"""CPU checks that the inputs of tests/kd_edge_cases.py hold what they claim, on the ANN 1.1.2 restatement alone
(oracle/ann_kdtree.c), so that test_gpu_kdtree_edges.py cannot pass vacuously: the sizes and dimensions sit on the
build's seams, the tie-heavy sets tie at the median, the zero-spread and equal-spread sets make annMaxSpread answer as
stated, both zero signs meet in the root's cut dimension and the searches there resolve real ties, the subnormal
spreads are subnormal and decide the cut, and the bucket sizes straddle n."""
import kd_edge_cases as kc
import numpy as np


def _tree(oracle, rows, bs):
    """-> (positions, split arrays by split position); the root splits at n // 2."""
    kd = oracle.KDTree(rows, bs=bs)
    pos, spl = kd.positions(), kd.splits()
    kd.close()
    assert sorted(pos.tolist()) == list(range(rows.shape[0]))
    return pos, spl


def _root_cut(oracle, rows, bs=1):
    n = rows.shape[0]
    assert n > bs
    return int(_tree(oracle, rows, bs)[1][0][n // 2])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _finite(rows):
    assert rows.dtype == np.float32 and np.isfinite(rows).all()
    with np.errstate(over="raise"):
        assert np.isfinite(np.ptp(rows, 0)).all()  # every spread finite


def test_size_seams(oracle):
    seen = set()
    for name in kc.names("size"):
        rows, bs, q = kc.make(name)
        _finite(rows)
        n, dd = rows.shape
        seen.add((n, dd, name.rsplit("-", 1)[1]))
        assert bs == 1 and q is None
        cut = _root_cut(oracle, rows)
        col = np.sort(rows[:, cut])
        if name.endswith("tie"):
            assert set(np.unique(rows).tolist()) == {0.0, 0.25}
            assert np.unique(col).size == 2  # n keys of two values: which equal keys go LO is the quickselect's
        else:
            assert np.unique(col).size == n
    want = {(n, 8, k) for n in kc.SEAM_N for k in ("cont", "tie")} | {(n, 192, "cont") for n in kc.SEAM_N_WIDE}
    assert seen == want and kc.SEAM_N_WIDE == (33, 129, 1025, 2049)
    assert kc.SEAM_N == (31, 32, 33, 127, 128, 129, 257, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 2050, 4097)
    # the children of 2049 / 2050 / 4097 fall on either side of KD_SUB 1024 and KD_TAIL 2048
    assert {2049 // 2, 2049 - 2049 // 2, 2050 // 2} == {1024, 1025} and {4097 // 2, 4097 - 4097 // 2} == {2048, 2049}


def test_dimension_seams(oracle):
    seen = set()
    for name in kc.names("dim"):
        rows, bs, q = kc.make(name)
        _finite(rows)
        n, dd = rows.shape
        kind = name.rsplit("-", 1)[1]
        seen.add((n, dd, kind))
        assert bs == 1 and q is None
        spr = np.ptp(rows, 0)
        if kind == "last":
            assert not spr[:dd - 1].any() and spr[dd - 1] > 0
            assert rows[0, :dd - 1].any() or dd == 1  # the constant columns are not all zero
            assert _root_cut(oracle, rows) == dd - 1
            assert np.unique(rows[:, dd - 1]).size == 7  # tie-heavy: deep nodes of one value have no spread at all
        elif kind == "three":
            assert set(np.unique(rows).tolist()) == {0.0, 0.25, 0.5}
            assert (spr == 0.5).all()  # every dimension ties for the maximum: the first one wins
            assert _root_cut(oracle, rows) == 0
        else:
            assert np.unique(spr).size == dd and _root_cut(oracle, rows) == int(np.argmax(spr))
    assert seen == {(n, dd, k) for n in kc.DIM_N for dd in kc.SEAM_DD for k in ("three", "cont", "last")}
    assert kc.SEAM_DD == (1, 2, 63, 64, 65, 255, 256, 257, 511, 513) and kc.DIM_N == (1500, 3000)


def test_zero_and_equal_spreads(oracle):
    seen = set()
    for name in kc.names("spread"):
        rows, bs, q = kc.make(name)
        _finite(rows)
        n, dd = rows.shape
        kind = name.split("-")[1]
        assert q is not None and q.shape[1] == dd
        spr = np.ptp(rows, 0)
        if kind == "identical":
            seen.add((kind, n, bs))
            assert (rows == rows[0]).all() and rows[0].all()
            pos, (cd, cv, _, _) = _tree(oracle, rows, bs)
            if n > bs:
                assert not cd.any()  # every node: dimension 0
                assert cv[n // 2] == rows[0, 0]
        elif kind == "oneoff":
            seen.add((kind, n, bs))
            differs = (rows != rows[0]).any(1)
            assert differs.sum() == 1 and np.flatnonzero(spr).tolist() == [5]
            pos, (cd, _, _, _) = _tree(oracle, rows, bs)
            assert cd[n // 2] == 5
            m = np.ones(n, bool)
            m[[0, n // 2]] = False
            assert (cd[m] == 0).sum() > (n - 2) // (2 * bs)  # the nodes off the odd row's path have no spread
        else:
            d1, d2 = int(name.split("-")[2]), int(name.split("-")[3])
            seen.add((kind, d1, d2, dd, n))
            assert bs == 1
            assert _bits(spr[d1]) == _bits(spr[d2]) and spr[d1] == 16.0
            others = np.delete(spr, [d1, d2])
            assert others.max() < spr[d1]
            assert int(np.argmax(spr)) == min(d1, d2)  # numpy's first maximum
            assert _root_cut(oracle, rows) == min(d1, d2)
            # the other choice would sort the node the other way round
            assert np.array_equal(rows[:, d2], np.float32(16.0) - rows[:, d1]) and np.unique(rows[:, d1]).size > 32
            half = rows[np.argsort(rows[:, d1], kind="stable")[:n // 4]]  # a deep node's like: still equal bits
            assert _bits(np.ptp(half[:, d1])) == _bits(np.ptp(half[:, d2]))
    want = {(k, n, bs) for bs in (1, 4) for k, ns in (("identical", kc.IDENT_N), ("oneoff", kc.ONE_OFF_N)) for n in ns}
    want |= {("equal", d1, d2, dd, n) for d1, d2, dd in kc.EQUAL_PAIRS for n in kc.EQUAL_N}
    assert seen == want
    assert kc.IDENT_N == (2, 33, 129, 1025, 2500)
    assert {(a, b) for a, b, _ in kc.EQUAL_PAIRS} == {(3, 40), (5, 69), (5, 261), (260, 7)}
    assert 3 // 64 == 40 // 64 and 5 % 64 == 69 % 64 and 69 // 64 == 1 and 5 % 64 == 261 % 64 and 261 // 256 == 1


def test_signed_zeros(oracle):
    seen = set()
    for name in kc.names("zero"):
        rows, bs, q = kc.make(name)
        _finite(rows)
        n, dd = rows.shape
        seen.add((name.split("-")[1], n))
        assert bs == 1 and dd == 6
        if "signed" in name:
            assert set(np.unique(np.abs(rows)).tolist()) == {0.0, 1.0}
            # duplicated rows whose copies differ in zero signs only
            assert np.unique(_bits(rows), axis=0).shape[0] > 2 * np.unique(rows, axis=0).shape[0]
        else:
            assert np.array_equal(_bits(rows[n // 2:]), _bits(-rows[:n // 2]))
            assert not np.signbit(rows[:n // 2][rows[:n // 2] == 0]).any()  # A's zeros are +0.0, their twins -0.0
            assert (rows[:n // 2] == 0).mean() > 0.4
        col = rows[:, _root_cut(oracle, rows)]
        assert (np.signbit(col) & (col == 0)).any() and (~np.signbit(col) & (col == 0)).any()
        assert np.unique(rows, axis=0).shape[0] < n / 2
        # queries: rows of the set and their negations
        h = q.shape[0] // 2
        assert np.array_equal(_bits(q[h:]), _bits(-q[:h]))
        assert all((rows == r).all(1).any() for r in q[:h])
        kd = oracle.KDTree(rows)
        ki, ke = kd.search_batch(q)
        pi_, pe = kd.pri_search_batch(q, 0.0)
        kd.close()
        li, le = oracle.nn_batch(rows, q)
        assert np.array_equal(_bits(ke), _bits(le)) and np.array_equal(_bits(pe), _bits(le))
        assert np.count_nonzero(ki != li) > 0  # the tree's order answers, not the lowest index
    assert seen == {("signed", n) for n in kc.ZERO_N} | {("mirror", n) for n in kc.MIRROR_N}
    assert kc.ZERO_N == (129, 1025, 3000)


def test_subnormals_and_large_magnitudes(oracle):
    kinds = set()
    for name in kc.names("scale"):
        rows, bs, q = kc.make(name)
        _finite(rows)
        n, dd = rows.shape
        kind = name[len("scale-"):name.rindex("-n")]
        kinds.add(kind)
        assert bs == 1 and dd == 8
        spr = np.ptp(rows, 0)
        cut = _root_cut(oracle, rows)
        sub = (np.abs(rows) < kc.TINY) & (rows != 0)
        if kind == "subnormal":
            assert (sub | (rows == 0)).all() and sub.mean() > 0.99
            k = rows.astype(np.float64) / 1e-41
            assert np.abs(k - np.rint(k)).max() < 0.08  # integer multiples of 1e-41, to the subnormal grid (1.4e-45)
            assert cut == 5 == int(np.argmax(spr)) and spr[5] > spr[0]  # flushed spreads would all be 0: dimension 0
        elif kind == "mixed-sub":
            assert (sub | (rows == 0))[:, :4].all() and (np.abs(rows[:, 4:]) >= kc.TINY).all()
            assert 0 < spr.max() < kc.TINY and cut == 2 == int(np.argmax(spr))
            assert (spr[4:] > 0).all() and (spr[4:] < kc.TINY).all()  # normal keys, subnormal differences
        elif kind == "mixed-normal":
            assert (sub | (rows == 0))[:, :4].all() and spr[6] == 1.0 and cut == 6
            assert np.sort(spr)[-2] < kc.TINY  # below the first cuts the subnormal spreads decide
            _, (cd, _, _, _) = _tree(oracle, rows, 1)
            assert (cd[1:] == 2).sum() > 2
        else:
            assert q is None  # squared distances overflow fp32: the reference leaves the search undefined
            assert np.abs(rows).max() > 5e29 and np.abs(rows).max() <= np.float32(1e30)
            if kind == "large-tie":
                assert set(np.unique(rows).tolist()) == {float(np.float32(-1e30)), 0.0, float(np.float32(1e30))}
        if q is not None:
            assert all((rows == r).all(1).any() for r in q)
    assert kinds == {"subnormal", "mixed-sub", "mixed-normal", "large-cont", "large-tie"}


def test_bucket_sizes(oracle):
    seen = set()
    for name in kc.names("bucket"):
        rows, bs, q = kc.make(name)
        _finite(rows)
        n, dd = rows.shape
        seen.add((bs, n))
        assert dd == 16 and set(np.unique(rows).tolist()) <= {0.0, 0.25} and q.shape == (96, 16)
        pos, (cd, cv, _, _) = _tree(oracle, rows, bs)
        if n <= bs:
            assert np.array_equal(pos, np.arange(n))  # one bucket: no split
        else:
            assert n < 3 or np.unique(rows[:, cd[n // 2]]).size < n  # equal keys at the root: the quickselect's order
    assert seen == {(bs, n) for bs in kc.BUCKETS for n in kc.bucket_ns(bs)}
    assert kc.BUCKETS == (2, 3, 4, 8, 64)
    assert all(kc.bucket_ns(bs) == (bs - 1, bs, bs + 1, 2 * bs + 1, 1025, 5000) for bs in kc.BUCKETS)
    # the large ones resolve real ties: the tree's order differs from the lowest index for some query
    rows, bs, q = kc.make("bucket-bs4-n5000")
    kd = oracle.KDTree(rows, bs=bs)
    ki, _ = kd.search_batch(q)
    kd.close()
    assert np.count_nonzero(ki != oracle.nn_batch(rows, q)[0]) > 0


def test_scratch_reuse_inputs(oracle):
    shapes = []
    for name in kc.names("reuse"):
        rows, bs, q = kc.make(name)
        _finite(rows)
        shapes.append(rows.shape)
        assert bs == 1 and q is None and np.unique(rows).size == 4
    assert tuple(shapes) == kc.REUSE == ((20000, 64), (130, 64), (20000, 3))  # big, then small, then big and narrow
