"""Smooth's compare on its boundary, CPU part: the pairs of smooth_pairs.py against the restatement alone.

Smooth (DoTemporalSmoothing main.pas:4071-4119) merges when |cmp| <= Strength.  For 32 kept item pairs cmp is
recomputed in numpy in the reference's order (CompareEuclideanDCTPtr main.pas:659-675: 192 sequential fp64 adds, then
sqrt(acc * 1/192)), and oracle.smooth must merge at Strength = cmp and must not one ulp below: the boundary the GPU
tests (test_gpu_smooth_boundary.py) stand on is the restatement's own.  The kept pairs are also chosen so that the sums
an optimised kernel would take (8 partial sums of 24 terms, a pairwise tree, t*t fused into the add) give another cmp.

Measured on the pool of 384 pairs of real DCT descriptors (48 random 16-colour tiles with one-pixel and five-pixel
twins, 4 palettes of which two lie 1 and up to 6 RGB steps from the first; one-pixel twins, five-pixel twins, other
mirrors of one tile, one tile under two near palettes, unrelated tiles; cmp from 0.004 to 1.17), the share of pairs
whose cmp a variant changes:
    8 partial sums of 24 terms, added in order   74.7 %
    pairwise tree over neighbours                74.7 %
    t*t fused into the add (fma)                 19.5 %
(math.fma where this Python has it, else the exact rational sum rounded once, which is the same value.)
"""
import numpy as np
import smooth_pairs as sp


def test_pool_and_kept_pairs_are_sensitive(oracle):
    """The conditions of the boundary tests: 32 pairs, half on each side of tile[cur] >= tile[prev], every kind of
    pair present, cmp over several magnitudes, each variant sum changing at least 8 of them, both signs present."""
    P = sp.pairs(oracle)
    assert len(P["cmp"]) == 32 and P["pool"] >= 300
    ge = P["cur"][:, 0] >= P["prev"][:, 0]
    assert int(ge.sum()) == 16 and int((~ge).sum()) == 16
    assert set(P["kind"]) == set(sp.KINDS)
    assert np.all(P["cmp"] > 0) and P["cmp"].max() / P["cmp"].min() > 100
    both_signs = 0
    for name, v in P["var"].items():
        assert int(np.count_nonzero(v != P["cmp"])) >= 8, name
        both_signs += bool(np.any(v > P["cmp"]) and np.any(v < P["cmp"]))
    assert both_signs >= 1
    # the variants are different sums, not one sum under three names
    assert np.any(P["var"]["partial8"] != P["var"]["tree"]) and np.any(P["var"]["fma"] != P["var"]["tree"])
    # the docstring's shares are this pool's (to the printed digit)
    for name, pct in (("partial8", 74.7), ("tree", 74.7), ("fma", 19.5)):
        assert abs(100 * P["share"][name] - pct) < 0.05, (name, P["share"][name])


def test_numpy_cmp_is_the_restatements_boundary(oracle):
    """Each kept pair alone (F = 2, Q = 1): oracle.smooth merges at Strength = cmp, in the branch the tile indices
    pick, and leaves both frames alone at nextafter(cmp, 0)."""
    P = sp.pairs(oracle)
    for j in range(32):
        prev, cur, c = P["prev"][j], P["cur"][j], float(P["cmp"][j])
        cols = [np.array([[prev[k]], [cur[k]]]) for k in range(4)]
        sm = np.array([[1], [0]], np.uint8)
        tmp = np.array([[11], [22]], np.int32)
        t, p, h, v, s, ti = oracle.smooth(*cols, sm, P["palpix"], P["pals"], c, tmpidx=tmp)
        win = prev if cur[0] >= prev[0] else cur
        for f in range(2):
            assert (t[f, 0], p[f, 0], h[f, 0], v[f, 0]) == tuple(win), j
        assert s[1, 0] == 1 and s[0, 0] == (1 if cur[0] >= prev[0] else 0), j
        assert ti[0, 0] == ti[1, 0] == (11 if cur[0] >= prev[0] else 22), j
        below = float(np.nextafter(c, 0.0))
        assert below < c
        t, p, h, v, s, ti = oracle.smooth(*cols, sm, P["palpix"], P["pals"], below, tmpidx=tmp)
        for k, a in enumerate((t, p, h, v)):
            assert a[0, 0] == prev[k] and a[1, 0] == cur[k], j
        assert s[0, 0] == 1 and s[1, 0] == 0 and ti[0, 0] == 11 and ti[1, 0] == 22, j


def test_boundary_maps_isolate_one_pair_per_call(oracle):
    """In the 33-position maps, position j merges at cmp_j and not one ulp below (the GPU test asserts the same of
    the device's output)."""
    P = sp.pairs(oracle)
    maps, exp = sp.boundary_expected(oracle)
    assert maps[0].shape == (2, 33)
    for j, (at, below) in enumerate(exp):
        assert at[4][1, j] == 1 and below[4][1, j] == 0, j
        assert at[0][0, j] == at[0][1, j] and below[0][1, j] == P["cur"][j][0] and below[0][0, j] == P["prev"][j][0]
