"""Smooth's compare on the GPU at the last bit (smooth.hip against DoTemporalSmoothing main.pas:4071-4119).

Strength is put exactly on cmp = sqrt(sum_k (cur_k - prev_k)^2 * (1/192)) of a pair, and one ulp below it, for the 32
pairs of smooth_pairs.py (cmp in the reference's sequential order; test_smooth_boundary.py proves on the restatement
alone that this is its boundary, and that another summation order or a fused multiply-add moves cmp on these pairs).
A kernel whose fp64 cmp differs in the last bit merges, or fails to merge, in one of the two calls.
"""
import numpy as np
import pytest
import smooth_pairs as sp
from test_gpu_psyv_items import LANE_PER_ITEM, lane_items

from tiler_amd.smooth import smooth_keyframe

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("min_items", [0, LANE_PER_ITEM], ids=["default_dispatch", "lane_per_item"])
def test_smooth_boundary_pairs(gpu, oracle, min_items):
    """F = 2, Q = 33 (last block ragged): position j holds pair j, position 32 a far pair; one call per pair at
    Strength = cmp_j and one at nextafter(cmp_j, 0), random incoming smoothed, a tmpidx.  All six outputs equal the
    restatement's; position j merged in the first call and not in the second.  Run with the descriptors from the
    wave-per-item kernel (the default at this size) and from the lane-per-item kernel (hook at 1)."""
    P = sp.pairs(oracle)
    (tile, pal, hm, vm, sm, tmp), exp = sp.boundary_expected(oracle)
    with lane_items(gpu, min_items):
        for j in range(32):
            c = float(P["cmp"][j])
            for strength, o, merged in ((c, exp[j][0], True), (float(np.nextafter(c, 0.0)), exp[j][1], False)):
                g = smooth_keyframe(tile, pal, hm, vm, sm, P["palpix"], P["pals"], strength, tmpidx=tmp)
                where = f"pair {j} ({P['kind'][j]}) cmp {c!r} strength {strength!r}"
                for a, b in zip(g, o):
                    assert np.array_equal(a, b), where
                item = lambda f: tuple(int(x[f, j]) for x in g[:4])  # noqa: E731
                if merged:
                    win = P["prev"][j] if P["cur"][j][0] >= P["prev"][j][0] else P["cur"][j]
                    assert g[4][1, j] == 1 and item(0) == item(1) == tuple(int(x) for x in win), where
                else:
                    assert g[4][1, j] == 0 and item(0) == tuple(int(x) for x in P["prev"][j]) \
                        and item(1) == tuple(int(x) for x in P["cur"][j]), where


def _chain_cases(oracle):
    """(A, A', X, B) with A a base tile, A' its one-pixel twin (a higher tile index, cmp(A, A') far below cmp(A, B)),
    X and B unrelated tiles: the boundary pair is (A, B)."""
    pp, pals = sp.tileset()
    rng = np.random.default_rng(4102)
    cases = []
    for a_t in (3, 17, 30, 41):
        p, h, v = (int(x) for x in rng.integers(0, [sp.N_PALS, 2, 2]))
        A, A1 = (a_t, p, h, v), (a_t + sp.N_BASE, p, h, v)
        # B below A in tile index for two cases (step 2 rewrites frame 1), above for the others
        B = ((a_t - 2) if len(cases) % 2 else (a_t + 100), int(rng.integers(0, sp.N_PALS)), v, h)
        xs = [(t, 3, h ^ 1, v ^ 1) for t in range(sp.N_BASE) if t != a_t]  # X: the farthest of these from A
        d = sp.descriptors(oracle, pp, pals, [A, A1, B] + xs)
        c_ab = float(sp.cmp_reference(d[2:3], d[0:1])[0])
        c_aa1 = float(sp.cmp_reference(d[1:2], d[0:1])[0])
        c_a1b = float(sp.cmp_reference(d[2:3], d[1:2])[0])
        c_x = sp.cmp_reference(np.repeat(d[0:1], len(xs), 0), d[3:])
        X, c_xa = xs[int(np.argmax(c_x))], float(c_x.max())
        # step 1 merges the twins and not X; a kernel holding the twin's row at step 2 would compare another cmp
        assert 0 < c_aa1 < 0.5 * c_ab and c_xa > 1.05 * c_ab and c_a1b != c_ab, (c_aa1, c_ab, c_xa, c_a1b)
        cases.append((A, A1, X, B, c_ab))
    return pp, pals, cases


def test_smooth_three_frame_chains_on_boundary(gpu, oracle):
    """F = 3, the boundary pair (A, B) at step 2, step 1 ending each of its three ways: position 0 no merge (X, A,
    B), position 1 a merge that keeps the previous item (A, A', B: frame 1 becomes A), position 2 a merge that
    rewrites frame 0 (A', A, B).  At step 2 the row in the prev registers must be A's in all three: merged at
    Strength = cmp(A, B), not merged one ulp below, everything equal to the restatement."""
    pp, pals, cases = _chain_cases(oracle)
    rng = np.random.default_rng(5)
    for A, A1, X, B, c in cases:
        m = np.array([[X, A, A1], [A, A1, A], [B, B, B]], np.int32)  # [F = 3, Q = 3, 4]
        tile, pal = np.ascontiguousarray(m[..., 0]), np.ascontiguousarray(m[..., 1])
        hm, vm = m[..., 2].astype(np.uint8), m[..., 3].astype(np.uint8)
        sm = rng.integers(0, 2, tile.shape).astype(np.uint8)
        tmp = rng.integers(-1, 1000, tile.shape).astype(np.int32)
        for strength, merged in ((c, True), (float(np.nextafter(c, 0.0)), False)):
            g = smooth_keyframe(tile, pal, hm, vm, sm, pp, pals, strength, tmpidx=tmp)
            o = oracle.smooth(tile, pal, hm, vm, sm, pp, pals, strength, tmpidx=tmp)
            where = f"A {A} B {B} cmp {c!r} strength {strength!r}"
            for a, b in zip(g, o):
                assert np.array_equal(a, b), where
            assert g[0][0].tolist() == [X[0], A[0], A[0]], where  # step 1's three ends
            if merged and B[0] < A[0]:  # step 2 rewrote frame 1: B's item and B's incoming flag
                assert g[0][1].tolist() == [B[0]] * 3 and g[4][1].tolist() == sm[2].tolist(), where
            else:
                assert g[0][1].tolist() == [A[0]] * 3 and g[4][1].tolist() == [0, 1, 1], where
            assert g[4][2].tolist() == [int(merged)] * 3, where
            last = min(A[0], B[0]) if merged else B[0]
            assert g[0][2].tolist() == [last] * 3, where
