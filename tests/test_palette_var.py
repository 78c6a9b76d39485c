"""The CPU restatement of the value-at-risk palette path (tests/var_palette_ref.py, DoValueAtRiskBased
main.pas:2256-2394) against hand-worked cases, the oracle's RGBToHSV / luma, and its own invariants."""
import ctypes

import numpy as np
import pytest

import var_palette_ref as ref


def grey(g):
    return g | (g << 8) | (g << 16)


def rgb(r, g, b):
    return r | (g << 8) | (b << 16)


PAT2 = ref.pattern_table(2, 16)
BIG = 1 << 30  # an acc0 the counts never reach: CmlPct comes from the min term


def test_pattern_row_by_hand():
    """P = 2, palsize 16: f - fp is 4 at i = 0 and 2 i + 3 after it, the table's last entry is 33 + 256 = 17^2, so
    row 0 is (i + 1)^2 + i + 1.5 over 289 from i = 1 on: it passes one half between i = 10 and i = 11."""
    assert PAT2[0, 0] == 2.0 / 289.0 and PAT2[1, 15] == 1.0
    assert PAT2[0, 10] == 132.5 / 289.0 and PAT2[0, 11] == 156.5 / 289.0
    assert [ref.fpc_round(x) for x in PAT2[0]] == [0] * 11 + [1] * 5


def test_three_colours_one_merge_body_runs_once():
    """U = 3 <= CmlPct = min(3, 16 * 2): the repeat-until body still runs once.  Greys (h = s = 0, v = luma = g):
    counts 3, 2, 1 order them 10, 200, 204; ColorCompare is 71 d^2 on greys, so the first minimum is 71 * 16 at i = 2,
    and grey 204 absorbs grey 200: v = (204 * 1 + 200 * 2) div 3 = 201.  Two items are left: stop by count."""
    assert ref.color_compare(grey(200), grey(10)) == 71 * 190 * 190
    assert ref.color_compare(grey(204), grey(200)) == 71 * 16
    picked, stats = ref.var_pair([grey(204), grey(10), grey(200)], [1, 3, 2], BIG, 0, 2, 16, PAT2)
    assert stats == [3, 3, 1, 0]
    assert [it.index for it in picked] == [grey(10)] * 11 + [grey(201)] * 5
    assert picked[15].keys() == (grey(201), 201, 0, 0, 201) and picked[15].count == 3


def test_single_colour():
    """U = 1: no difference exists, best stays High(Int64) as PrevBest, nothing merges, every pick is the colour."""
    picked, stats = ref.var_pair([rgb(12, 34, 56)], [640], 608, 1, 2, 16, PAT2)
    assert stats == [1, 1, 0, 0]
    assert [it.index for it in picked] == [rgb(12, 34, 56)] * 16


def test_merge_colour_differs_from_both_parents():
    """Black (5), red (255, 0, 0) and (200, 100, 0) (1 each): red is h 0 s 255 v 255 luma 54, the other h 21 s 255
    v 200 luma 114, so the order is black, red, (200, 100, 0).  The differences are 938637 and 280717; the merge gives
    h 10, s 255, v 227, luma 84 and HSVToRGB(10, 255, 227) = (227, 55, 0) -- neither parent, and its own luma is 87:
    the item keeps 84."""
    red, other = rgb(255, 0, 0), rgb(200, 100, 0)
    assert ref.rgb_to_hsv(red) == (0, 255, 255) and ref.color_luma(red) == 54
    assert ref.rgb_to_hsv(other) == (21, 255, 200) and ref.color_luma(other) == 114
    assert ref.color_compare(red, 0) == 938637 and ref.color_compare(other, red) == 280717
    assert ref.hsv_to_rgb(10, 255, 227) == rgb(227, 55, 0) and ref.color_luma(rgb(227, 55, 0)) == 87
    picked, stats = ref.var_pair([0, red, other], [5, 1, 1], BIG, 0, 2, 16, PAT2)
    assert stats == [3, 3, 1, 0]
    assert picked[0].keys() == (0, 0, 0, 0, 0)
    assert picked[15].keys() == (rgb(227, 55, 0), 84, 10, 255, 227) and picked[15].count == 2


def test_lumadiff_truncates_toward_zero():
    """(0, 0, 0) against (0, 2, 0): the un-divided lumas differ by -14304, `div` gives -1 (a floor would give -2),
    so the result is 13 * 4 + (1 shl 5)."""
    assert ref.color_compare(0, rgb(0, 2, 0)) == 13 * 4 + 32
    assert ref.color_compare(rgb(0, 2, 0), 0) == 13 * 4 + 32


def test_stop_by_repeated_best():
    """Greys 0, 10, 20, 30 with counts 8, 4, 2, 1, one palette of one colour (CmlPct = 1): round 1 finds 7100 first
    at i = 1, grey 10 absorbs grey 0 -> v = 40 div 12 = 3; round 2 finds 20519 and 7100, merges 30 and 20 into
    v = 70 div 3 = 23, and its best equals the previous round's: stop with two items left."""
    pat = ref.pattern_table(1, 1)
    assert pat[0, 0] == 1.0
    picked, stats = ref.var_pair([grey(0), grey(10), grey(20), grey(30)], [8, 4, 2, 1], BIG, 0, 1, 1, pat)
    assert stats == [4, 1, 2, 1]
    assert picked[0].keys() == (grey(23), 23, 0, 0, 23) and picked[0].count == 3


def test_cutoff():
    """acc0 against the sorted counts (9, 5, 3, 1): CmlPct is the first i at which the running remainder is <= 0,
    0 if never; then at least min(U, palsize * P)."""
    cols, cnts = [grey(0), grey(60), grey(120), grey(180)], [9, 5, 3, 1]
    pat = ref.pattern_table(1, 2)
    for acc0, want in ((0, 2), (9, 2), (10, 2), (15, 2), (17, 2), (18, 3), (19, 2)):
        assert ref.var_pair(cols, cnts, acc0, 0, 1, 2, pat)[1][1] == want, acc0
    pat1 = ref.pattern_table(1, 1)
    for acc0, want in ((0, 1), (9, 1), (10, 1), (14, 1), (15, 2), (17, 2), (18, 3), (19, 1)):
        assert ref.var_pair(cols, cnts, acc0, 0, 1, 1, pat1)[1][1] == want, acc0


def test_hsv_luma_match_oracle(oracle):
    rng = np.random.default_rng(5)
    cols = rng.integers(0, 1 << 24, 10000).tolist()
    cols += [grey(g) for g in (0, 1, 127, 255)]
    cols += [rgb(255, 0, 0), rgb(0, 255, 0), rgb(0, 0, 255), rgb(255, 255, 0), rgb(0, 255, 255), rgb(255, 0, 255)]
    for mn in (0, 100, 212):  # mx - mn = 43: the hue bytes of saturated colours start to repeat
        cols += [rgb(mn + 43, mn, mn + k) for k in range(44)] + [rgb(mn, mn + 43, mn + k) for k in range(44)]
        cols += [rgb(mn + k, mn, mn + 43) for k in range(44)]
    luma = oracle.lib().or_color_luma
    luma.restype = ctypes.c_int32
    for c in cols:
        assert ref.rgb_to_hsv(c) == oracle.rgb_to_hsv(c), hex(c)
        assert ref.color_luma(c) == luma(ctypes.c_int32(c)), hex(c)


def test_hsv_round_trip_bytes():
    """HSVToRGB's components stay bytes for every hue byte RGBToHSV can give (0..251 and the wrapped negatives
    214..255) at full and partial saturation."""
    for h in range(256):
        for s, v in ((255, 255), (1, 255), (128, 77), (255, 1)):
            c = ref.hsv_to_rgb(h, s, v)
            assert 0 <= c < (1 << 24) and max(ref.from_rgb(c)) == v


def _tiles_without_ties(rng, n_tiles, n_pairs):
    """Tiles over a few colours whose (Hue, Val, Sat) all differ, so no two items of a pair can tie."""
    cols, seen = [], set()
    while len(cols) < 12:
        c = int(rng.integers(0, 1 << 24))
        k = ref.rgb_to_hsv(c)
        if (k[0], k[2], k[1]) not in seen:
            seen.add((k[0], k[2], k[1]))
            cols.append(c)
    cols = np.asarray(cols, np.int32)
    rgbt = cols[rng.integers(0, cols.size, (n_tiles, 64))]
    pal_of = rng.integers(0, n_pairs, n_tiles).astype(np.int32)
    pal_of[:n_pairs] = np.arange(n_pairs)
    return rgbt, pal_of


def test_tile_order_does_not_matter():
    rng = np.random.default_rng(9)
    rgbt, pal_of = _tiles_without_ties(rng, 40, 4)
    acc0 = np.full(4, ref.fpc_round(40 * 64 * 0.95), np.int32)
    want = ref.quantize_palettes_var(rgbt, pal_of, 4, 2, acc0)
    for seed in (1, 2, 3):
        perm = np.random.default_rng(seed).permutation(40)
        got = ref.quantize_palettes_var(rgbt[perm], pal_of[perm], 4, 2, acc0)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)


def test_inactive_and_empty_pair():
    rng = np.random.default_rng(10)
    rgbt, pal_of = _tiles_without_ties(rng, 30, 2)
    active = np.ones(30, np.uint8)
    active[pal_of == 1] = 0
    with pytest.raises(ValueError, match="pair 1"):
        ref.quantize_palettes_var(rgbt, pal_of, 2, 2, np.zeros(2, np.int32), active=active)
    active[np.flatnonzero(pal_of == 1)[0]] = 1
    _, uc, stats = ref.quantize_palettes_var(rgbt, pal_of, 2, 2, np.zeros(2, np.int32), active=active)
    assert uc[1] == 1 and uc[0] == (pal_of == 0).sum() and stats[1, 0] <= 12


@pytest.mark.parametrize("P,palsize", [(2, 16), (128, 16)])
def test_pattern_closed_form(P, palsize):
    """gPalettePattern written out: with fp_i = (i + 1)^2 (0 at i = 0) and gap_i = (i + 2)^2 - fp_i, entry (j, i) is
    ((j + 1) / P * max(P, gap_i) + fp_i) over the last entry max(P, gap_last) + fp_last."""
    i = np.arange(palsize, dtype=np.float64)
    fp = np.where(i == 0, 0.0, (i + 1) * (i + 1))
    gap = (i + 2) * (i + 2) - fp
    j = np.arange(P, dtype=np.float64)[:, None]
    want = ((j + 1) / P * np.maximum(float(P), gap)[None, :] + fp[None, :]) / (max(float(P), gap[-1]) + fp[-1])
    want[P - 1, palsize - 1] = 1.0
    got = ref.pattern_table(P, palsize)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.all(np.diff(got, axis=1) > 0) and got.max() == 1.0
