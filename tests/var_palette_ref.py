"""CPU restatement of the value-at-risk palette path, DoValueAtRiskBased (main.pas:2256-2394) with QuantizePalette's
common tail (main.pas:2413-2417), in plain Python / numpy.  It is what tiler_quantize_palettes_var is compared against.

One deviation from the reference, shared with the GPU path: CMUsage.Sort(@CompareCMUCntHLS) (main.pas:2314) is the
unstable RTL QuickSort over all 2^24 entries with a comparator that is no total order, so the order among used
colours of equal (Count, Hue, Val, Sat) is implementation-defined there; here such ties are in ascending colour value.
"""
from __future__ import annotations

import numpy as np

RED_MUL, GREEN_MUL, BLUE_MUL, LUMA_DIV = 2126, 7152, 722, 10000  # main.pas:25-27, 37
RGB_W = 13                                                       # cRGBw, main.pas:33
CURVATURE = 2.0                                                  # cCurvature, main.pas:594
NO_BEST = (1 << 63) - 1                                          # High(Int64)


def _tdiv(a: int, b: int) -> int:
    """Pascal `div` / C `/`: truncation toward zero."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def muldiv_win(a: int, b: int, c: int) -> int:
    """Windows MulDiv (unit windows in main.pas's uses): a * b / c rounded half away from zero."""
    if c == 0:
        return -1
    if c < 0:
        a, c = -a, -c
    prod = a * b
    add = (a < 0 and b < 0) or (a >= 0 and b >= 0)
    r = _tdiv(prod + c // 2, c) if add else _tdiv(prod - c // 2, c)
    return r if -2147483647 <= r <= 2147483647 else -1


def from_rgb(col: int):  # main.pas:571-576
    return col & 255, (col >> 8) & 255, (col >> 16) & 255


def to_rgb(r: int, g: int, b: int) -> int:  # main.pas:566-569
    return (b << 16) | (g << 8) | r


def rgb_to_hsv(col: int):
    """RGBToHSV, main.pas:3496-3543 -> (h, s, v) bytes."""
    rr, gg, bb = from_rgb(col)
    mx, mn = max(rr, gg, bb), min(rr, gg, bb)
    hh = ss = 0
    ll = mx
    if ll != mn:
        delta = ll - mn
        ss = muldiv_win(delta, 255, ll)
        if rr == ll:
            hh = muldiv_win(42, gg - bb, delta)
        elif gg == ll:
            hh = muldiv_win(42, bb - rr, delta) + 84
        elif bb == ll:
            hh = muldiv_win(42, rr - gg, delta) + 168
        hh = hh % 252 if hh >= 0 else -((-hh) % 252)  # Pascal mod: the dividend's sign
    return hh & 255, ss & 255, ll & 255


def hsv_to_rgb(h: int, s: int, v: int) -> int:
    """HSVToRGB, main.pas:3545-3579 (h, s, v bytes)."""
    if s == 0:
        return to_rgb(v, v, v)
    h = h % 252
    f = h % 42
    h = h // 42
    ls = v * s
    p = v - ls // 255
    q = v - (ls * f) // (255 * 42)
    r = v - (ls * (42 - f)) // (255 * 42)
    return (to_rgb(v, r, p), to_rgb(q, v, p), to_rgb(p, v, r), to_rgb(p, q, v), to_rgb(r, p, v), to_rgb(v, p, q))[h]


def color_luma(col: int) -> int:  # FColorMapLuma, main.pas:4846
    r, g, b = from_rgb(col)
    return (r * RED_MUL + g * GREEN_MUL + b * BLUE_MUL) // LUMA_DIV


def color_compare(c1: int, c2: int) -> int:
    """ColorCompare (main.pas:1557-1571) of two 0x00BBGGRR colours."""
    r1, g1, b1 = from_rgb(c1)
    r2, g2, b2 = from_rgb(c2)
    luma1 = r1 * RED_MUL + g1 * GREEN_MUL + b1 * BLUE_MUL
    luma2 = r2 * RED_MUL + g2 * GREEN_MUL + b2 * BLUE_MUL
    lumadiff = _tdiv(luma1 - luma2, LUMA_DIV)
    dr, dg, db = r1 - r2, g1 - g2, b1 - b2
    return dr * dr * RGB_W + dg * dg * RGB_W + db * db * RGB_W + ((lumadiff * lumadiff) << 5)


def fpc_round(x: float) -> int:
    """FPC Round: to nearest, halves to even (Python's round on a float)."""
    return int(round(x))


def pattern_table(n_palettes: int, palsize: int) -> np.ndarray:
    """gPalettePattern, InitLuts main.pas:627-641, in fp64.  power(i + 2, 2.0) is the exact square."""
    pat = np.zeros((n_palettes, palsize), np.float64)
    f = 0.0
    for i in range(palsize):
        fp = f
        f = float((i + 2) * (i + 2))
        for j in range(n_palettes):
            pat[j, i] = ((j + 1) / n_palettes) * max(float(n_palettes), f - fp) + fp
    for j in range(n_palettes):
        for i in range(palsize):
            pat[j, i] = pat[j, i] / pat[n_palettes - 1, palsize - 1]
    return pat


class Item:  # TCountIndexArray, main.pas:193-196
    __slots__ = ("count", "index", "luma", "hue", "sat", "val")

    def __init__(self, count, index):
        self.count, self.index = int(count), int(index)
        self.hue, self.sat, self.val = rgb_to_hsv(self.index)
        self.luma = color_luma(self.index)

    def keys(self):
        return (self.index, self.luma, self.hue, self.sat, self.val)


def compare_cmulhs(a: Item, b: Item) -> int:  # main.pas:2081-2090
    for x, y in ((a.luma, b.luma), (a.val, b.val), (a.sat, b.sat), (a.hue, b.hue)):
        if x != y:
            return -1 if x < y else 1
    return 0


def fpc_tlist_sort(lst: list, L: int, R: int, compare) -> None:
    """TFPList.Sort: the classic FPC RTL QuickSort."""
    while True:
        i, j = L, R
        p = lst[(L + R) // 2]
        while True:
            while compare(p, lst[i]) > 0:
                i += 1
            while compare(p, lst[j]) < 0:
                j -= 1
            if i <= j:
                lst[i], lst[j] = lst[j], lst[i]
                i += 1
                j -= 1
            if i > j:
                break
        if L < j:
            fpc_tlist_sort(lst, L, j, compare)
        L = i
        if i >= R:
            break


def var_pair(colours, counts, acc0: int, pal_idx: int, n_palettes: int, palsize: int, pattern):
    """One (keyframe, palette) pair from its distinct colours and their counts: steps 2-6 of DoValueAtRiskBased ->
    (the palsize picked items in pick order, [U, CmlPct, merges, stop reason])."""
    # items (main.pas:2301-2310) and the sort (2314): Count descending, Hue, Val, Sat ascending; ties by colour
    usage = [Item(n, c) for c, n in zip(colours, counts)]
    usage.sort(key=lambda it: (-it.count, it.hue, it.val, it.sat, it.index))
    U = len(usage)  # LastUsed + 1 (2316-2322)
    # cut-off (2324-2340)
    cml = 0
    acc = int(acc0)
    for i in range(U):
        acc -= usage[i].count
        if acc <= 0:
            cml = i
            break
    cml = max(cml, min(U, palsize * n_palettes))
    # prune (2348-2388)
    best = NO_BEST
    merges = 0
    while True:
        best_i = -1
        prev_best = best
        best = NO_BEST
        prev = usage[0].index
        for i in range(1, len(usage)):
            cur = usage[i].index
            diff = color_compare(cur, prev)
            if diff < best:
                best, best_i = diff, i
            prev = cur
        if best_i > 0:
            ci, cj = usage[best_i], usage[best_i - 1]
            acc = ci.count + cj.count
            ci.hue = (ci.hue * ci.count + cj.hue * cj.count) // acc
            ci.sat = (ci.sat * ci.count + cj.sat * cj.count) // acc
            ci.val = (ci.val * ci.count + cj.val * cj.count) // acc
            ci.luma = (ci.luma * ci.count + cj.luma * cj.count) // acc
            ci.count = acc
            ci.index = hsv_to_rgb(ci.hue, ci.sat, ci.val)
            del usage[best_i - 1]
            merges += 1
        if len(usage) <= cml or best == prev_best:
            break
    reason = 0 if len(usage) <= cml else 1
    # pick (2391-2393)
    picked = [usage[fpc_round(float(pattern[pal_idx, i]) * (len(usage) - 1))] for i in range(palsize)]
    return picked, [U, cml, merges, reason]


def pair_usage(rgb, pal_of, n_pairs: int, active=None):
    """TrueColorUsage of every pair (main.pas:2270-2299): (colours, counts) per pair, and the pairs' use counts."""
    rgb = np.asarray(rgb, np.int32).reshape(-1, 64)
    pal_of = np.asarray(pal_of, np.int64)
    ok = (pal_of >= 0) & (pal_of < n_pairs)
    if active is not None:
        ok &= np.asarray(active).astype(bool)
    use_count = np.bincount(pal_of[ok], minlength=n_pairs).astype(np.int32)
    keys = (pal_of[ok, None] << 24) | (rgb[ok].astype(np.int64) & 0xFFFFFF)
    uk, cnt = np.unique(keys.reshape(-1), return_counts=True)
    lo = np.searchsorted(uk, np.arange(n_pairs + 1, dtype=np.int64) << 24)
    return [((uk[lo[p]:lo[p + 1]] & 0xFFFFFF).tolist(), cnt[lo[p]:lo[p + 1]].tolist()) for p in range(n_pairs)], \
        use_count


def quantize_palettes_var(rgb, pal_of, n_pairs: int, n_palettes: int, acc0, palsize: int = 16, active=None,
                          pairs=None):
    """QuantizePalette(UseDLv3 = False) for n_pairs (keyframe, palette) pairs, pair = keyframe * n_palettes + palette:
    rgb [n][64] 0x00BBGGRR, pal_of [n], acc0 [n_pairs] -> (palettes [n_pairs][palsize], use_count [n_pairs],
    stats [n_pairs][4]).  A pair without a colour raises ValueError, where the reference reads CMUsage[0] of an empty
    list.  pairs: only these are computed (the others' rows stay 0)."""
    usage, use_count = pair_usage(rgb, pal_of, n_pairs, active)
    pattern = pattern_table(n_palettes, palsize)
    pal = np.zeros((n_pairs, palsize), np.int32)
    stats = np.zeros((n_pairs, 4), np.int32)
    for p in (range(n_pairs) if pairs is None else pairs):
        cols, cnts = usage[p]
        if not cols:
            raise ValueError(f"quantize_palettes_var: pair {p} has no Active tile")
        picked, stats[p] = var_pair(cols, cnts, int(acc0[p]), p % n_palettes, n_palettes, palsize, pattern)
        if palsize > 1:
            fpc_tlist_sort(picked, 0, palsize - 1, compare_cmulhs)  # CMPal.Sort (2413)
        pal[p] = [it.index for it in picked]                        # PaletteIndexes (2415-2417)
    return pal, use_count, stats
