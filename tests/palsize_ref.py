"""The CPU restatement at palette sizes 32 and 64.

or_psyv_batch, or_build_ft_dataset and or_smooth stride the palette table by 16 (`palettes + 16 * p`).  A [P][size]
table (size = 16 k) is the same memory as a [k P][16] table, and palette p of the first starts where palette k p of
the second does: with every palette index multiplied by k the restatement reads palettes[p][v] for a tile byte v up
to size - 1, unchanged.  Where it hands palette indices back (or_smooth copies them between items, or_build_ft_dataset
lists them) they are divided by k again."""
import numpy as np


def stride_k(palettes) -> int:
    size = np.asarray(palettes).shape[-1]
    assert size % 16 == 0, size
    return size // 16


def as16(palettes) -> np.ndarray:
    """[P][size] -> the same memory as [k P][16]."""
    return np.ascontiguousarray(palettes, np.int32).reshape(-1, 16)


def psyv_batch(oracle, n, palpix, palettes, pal_of=None, flags_per=None, flags=0, gamma=-1):
    """oracle.psyv_batch for palettes [P][size]; palpix is [n][64], gathered per item."""
    k = stride_k(palettes)
    po = None if pal_of is None else np.asarray(pal_of, np.int32) * k
    return oracle.psyv_batch(n, palpix=palpix, pals=as16(palettes), pal_of=po, flags_per=flags_per, flags=flags,
                             gamma=gamma)


def build_ft_dataset(oracle, used, palpix, thm, tvm, palettes, use_wavelets=True, gamma=-1):
    """oracle.build_ft_dataset for palettes [P][size]: `used` widened to [k P][T][4] with only rows k p populated."""
    k = stride_k(palettes)
    P, T, _ = used.shape
    wide = np.zeros((k * P, T, 4), np.uint8)
    wide[::k] = used
    ds, ti, pi, at = oracle.build_ft_dataset(wide, palpix, thm, tvm, as16(palettes), use_wavelets, gamma)
    assert np.all(pi % k == 0)
    return ds, ti, pi // k, at


def smooth(oracle, tile, pal, hm, vm, smoothed, palpix, palettes, strength, tmpidx=None):
    """oracle.smooth for palettes [P][size]; the palette indices it copies between items are divided back."""
    k = stride_k(palettes)
    t, p, h, v, s, tmp = oracle.smooth(tile, np.asarray(pal, np.int32) * k, hm, vm, smoothed, palpix, as16(palettes),
                                       strength, tmpidx=tmpidx)
    assert np.all(p % k == 0)
    return t, p // k, h, v, s, tmp
