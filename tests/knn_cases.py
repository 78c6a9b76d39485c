"""TEST INFRASTRUCTURE ONLY: named, seeded, small inputs for the k-nearest searches at every k the suite did not reach
(include/tiler_ann.h promises 1..32), shared by test_knn_case_inputs.py (the oracle alone: every input holds the ties
it claims) and test_gpu_knn_k.py (the GPU searches against the oracle).  make(name) -> (data float32 [n, d], queries
float32 [nq, d]), read-only and built once; every case is searched on trees of bucket size 1 and 4 (BS).  No GPU code.

  ints2    2,000 two-colour 64-d tiles in their 4 orientations (PrepareGlobalDS rows); queries: 120 dataset tiles and
           120 fresh ones.  Dozens of rows share each (integer) distance.
  dups     600 normal rows of d = 24, every row present 2 or 3 times; queries: rows, rows plus small integer offsets,
           random rows.
  orbit    PsyV rows of a 400-tile tileset in 4 orientations (a mirror-orbit index; a fifth of the tiles symmetric, so
           their mirrors are identical rows); queries: 150 frame tiles and 50 dataset rows.
  odd17    1,500 x 17 in 0..3: d % 4 != 0, the small-batch scan is never taken.
  odd300   1,500 x 300 in 0..3: d beyond the scan's and the MFMA shortlist's widths, the exact kernel for every k.
  tiny<n>  n in TINY_N rows of d = 8 in 0..3, for k >= n.
"""
import functools

import numpy as np

BS = (1, 4)
K_SWEEP = (2, 3, 5, 7, 9, 16, 31, 32)  # the batched sweep: K = 8 instances with k < 8, K = 32 instances up to full
K_TINY = (8, 9, 32)
TINY_N = (1, 5, 9, 31, 32, 33)
TIE_CASES = ("ints2", "dups", "orbit")  # >= MIN_TIED queries with a tie across the last slot at every k of K_SWEEP
ORDER_CASES = ("ints2", "dups")  # kd order != index order for >= MIN_ORDER queries at each k of K_ORDER
K_ORDER = (3, 20)
MIN_TIED, MIN_ORDER = 20, 10
INTEGER_CASES = ("ints2", "odd17", "odd300") + tuple(f"tiny{n}" for n in TINY_N)  # fp32 distances exact in any order
SWEEP_CASES = ("ints2", "dups", "orbit", "odd17", "odd300")
TINY_CASES = tuple(f"tiny{n}" for n in TINY_N)


def _ints2(rng):
    import pyoracle
    tiles = (rng.random((2000, 64)) < 0.1).astype(np.uint8)
    gds, _, _ = pyoracle.prepare_global_ds(tiles)
    qs = np.concatenate([tiles[rng.integers(0, 2000, 120)], rng.random((120, 64)) < 0.1])
    return gds, qs


def _dups(rng):
    base = rng.normal(0, 1, (600, 24)).astype(np.float32)
    data = np.concatenate([base, base[::-1], base[:300]])  # every row twice, the first 300 three times
    n, d = data.shape
    qs = np.concatenate([data[rng.integers(0, n, 80)],
                         data[rng.integers(0, n, 80)] + rng.integers(-1, 2, (80, d)),
                         rng.normal(0, 1, (80, d))])
    return data, qs


def _orbit(rng):
    import pyoracle
    from tiler_amd import synth
    tiles, thm, tvm = synth.tileset(rng, 400, sym_share=0.2)
    pals = synth.palettes(rng, 4)
    used = synth.used_one_palette(rng.integers(0, 4, 400).astype(np.int32), 4)
    ods, *_ = pyoracle.build_ft_dataset(used, tiles, thm, tvm, pals)
    q = pyoracle.psyv_batch(150, rgb=synth.frame_tiles(rng, 150), flags=2).astype(np.float32)
    return ods, np.concatenate([q, ods[rng.integers(0, ods.shape[0], 50)]])


def _odd(rng, d):
    data = rng.integers(0, 4, (1500, d))
    qs = np.concatenate([data[rng.integers(0, 1500, 50)], rng.integers(0, 4, (50, d))])
    return data, qs


def _tiny(rng, n):
    return rng.integers(0, 4, (n, 8)), rng.integers(0, 4, (20, 8))


_REG = {"ints2": (15, _ints2), "dups": (16, _dups), "orbit": (23, _orbit), "odd17": (18, _odd, 17),
        "odd300": (19, _odd, 300)}
_REG.update({f"tiny{n}": (100 + n, _tiny, n) for n in TINY_N})


@functools.lru_cache(maxsize=None)
def make(name):
    seed, fn, *args = _REG[name]
    out = tuple(np.ascontiguousarray(a, np.float32) for a in fn(np.random.default_rng(seed), *args))
    for a in out:
        a.setflags(write=False)
    return out


def cases(names=SWEEP_CASES):
    """(name, data, queries, bs) for every named case on both bucket sizes"""
    return [(name,) + make(name) + (bs,) for name in names for bs in BS]
