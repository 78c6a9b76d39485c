"""Item pairs whose Smooth distance is known to the last bit (shared by test_smooth_boundary.py and
test_gpu_smooth_boundary.py; not a test module).

DoTemporalSmoothing (main.pas:4071-4119) merges two items when |cmp| <= Strength with
cmp = sqrt(sum_k (cur_k - prev_k)^2 * (1/192)), the 192 terms added one after the other in index order
(CompareEuclideanDCTPtr main.pas:659-675).  Here cmp is recomputed in numpy in exactly that order from the
restatement's descriptors, so a test can put Strength on cmp and one ulp below it; the same sum is also taken in
the orders an optimised kernel would use, to pick pairs on which such a kernel gives another cmp.
"""
import functools
import math
from fractions import Fraction

import numpy as np

INV192 = 1.0 / (64.0 * 3.0)  # cSqrtFactor main.pas:4073
N_BASE = 48                  # tiles [0, 48) random, [48, 96) one-pixel twins, [96, 144) five-pixel twins
N_TILES = 3 * N_BASE
N_PALS = 4
KINDS = ("twin1", "twin5", "mirror", "palstep", "far")
QUOTA = {True: {"twin1": 4, "twin5": 3, "mirror": 3, "palstep": 3, "far": 3},  # tile[cur] >= tile[prev]
         False: {"twin1": 6, "twin5": 5, "far": 5}}                            # tile[cur] <  tile[prev]
HAVE_NATIVE_FMA = hasattr(math, "fma")


def tileset():
    rng = np.random.default_rng(4071)
    pp = np.zeros((N_TILES, 64), np.uint8)
    pp[:N_BASE] = rng.integers(0, 16, (N_BASE, 64))
    pp[N_BASE:2 * N_BASE] = pp[:N_BASE]
    px = rng.integers(0, 64, N_BASE)
    pp[np.arange(N_BASE, 2 * N_BASE), px] = (pp[np.arange(N_BASE), px] + 1) % 16
    pp[2 * N_BASE:] = pp[:N_BASE]
    for t in range(N_BASE):
        px5 = rng.choice(64, 5, replace=False)
        pp[2 * N_BASE + t, px5] = (pp[t, px5] + rng.integers(1, 16, 5)) % 16
    c = rng.integers(0, 256, (N_PALS, 16, 3))
    c[1] = np.clip(c[0] + rng.integers(-1, 2, (16, 3)), 0, 255)  # palette 1: palette 0 one RGB step away
    c[2] = np.clip(c[0] + rng.integers(-6, 7, (16, 3)), 0, 255)  # palette 2: a few steps away
    pals = (c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16)).astype(np.int32)
    return pp, pals


def descriptors(oracle, pp, pals, items):
    """items [n, 4] (tile, pal, hm, vm) -> the restatement's Smooth descriptors [n, 192] (DCT, Q-weighting, gamma -1)."""
    items = np.asarray(items)
    fper = (items[:, 2] * 16 + items[:, 3] * 32).astype(np.uint8)
    return oracle.psyv_batch(items.shape[0], palpix=pp[items[:, 0]], pals=pals, pal_of=items[:, 1].astype(np.int32),
                             flags_per=fper, flags=1 | 8, gamma=-1)


def _terms(a, b):
    t = a - b
    return t * t  # [n, 192], every term rounded on its own


def cmp_reference(a, b):
    """cmp in the reference's order: one fp64 add per term, k = 0..191, for every pair (row) at once."""
    sq = _terms(a, b)
    acc = np.zeros(sq.shape[0], np.float64)
    for k in range(192):
        acc = acc + sq[:, k]
    return np.sqrt(acc * INV192)


def cmp_partial8(a, b):
    """8 partial sums of 24 consecutive terms (one per lane of the chain kernel's group), added in order."""
    sq = _terms(a, b)
    acc = np.zeros(sq.shape[0], np.float64)
    for g in range(8):
        part = np.zeros(sq.shape[0], np.float64)
        for k in range(24 * g, 24 * g + 24):
            part = part + sq[:, k]
        acc = acc + part
    return np.sqrt(acc * INV192)


def cmp_tree(a, b):
    """Pairwise tree over neighbours: 192 -> 96 -> ... -> 3, then (x0 + x1) + x2."""
    v = _terms(a, b)
    while v.shape[1] % 2 == 0:
        v = v[:, 0::2] + v[:, 1::2]
    acc = v[:, 0]
    for k in range(1, v.shape[1]):
        acc = acc + v[:, k]
    return np.sqrt(acc * INV192)


def _fma(x, y, z):
    if HAVE_NATIVE_FMA:
        return math.fma(x, y, z)
    return float(Fraction(x) * Fraction(y) + Fraction(z))  # exact, rounded once: what an fma returns


def cmp_fma(a, b):
    """The sequential sum with t*t contracted into the add (acc = fma(t, t, acc))."""
    t = a - b
    out = np.zeros(t.shape[0], np.float64)
    for r in range(t.shape[0]):
        acc = 0.0
        for k in range(192):
            x = float(t[r, k])
            acc = _fma(x, x, acc)
        out[r] = acc
    return np.sqrt(out * INV192)


VARIANTS = {"partial8": cmp_partial8, "tree": cmp_tree, "fma": cmp_fma}


def _pool_items():
    """(kind, prev item, cur item) candidates; items are (tile, pal, hm, vm)."""
    rng = np.random.default_rng(659)
    out = []
    for t in range(N_BASE):
        p, h, v = int(rng.integers(0, N_PALS)), int(rng.integers(0, 2)), int(rng.integers(0, 2))
        for kind, tw in (("twin1", t + N_BASE), ("twin5", t + 2 * N_BASE)):
            out.append((kind, (t, p, h, v), (tw, p, h, v)))  # cur >= prev
            out.append((kind, (tw, p, h, v), (t, p, h, v)))  # cur <  prev: the branch that rewrites frame i-1
        m = int(rng.integers(1, 4))
        out.append(("mirror", (t, p, h, v), (t, p, h ^ (m & 1), v ^ (m >> 1))))
        out.append(("palstep", (t, 0, h, v), (t, 1 + t % 2, h, v)))
        o = int(rng.integers(0, N_TILES - 1))
        o += o >= t
        out.append(("far", (t, p, h, v), (o, int(rng.integers(0, N_PALS)), int(rng.integers(0, 2)),
                                          int(rng.integers(0, 2)))))
        out.append(("far", (o, p, v, h), (t, int(rng.integers(0, N_PALS)), h, v)))
    return out


@functools.lru_cache(maxsize=None)
def _build(oracle):
    pp, pals = tileset()
    cand = _pool_items()
    kinds = np.array([c[0] for c in cand])
    prev = np.array([c[1] for c in cand], np.int32)
    cur = np.array([c[2] for c in cand], np.int32)
    dp, dc = descriptors(oracle, pp, pals, prev), descriptors(oracle, pp, pals, cur)
    ref = cmp_reference(dc, dp)
    var = {name: fn(dc, dp) for name, fn in VARIANTS.items()}
    ok = ref > 0.0
    share = {name: float(np.mean(v[ok] != ref[ok])) for name, v in var.items()}
    nchg = sum((v != ref).astype(int) for v in var.values())
    ge = cur[:, 0] >= prev[:, 0]
    keep = []
    for side in (True, False):
        for kind, quota in QUOTA[side].items():
            idx = np.nonzero(ok & (ge == side) & (kinds == kind))[0]
            idx = idx[np.argsort(-nchg[idx], kind="stable")]  # pairs that the variant sums move come first
            keep.extend(idx[:quota].tolist())
    keep = np.array(sorted(keep))
    return {"palpix": pp, "pals": pals, "pool": len(cand), "pool_kinds": kinds, "pool_ref": ref, "share": share,
            "kind": kinds[keep], "prev": prev[keep], "cur": cur[keep], "cmp": ref[keep],
            "var": {name: v[keep] for name, v in var.items()}}


def pairs(oracle):
    """The pool (size, the share of it that each variant sum changes) and the 32 kept pairs: prev / cur items, their
    cmp in the reference's order and under each variant."""
    return _build(oracle)


FAR_PAIR = ((5, 3, 0, 0), (77, 0, 1, 1))  # a plain far pair for the spare position


def boundary_maps(P, j=None):
    """F = 2, Q = 33 maps: position q holds kept pair q (frame 0 its prev item, frame 1 its cur item), position 32
    the far pair; smoothed and tmpidx random."""
    rng = np.random.default_rng(1338)
    prev = np.concatenate([P["prev"], np.array([FAR_PAIR[0]], np.int32)])
    cur = np.concatenate([P["cur"], np.array([FAR_PAIR[1]], np.int32)])
    m = np.stack([prev, cur])  # [2, 33, 4]
    tile, pal = m[..., 0].astype(np.int32), m[..., 1].astype(np.int32)
    hm, vm = m[..., 2].astype(np.uint8), m[..., 3].astype(np.uint8)
    sm = rng.integers(0, 2, tile.shape).astype(np.uint8)
    tmp = rng.integers(-1, 1000, tile.shape).astype(np.int32)
    return tile, pal, hm, vm, sm, tmp


@functools.lru_cache(maxsize=None)
def boundary_expected(oracle):
    """oracle.smooth of the boundary maps at Strength = cmp_j and one ulp below, for every kept pair j: computed
    once, shared by the runs of both descriptor kernels."""
    P = pairs(oracle)
    maps = boundary_maps(P)
    out = []
    for j in range(len(P["cmp"])):
        c = float(P["cmp"][j])
        out.append(tuple(oracle.smooth(*maps[:5], P["palpix"], P["pals"], s, tmpidx=maps[5])
                         for s in (c, float(np.nextafter(c, 0.0)))))
    return maps, out
