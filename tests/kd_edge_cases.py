"""TEST INFRASTRUCTURE ONLY: named, seeded inputs at the seams of the GPU kd-tree build (tiler_amd/csrc/kdtree.hip) and
where its shortcuts could part from ANN 1.1.2's plain fp32 compares, shared by test_kdtree_edge_inputs.py (the
restatement alone: every input holds what it claims) and test_gpu_kdtree_edges.py (the GPU build and searches against
the restatement).  make(name) -> (rows float32 [n, dd], bs, queries float32 [nq, dd] or None); names(family) lists a
family's cases.  No GPU code and no oracle here.

Families (the constants are kdtree.hip's):
  a size   n on either side of KD_DFS 32, KD_CH 128, 256, KD_SUB 1024, KD_TAIL 2048 and of 2 * 1024 and 4 * 1024 (the
           children of a big node on either side of KD_SUB / KD_TAIL), dd = 8 continuous and two-valued, dd = 192
  b dim    dd on either side of the 64-lane and 256-dimension strides of kd_minmax and of KD_PD 256, at n = 1,500 (one
           level above the subtree roots) and 3,000 (two), three-valued and continuous, and with only the last
           dimension varying (the cut dimension is the lane past a full stride)
  c spread all rows identical (every spread zero: annMaxSpread answers dimension 0), identical but one row, and two
           dimensions of exactly equal spread in different lanes / 64-blocks / 256-blocks (the first one wins): column
           d2 = 16 - column d1 on a 0.25 grid, so the two spreads are equal in every node, their key orders opposite
  d zero   rows from {-0.0, +0.0, 1, -1} with the zero signs drawn per entry over duplicated rows, and a mirror set
           [A, -A]; ANN compares -0.0 == +0.0, an integer-encoded compare does not
  e scale  subnormal rows (multiples of 1e-41), subnormal beside normal columns with the widest spread on either kind,
           and magnitudes up to 1e30 (spreads finite; squared distances overflow, so no queries there)
  f bucket bs in {2, 3, 4, 8, 64} at n = bs - 1, bs, bs + 1, 2 bs + 1, 1,025 and 5,000, two-valued, dd = 16
  g reuse  the three datasets of the scratch-reuse sequence (20,000 x 64, 130 x 64, 20,000 x 3)
"""
import zlib

import numpy as np

SEAM_N = (31, 32, 33, 127, 128, 129, 257, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 2050, 4097)
SEAM_N_WIDE = (33, 129, 1025, 2049)
SEAM_DD = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513)
DIM_N = (1500, 3000)
IDENT_N = (2, 33, 129, 1025, 2500)
ONE_OFF_N = (33, 1025, 2500)
EQUAL_PAIRS = ((3, 40, 70), (5, 69, 70), (5, 261, 300), (260, 7, 300))  # (d1, d2, dd)
EQUAL_N = (600, 3000)
ZERO_N = (129, 1025, 3000)
MIRROR_N = (130, 1026, 3000)  # even: A and -A
BUCKETS = (2, 3, 4, 8, 64)
REUSE = ((20000, 64), (130, 64), (20000, 3))
TINY = float(np.finfo(np.float32).tiny)  # the smallest normal fp32

_REG = {}  # name -> (family, fn, args)


def _case(family, name, fn, *args):
    assert name not in _REG
    _REG[name] = (family, fn, args)


def names(family):
    return [k for k, v in _REG.items() if v[0] == family]


def make(name):
    _, fn, args = _REG[name]
    rows, bs, q = fn(np.random.default_rng(zlib.crc32(name.encode())), *args)
    rows = np.ascontiguousarray(rows, np.float32)
    return rows, bs, None if q is None else np.ascontiguousarray(q, np.float32)


def _grid(rng, n, dd, levels):
    return (rng.integers(0, levels, (n, dd)) * 0.25).astype(np.float32)


def _queries(rng, rows, nq=96, step=0.25):
    """Rows of the set (distance 0, every duplicate a tie) and rows moved by one grid step in two dimensions."""
    n, dd = rows.shape
    a = rows[rng.integers(0, n, nq // 2)]
    b = rows[rng.integers(0, n, nq - nq // 2)].copy()
    for r in b:
        r[rng.integers(0, dd, 2)] += np.float32(step)
    return np.concatenate([a, b])


# ---- a: size seams
def _size(rng, n, dd, levels):
    return (_grid(rng, n, dd, levels) if levels else rng.standard_normal((n, dd))), 1, None


for _n in SEAM_N:
    _case("size", "size-n%d-dd8-cont" % _n, _size, _n, 8, 0)
    _case("size", "size-n%d-dd8-tie" % _n, _size, _n, 8, 2)
for _n in SEAM_N_WIDE:
    _case("size", "size-n%d-dd192-cont" % _n, _size, _n, 192, 0)


# ---- b: dimension seams
def _dim(rng, n, dd, kind):
    if kind == "last":  # every other column constant: only dimension dd - 1 has a spread
        rows = np.repeat(_grid(rng, 1, dd, 9) + np.float32(0.25), n, 0)
        rows[:, dd - 1] = _grid(rng, n, 1, 7)[:, 0]
        return rows, 1, None
    return (_grid(rng, n, dd, 3) if kind == "three" else rng.standard_normal((n, dd))), 1, None


for _n in DIM_N:
    for _dd in SEAM_DD:
        for _kind in ("three", "cont", "last"):
            _case("dim", "dim-n%d-dd%d-%s" % (_n, _dd, _kind), _dim, _n, _dd, _kind)


# ---- c: zero and equal spreads
def _identical(rng, n, bs):
    row = _grid(rng, 1, 8, 9) + np.float32(0.25)
    rows = np.repeat(row, n, 0)
    q = np.concatenate([row, row + np.float32(0.25), _grid(rng, 68, 8, 9)])  # 70 queries: every row ties for each
    return rows, bs, q


def _one_off(rng, n, bs):
    rows, _, q = _identical(rng, n, bs)
    rows[n // 3, 5] += np.float32(2.0)
    return rows, bs, np.concatenate([q, rows[n // 3:n // 3 + 1]])


def _equal_spread(rng, n, d1, d2, dd):
    rows = _grid(rng, n, dd, 2)  # spreads <= 0.25
    rows[:, d1] = _grid(rng, n, 1, 65)[:, 0]  # 0 .. 16 in steps of 0.25
    rows[:n // 8, d1] = np.tile(np.float32([0.0, 16.0]), n)[:n // 8]  # the root certainly spans the whole range
    rows[:, d2] = np.float32(16.0) - rows[:, d1]  # exact: the same spread over any subset, the opposite order
    return rows, 1, _queries(rng, rows)


for _bs in (1, 4):
    for _n in IDENT_N:
        _case("spread", "spread-identical-n%d-bs%d" % (_n, _bs), _identical, _n, _bs)
    for _n in ONE_OFF_N:
        _case("spread", "spread-oneoff-n%d-bs%d" % (_n, _bs), _one_off, _n, _bs)
for _d1, _d2, _dd in EQUAL_PAIRS:
    for _n in EQUAL_N:
        _case("spread", "spread-equal-%d-%d-n%d" % (_d1, _d2, _n), _equal_spread, _n, _d1, _d2, _dd)


# ---- d: signed zeros
def _resign_zeros(rng, rows):
    z = rows == 0
    rows[z] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    return rows


def _zero_queries(rng, rows, nq=96):
    a = rows[rng.integers(0, rows.shape[0], nq // 2)]
    return np.concatenate([a, -a])


def _signed_zero(rng, n):
    base = rng.choice(np.array([0.0, 0.0, 1.0, -1.0], np.float32), (max(4, n // 5), 6))
    rows = _resign_zeros(rng, base[rng.integers(0, base.shape[0], n)].copy())  # duplicates differ in zero signs only
    return rows, 1, _zero_queries(rng, rows)


def _mirror_zero(rng, n):
    base = rng.choice(np.array([0.0, 0.0, 0.0, 1.0, -1.0, 0.5], np.float32), (max(4, n // 6), 6))
    a = base[rng.integers(0, base.shape[0], n // 2)]  # +0.0 only
    rows = np.concatenate([a, -a])  # every +0.0 of A meets a -0.0 twin
    return rows, 1, _zero_queries(rng, rows)


for _n in ZERO_N:
    _case("zero", "zero-signed-n%d" % _n, _signed_zero, _n)
for _n in MIRROR_N:
    _case("zero", "zero-mirror-n%d" % _n, _mirror_zero, _n)


# ---- e: subnormals and large magnitudes
def _sub(rng, n, dd, width):
    return rng.integers(-width, width + 1, (n, dd)).astype(np.float64) * 1e-41


def _subnormal(rng, n):
    rows = _sub(rng, n, 8, 300)
    rows[:, 5] = _sub(rng, n, 1, 1000)[:, 0]  # the widest (not dimension 0, which a flushed spread would pick)
    rows = rows.astype(np.float32)
    return rows, 1, rows[rng.integers(0, n, 70)]  # every squared distance underflows to 0: all rows tie


def _mixed(rng, n, widest):
    """Columns 0-3 subnormal, 4-7 normal values whose differences are subnormal (3e-38 + k * 1e-41); widest = 'sub':
    column 2 carries the widest spread, 8e-39; widest = 'normal': column 6 is two-valued {0, 1} on top, so it is cut
    first and the subnormal-scale spreads decide below."""
    rows = _sub(rng, n, 8, 300)
    rows[:, 4:] = 3e-38 + np.abs(_sub(rng, n, 4, 100))
    rows[:, 2] = _sub(rng, n, 1, 400)[:, 0]
    if widest == "normal":
        rows[:, 6] = rng.integers(0, 2, n)
    rows = rows.astype(np.float32)
    return rows, 1, rows[rng.integers(0, n, 70)]


def _large(rng, n, levels):
    if levels:
        return (rng.integers(-1, 2, (n, 8)) * 1e30), 1, None
    return rng.uniform(-1e30, 1e30, (n, 8)), 1, None


for _n in (300, 2500):
    _case("scale", "scale-subnormal-n%d" % _n, _subnormal, _n)
    _case("scale", "scale-mixed-sub-n%d" % _n, _mixed, _n, "sub")
    _case("scale", "scale-mixed-normal-n%d" % _n, _mixed, _n, "normal")
    _case("scale", "scale-large-cont-n%d" % _n, _large, _n, 0)
    _case("scale", "scale-large-tie-n%d" % _n, _large, _n, 3)


# ---- f: bucket sizes
def bucket_ns(bs):
    return (bs - 1, bs, bs + 1, 2 * bs + 1, 1025, 5000)


def _bucket(rng, n, bs):
    rows = _grid(rng, n, 16, 2)
    return rows, bs, _queries(rng, rows)


for _bs in BUCKETS:
    for _n in bucket_ns(_bs):
        _case("bucket", "bucket-bs%d-n%d" % (_bs, _n), _bucket, _n, _bs)


# ---- g: scratch reuse
def _reuse(rng, n, dd):
    return _grid(rng, n, dd, 4), 1, None


for _n, _dd in REUSE:
    _case("reuse", "reuse-n%d-dd%d" % (_n, _dd), _reuse, _n, _dd)
