"""TEST INFRASTRUCTURE ONLY: the Dither step's k-means once more, in plain Python, written from the text in the head
of oracle/kmeans.c (not from its code) so that the C restatement has an independent check, plus the input families
that the host test (test_kmeans_restatement.py) and the GPU test (test_gpu_kmeans_edges.py) share.

Every sum whose order matters is an explicit Python loop over Python floats (IEEE fp64, one rounding per operation,
nothing fused, nothing pairwise):
  distance   sum over d ascending of (x_d - c_d)^2; ties -> the lowest centroid index
  seeding    MT19937(seed), u = genrand_int32 / 2^32 per draw (k draws up front); centre 0 = point floor(u * n);
             centre s with probability D^2 / sum D^2: the sum over 1024 runs of L = ceil(n / 1024) points (sequential
             in a run, then the run sums in order), the pick the first point whose running sum (the runs before it,
             then the points of its run) exceeds u * sum; floor(u * n) when the sum is 0
  Lloyd      assign; stop when no label changes or after max_iter assignments; else every non-empty centroid = the
             mean of its members in point order, summed in runs of 256 members (run sums in order), / count; an empty
             cluster keeps its centroid
"""
import numpy as np

MAX_ITER = 0x7FFFFFFF


# ---- MT19937 (Matsumoto & Nishimura 1998: init_genrand, genrand_int32) ---------------------------------------------
def mt19937_uint32(seed, count):
    """The first `count` outputs of genrand_int32 after init_genrand(seed)."""
    mt = [0] * 624
    mt[0] = seed & 0xFFFFFFFF
    for i in range(1, 624):
        mt[i] = (1812433253 * (mt[i - 1] ^ (mt[i - 1] >> 30)) + i) & 0xFFFFFFFF
    out = []
    pos = 624
    while len(out) < count:
        if pos == 624:
            for i in range(624):
                y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
                v = mt[(i + 397) % 624] ^ (y >> 1)
                if y & 1:
                    v ^= 0x9908B0DF
                mt[i] = v
            pos = 0
        y = mt[pos]
        pos += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        out.append(y)
    return out


def uniforms(seed, count):
    return [float(v) * (1.0 / 4294967296.0) for v in mt19937_uint32(seed, count)]


# ---- the restatement -----------------------------------------------------------------------------------------------
def dist2(x, c):
    acc = 0.0
    for a, b in zip(x, c):
        t = a - b
        acc = acc + t * t
    return acc


def seed_centres(rows, k, seed=0):
    """k-means++ -> (centres as row copies, picked point indices)."""
    n = len(rows)
    u = uniforms(seed, k)
    picks = [min(int(u[0] * float(n)), n - 1)]
    L = (n + 1023) // 1024
    mind2 = None
    for s in range(1, k):
        c = rows[picks[-1]]
        d2 = [dist2(x, c) for x in rows]
        mind2 = d2 if mind2 is None else [v if v < m else m for v, m in zip(d2, mind2)]
        part = []
        for r in range(1024):
            acc = 0.0
            for i in range(r * L, min((r + 1) * L, n)):
                acc = acc + mind2[i]
            part.append(acc)
        S = 0.0
        for v in part:
            S = S + v
        if S > 0.0:
            target = u[s] * S
            run = 0.0
            p = None
            for r in range(1024):
                if run + part[r] > target:
                    acc = run
                    end = min((r + 1) * L, n)
                    for i in range(r * L, end):
                        acc = acc + mind2[i]
                        if acc > target:
                            p = i
                            break
                    if p is None:  # the run's sum passed the target, its points summed from `run` did not
                        p = end - 1
                    break
                run = run + part[r]
            if p is None:
                p = n - 1
        else:
            p = min(int(u[s] * float(n)), n - 1)
        picks.append(p)
    return [list(rows[p]) for p in picks], picks


def kmeans(X, k, max_iter=MAX_ITER, seed=0):
    """X [n][d] fp64 -> (labels int32 [n], centroids fp64 [k][d], assignments made)."""
    X = np.ascontiguousarray(X, np.float64)
    n, d = X.shape
    rows = [[float(v) for v in r] for r in X]
    cent, _ = seed_centres(rows, k, seed)
    labels = [-1] * n
    it = 0
    while it < max_iter:
        changed = 0
        for i, x in enumerate(rows):
            best, bc = None, -1
            for c in range(k):
                v = dist2(x, cent[c])
                if best is None or v < best:
                    best, bc = v, c
            if labels[i] != bc:
                labels[i] = bc
                changed += 1
        it += 1
        if changed == 0 or it >= max_iter:
            break
        members = [[] for _ in range(k)]
        for i, c in enumerate(labels):
            members[c].append(i)
        for c in range(k):
            m = members[c]
            if not m:
                continue
            total = [0.0] * d
            for b in range(0, len(m), 256):
                run = [0.0] * d
                for i in m[b:b + 256]:
                    x = rows[i]
                    for t in range(d):
                        run[t] = run[t] + x[t]
                for t in range(d):
                    total[t] = total[t] + run[t]
            cent[c] = [v / float(len(m)) for v in total]
    return np.asarray(labels, np.int32), np.asarray(cent, np.float64).reshape(k, d), it


# ---- input families (host sizes: n <= 300, d <= 12, k <= 40; the GPU test passes the issue's sizes) -----------------
def identical_points(n, d, seed=0):
    """n copies of one random row: every D^2 is 0 (the S == 0 picks), every distance ties over all centroids, and the
    mean of n equal doubles is in general not that double, so the labels walk from centroid to centroid."""
    row = np.random.default_rng(seed).normal(0, 10, d)
    return np.repeat(row[None, :], n, 0)


def few_distinct(n, d, distinct, seed=0):
    """`distinct` random rows repeated round-robin to n points: once every distinct row is a centre the remaining
    D^2 sum is 0."""
    rows = np.random.default_rng(seed).normal(0, 10, (distinct, d))
    return rows[np.arange(n) % distinct].copy()


def tie_points(m, d, seed=0):
    """4 m integer-valued points c0 +- v_j, c1 +- v_j, the v_j with pairwise disjoint supports (orthogonal): once
    c + v_a and c - v_a are both centres, every c +- v_j (j != a) is at exactly the same distance from the two
    (|v_j - v_a|^2 = |v_j + v_a|^2 = |v_j|^2 + |v_a|^2, exact in fp64 at these magnitudes).  Needs d >= m."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-20, 21, (2, d)).astype(np.float64)
    c[1] += 300.0 * (rng.integers(0, 2, d) * 2 - 1)
    v = np.zeros((m, d))
    dims = rng.permutation(d)
    for j in range(m):
        own = dims[j::m]
        v[j, own] = rng.integers(1, 9, own.size) * (rng.integers(0, 2, own.size) * 2 - 1)
    pts = np.concatenate([c[0] + v, c[0] - v, c[1] + v, c[1] - v])
    return pts[rng.permutation(pts.shape[0])]


def cloud(n, d, k, seed=0, spread=3.0):
    """Gaussian blobs around max(2, k // 2) centres (fewer blobs than centroids: Lloyd takes a while)."""
    rng = np.random.default_rng(seed)
    centers = rng.normal(0, 10, (max(2, k // 2), d))
    return centers[rng.integers(0, centers.shape[0], n)] + rng.normal(0, spread, (n, d))


def blobs(sizes, d, seed=0):
    """Well-separated blobs of the given sizes, shuffled: with one seed in each, the first assignment gives clusters of
    exactly these sizes."""
    rng = np.random.default_rng(seed)
    centers = rng.normal(0, 1000, (len(sizes), d))
    pts = np.concatenate([c + rng.normal(0, 1, (s, d)) for c, s in zip(centers, sizes)])
    return pts[rng.permutation(pts.shape[0])]


def tied_points_of(X, cent):
    """Indices of the points whose smallest distance (the text's sequential sum) is attained by two centroids that
    are different rows: an exact tie that is no duplicate centre."""
    rows = [[float(v) for v in r] for r in np.asarray(X, np.float64)]
    cs = [[float(v) for v in r] for r in np.asarray(cent, np.float64)]
    out = []
    for i, x in enumerate(rows):
        ds = [dist2(x, c) for c in cs]
        best = min(ds)
        at = [j for j, v in enumerate(ds) if v == best]
        if any(cs[j] != cs[at[0]] for j in at[1:]):
            out.append(i)
    return out


def same(a, b):
    """(labels, centroids, iterations) equal bit for bit."""
    return (a[2] == b[2] and np.array_equal(a[0], b[0]) and a[1].shape == b[1].shape and
            np.array_equal(np.ascontiguousarray(a[1]).view(np.uint64), np.ascontiguousarray(b[1]).view(np.uint64)))
