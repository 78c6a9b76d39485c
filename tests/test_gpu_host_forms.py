"""GPU tests of the host-buffer entry points as a family (tiler_amd/csrc/stage.hpp): every host form against its _dev
form on the same inputs byte for byte, optional arrays passed as NULL, the _dev callee's error message after staging,
and the stream / block pool under concurrent callers.  What each operation computes is checked by its own module."""
import ctypes
import threading

import numpy as np
import pytest

from tiler_amd import global_tiling as gt

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
SIZES = (1, 257)  # 257: odd, no multiple of 4 -- byte arrays end inside a 256-byte block
FRAMES = ((2, 1, 1), (3, 3, 1))  # (F, tm_w, tm_h): Q = 1 and Q = 3


def hp(a):
    return None if a is None else a.ctypes.data_as(vp)


def dp(t):
    return None if t is None else vp(t.data_ptr())


def dev(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(a).cuda() for a in arrays]


def same(got, want, names):
    for name, g, w in zip(names, got, want):
        g = g if isinstance(g, np.ndarray) else g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), name


def ok(gpu, rc):
    assert rc == 0, gpu.last_error()


# ---- inputs ----
def dither_case(n, seed=1):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 1 << 24, (n, 64)).astype(np.int32)
    pal_of = rng.integers(0, 3, n).astype(np.int32)
    palettes = rng.integers(0, 1 << 24, (3, 16)).astype(np.int32)
    return rgb, pal_of, palettes


def dither_host(lib, case, mixed):
    rgb, pal_of, palettes = case
    n = rgb.shape[0]
    out = np.zeros((n, 64), np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    if mixed == 0:
        rc = lib.tiler_dither_tiles(n, hp(rgb), hp(pal_of), hp(palettes), 3, 16, *map(hp, out))
    else:
        rc = lib.tiler_dither_tiles_yliluoma(n, hp(rgb), hp(pal_of), hp(palettes), 3, 16, mixed, *map(hp, out))
    return rc, out


def unique_case(nt, seed=2):
    rng = np.random.default_rng(seed)
    protos = rng.integers(0, 16, (max(1, nt // 4), 64)).astype(np.uint8)
    pp = protos[rng.integers(0, protos.shape[0], nt)]
    act = (rng.random(nt) >= 0.1).astype(np.uint8)
    uc = rng.integers(1, 1001, nt).astype(np.int64)
    return np.ascontiguousarray(pp), act, uc


def unique_host(lib, case):
    pp, act, uc = (a.copy() for a in case)
    nt = pp.shape[0]
    mi = np.zeros(nt, np.int64)
    seg = np.array([0, nt], np.int64)
    rc = lib.tiler_make_tiles_unique(hp(pp), hp(act), hp(uc), hp(mi), nt, hp(seg), 1)
    return rc, (pp, act, uc, mi)


def frames_case(F, tm_w, tm_h, seed=3):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 1 << 24, (F, tm_w * tm_h, 64)).astype(np.int32)
    dst = (src ^ rng.integers(0, 16, src.shape).astype(np.int32)).astype(np.int32)
    return src, dst


def quality_host(lib, case, tm_w, tm_h):
    src, dst = case
    F = src.shape[0]
    corr, sse = np.zeros(F, np.float64), np.zeros((F, 3), np.uint64)
    rc = lib.tiler_frame_quality(hp(src), hp(dst), F, tm_w, tm_h, hp(corr), hp(sse))
    return rc, (corr, sse)


def kmodes_case(sizes, seed=4):
    rng = np.random.default_rng(seed)
    N = sum(sizes)
    X = rng.integers(0, 16, (N, 80)).astype(np.uint8)
    X[:, 64:] = rng.integers(0, 2, (N, 16))
    boff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return X, boff


def kmodes_host(lib, case, k):
    X, boff = case
    k = np.asarray(k, np.int32)
    start = np.zeros(k.size, np.int32)
    labels, cent = np.zeros(X.shape[0], np.int32), np.zeros((int(k.sum()), 80), np.uint8)
    it, cost = np.zeros(k.size, np.int32), np.zeros(k.size, np.uint64)
    rc = lib.tiler_kmodes_batch(hp(X), hp(boff), k.size, hp(k), hp(start), 16, hp(labels), hp(cent), hp(it), hp(cost))
    return rc, (labels, cent, it, cost)


# ---- 1. host form against device form ----
@pytest.mark.parametrize("mixed", [0, 4])
@pytest.mark.parametrize("n", SIZES)
def test_dither(gpu, n, mixed):
    lib = gpu.load()
    case = dither_case(n)
    rc, want = dither_host(lib, case, mixed)
    ok(gpu, rc)
    d_in = dev(*case)
    d_out = dev(*(np.zeros_like(w) for w in want))
    if mixed == 0:
        rc = lib.tiler_dither_tiles_dev(n, *map(dp, d_in), 3, 16, *map(dp, d_out), None)
    else:
        rc = lib.tiler_dither_tiles_yliluoma_dev(n, *map(dp, d_in), 3, 16, mixed, *map(dp, d_out), None)
    ok(gpu, rc)
    same(d_out, want, ("palpix", "hm", "vm"))


def smooth_case(F, Q, T, seed=5):
    rng = np.random.default_rng(seed)
    tile = rng.integers(0, T, (F, Q)).astype(np.int32)
    tile[1:] = np.where(rng.random((F - 1, Q)) < 0.5, tile[:-1], tile[1:])
    pal = rng.integers(0, 2, (F, Q)).astype(np.int32)
    hm, vm = (rng.integers(0, 2, (F, Q)).astype(np.uint8) for _ in range(2))
    palpix = rng.integers(0, 16, (T, 64)).astype(np.uint8)
    palpix[1::2] = palpix[0::2][:palpix[1::2].shape[0]] ^ (rng.random(palpix[1::2].shape) < 0.05)  # near neighbours
    palettes = rng.integers(0, 1 << 24, (2, 16)).astype(np.int32)
    return [tile, tile.copy(), pal, hm, vm, np.zeros((F, Q), np.uint8)], palpix, palettes


def smooth_host(lib, case, with_tmp=True):
    items, palpix, palettes = case
    items = [a.copy() for a in items]
    if not with_tmp:
        items[1] = None
    F, Q = items[0].shape
    rc = lib.tiler_smooth_keyframe(F, Q, *map(hp, items), palpix.shape[0], hp(palpix), 2, hp(palettes), 0.9)
    return rc, items


@pytest.mark.parametrize("F,Q,T", [(2, 1, 1), (3, 3, 257)])
def test_smooth(gpu, F, Q, T):
    lib = gpu.load()
    case = smooth_case(F, Q, T)
    rc, want = smooth_host(lib, case)
    ok(gpu, rc)
    d_items = dev(*case[0])
    d_pp, d_pals = dev(case[1], case[2])
    ok(gpu, lib.tiler_smooth_keyframe_dev(F, Q, *map(dp, d_items), dp(d_pp), dp(d_pals), 0.9, None))
    names = ("tile", "tmpidx", "pal", "hm", "vm", "smoothed")
    same(d_items, want, names)
    # tmpidx is optional: the other five arrays come out the same without it
    rc, got = smooth_host(lib, case, with_tmp=False)
    ok(gpu, rc)
    assert got[1] is None
    same(got[:1] + got[2:], want[:1] + want[2:], names[:1] + names[2:])


def render_case(F, Q, T, seed=6):
    rng = np.random.default_rng(seed)
    items = [rng.integers(0, T, (F, Q)).astype(np.int32), rng.integers(0, 2, (F, Q)).astype(np.int32),
             rng.integers(0, 2, (F, Q)).astype(np.uint8), rng.integers(0, 2, (F, Q)).astype(np.uint8)]
    sm = [rng.integers(0, T, (F, Q)).astype(np.int32), rng.integers(0, 2, (F, Q)).astype(np.int32),
          rng.integers(0, 2, (F, Q)).astype(np.uint8), rng.integers(0, 2, (F, Q)).astype(np.uint8),
          rng.integers(0, 2, (F, Q)).astype(np.uint8)]
    items[0][-1, -1] = T  # one position out of range: counted in invalid, rendered 0
    tiles = [rng.integers(0, 16, (T, 64)).astype(np.uint8), rng.integers(0, 2, T).astype(np.uint8),
             rng.integers(0, 2, T).astype(np.uint8)]
    palettes = rng.integers(0, 1 << 24, (4, 16)).astype(np.int32)
    row0 = (2 * (np.arange(F) % 2)).astype(np.int32)
    return items, sm, tiles, palettes, row0


def render_call(fn, p, case, with_sm, out, invalid, *tail):
    items, sm, tiles, palettes, row0 = case
    F, Q = items[0].shape
    sm = sm if with_sm else [None] * 5
    return fn(F, Q, *map(p, items), *map(p, sm), tiles[0].shape[0], *map(p, tiles), 4, 16, p(palettes), p(row0), 2,
              p(out), p(invalid), *tail)


@pytest.mark.parametrize("F,Q,T", [(2, 1, 1), (3, 3, 257)])
def test_render(gpu, F, Q, T):
    lib = gpu.load()
    case = render_case(F, Q, T)
    d_case = [dev(*case[0]), dev(*case[1]), dev(*case[2])] + dev(case[3], case[4])
    for with_sm in (True, False):  # the smoothed set comes all together or not at all
        out, inv = np.zeros((F, Q, 64), np.int32), np.zeros(F, np.int32)
        ok(gpu, render_call(lib.tiler_render_frames, hp, case, with_sm, out, inv))
        assert inv[-1] >= (0 if with_sm else 1)
        d_out, d_inv = dev(np.zeros_like(out), np.full_like(inv, 7))
        ok(gpu, render_call(lib.tiler_render_frames_dev, dp, d_case, with_sm, d_out, d_inv, None))
        same((d_out, d_inv), (out, inv), ("rgb", "invalid"))
        out2 = np.zeros_like(out)
        ok(gpu, render_call(lib.tiler_render_frames, hp, case, with_sm, out2, None))  # invalid is optional
        same((out2,), (out,), ("rgb without invalid",))


@pytest.mark.parametrize("F,tm_w,tm_h", FRAMES)
def test_frame_quality_and_interframe_correlation(gpu, F, tm_w, tm_h):
    lib = gpu.load()
    case = frames_case(F, tm_w, tm_h)
    rc, want = quality_host(lib, case, tm_w, tm_h)
    ok(gpu, rc)
    d_src, d_dst = dev(*case)
    corr, sse = np.zeros(F, np.float64), np.zeros((F, 3), np.uint64)
    ok(gpu, lib.tiler_frame_quality_dev(dp(d_src), dp(d_dst), F, tm_w, tm_h, hp(corr), hp(sse), None))
    same((corr, sse), want, ("corr", "sse"))
    assert sse.any()
    ic_h, ic_d = np.zeros(F - 1, np.float64), np.zeros(F - 1, np.float64)
    ok(gpu, lib.tiler_interframe_correlation(hp(case[0]), F, tm_w, tm_h, hp(ic_h)))
    ok(gpu, lib.tiler_interframe_correlation_dev(dp(d_src), F, tm_w, tm_h, hp(ic_d), None))
    same((ic_d,), (ic_h,), ("interframe corr",))


def quantize_host(lib, rgb, pal_of, active, bpc=5):
    out = np.zeros((3, 16), np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)
    rc = lib.tiler_quantize_palettes(rgb.shape[0], hp(rgb), hp(pal_of), hp(active), 3, 16, bpc, *map(hp, out))
    return rc, out


@pytest.mark.parametrize("n", SIZES)
def test_quantize_palettes(gpu, n):
    lib = gpu.load()
    rgb, pal_of, _ = dither_case(n, 7)
    active = (np.arange(n) % 5 != 3).astype(np.uint8)
    names = ("palettes", "use_count", "colors")
    rc, want = quantize_host(lib, rgb, pal_of, active)
    ok(gpu, rc)
    got = np.zeros((3, 16), np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)
    ok(gpu, lib.tiler_quantize_palettes_dev(n, *map(dp, dev(rgb, pal_of, active)), 3, 16, 5, *map(hp, got), None))
    same(got, want, names)
    # active is optional: NULL means every tile counts
    rc, all_on = quantize_host(lib, rgb, pal_of, np.ones(n, np.uint8))
    ok(gpu, rc)
    rc, got = quantize_host(lib, rgb, pal_of, None)
    ok(gpu, rc)
    same(got, all_on, names)


def test_kmodes_batch(gpu):
    import torch
    lib = gpu.load()
    case = kmodes_case((5, 12))
    rc, want = kmodes_host(lib, case, (2, 3))
    ok(gpu, rc)
    X, boff = case
    k, start = np.array([2, 3], np.int32), np.zeros(2, np.int32)
    d_X, = dev(X)
    d_l = torch.zeros(17, dtype=torch.int32, device="cuda")
    d_c = torch.zeros((5, 80), dtype=torch.uint8, device="cuda")
    it, cost = np.zeros(2, np.int32), np.zeros(2, np.uint64)
    ok(gpu, lib.tiler_kmodes_batch_dev(dp(d_X), hp(boff), 2, hp(k), hp(start), 16, dp(d_l), dp(d_c), hp(it), hp(cost),
                                       None))
    same((d_l, d_c, it, cost), want, ("labels", "centroids", "n_iter", "cost"))


@pytest.mark.parametrize("nt", SIZES)
def test_make_tiles_unique(gpu, nt):
    lib = gpu.load()
    case = unique_case(nt)
    rc, want = unique_host(lib, case)
    ok(gpu, rc)
    d = dev(*case, np.zeros(nt, np.int64))
    seg = np.array([0, nt], np.int64)
    ok(gpu, lib.tiler_make_tiles_unique_dev(*map(dp, d), nt, hp(seg), 1, None))
    same(d, want, ("palpix", "active", "use_count", "merge_index"))


@pytest.mark.parametrize("nt", SIZES)
def test_tileset_match(gpu, nt):
    lib = gpu.load()
    rng = np.random.default_rng(8)
    saved = rng.integers(0, 16, (40, 64)).astype(np.uint8)
    tiles = rng.integers(0, 16, (nt, 64)).astype(np.uint8)
    tiles[::3] = saved[rng.integers(0, 40, tiles[::3].shape[0])]
    active = (np.arange(nt) % 7 != 2).astype(np.uint8)
    with gt.Tileset(gt.write_tileset(saved, np.ones(40, np.uint8), 16), 16) as ts:
        def host(want_idx, want_dis):
            pp = tiles.copy()
            idx = np.zeros(nt, np.int32) if want_idx else None
            dis = np.zeros(nt, np.uint64) if want_dis else None
            ok(gpu, lib.tiler_tileset_match(ts._h, hp(pp), hp(active), nt, hp(idx), hp(dis)))
            return pp, idx, dis

        want = host(True, True)
        d = dev(tiles, active, np.zeros(nt, np.int32), np.zeros(nt, np.uint64))
        ok(gpu, lib.tiler_tileset_match_dev(ts._h, dp(d[0]), dp(d[1]), nt, dp(d[2]), dp(d[3]), None))
        same((d[0], d[2], d[3]), want, ("palpix", "idx", "dis"))
        pp, idx, dis = host(True, False)  # idx / dis are optional
        assert dis is None
        same((pp, idx), want[:2], ("palpix", "idx only"))
        pp, idx, dis = host(False, True)
        assert idx is None
        same((pp, dis), (want[0], want[2]), ("palpix", "dis only"))


@pytest.mark.parametrize("n", SIZES)
def test_min_matching_dissim_groups(gpu, n):
    lib = gpu.load()
    rows, _ = kmodes_case((n,), 9)
    items, _ = kmodes_case((n,), 10)
    off = np.array([0, n // 3, n], np.int32)  # n = 1: group 0 is empty -> the whole set
    grp = (np.arange(n) % 3 - 1).astype(np.int32)  # -1: no group

    def host(want_idx, want_dis):
        idx = np.zeros(n, np.int32) if want_idx else None
        dis = np.zeros(n, np.uint64) if want_dis else None
        ok(gpu, lib.tiler_min_matching_dissim_groups(hp(rows), n, hp(off), 2, hp(items), hp(grp), n, hp(idx), hp(dis)))
        return idx, dis

    want = host(True, True)
    d = dev(rows, items, grp, np.zeros(n, np.int32), np.zeros(n, np.uint64))
    ok(gpu, lib.tiler_min_matching_dissim_groups_dev(dp(d[0]), n, hp(off), 2, dp(d[1]), dp(d[2]), n, dp(d[3]), dp(d[4]),
                                                     None))
    same(d[3:], want, ("idx", "dis"))
    same(host(True, False)[:1], want[:1], ("idx only",))
    same(host(False, True)[1:], want[1:], ("dis only",))


@pytest.mark.parametrize("n", SIZES)
def test_psyv(gpu, n):
    lib = gpu.load()
    rng = np.random.default_rng(11)
    rgb, pal_of, palettes = dither_case(n, 12)
    palpix = rng.integers(0, 16, (n, 64)).astype(np.uint8)
    tile_of = rng.permutation(n).astype(np.int32)
    flags_per = (16 * rng.integers(0, 4, n)).astype(np.uint8)  # the mirror bits
    # (inputs, flags): descriptors from palettes (DCT, every index array given), and the RGB Haar path
    for ins, flags in (((None, palpix, tile_of, palettes, pal_of, flags_per), 1), ((rgb, None, None, None, None, None), 2)):
        nt, npal = (n, 3) if ins[1] is not None else (0, 0)

        def host(want64):
            o64 = np.zeros((n, 192), np.float64) if want64 else None
            o32 = np.zeros((n, 192), np.float32)
            ok(gpu, lib.tiler_psyv_batch(n, hp(ins[0]), nt, hp(ins[1]), hp(ins[2]), npal, hp(ins[3]), hp(ins[4]),
                                         hp(ins[5]), flags, -1, hp(o64), hp(o32)))
            return o64, o32

        want = host(True)
        assert np.isfinite(want[0]).all() and want[0].any()
        d_in = dev(*ins)
        d_out = dev(np.zeros((n, 192), np.float64), np.zeros((n, 192), np.float32))
        ok(gpu, lib.tiler_psyv_batch_dev(n, *map(dp, d_in), flags, -1, dp(d_out[0]), dp(d_out[1]), None))
        same(d_out, want, ("out64", "out32"))
        same(host(False)[1:], want[1:], ("out32 only",))  # out64 is optional


# ---- 2. the callee's message survives staging ----
def test_callee_message_survives(gpu):
    lib = gpu.load()

    def stale():  # the thread's previous call left another message
        assert lib.tiler_debug_unique(99) == -1 and "hash_bits" in gpu.last_error()

    rgb, pal_of, _ = dither_case(4)
    stale()
    rc, _ = quantize_host(lib, rgb, pal_of, None, bpc=9)
    assert rc == -1 and "bpc in 1..8" in gpu.last_error()
    stale()
    rc, _ = kmodes_host(lib, kmodes_case((3,)), (4,))
    assert rc == -1 and "invalid bin" in gpu.last_error()
    stale()
    palettes = np.zeros((3, 3), np.int32)
    out = np.zeros((4, 64), np.uint8), np.zeros(4, np.uint8), np.zeros(4, np.uint8)
    assert lib.tiler_dither_tiles(4, hp(rgb), hp(pal_of), hp(palettes), 3, 3, *map(hp, out)) == -1
    assert "palette size" in gpu.last_error() and "HIP failure" not in gpu.last_error()
    rc, _ = dither_host(lib, dither_case(4), 0)  # and the next call is served
    ok(gpu, rc)


# ---- 3. the pool under concurrency ----
def test_concurrent_host_forms(gpu):
    lib = gpu.load()
    calls = [lambda: dither_host(lib, dither_case(65), 0), lambda: unique_host(lib, unique_case(130)),
             lambda: quality_host(lib, frames_case(2, 3, 2), 3, 2), lambda: kmodes_host(lib, kmodes_case((12,)), (3,))]
    alone = [c() for c in calls]
    assert all(rc == 0 for rc, _ in alone), gpu.last_error()
    failures = []

    def worker(t):
        for j in range(8):
            i = (t + j) % 4
            rc, got = calls[i]()
            if rc != 0 or any(g.tobytes() != w.tobytes() for g, w in zip(got, alone[i][1])):
                failures.append((t, j, rc))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not failures
