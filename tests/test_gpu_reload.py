"""GPU tests of the GlobalTiling reload branch (tiler_amd/csrc/reload.hip): the batched GetMinMatchingDissim against
pyoracle.km_get_min, tiler_tileset_match against the restatement of test_reload.py, and the chain end to end."""
import ctypes

import numpy as np
import pytest

from test_reload import parse_gts, restate_match, restate_reload
from tiler_amd import global_tiling as gt
from tiler_amd import synth

pytestmark = pytest.mark.gpu

GROUP_SIZES = (0, 1, 63, 65, 571)  # off the 64-row LDS stage on both sides; the last crosses slice boundaries
# (first, second) rows of the 571-row group made identical: across the stage boundaries of a 2-slice launch (64, 128
# of slice 0; 286 + 64 of slice 1), across its slice boundary (285 | 286), across the 36-row slices of the default
# 16-slice launch, and inside one stage
DUP_571 = [(63, 64), (127, 128), (285, 286), (280, 290), (349, 350), (35, 36), (71, 72), (107, 108), (143, 144),
           (200, 500), (1, 569), (300, 301), (10, 20), (400, 450), (64, 570), (0, 2), (215, 216), (251, 252),
           (330, 470), (511, 512)]
DUP_65 = [(0, 64), (32, 33), (5, 60)]  # the 65-row group: rows 0 and 64 lie in different stages


def np_dissim(rows, item):
    """kmodes.pas:341-412 on every row at once (to count ties; the oracle is the checker)."""
    r, x = rows.astype(np.int64), item.astype(np.int64)
    mism = (r != x).sum(1)
    ad = np.abs(r - x)
    a8 = np.abs(((r - x + 128) % 256) - 128)  # psubb + pabsb
    slo = sum(ad[:, b:b + 8].sum(1) for b in (16, 32, 48, 64))
    shi = sum(ad[:, b + 8:b + 16].sum(1) for b in (16, 32, 48, 64))
    w0 = (a8[:, 0] + 256 * a8[:, 1] + slo) & 0xFFFF
    w4 = (a8[:, 8] + 256 * a8[:, 9] + shi) & 0xFFFF
    return mism * 2048 + w0 + w4


def primitive_case(kind):
    rng = np.random.default_rng({"lt16": 11, "lt64": 12, "wrap": 13}[kind])
    hi = 16 if kind == "lt16" else 64
    n = sum(GROUP_SIZES)
    rows = rng.integers(0, hi, (n, 80)).astype(np.uint8)
    rows[:, 64:] = rng.integers(0, 2, (n, 16))
    off = np.concatenate([[0], np.cumsum(GROUP_SIZES)]).astype(np.int32)
    for a, b in DUP_571:
        rows[off[4] + b] = rows[off[4] + a]
    for a, b in DUP_65:
        rows[off[3] + b] = rows[off[3] + a]
    m = 300
    items = rng.integers(0, hi, (m, 80)).astype(np.uint8)
    items[:, 64:] = rng.integers(0, 2, (m, 16))
    grp = (np.arange(m) % 5).astype(np.int32)  # group 0 is empty: those items search the whole set
    grp[7::50] = -1
    # items that equal (or nearly equal) a duplicated row: their minimum is a tie
    for t, (a, _) in enumerate(DUP_571):
        items[4 + 5 * t] = rows[off[4] + a]          # searched in the 571-row group
        items[5 * t] = rows[off[4] + a]              # group 0 -> whole set
        items[5 * t, 70] ^= 1                        # (one flag off: still closest to both copies)
    for t, (a, _) in enumerate(DUP_65):
        items[3 + 5 * t] = rows[off[3] + a]
    if kind == "wrap":  # full-range bytes where the asm takes int8 differences and builds the 16-bit words
        for c in (0, 1, 8, 9):
            rows[:, c] = rng.integers(0, 256, n)
            items[:, c] = rng.integers(0, 256, m)
        for a, b in DUP_571:
            rows[off[4] + b] = rows[off[4] + a]
        for t, (a, _) in enumerate(DUP_571):
            items[4 + 5 * t] = rows[off[4] + a]
            items[5 * t, :64] = rows[off[4] + a, :64]
    return rows, off, items, grp


@pytest.fixture(scope="module")
def primitive_refs(oracle):
    """(rows, off, items, grp, idx, dis, ties, fallbacks) per byte range, computed once."""
    refs = {}
    for kind in ("lt16", "lt64", "wrap"):
        rows, off, items, grp = primitive_case(kind)
        idx = np.zeros(items.shape[0], np.int32)
        dis = np.zeros(items.shape[0], np.uint64)
        ties = fallbacks = 0
        for i in range(items.shape[0]):
            g = grp[i]
            whole = g < 0 or off[g + 1] == off[g]
            lo, hi = (0, rows.shape[0]) if whole else (off[g], off[g + 1])
            j, d = oracle.km_get_min(rows[lo:hi], items[i])
            idx[i], dis[i] = lo + j, d
            dd = np_dissim(rows[lo:hi], items[i])
            assert dd.min() == d
            ties += int((dd == d).sum() >= 2)
            fallbacks += int(whole)
        refs[kind] = (rows, off, items, grp, idx, dis, ties, fallbacks)
    return refs


@pytest.mark.parametrize("slices", [0, 2])
@pytest.mark.parametrize("kind", ["lt16", "lt64", "wrap"])
def test_min_matching_dissim_groups(gpu, primitive_refs, kind, slices):
    rows, off, items, grp, idx, dis, ties, fallbacks = primitive_refs[kind]
    assert ties >= 10 and fallbacks >= 10  # a first-wins argmin or a lost fallback cannot pass
    lib = gpu.load()
    assert lib.tiler_debug_reload(0, 0, slices) == 0
    try:
        gi, gd = gt.min_matching_dissim_groups(rows, off, items, grp)
    finally:
        lib.tiler_debug_reload(0, 0, 0)
    assert np.array_equal(gi, idx) and np.array_equal(gd, dis)


def test_min_matching_dissim_groups_two_queries_per_thread(gpu, primitive_refs):
    lib = gpu.load()
    for kind in ("lt16", "wrap"):
        rows, off, items, grp, idx, dis, _, _ = primitive_refs[kind]
        assert lib.tiler_debug_reload(0, 2, 2) == 0
        try:
            gi, gd = gt.min_matching_dissim_groups(rows, off, items, grp)
        finally:
            lib.tiler_debug_reload(0, 0, 0)
        assert np.array_equal(gi, idx) and np.array_equal(gd, dis)


def test_min_matching_dissim_no_rows(gpu):
    items = np.zeros((3, 80), np.uint8)
    gi, gd = gt.min_matching_dissim_groups(np.zeros((0, 80), np.uint8), [0], items, [-1, 0, 5])
    assert (gi == -1).all() and (gd == np.iinfo(np.uint64).max).all()


def test_min_matching_dissim_against_reference_asm(gpu, oracle, primitive_refs):
    ref = oracle.ref_kmodes_lib()
    if ref is None:
        pytest.skip("reference asm not built here: pyoracle.km_get_min (pinned to it by test_oracle_kats) checks")
    rows, off, items, grp, _, _, _, _ = primitive_refs["wrap"]
    gi, gd = gt.min_matching_dissim_groups(rows, off, items, grp)
    for i in range(items.shape[0]):
        g = grp[i]
        lo, hi = (0, rows.shape[0]) if g < 0 or off[g + 1] == off[g] else (off[g], off[g + 1])
        ptrs = (ctypes.c_void_p * int(hi - lo))(*[rows[r].ctypes.data for r in range(lo, hi)])
        best = ctypes.c_uint64()
        bi = ref.ref_get_min(items[i].ctypes.data_as(ctypes.c_void_p), ptrs, ctypes.c_uint64(int(hi - lo)),
                             ctypes.byref(best))
        assert (lo + bi, best.value) == (gi[i], gd[i]), i


# ---- tiler_tileset_match ----
@pytest.fixture(scope="module")
def match_case(oracle):
    rng = np.random.default_rng(21)
    tiles, thm, tvm = synth.tileset(rng, 3000, 16)
    tiles[:300] %= 4                                                  # few colours: other PalSigni values
    tiles[300:400] = (np.arange(100) % 16)[:, None]                   # flat tiles: PalSigni 0
    active = (rng.random(3000) >= 0.1).astype(np.uint8)
    saved = np.concatenate([tiles[rng.choice(3000, 250, replace=False)],      # exact matches exist (dis = 0)
                            rng.integers(0, 16, (150, 64)).astype(np.uint8)])
    saved[390:400] = saved[40:50]  # equal saved tiles: ties
    data16 = gt.write_tileset(saved, np.ones(400, np.uint8), 16)
    data64 = (saved.astype(np.int64) * 4 + rng.integers(0, 4, saved.shape)).astype(np.uint8).tobytes()  # header-less
    ref = {k: restate_match(oracle, tiles, active, parse_gts(d, 16)[0], 16) for k, d in (("16", data16), ("64", data64))}
    return tiles, thm, tvm, active, {"16": data16, "64": data64}, ref


@pytest.mark.parametrize("which,chunk", [("16", 0), ("64", 0), ("16", 1000)])
def test_tileset_match(gpu, match_case, which, chunk):
    tiles, thm, tvm, active, data, ref = match_case
    rpp, ridx, rdis = ref[which]
    assert (rdis[active.astype(bool)] == 0).sum() >= 100 and len(set(ridx.tolist())) > 50
    lib = gpu.load()
    assert lib.tiler_debug_reload(chunk, 0, 0) == 0  # 1000: more tiles than one pass holds
    try:
        with gt.Tileset(data[which], 16) as ts:
            assert ts.n == 400 and ts.file_palsize == int(which)
            pp, idx, dis = ts.match(tiles, active)
    finally:
        lib.tiler_debug_reload(0, 0, 0)
    assert np.array_equal(idx, ridx) and np.array_equal(pp, rpp)
    on = active.astype(bool)
    assert np.array_equal(dis[on], rdis[on])
    assert (idx[~on] == -1).all() and np.array_equal(pp[~on], tiles[~on])  # inactive tiles untouched


def test_tileset_match_wide_palette(gpu, oracle):
    """Bytes >= 16 on both sides (palette size 64): the general kernel."""
    rng = np.random.default_rng(22)
    tiles = rng.integers(0, 64, (500, 64)).astype(np.uint8)
    tiles[:100] = rng.integers(0, 8, (100, 64))
    saved = np.concatenate([tiles[:60], rng.integers(0, 64, (70, 64)).astype(np.uint8)])
    active = np.ones(500, np.uint8)
    data = gt.write_tileset(saved, np.ones(130, np.uint8), 64)
    rpp, ridx, rdis = restate_match(oracle, tiles, active, parse_gts(data, 64)[0], 64)
    with gt.Tileset(data, 64) as ts:
        pp, idx, dis = ts.match(tiles, active)
    assert np.array_equal(idx, ridx) and np.array_equal(pp, rpp) and np.array_equal(dis, rdis)


def test_tileset_match_empty_tileset(gpu):
    tiles = np.arange(128, dtype=np.uint8).reshape(2, 64) % 16
    with gt.Tileset(bytes([16]), 16) as ts:
        pp, idx, _ = ts.match(tiles, np.ones(2, np.uint8))
    assert (idx == -1).all() and np.array_equal(pp, tiles)


# ---- the chain ----
def test_reload_chain_end_to_end(gpu, oracle):
    """Clip A: run_all + save_tileset.  Clip B (another seed, same shape): run_all(reload=...) -- after the reload step
    the tile list equals the restatement + MakeTilesUnique, and the rest of the chain runs to a decodable .gtm."""
    from gtm_read import read_gtm
    from tiler_amd.encoder import Encoder
    from tiler_amd.frame_tiling import FT_MEDIUM
    a = Encoder(synth.video(71, 320, 240, kf_frames=(3, 3), n_palettes=8))
    a.run_all(700, FT_MEDIUM, 0.2)
    data = a.save_tileset()
    assert data[0] == 16 and len(data) == 1 + 64 * int(a.active.sum())
    vb = synth.video(72, 320, 240, kf_frames=(3, 3), n_palettes=8)
    b = Encoder(vb)
    b.do_make_unique()
    thm, tvm, dith, tile0 = b.thm.copy(), b.tvm.copy(), b.dith_pal.copy(), b.tile.copy()
    rpp, ract, ruc, rmi, ridx, rdis = restate_reload(oracle, b.palpix, b.active, b.use_count.astype(np.int32), data, 16)
    idx, dis = b.do_reload_tiling(data)
    assert np.array_equal(idx, ridx)
    assert np.array_equal(b.palpix, rpp) and np.array_equal(b.active, ract) and np.array_equal(b.use_count, ruc)
    assert np.array_equal(b.tile, np.where(rmi[tile0] >= 0, rmi[tile0], tile0))
    assert np.array_equal(b.thm, thm) and np.array_equal(b.tvm, tvm) and np.array_equal(b.dith_pal, dith)
    # the same through run_all, to the end of the chain
    c = Encoder(vb)
    sm = c.run_all(700, FT_MEDIUM, 0.2, reload=data)
    assert sm["tile"].shape == c.tile.shape
    g = read_gtm(oracle, c.save_stream(320, 240, 24.0))
    assert len(g.frames) == c.frames and np.array_equal(g.tiles, c.palpix)
    saved = {bytes(r) for r in parse_gts(data, 16)[0]}
    assert all(bytes(t) in saved for t in c.palpix)
