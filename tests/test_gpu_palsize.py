"""GPU tests for tile palettes of 32 and 64 colours (cbxPalSize main.lfm:452-470 -> FTilePaletteSize): Dither
(Thomas Knoll and Yliluoma), PsyV from palettes, PrepareFrameTiling's candidates, FrameTiling, the k = 8 preselection
over 64-d rows with values to 63, Smooth and the chain to the .gtm file, each against the CPU restatement (through the
stride-16 view of palsize_ref.py where the restatement strides palettes by 16), and the 16-entry entry points against
their _ps forms."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

import dither_extremes as dx
import palsize_ref
from tiler_amd import synth
from tiler_amd._lib import TilerError
from tiler_amd.dither import dither_tiles

pytestmark = pytest.mark.gpu

GREY, GREY_TWIN = (100, 100, 100), (117, 90, 149)  # distinct colours, LumaPal 1,000,000 each


def _luma(pals):
    return (pals & 255) * 2126 + ((pals >> 8) & 255) * 7152 + ((pals >> 16) & 255) * 722


def _dither_palettes(rng, P, size):
    """Even palettes carry ties above entry 16 (a duplicate colour, and a pair of distinct colours of equal luma);
    odd palettes have distinct lumas."""
    dup, pair = ((19, 41), (37, 52)) if size == 64 else ((19, 27), (21, 30))
    while True:
        pals = synth.rgb_pack(*rng.integers(0, 256, (3, P, size))).astype(np.int32)
        pals[0::2, dup[1]] = pals[0::2, dup[0]]
        pals[0::2, pair[0]], pals[0::2, pair[1]] = synth.rgb_pack(*GREY), synth.rgb_pack(*GREY_TWIN)
        ties = np.array([np.unique(_luma(p)).size < size for p in pals])
        if ties[0::2].all() and not ties[1::2].any():
            return pals, ties


@pytest.mark.parametrize("n,P,size", [(1, 1, 32), (5, 3, 32), (131, 4, 64), (333, 8, 64)])
def test_dither_thomas_knoll_bit_exact(gpu, oracle, n, P, size):
    rng = np.random.default_rng(n * 7 + size)
    rgb = synth.frame_tiles(rng, n)
    pal_of = (np.arange(n) % P).astype(np.int32)  # every palette used, the tie palettes among them
    pals, ties = _dither_palettes(rng, P, size)
    assert _luma(pals[0])[[37, 52] if size == 64 else [21, 30]].tolist() == [1000000, 1000000]
    assert ties[pal_of].any() and (P == 1 or not ties[pal_of].all())  # both result paths run
    g = dither_tiles(rgb, pal_of, pals)
    o = oracle.dither_tiles_tk(rgb, pal_of, pals)
    for a, b, what in zip(g, o, ("palpix", "hm", "vm")):
        assert np.array_equal(a, b), (what, int(np.count_nonzero(a != b)))
    assert int(g[0].max()) < size
    if size == 64 and n > 100:
        assert int(g[0].max()) > 31
        assert int(g[0][ties[pal_of]].max()) > 31 and int(g[0][~ties[pal_of]].max()) > 31


@pytest.mark.parametrize("mixed", [1, 4, 16])
@pytest.mark.parametrize("size", [32, 64])
def test_dither_yliluoma_bit_exact(gpu, oracle, size, mixed):
    rng = np.random.default_rng(size * 100 + mixed)
    n, P = 97, 4
    rgb = synth.frame_tiles(rng, n)
    pal_of = rng.integers(0, P, n).astype(np.int32)
    pals, _ = _dither_palettes(rng, P, size)
    g = dither_tiles(rgb, pal_of, pals, yliluoma_mix=mixed)
    o = oracle.dither_tiles_yl(rgb, pal_of, pals, mixed)
    for a, b, what in zip(g, o, ("palpix", "hm", "vm")):
        assert np.array_equal(a, b), (what, int(np.count_nonzero(a != b)))
    assert int(g[0].max()) > 16


@pytest.mark.parametrize("mixed", [0, 1, 4, 16], ids=["thomas_knoll", "yliluoma1", "yliluoma4", "yliluoma16"])
@pytest.mark.parametrize("size", [32, 64])
def test_dither_extremes(gpu, oracle, size, mixed):
    """The _big kernels on tests/dither_extremes.py: saturated tiles against the opposite corner, palettes of one
    colour or one luma, sorted palettes with ties, flat and mirror-symmetric tiles whose quadrant sums tie."""
    rgb, pal_of, pals, tname, kind = dx.cases(size)
    o = oracle.dither_tiles_yl(rgb, pal_of, pals, mixed) if mixed else oracle.dither_tiles_tk(rgb, pal_of, pals)
    dx.check_preconditions(size, o, tname, kind)
    g = dither_tiles(rgb, pal_of, pals, yliluoma_mix=mixed)
    for a, b, what in zip(g, o, ("palpix", "hm", "vm")):
        bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(1))
        assert bad.size == 0, (what, [(tname[i], kind[i]) for i in bad[:6]])


@pytest.mark.parametrize("size", [17, 24, 48])
def test_dither_other_sizes_above_16_fail(gpu, size):
    rgb = np.zeros((2, 64), np.int32)
    pal_of = np.zeros(2, np.int32)
    for mixed in (0, 4):
        with pytest.raises(TilerError, match="1..16, 32 or 64|1, 2, 4, 8, 16, 32 or 64"):
            dither_tiles(rgb, pal_of, np.zeros((1, size), np.int32), yliluoma_mix=mixed)


# ---- PsyV from palettes -------------------------------------------------------------------------------------------
N_ITEMS, N_TILES, N_PALS = 70, 50, 5


@functools.lru_cache(maxsize=None)
def _psyv_inputs(size):
    rng = np.random.default_rng(400 + size)
    pp = rng.integers(0, size, (N_TILES, 64)).astype(np.uint8)
    pp[0] = size - 1  # the last entry of a palette: a wrong stride shows at both ends of the table
    pals = synth.palettes(rng, N_PALS, size).astype(np.int32)
    tile_of = rng.integers(0, N_TILES, N_ITEMS).astype(np.int32)
    pal_of = rng.integers(0, N_PALS, N_ITEMS).astype(np.int32)
    tile_of[:2], pal_of[:2] = 0, (0, N_PALS - 1)
    fper = (rng.integers(0, 4, N_ITEMS) * 16).astype(np.uint8)  # per-item HMirror / VMirror
    for a in (pp, pals, tile_of, pal_of, fper):
        a.setflags(write=False)
    return pp, pals, tile_of, pal_of, fper


@contextlib.contextmanager
def _lane_items(gpu, min_items):
    lib = gpu.load()
    assert lib.tiler_debug_psyv_lane_items(min_items) == 0
    try:
        yield
    finally:
        lib.tiler_debug_psyv_lane_items(0)


# Haar / DCT, Q-weighting, global mirrors, gamma -1 / 0; each with and without per-item mirrors
PSYV_CASES = [(1 | 2, -1), (1 | 2 | 8, 0), (1, -1), (1 | 8, -1), (1 | 8, 0), (1 | 8 | 16, -1), (1 | 2 | 32, 0),
              (1 | 8 | 48, 0)]


@pytest.mark.parametrize("per_item", [False, True], ids=["global_flags", "per_item_mirrors"])
@pytest.mark.parametrize("size", [32, 64])
def test_psyv_from_palette_bit_exact(gpu, oracle, size, per_item):
    pp, pals, tile_of, pal_of, fper = _psyv_inputs(size)
    fp = fper if per_item else None
    for flags, gamma in PSYV_CASES:
        o64 = palsize_ref.psyv_batch(oracle, N_ITEMS, pp[tile_of], pals, pal_of, fp, flags, gamma)
        assert not np.array_equal(o64[0], o64[1])
        for lane in (0, 1):  # wave per item, then one lane per item (the DCT items kernel, where it applies)
            with _lane_items(gpu, lane):
                g64, g32 = gpu.psyv_batch(palpix=pp, tile_of=tile_of, palettes=pals, pal_of=pal_of, flags_per=fp,
                                          flags=flags, gamma=gamma, n=N_ITEMS, want64=True, want32=True)
            where = (size, flags, gamma, per_item, lane)
            assert np.array_equal(g64.view(np.uint64), o64.view(np.uint64)), where
            assert np.array_equal(g32.view(np.uint32), o64.astype(np.float32).view(np.uint32)), where


@pytest.mark.parametrize("size", [32, 64])
def test_psyv_host_form_rejects_a_byte_past_the_palette(gpu, size):
    pp, pals, tile_of, pal_of, _ = _psyv_inputs(size)
    bad = pp.copy()
    bad[7, 13] = size
    bad[9, 0] = 255
    with pytest.raises(TilerError, match="tile 7 "):
        gpu.psyv_batch(palpix=bad, tile_of=tile_of, palettes=pals, pal_of=pal_of, flags=1, n=N_ITEMS)


def test_psyv_dev_form_reads_colour_0_for_a_byte_past_the_palette(gpu):
    """The _dev form cannot report a bad byte: it reads colour 0 of the item's palette, never past the table (the
    last palette's rows end the allocation)."""
    import torch
    from tiler_amd.psyv import psyv_batch_dev
    size = 64
    pp, pals, _, _, _ = _psyv_inputs(size)
    bad = pp[:4].copy()
    bad[:, ::3] = 200
    zero = bad.copy()
    zero[:, ::3] = 0
    dev = torch.device("cuda", 0)
    out = []
    for tiles in (bad, zero):
        d_pp = torch.from_numpy(tiles).to(dev)
        d_pal = torch.from_numpy(pals.copy()).to(dev)
        d_po = torch.full((4,), N_PALS - 1, dtype=torch.int32, device=dev)
        d_out = torch.zeros((4, 192), dtype=torch.float64, device=dev)
        for lane in (0, 1):
            with _lane_items(gpu, lane):
                psyv_batch_dev(4, palpix=d_pp.data_ptr(), palettes=d_pal.data_ptr(), pal_of=d_po.data_ptr(),
                               flags=1 | 8, out64=d_out.data_ptr(), palsize=size)
                torch.cuda.synchronize(dev)
            out.append(d_out.cpu().numpy().copy())
    assert all(np.array_equal(out[0], o) for o in out[1:])


# ---- candidates, FrameTiling, k = 8 -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ft_case():
    rng = np.random.default_rng(640)
    T, P, size = 40, 3, 64
    tiles, thm, tvm = synth.tileset(rng, T, size, sym_share=0.0)
    t = tiles.reshape(T, 8, 8).copy()
    t[:4, :, 4:] = t[:4, :, 3::-1]                         # 10 symmetric tiles: 4 H, 3 V, 3 both
    t[4:7, 4:, :] = t[4:7, 3::-1, :]
    t[7:10, :, 4:] = t[7:10, :, 3::-1]
    t[7:10, 4:, :] = t[7:10, 3::-1, :]
    tiles, thm, tvm = synth.prepare_tile_mirrors(t.reshape(T, 64))
    pals = synth.palettes(rng, P, size).astype(np.int32)
    items_t = rng.integers(0, T, 400).astype(np.int32)
    items_p = rng.integers(0, P, 400).astype(np.int32)
    frames = synth.frame_tiles(rng, 300)
    return T, P, size, tiles, thm, tvm, pals, items_t, items_p, frames


@pytest.mark.parametrize("quality", [0, 2], ids=["fast", "slow"])
def test_prepare_and_frame_tiling_at_64(gpu, oracle, quality):
    """tiler_prepare_frame_tiling_ps_dev at palette size 64: the candidate maps equal or_mark_used +
    or_build_ft_dataset, the descriptors of those candidates equal the restatement's rows bit for bit, and
    FrameTiling of 300 frame tiles over the handle equals or_frame_tiling (ANN's kd order)."""
    import torch
    from tiler_amd import frame_tiling as ft
    T, P, size, tiles, thm, tvm, pals, items_t, items_p, frames = _ft_case()
    assert int(tiles.max()) == size - 1
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in
         (("t", items_t), ("p", items_p), ("tiles", tiles), ("thm", thm), ("tvm", tvm), ("pals", pals))}
    gds = ft.prepare_global_ft(tiles)
    try:
        ogds, ogt, oga = oracle.prepare_global_ds(tiles)
        kt, info = ft.prepare_frame_tiling_dev(gds, d["t"].data_ptr(), d["p"].data_ptr(), items_t.size,
                                               d["tiles"].data_ptr(), d["thm"].data_ptr(), d["tvm"].data_ptr(), T,
                                               d["pals"].data_ptr(), P, quality, None, palsize=size)
        torch.cuda.synchronize(dev)
        try:
            uo = oracle.mark_used(ogds, ogt, oga, items_p, items_t, tiles, P, quality)
            ods, ot, op, oa = palsize_ref.build_ft_dataset(oracle, uo, tiles, thm, tvm, pals)
            assert info["candidates"] == int(uo.sum()) == ods.shape[0] > 0
            gt_, gp_, ga_ = kt.maps()
            assert np.array_equal(gt_, ot) and np.array_equal(gp_, op) and np.array_equal(ga_, oa)
            fl = ((((ga_ & 1) ^ thm[gt_]) * 16) | (((ga_ >> 1) ^ tvm[gt_]) * 32)).astype(np.uint8)
            _, rows = gpu.psyv_batch(palpix=tiles, tile_of=gt_, palettes=pals, pal_of=gp_, flags_per=fl, flags=1 | 2,
                                     want64=False, want32=True)
            assert np.array_equal(rows.view(np.uint32), ods.view(np.uint32))
            g = ft.KeyframeTiler.__new__(ft.KeyframeTiler)
            g.kdt, g.use_wavelets, g.gamma = kt, True, -1
            got = g.do_frame_tiling(frames)
            o = oracle.frame_tiling(frames, ods, ot, op, oa)
            assert np.array_equal(got[4].view(np.uint32), o[4].view(np.uint32))
            for a, b in zip(got[:4], o[:4]):
                assert np.array_equal(a, b), int(np.count_nonzero(a != b))
        finally:
            kt.close()
    finally:
        gds.kdt.close()


def test_k8_preselection_rows_to_63_stay_off_tier_3(gpu, oracle):
    """PrepareGlobalFT-style 64-d rows with values to 63 (squared distances to 254,016): the k = 8 search equals the
    kd-tree restatement, duplicates included, on the exact-integer path, with no query in the exhaustive tier."""
    from tiler_amd.ann import KDTree
    rng = np.random.default_rng(63)
    rows = rng.integers(0, 64, (2000, 64)).astype(np.float32)
    rows[1000:1200] = rows[:200]           # duplicate rows
    rows[0], rows[1] = 0.0, 63.0            # the extreme rows
    q = np.concatenate([rows[rng.integers(0, 2000, 100)], rng.integers(0, 64, (100, 64)).astype(np.float32)])
    q[0] = rows[0]
    okd = oracle.KDTree(rows)
    oi, oe = okd.search_batch(q, k=8)
    okd.close()
    with KDTree(rows) as kd:
        gi, ge = kd.search_batch(q, k=8)
        st = kd.stats()
    assert np.array_equal(ge.view(np.uint32), oe.view(np.uint32))
    assert np.array_equal(gi, oi)
    assert st["exact_integer"] == 1 and st["exhaustive_queries"] == 0, st


# ---- Smooth -------------------------------------------------------------------------------------------------------
def test_smooth_at_64(gpu, oracle):
    from tiler_amd.smooth import smooth_keyframe
    rng = np.random.default_rng(64)
    F, Q, T, P, size = 6, 50, 24, 3, 64
    palpix = rng.integers(0, size, (T, 64)).astype(np.uint8)
    palpix[T // 2:] = palpix[:T // 2]      # one-pixel twins, the differing index above 16
    palpix[T // 2:, 5] = 40 + (palpix[T // 2:, 5] + 1) % 24
    palpix[:T // 2, 5] = 40 + palpix[:T // 2, 5] % 24
    pals = synth.palettes(rng, P, size).astype(np.int32)
    pals[1] = pals[0] + 1
    tile = np.zeros((F, Q), np.int32)
    tile[0] = rng.integers(0, T, Q)
    pal = np.zeros((F, Q), np.int32)
    pal[0] = rng.integers(0, P, Q)
    for f in range(1, F):
        r = rng.random(Q)
        tile[f] = np.where(r < 0.3, tile[f - 1], np.where(r < 0.7, (tile[f - 1] + T // 2) % T, rng.integers(0, T, Q)))
        pal[f] = np.where(r < 0.7, pal[f - 1], rng.integers(0, P, Q))
    hm = np.repeat(rng.integers(0, 2, (1, Q)), F, 0).astype(np.uint8)
    vm = np.repeat(rng.integers(0, 2, (1, Q)), F, 0).astype(np.uint8)
    sm = rng.integers(0, 2, (F, Q)).astype(np.uint8)
    tmp = rng.integers(-1, 100, (F, Q)).astype(np.int32)
    merged = kept = 0
    for strength in (0.08, 0.2):  # one-pixel twins land on both sides of either
        g = smooth_keyframe(tile, pal, hm, vm, sm, palpix, pals, strength, tmpidx=tmp)
        o = palsize_ref.smooth(oracle, tile, pal, hm, vm, sm, palpix, pals, strength, tmpidx=tmp)
        for a, b, what in zip(g, o, ("tile", "pal", "hm", "vm", "smoothed", "tmpidx")):
            assert np.array_equal(a, b), (strength, what)
        changed = g[0] != tile
        merged += int(changed.sum())
        kept += int((~changed[1:] & (tile[1:] != tile[:-1])).sum())
    assert merged > 0 and kept > 0
    bad = palpix.copy()
    bad[3, 9] = size
    with pytest.raises(TilerError, match="tile 3 "):
        smooth_keyframe(tile, pal, hm, vm, sm, bad, pals, 0.02)


# ---- the chain ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [32, 64])
def test_chain_to_gtm(gpu, size, tmp_path):
    """6 frames of 8 x 6 tiles with a scene cut: load_and_dither(palsize) -> Encoder.run_all -> .gtm, written by the
    Python and the native writer alike, played back equal to render(); the tileset saved and reloaded."""
    from tiler_amd import gtm
    from tiler_amd.encoder import Encoder, load_and_dither
    from tiler_amd.frame_tiling import FT_MEDIUM
    rng = np.random.default_rng(size)
    tm_w, tm_h = 8, 6
    frames, starts = synth.shot_frames(rng, 6, tm_w, tm_h, shot_len=(3, 3))
    assert len(starts) == 2
    v = load_and_dither(frames, tm_w, tm_h, n_palettes=4, palsize=size)
    assert v.palettes.shape[1:] == (4, size) and int(v.palpix.max()) < size
    assert int(v.palpix.max()) >= 16  # the upper entries are in use
    with pytest.raises(ValueError):
        Encoder(v, palsize=16)
    e = Encoder(v)
    assert e.palsize == size
    e.run_all(120, FT_MEDIUM, 0.2)
    W, H = tm_w * 8, tm_h * 8
    data = e.save_stream(W, H, 24.0, gpu=False)
    assert data == e.save_stream(W, H, 24.0, gpu=True)
    res = e.verify_stream(data, width=W, height=H)
    assert res["frames"] == 6 and res["differing_frames"] == 0, res
    path = tmp_path / "clip.gtm"
    path.write_bytes(data)
    with gtm.load_stream(str(path)) as st:
        assert st.palsize == size and st.frames == 6
    q = e.quality(width=W, height=H)
    assert np.isfinite(q["corr"]).all() and np.isfinite(q["psnr"]).all()
    gts = e.save_tileset()
    assert gts[0] == size
    b = Encoder(v)
    b.do_make_unique()
    idx, dis = b.do_reload_tiling(gts)
    assert idx.shape[0] == v.palpix.shape[0] and int(b.palpix.max()) < size


# ---- control: the 16-entry entry points are the _ps forms at 16 ---------------------------------------------------
def test_entry_points_at_16_equal_the_ps_forms(gpu):
    lib = gpu.load()
    rng = np.random.default_rng(16)
    n, T, P = 40, 20, 3
    pp = rng.integers(0, 16, (T, 64)).astype(np.uint8)
    pals = synth.palettes(rng, P).astype(np.int32)
    tile_of = rng.integers(0, T, n).astype(np.int32)
    pal_of = rng.integers(0, P, n).astype(np.int32)
    fper = (rng.integers(0, 4, n) * 16).astype(np.uint8)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    a64, b64 = np.zeros((n, 192)), np.zeros((n, 192))
    a32, b32 = np.zeros((n, 192), np.float32), np.zeros((n, 192), np.float32)
    for flags in (1 | 2, 1 | 8):
        assert lib.tiler_psyv_batch(n, None, T, hp(pp), hp(tile_of), P, hp(pals), hp(pal_of), hp(fper), flags, -1,
                                    hp(a64), hp(a32)) == 0, gpu.last_error()
        assert lib.tiler_psyv_batch_ps(n, None, T, hp(pp), hp(tile_of), P, 16, hp(pals), hp(pal_of), hp(fper), flags,
                                       -1, hp(b64), hp(b32)) == 0, gpu.last_error()
        assert a64.tobytes() == b64.tobytes() and a32.tobytes() == b32.tobytes() and np.abs(a64).sum() > 0
    F, Q = 4, 30
    tile = rng.integers(0, T, (F, Q)).astype(np.int32)
    tile[1::2] = tile[0::2]
    pal = np.repeat(rng.integers(0, P, (1, Q)), F, 0).astype(np.int32)
    z = np.zeros((F, Q), np.uint8)
    outs = []
    for ps in (False, True):
        it = [tile.copy(), np.zeros((F, Q), np.int32), pal.copy(), z.copy(), z.copy(), z.copy()]
        if ps:
            rc = lib.tiler_smooth_keyframe_ps(F, Q, *map(hp, it), T, hp(pp), P, 16, hp(pals), 0.05)
        else:
            rc = lib.tiler_smooth_keyframe(F, Q, *map(hp, it), T, hp(pp), P, hp(pals), 0.05)
        assert rc == 0, gpu.last_error()
        outs.append(b"".join(a.tobytes() for a in it))
    assert outs[0] == outs[1]
