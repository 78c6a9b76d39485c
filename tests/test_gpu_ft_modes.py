"""FrameTiling at the reference's other form settings: chkUseWL off (the DCT PsyV descriptor) and chkFTGamma on
(AFTGamma 0, main.pas:962-963; 1 is the form's other exponent), and with other exponents behind them
(tiler_set_gamma, main.pas:1443-1444).  The rest of the suite runs FrameTiling at (wavelets, gamma -1) only.

What differs on the device away from that setting:
  * wavelets, gamma 0 / 1: the LUT + true-division instantiation of the fused query kernel (orbit.hip,
    orbit_ft_query2_kernel<false, 1>) on mirror-orbit handles, of psyv_rgb_haar_kernel<false> on the others;
  * DCT: query descriptors from psyv_kernel, no fused kd root box, no orbit search, no flat grouping, no dedupe:
    the generic 16x16x32 shortlist with its error bound on DCT rows;
  * tiler_prepare_frame_tiling_dev's candidate descriptors at either switch.
Every comparison is of bytes: tilemap items with array_equal, distances and rows as uint32 / uint64 words, against the
CPU restatement (oracle/) called with the same two arguments.
"""
import numpy as np
import pytest
from test_gpu_frame_tiling import _rgb_tiles
from test_gpu_ft_dedup import _distinct, _per_frame, _run, _same, generic_inputs

from tiler_amd import synth

pytestmark = pytest.mark.gpu

MODES = [(True, 0), (True, 1), (False, -1), (False, 0), (False, 1)]


def _mode_id(m):
    return f"{'wl' if m[0] else 'dct'}_g{m[1]}"


def _eq_oracle(g, o, what, pick=None):
    """The five outputs (of the picked tiles) equal the oracle's: items as values, distances as words."""
    for name, a, b in zip(("tile", "pal", "hmirror", "vmirror"), g[:4], o[:4]):
        a = np.asarray(a) if pick is None else np.asarray(a)[pick]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        assert np.array_equal(a, b), f"{what}: {name} differs in {np.count_nonzero(a != b)} of {a.size} tiles"
    e = np.asarray(g[4]) if pick is None else np.asarray(g[4])[pick]
    assert e.dtype == o[4].dtype == np.float32
    assert np.array_equal(e.view(np.uint32), o[4].view(np.uint32)), f"{what}: err words differ"


def _items(o):
    return np.stack([np.asarray(a).astype(np.int64) for a in o[:4]], 1)


def _flat(rows):
    return (rows == rows[:, :1]).all(axis=1)


@pytest.fixture(scope="module")
def c1(oracle):
    """The C1 shape (320x240, 1k tileset, 16 palettes) and the oracle's items of frame 0 at (wavelets, -1)."""
    wl = synth.make_workload(21, 320, 240, 3, 1000, n_palettes=16)
    used = synth.used_one_palette(wl.tile_pal, 16)
    ods, ot, op, oa = oracle.build_ft_dataset(used, wl.tiles, wl.thm, wl.tvm, wl.palettes)
    base = _items(oracle.frame_tiling(wl.frame_rgb[0], ods, ot, op, oa))
    return {"wl": wl, "used": used, "base": base}


@pytest.fixture(scope="module")
def wl23():
    """The 40,000-tile workload of test_gpu_ft_dedup's orbit_case: 8 frames of 1,200 tiles, 9,600 rows."""
    wl = synth.make_workload(23, 320, 240, 8, 40000, n_palettes=16)
    frames = np.stack([wl.frame_rgb[f] for f in range(wl.frames)])
    return {"wl": wl, "frames": frames, "rows": np.ascontiguousarray(frames.reshape(-1, 64))}


# ---- 1. per-frame parity on the C1 shape, every mode ----------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=_mode_id)
def test_c1_frames_every_mode(gpu, oracle, c1, mode):
    from tiler_amd.frame_tiling import KeyframeTiler
    uw, gamma = mode
    wl = c1["wl"]
    ods, ot, op, oa = oracle.build_ft_dataset(c1["used"], wl.tiles, wl.thm, wl.tvm, wl.palettes, uw, gamma)
    kt = KeyframeTiler(wl.tiles, wl.thm, wl.tvm, wl.palettes, wl.ds, uw, gamma)
    try:
        assert np.array_equal(kt.rows.view(np.uint32), ods.view(np.uint32))
        assert np.array_equal(ot, wl.ds.tile_of) and np.array_equal(op, wl.ds.pal_of)
        assert np.array_equal(oa, wl.ds.attrs)
        for f in range(wl.frames):
            g = kt.do_frame_tiling(wl.frame_rgb[f])
            st = kt.kdt.stats()
            o = oracle.frame_tiling(wl.frame_rgb[f], ods, ot, op, oa, uw, gamma)
            _eq_oracle(g, o, (mode, f))
            if f == 0:  # the mode is not a restatement of (wavelets, -1): the oracle itself answers differently
                changed = int((_items(o) != c1["base"]).any(axis=1).sum())
                assert o[0].size == 1200 and changed > 600, changed
            assert st["queries"] == 1200
            if uw:  # the fused query kernel (its LUT instantiation: gamma != -1) fed the orbit search
                assert st["orbit_groups"] > 0 and st["orbit_search"] == 1
            else:   # orbit detection is a property of Haar rows, and the orbit search is gated on use_wavelets
                assert st["orbit_search"] == 0
    finally:
        kt.finish_frame_tiling()


# ---- 2. small batches, both scan states -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [(True, 0), (False, -1)], ids=_mode_id)
def test_small_batches_both_scan_states(gpu, oracle, mode):
    """Batches of <= 64 tiles take the small-batch exact scan by default and the MFMA tiers with the scan disabled
    (tiler_set_scan_limits(0, 0)); both give the restatement's outputs at the mode."""
    from tiler_amd.frame_tiling import KeyframeTiler
    uw, gamma = mode
    wl = synth.make_workload(29, 320, 240, 1, 3000, n_palettes=16)
    used = synth.used_one_palette(wl.tile_pal, 16)
    ods, ot, op, oa = oracle.build_ft_dataset(used, wl.tiles, wl.thm, wl.tvm, wl.palettes, uw, gamma)
    kt = KeyframeTiler(wl.tiles, wl.thm, wl.tvm, wl.palettes, wl.ds, uw, gamma)
    lib = gpu.load()
    try:
        if uw:
            assert kt.kdt.stats()["orbit_groups"] > 0
        for limits in ((64, 16), (0, 0)):
            assert lib.tiler_set_scan_limits(*limits) == 0
            for q0, nq in ((0, 1), (5, 17), (100, 64)):
                rgb = wl.frame_rgb[0][q0:q0 + nq]
                g = kt.do_frame_tiling(rgb)
                _eq_oracle(g, oracle.frame_tiling(rgb, ods, ot, op, oa, uw, gamma), (mode, limits, q0, nq))
    finally:
        lib.tiler_set_scan_limits(64, 16)
        kt.finish_frame_tiling()


# ---- 3. batches of >= 8,192 tiles -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def orbit_g0(gpu, wl23):
    """(a) the mirror-orbit handle over 40,000 tiles x 4 orientations at (wavelets, gamma 0)."""
    from tiler_amd.frame_tiling import KeyframeTiler
    wl = wl23["wl"]
    kt = KeyframeTiler(wl.tiles, wl.thm, wl.tvm, wl.palettes, wl.ds, True, 0)
    yield kt
    kt.finish_frame_tiling()


@pytest.fixture(scope="module")
def generic_g1(gpu):
    """(b) test_gpu_ft_dedup's generic candidate set (no mirror orbits) at (wavelets, gamma 1)."""
    from tiler_amd.frame_tiling import KeyframeTiler
    oracle_args, ds, frames = generic_inputs()
    _, tiles, thm, tvm, pals = oracle_args
    kt = KeyframeTiler(tiles, thm, tvm, pals, ds, True, 1)
    yield {"kt": kt, "frames": frames, "rows": np.ascontiguousarray(frames.reshape(-1, 64)),
           "oracle_args": oracle_args}
    kt.finish_frame_tiling()


def test_orbit_batch_gamma0(gpu, oracle, wl23, orbit_g0):
    """The fused query kernel's LUT instantiation behind grouping, dedupe and the permutation: the 9,600-tile batch,
    switch on and off, equals the eight per-frame calls; a sample equals the oracle's search over the handle's rows
    (test_c1_frames_every_mode pins such rows to the oracle's dataset bit for bit)."""
    kt, rows, wl = orbit_g0, wl23["rows"], wl23["wl"]
    Q, distinct = rows.shape[0], _distinct(rows)
    assert Q == 9600 and distinct <= Q - Q // 8
    assert kt.kdt.stats()["orbit_groups"] >= 1024 * 32
    per_frame = _per_frame(kt, wl23["frames"])
    on, st = _run(gpu, kt, rows, 1)
    assert st["orbit_search"] == 1 and st["queries"] == Q
    assert st["searched_queries"] == distinct and st["dup_queries"] == Q - distinct
    assert st["flat_queries"] > 0
    _same(on, per_frame, "orbit gamma 0: batch vs per-frame calls")
    off, st_off = _run(gpu, kt, rows, 0)
    assert st_off["orbit_search"] == 1 and st_off["searched_queries"] == Q and st_off["dup_queries"] == 0
    assert st_off["flat_queries"] == st["flat_queries"]
    _same(off, per_frame, "orbit gamma 0: switch off vs per-frame calls")
    flat = _flat(rows)
    pick = np.concatenate([np.nonzero(flat)[0][:200], np.nonzero(~flat)[0][:200]])
    assert pick.size == 400
    o = oracle.frame_tiling(rows[pick], kt.rows, wl.ds.tile_of, wl.ds.pal_of, wl.ds.attrs, True, 0)
    _eq_oracle(on, o, "orbit gamma 0 vs oracle", pick)


def test_generic_batch_gamma1(gpu, oracle, generic_g1):
    """psyv.hip's Haar query kernel with the true division and a query permutation, on the generic shortlist."""
    c = generic_g1
    kt, rows = c["kt"], c["rows"]
    Q, distinct = rows.shape[0], _distinct(rows)
    assert Q == 9600 and distinct <= Q - Q // 8
    per_frame = _per_frame(kt, c["frames"])
    on, st = _run(gpu, kt, rows, 1)
    assert st["orbit_search"] == 0 and st["flat_queries"] > 0
    assert st["queries"] == Q and st["searched_queries"] == distinct and st["dup_queries"] == Q - distinct
    _same(on, per_frame, "generic gamma 1: batch vs per-frame calls")
    off, st_off = _run(gpu, kt, rows, 0)
    assert st_off["orbit_search"] == 0 and st_off["flat_queries"] == st["flat_queries"]
    assert st_off["searched_queries"] == Q and st_off["dup_queries"] == 0
    _same(off, per_frame, "generic gamma 1: switch off vs per-frame calls")
    flat = _flat(rows)
    pick = np.concatenate([np.nonzero(flat)[0][:300], np.nonzero(~flat)[0][:300]])
    assert pick.size == 600
    ods, ot, op, oa = oracle.build_ft_dataset(*c["oracle_args"], True, 1)
    assert np.array_equal(kt.rows.view(np.uint32), ods.view(np.uint32))
    _eq_oracle(on, oracle.frame_tiling(rows[pick], ods, ot, op, oa, True, 1), "generic gamma 1 vs oracle", pick)


@pytest.mark.parametrize("gamma", [-1, 0])
def test_dct_batch_at_scale(gpu, oracle, c1, wl23, gamma):
    """9,600 tiles in one DCT call on the C1 tileset: nothing Haar-only engages (no orbit search, no grouping, no
    dedupe) and the batch equals the per-frame calls; at gamma -1 a 400-tile sample equals the oracle."""
    from tiler_amd.frame_tiling import KeyframeTiler
    wl, rows = c1["wl"], wl23["rows"]
    Q = rows.shape[0]
    kt = KeyframeTiler(wl.tiles, wl.thm, wl.tvm, wl.palettes, wl.ds, False, gamma)
    try:
        per_frame = _per_frame(kt, wl23["frames"])
        big, st = _run(gpu, kt, rows, 1)
        assert st["orbit_search"] == 0
        assert st["queries"] == Q and st["searched_queries"] == Q
        assert st["dup_queries"] == 0 and st["flat_queries"] == 0
        _same(big, per_frame, f"DCT gamma {gamma}: batch vs per-frame calls")
    finally:
        kt.finish_frame_tiling()
    if gamma == -1:
        flat = _flat(rows)
        pick = np.concatenate([np.nonzero(flat)[0][:200], np.nonzero(~flat)[0][:200]])
        assert pick.size == 400
        ods, ot, op, oa = oracle.build_ft_dataset(c1["used"], wl.tiles, wl.thm, wl.tvm, wl.palettes, False, -1)
        _eq_oracle(big, oracle.frame_tiling(rows[pick], ods, ot, op, oa, False, -1), "DCT batch vs oracle", pick)


# ---- 4. device-side prepare at non-default settings -----------------------------------------------------------------
@pytest.mark.parametrize("mode", [(False, -1), (True, 0)], ids=_mode_id)
def test_prepare_frame_tiling_dev_modes(gpu, oracle, mode):
    """tiler_prepare_frame_tiling_dev (Medium) with the switches: the candidates' descriptors are the mode's, so the
    FrameTiling outputs over the adopted handle equal the oracle's over its own dataset at the mode.  Setup as
    test_prepare_frame_tiling_dev_matches_restatement."""
    import torch
    from tiler_amd import frame_tiling as ft
    uw, gamma = mode
    rng = np.random.default_rng(18)
    P, T = 8, 700
    pals = synth.palettes(rng, P)
    pals[1::2] = pals[0::2] ^ rng.integers(0, 2, pals[1::2].shape)  # near-identical pairs: Medium marks both
    tiles, thm, tvm = synth.tileset(rng, T)
    cent = synth.palette_centroids(pals)
    items_t = rng.integers(0, T, 6000).astype(np.int32)
    items_p = rng.integers(0, P, 6000).astype(np.int32)
    items_t[::97] = -1
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in
         (("t", items_t), ("p", items_p), ("tiles", tiles), ("thm", thm), ("tvm", tvm), ("pals", pals))}
    frames = synth.frame_tiles(rng, 1500)
    gds = ft.prepare_global_ft(tiles)
    ogds, ogt, oga = oracle.prepare_global_ds(tiles)
    corr_o, hi_o = oracle.palette_corr(cent)
    near = ft.near_palettes(cent)
    assert near.sum() > P
    keep = items_t >= 0
    q = ft.FT_MEDIUM
    try:
        kt, info = ft.prepare_frame_tiling_dev(gds, d["t"].data_ptr(), d["p"].data_ptr(), items_t.size,
                                               d["tiles"].data_ptr(), d["thm"].data_ptr(), d["tvm"].data_ptr(), T,
                                               d["pals"].data_ptr(), P, q, near, uw, gamma)
        try:
            torch.cuda.synchronize(dev)
            uo = oracle.mark_used(ogds, ogt, oga, items_p[keep], items_t[keep], tiles, P, q, corr_o, hi_o)
            assert info["candidates"] == int(uo.sum())
            ods, ot, op, oa = oracle.build_ft_dataset(uo, tiles, thm, tvm, pals, uw, gamma)
            g = ft.KeyframeTiler.__new__(ft.KeyframeTiler)
            g.kdt, g.use_wavelets, g.gamma = kt, uw, gamma
            got = g.do_frame_tiling(frames)
        finally:
            kt.close()
        _eq_oracle(got, oracle.frame_tiling(frames, ods, ot, op, oa, uw, gamma), mode)
    finally:
        gds.kdt.close()


# ---- 5. tiler_set_gamma ---------------------------------------------------------------------------------------------
def test_set_gamma(gpu, oracle, c1):
    """tiler_set_gamma rebuilds the gamma 0 / 1 rows of the gamma LUT and of the LAB linearisation table on the bound
    devices; gamma -1 does not move; the defaults come back bit for bit."""
    from tiler_amd.frame_tiling import KeyframeTiler
    lib = gpu.load()
    n = 600
    rgb = _rgb_tiles(np.random.default_rng(105), n)
    words = lambda a: a.view(np.uint64)  # noqa: E731
    try:
        before = {g: gpu.psyv_batch(rgb=rgb, flags=2, gamma=g)[0] for g in (0, -1)}
        assert lib.tiler_set_gamma(1.8, 0.7) == 0
        oracle.set_gamma(1.8, 0.7)
        for gamma in (0, 1):
            for flags in (2, 0):
                g64, _ = gpu.psyv_batch(rgb=rgb, flags=flags, gamma=gamma)
                o64 = oracle.psyv_batch(n, rgb=rgb, flags=flags, gamma=gamma)
                assert np.array_equal(words(g64), words(o64)), (gamma, flags)
        # the new exponents are in use on both sides, not the defaults on both
        assert not np.array_equal(words(gpu.psyv_batch(rgb=rgb, flags=2, gamma=0)[0]), words(before[0]))
        assert np.array_equal(words(gpu.psyv_batch(rgb=rgb, flags=2, gamma=-1)[0]), words(before[-1]))
        lab, _ = gpu.psyv_batch(rgb=rgb, flags=4 | 2, gamma=0)
        assert np.array_equal(words(lab), words(oracle.psyv_lab_batch(rgb, 0, True)))
        wl = c1["wl"]
        ods, ot, op, oa = oracle.build_ft_dataset(c1["used"], wl.tiles, wl.thm, wl.tvm, wl.palettes, True, 0)
        kt = KeyframeTiler(wl.tiles, wl.thm, wl.tvm, wl.palettes, wl.ds, True, 0)
        try:
            assert np.array_equal(kt.rows.view(np.uint32), ods.view(np.uint32))
            g = kt.do_frame_tiling(wl.frame_rgb[0])
            assert kt.kdt.stats()["orbit_search"] == 1
            _eq_oracle(g, oracle.frame_tiling(wl.frame_rgb[0], ods, ot, op, oa, True, 0), "after tiler_set_gamma")
        finally:
            kt.finish_frame_tiling()
    finally:
        rc = lib.tiler_set_gamma(2.0, 0.6)
        oracle.set_gamma(2.0, 0.6)
    assert rc == 0
    assert np.array_equal(words(gpu.psyv_batch(rgb=rgb, flags=2, gamma=0)[0]), words(before[0]))
    assert np.array_equal(words(oracle.psyv_batch(n, rgb=rgb, flags=2, gamma=0)), words(before[0]))
