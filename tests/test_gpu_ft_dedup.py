"""A FrameTiling call of >= 8,192 tiles searches each distinct tile once (nn_frame_tiling_dev, ft_dedup_* kernels):
a hash table groups the call's tiles, all 64 words are compared before two tiles share a result, the representatives
are searched (non-flat first, flat last) and every tile takes its representative's outputs.

The outputs must not change by a bit: against per-frame calls (below the threshold, checked against the oracle by
test_gpu_frame_tiling.py), against the switch off (tiler_debug_ft_dedup(0)) and with the hash cut to 4 bits (mode 2),
where nearly every lookup meets a different tile.  The statistics must count what ran.
"""
import numpy as np
import pytest
from test_gpu_scale import WG_QUERIES, _flat_layout

from tiler_amd import synth

pytestmark = pytest.mark.gpu

NAMES = ("tile", "pal", "hmirror", "vmirror", "err")


def _run(gpu, kt, rows, mode):
    lib = gpu.load()
    assert lib.tiler_debug_ft_dedup(mode) == 0
    try:
        out = kt.do_frame_tiling(rows)
        return [np.asarray(a).copy() for a in out], kt.kdt.stats()
    finally:
        lib.tiler_debug_ft_dedup(1)


def _same(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name)
        diff = np.count_nonzero(x.view(np.uint8).reshape(x.shape[0], -1) != y.view(np.uint8).reshape(y.shape[0], -1))
        assert diff == 0, f"{what}: {name} differs in {diff} bytes"


def _per_frame(kt, frames):
    parts = [kt.do_frame_tiling(f) for f in frames]
    return [np.concatenate([np.asarray(p[j]) for p in parts]) for j in range(5)]


def _distinct(rows):
    return int(np.unique(rows, axis=0).shape[0])


@pytest.fixture(scope="module")
def orbit_case(gpu):
    """9,600 tiles (8 frames of 1,200), 3,684 distinct, on a mirror-orbit handle long enough for flat grouping; the
    switch-off outputs of the batch are computed once."""
    from tiler_amd.frame_tiling import KeyframeTiler
    wl = synth.make_workload(23, 320, 240, 8, 40000, n_palettes=16)
    kt = KeyframeTiler(wl.tiles, wl.thm, wl.tvm, wl.palettes, wl.ds)
    assert kt.kdt.stats()["orbit_groups"] >= 1024 * 32
    frames = np.stack([wl.frame_rgb[f] for f in range(wl.frames)])
    rows = np.ascontiguousarray(frames.reshape(-1, 64))
    off, st_off = _run(gpu, kt, rows, 0)
    yield {"kt": kt, "frames": frames, "rows": rows, "off": off, "st_off": st_off, "distinct": _distinct(rows)}
    kt.finish_frame_tiling()


def generic_inputs():
    """The two-cells-per-tile candidate set (never a whole mirror orbit) and 8 x 1,200 frame tiles:
    ((used, tiles, thm, tvm, pals), ds, frames)."""
    rng = np.random.default_rng(29)
    P, T = 16, 6000
    tiles, thm, tvm = synth.tileset(rng, T)
    pals = synth.palettes(rng, P)
    used = np.zeros((P, T, 4), np.uint8)
    for _ in range(2):
        used[rng.integers(0, P, T), np.arange(T), rng.integers(0, 4, T)] = 1
    ds = synth.ft_dataset_from_used(used, thm, tvm)
    frames = synth.keyframe_frames(rng, 8, 1200)
    return (used, tiles, thm, tvm, pals), ds, frames


@pytest.fixture(scope="module")
def generic_case(gpu):
    """The two-cells-per-tile candidate set (no mirror orbits: the generic 16x16x32 shortlist) with 8 x 1,200 tiles."""
    from tiler_amd.frame_tiling import KeyframeTiler
    (used, tiles, thm, tvm, pals), ds, frames = generic_inputs()
    kt = KeyframeTiler(tiles, thm, tvm, pals, ds)
    rows = np.ascontiguousarray(frames.reshape(-1, 64))
    off, st_off = _run(gpu, kt, rows, 0)
    yield {"kt": kt, "frames": frames, "rows": rows, "off": off, "st_off": st_off, "distinct": _distinct(rows),
           "oracle_args": (used, tiles, thm, tvm, pals)}
    kt.finish_frame_tiling()


def _check_engaged(st, Q, distinct):
    assert st["queries"] == Q
    assert st["searched_queries"] == distinct
    assert st["dup_queries"] == Q - distinct


def test_orbit_batch_equals_per_frame_calls(gpu, orbit_case):
    c = orbit_case
    Q = c["rows"].shape[0]
    assert Q == 9600 and c["distinct"] == 3684
    big, st = _run(gpu, c["kt"], c["rows"], 1)
    _check_engaged(st, Q, c["distinct"])
    assert st["orbit_search"] == 1
    # flat_queries stays in the call's own units: the layout the call has with the switch off
    assert st["flat_queries"] == c["st_off"]["flat_queries"] > 0
    assert 0 <= st["searched_flat_queries"] <= st["searched_queries"]
    assert c["st_off"]["dup_queries"] == 0 and c["st_off"]["searched_queries"] == Q
    _same(big, _per_frame(c["kt"], c["frames"]), "orbit batch vs per-frame calls")
    _same(big, c["off"], "orbit batch vs switch off")


def test_generic_batch_equals_per_frame_calls_and_oracle(gpu, oracle, generic_case):
    c = generic_case
    Q = c["rows"].shape[0]
    big, st = _run(gpu, c["kt"], c["rows"], 1)
    _check_engaged(st, Q, c["distinct"])
    assert st["orbit_search"] == 0
    assert st["flat_queries"] == c["st_off"]["flat_queries"] > 0
    _same(big, _per_frame(c["kt"], c["frames"]), "generic batch vs per-frame calls")
    _same(big, c["off"], "generic batch vs switch off")
    flat = (c["rows"] == c["rows"][:, :1]).all(axis=1)
    pick = np.concatenate([np.nonzero(flat)[0][:300], np.nonzero(~flat)[0][:300]])
    ods, ot, op, oa = oracle.build_ft_dataset(*c["oracle_args"])
    o = oracle.frame_tiling(c["rows"][pick], ods, ot, op, oa)
    for a, b in zip(big[:4], o[:4]):
        assert np.array_equal(a[pick], b)
    assert np.array_equal(big[4][pick].view(np.uint32), o[4].view(np.uint32))


@pytest.mark.parametrize("which", ["orbit", "generic"])
def test_forced_collisions(gpu, orbit_case, generic_case, which):
    """Mode 2: 16 hash values for the whole batch, so a lookup nearly always returns a different tile and the word
    comparison must refuse the merge."""
    c = orbit_case if which == "orbit" else generic_case
    Q = c["rows"].shape[0]
    g, st = _run(gpu, c["kt"], c["rows"], 2)
    _same(g, c["off"], f"{which}: 4-bit hash vs switch off")
    assert st["queries"] == Q
    assert c["distinct"] <= st["searched_queries"] <= Q
    assert st["dup_queries"] in (0, Q - st["searched_queries"])


def _degenerate(name, c):
    rows, frames = c["rows"], c["frames"]
    flat = (rows == rows[:, :1]).all(axis=1)
    if name == "one_nonflat":
        return np.ascontiguousarray(np.tile(rows[np.nonzero(~flat)[0][0]], (8192, 1))), 1
    if name == "one_flat":
        return np.ascontiguousarray(np.tile(rows[np.nonzero(flat)[0][0]], (8192, 1))), 1
    if name == "pair_first_last":
        r = synth.frame_tiles(np.random.default_rng(5), 9600)
        r[-1] = r[0]
        return r, None  # 9,599 distinct: above Q - Q/8, searched tile by tile
    if name == "flat_around_nonflat":
        r = rows.copy()
        f = np.full(64, 0x123456, np.int32)  # a flat tile at both ends and in the middle of the repeating batch
        assert not (r == f).all(axis=1).any()
        r[0] = r[4800] = r[-1] = f
        return r, _distinct(r)
    raise AssertionError(name)


@pytest.mark.parametrize("name", ["one_nonflat", "one_flat", "pair_first_last", "flat_around_nonflat"])
def test_degenerate_layouts(gpu, orbit_case, name):
    rows, distinct = _degenerate(name, orbit_case)
    kt = orbit_case["kt"]
    Q = rows.shape[0]
    off, _ = _run(gpu, kt, rows, 0)
    g, st = _run(gpu, kt, rows, 1)
    _same(g, off, name)
    assert st["queries"] == Q
    if distinct is None:
        assert st["searched_queries"] == Q and st["dup_queries"] == 0
    else:
        assert st["searched_queries"] == distinct and st["dup_queries"] == Q - distinct
    if name == "one_flat":
        assert (np.asarray(g[0]) == np.asarray(g[0])[0]).all()


@pytest.fixture(scope="module")
def orbit_per_frame(orbit_case):
    """The per-frame-call outputs of the module's 9,600 rows (8 calls of 1,200, all below the threshold), once."""
    return _per_frame(orbit_case["kt"], orbit_case["frames"])


@pytest.mark.parametrize("mode", [1, 0])
def test_scratch_growth_on_one_handle(gpu, orbit_case, orbit_per_frame, mode):
    """8,192 tiles, then 12,288 (both buffer groups and the hash table outgrown), then 8,192 again (inside the larger
    capacities) on one handle: every call equals the per-frame calls of its rows byte for byte.  A tile's outputs
    depend on its own words only, so the per-frame outputs of a row set are those rows of orbit_per_frame."""
    rows, kt = orbit_case["rows"], orbit_case["kt"]
    for pick in (np.arange(8192), np.concatenate([np.arange(9600), np.arange(2688)]), np.arange(8192)):
        r = np.ascontiguousarray(rows[pick])
        Q, distinct = r.shape[0], _distinct(r)
        assert distinct <= Q - Q // 8  # enough repeats for the dedupe to engage
        got, st = _run(gpu, kt, r, mode)
        _same(got, [a[pick] for a in orbit_per_frame], f"{Q} tiles, mode {mode}")
        assert st["queries"] == Q
        if mode == 1:
            assert st["searched_queries"] == distinct and st["dup_queries"] == Q - distinct
        else:
            assert st["searched_queries"] == Q and st["dup_queries"] == 0


def test_not_engaged_without_repeats(gpu, orbit_case):
    """9,600 distinct tiles: the call pays the three passes and then runs as with the switch off."""
    kt = orbit_case["kt"]
    rows = synth.frame_tiles(np.random.default_rng(5), 9600)
    assert _distinct(rows) == 9600
    off, st_off = _run(gpu, kt, rows, 0)
    g, st = _run(gpu, kt, rows, 1)
    _same(g, off, "no repeats")
    Q = rows.shape[0]
    assert st["queries"] == Q and st["searched_queries"] == Q and st["dup_queries"] == 0
    _, _, wf0 = _flat_layout(rows)
    assert st["flat_queries"] == max(0, Q - wf0 * WG_QUERIES)
    assert st["flat_queries"] == st["searched_flat_queries"] == st_off["flat_queries"]
