"""GlobalTiling's K-Modes branch through one library call (tiler_global_tiling, tiler_amd/csrc/global_tiling.hip)
against the host plan (plan_global_tiling + kmodes_bins + apply_kmodes_merges), the dataset-line kernel against
write_tile_dataset_line / pal_signi, and the encoder chain with the flag on.  Every comparison is exact equality."""
import ctypes
import functools

import numpy as np
import pytest

from tiler_amd import _lib, synth
from tiler_amd import global_tiling as gt

pytestmark = pytest.mark.gpu


# ---- dataset lines ----
def _zone_tile(palsize, count):
    """A tile with `count` pixels in every zone the palette reaches, in zone order, until the 64 pixels run out; what
    is left over goes to the last zone written."""
    first = {}
    for idx in range(palsize):
        first.setdefault(idx * 16 // palsize, idx)
    t = np.zeros(64, np.uint8)
    pos, last = 0, first[0]
    for z in sorted(first):
        if pos + count > 64 or count == 0:
            break
        t[pos:pos + count] = last = first[z]
        pos += count
    t[pos:] = last
    return t


def _line_tiles(nt, palsize, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, palsize, (nt, 64)).astype(np.uint8)
    thr = palsize // 16
    special = [np.full(64, i, np.uint8) for i in (0, palsize // 2, palsize - 1)]  # one index throughout, the last too
    special += [_zone_tile(palsize, thr), _zone_tile(palsize, thr + 1)]  # zones exactly at / one above the threshold
    for i, s in enumerate(special[:nt]):
        t[(i * 97) % nt if nt > 97 else i] = s
    return t


@pytest.mark.parametrize("palsize", [2, 4, 16, 32, 64])
@pytest.mark.parametrize("nt", [0, 1, 255, 256, 257, 4099])
def test_dataset_lines(gpu, nt, palsize):
    t = _line_tiles(nt, palsize, 100 + palsize)
    lines, signi = gt.tile_dataset_lines_gpu(t, palsize)
    assert lines.shape == (nt, 80) and lines.dtype == np.uint8 and signi.shape == (nt,) and signi.dtype == np.int32
    assert np.array_equal(lines, gt.write_tile_dataset_line(t, palsize))
    assert np.array_equal(signi, gt.pal_signi(t, palsize))
    only_lines, none = gt.tile_dataset_lines_gpu(t, palsize, signi=False)
    assert none is None and np.array_equal(only_lines, lines)
    none, only_signi = gt.tile_dataset_lines_gpu(t, palsize, lines=False)
    assert none is None and np.array_equal(only_signi, signi)


def test_dataset_lines_threshold_tiles_are_what_they_claim():
    """The constructed tiles sit at the threshold and one above it (no device needed to see that)."""
    for palsize in (16, 32, 64):
        thr = palsize // 16
        at = gt.write_tile_dataset_line(_zone_tile(palsize, thr), palsize)[0, 64:]
        above = gt.write_tile_dataset_line(_zone_tile(palsize, thr + 1), palsize)[0, 64:]
        assert at.sum() <= 1 and above.sum() >= 12, (palsize, at, above)
    t = _zone_tile(64, 4)
    assert gt.write_tile_dataset_line(t, 64)[0, 64:].sum() == 0 and gt.pal_signi(t, 64)[0] == 60  # every zone at 4


# ---- the whole step ----
# name: (nt, n_palettes, desired, palsize, bins in use (None: all), what the plan must look like)
CASES = {
    "one_tile": (1, 1, 1, 16, None, "none"),
    "all_run": (257, 3, 1, 16, None, "all"),
    "none_run": (257, 3, 10 ** 6, 64, None, "none"),
    "mixed_8": (3000, 8, 2000, 64, None, "mixed"),
    "mixed_16": (3000, 8, 300, 16, None, "mixed"),
    "sparse_128": (20000, 128, 1500, 16, (0, 5, 77, 126, 127), "mixed"),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and the host path's result, computed once and never written to."""
    nt, n_pal, desired, palsize, used, shape = CASES[name]
    seed = sorted(CASES).index(name) + 40
    rng = np.random.default_rng(seed)
    tiles, _ = synth.globaltiling_workload(seed, nt, protos=max(1, nt // 12), n_palettes=n_pal, palsize=palsize)
    used = np.arange(n_pal) if used is None else np.asarray(used)
    w = 1.0 / np.arange(1, used.size + 1) ** 1.1
    dith = used[rng.choice(used.size, size=nt, p=w / w.sum())].astype(np.int32)
    active = (rng.random(nt) > 0.15).astype(np.uint8) if nt > 1 else np.ones(1, np.uint8)
    if shape == "mixed":  # two bins of one active tile each: EqualQualityTileCount(1) = 1 never exceeds ClusterCount
        lone = used[-2:]
        active[np.isin(dith, lone)] = 0
        for j, p in enumerate(lone):
            dith[11 + 500 * j] = p
            active[11 + 500 * j] = 1
    use_count = rng.integers(1, 6, nt).astype(np.int64)
    use_count[rng.random(nt) < 0.05] = (1 << 31) - rng.integers(1, 9)
    off = np.nonzero(active == 0)[0]  # what an inactive tile holds is never read as an index
    if off.size >= 3:
        dith[off[0]], dith[off[1]] = -1, n_pal
        tiles[off[2]] = 255
    for a in (tiles, dith, active, use_count):
        a.setflags(write=False)
    plan = gt.plan_global_tiling(tiles, dith, n_pal, desired, palsize, active=active)
    sizes = np.array([b.size for b in plan.bins])
    if shape == "none":
        assert plan.run == []
    elif shape == "all":
        assert plan.run == list(range(n_pal)) and sizes.min() >= 2
    else:
        assert plan.run and any(sizes[p] > 0 and p not in plan.run for p in range(n_pal))
        assert (sizes == 0).any() or n_pal == 8
    ref = gt.do_global_tiling(tiles, dith, n_pal, desired, palsize, active=active, use_count=use_count)
    for a in ref:
        a.setflags(write=False)
    return (tiles, dith, n_pal, desired, palsize, active, use_count), plan, sizes, ref


def _run_and_compare(name):
    (tiles, dith, n_pal, desired, palsize, active, use_count), plan, sizes, ref = _case(name)
    out = gt.do_global_tiling_gpu(tiles, dith, n_pal, desired, palsize, active=active, use_count=use_count,
                                  return_plan=True)
    for what, a, b in zip(("palpix", "active", "use_count", "merge_index", "k_per_bin"), out, ref):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (name, what)
    info = out[5]
    assert np.array_equal(info["bin_size"], sizes), name
    assert np.array_equal(info["k"], plan.k_per_bin), name
    assert info["start"].tolist() == plan.starts, name
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_whole_step_equals_host_path(gpu, name):
    out = _run_and_compare(name)
    ref = _case(name)[3]
    if CASES[name][5] != "none":
        assert (ref[3] >= 0).any()  # the case merges something
        assert ref[2].max() > (1 << 31)  # ... and a summed UseCount passes 2^31
    else:
        assert (out[3] == -1).all()
    five = gt.do_global_tiling_gpu(*_case(name)[0][:5], active=_case(name)[0][5], use_count=_case(name)[0][6])
    assert len(five) == 5 and all(np.array_equal(a, b) for a, b in zip(five, ref))


def test_default_active_and_use_count(gpu):
    tiles, dith, n_pal, desired, palsize, _, _ = _case("mixed_16")[0]
    tiles = np.where(tiles == 255, 0, tiles)
    dith = np.clip(dith, 0, n_pal - 1)
    ref = gt.do_global_tiling(tiles, dith, n_pal, desired, palsize)
    out = gt.do_global_tiling_gpu(tiles, dith, n_pal, desired, palsize)
    assert all(np.array_equal(a, b) for a, b in zip(out, ref))


def test_scratch_reuse_smaller_then_larger(gpu):
    for name in ("mixed_16", "all_run", "sparse_128", "one_tile", "mixed_8"):
        _run_and_compare(name)


# ---- StartingPoint ties ----
def _tie_tiles():
    """Bin 0: 90 tiles whose minimal line sum (32 ones: 32 + 2 flags) stands at rows 0, 41 and 89, three different
    tiles; bin 1: 60 tiles with the minimum at row 0 only.  Every other tile has all bytes >= 2."""
    rng = np.random.default_rng(77)
    protos = rng.integers(2, 16, (9, 64)).astype(np.uint8)
    n0, n1 = 90, 60
    tiles = protos[rng.integers(0, 9, n0 + n1)]
    flip = rng.random(tiles.shape) < 0.1
    tiles[flip] = rng.integers(2, 16, int(flip.sum())).astype(np.uint8)
    a, b, c = np.zeros(64, np.uint8), np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    a[:32], b[::2], c[32:] = 1, 1, 1
    # interleave the bins so that a bin's rows are not a contiguous tile range
    dith = np.zeros(n0 + n1, np.int32)
    dith[np.arange(n1) * 2 + 1] = 1
    rows0, rows1 = np.nonzero(dith == 0)[0], np.nonzero(dith == 1)[0]
    tiles[rows0[0]], tiles[rows0[41]], tiles[rows0[89]] = a, b, c
    tiles[rows1[0]] = b
    return tiles, dith, rows0, rows1


def test_starting_point_ties_go_to_the_last_row(gpu):
    from tiler_amd.kmodes import compute_kmodes_batch
    tiles, dith, rows0, rows1 = _tie_tiles()
    desired = 20
    plan = gt.plan_global_tiling(tiles, dith, 2, desired)
    assert plan.run == [0, 1] and plan.starts == [89, 0]
    sums = plan.lines[rows0].astype(np.int64).sum(1)
    assert np.nonzero(sums == sums.min())[0].tolist() == [0, 41, 89]
    # the choice matters: K-Modes from the first minimal row gives another clustering than from the last
    X = np.ascontiguousarray(plan.lines[rows0])
    off, ks = np.array([0, rows0.size], np.int32), np.array([plan.k_per_bin[0]], np.int32)
    res = [compute_kmodes_batch(X, off, ks, np.array([s], np.int32), 16) for s in (0, 89)]
    assert not (np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]))
    out = gt.do_global_tiling_gpu(tiles, dith, 2, desired, return_plan=True)
    assert out[5]["start"].tolist() == [89, 0]
    ref = gt.do_global_tiling(tiles, dith, 2, desired)
    assert all(np.array_equal(a, b) for a, b in zip(out[:5], ref))


# ---- refusals ----
def _raw_call(pp, dp, act, uc, mi, n_pal, palsize, desired):
    v = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    return _lib.load().tiler_global_tiling(v(pp), v(dp), v(act), v(uc), v(mi), pp.shape[0], n_pal, palsize, desired, 7,
                                           None, None, None)


@pytest.mark.parametrize("what", ["pal_negative", "pal_too_large", "byte_too_large"])
def test_refusals_name_the_lowest_tile(gpu, what):
    tiles, dith, n_pal, desired, palsize, active, use_count = (np.array(a) if isinstance(a, np.ndarray) else a
                                                               for a in _case("mixed_16")[0])
    on = np.nonzero(active)[0]
    lo, hi = int(on[40]), int(on[900])

    def spoil(t):
        if what == "pal_negative":
            dith[t] = -1
        elif what == "pal_too_large":
            dith[t] = n_pal
        else:
            tiles[t, 63 if t == lo else 0] = palsize

    spoil(hi)
    spoil(lo)
    mi = np.full(tiles.shape[0], 123, np.int64)
    before = [a.copy() for a in (tiles, dith, active, use_count, mi)]
    assert _raw_call(tiles, dith, active, use_count, mi, n_pal, palsize, desired) == -1
    msg = _lib.last_error()
    assert f"tile {lo} " in msg, msg
    assert ("dith_pal %d" % dith[lo] in msg) if what.startswith("pal") else ("palette index 16 at pixel 63" in msg), msg
    for a, b in zip((tiles, dith, active, use_count, mi), before):
        assert np.array_equal(a, b)  # the host form leaves its arrays as they were
    with pytest.raises(_lib.TilerError, match=f"tile {lo} "):
        gt.do_global_tiling_gpu(tiles, dith, n_pal, desired, palsize, active=active, use_count=use_count)
    # the same values on inactive tiles are accepted (and the call after a refusal is a normal one)
    active[[lo, hi]] = 0
    ref = gt.do_global_tiling(tiles, dith, n_pal, desired, palsize, active=active, use_count=use_count)
    out = gt.do_global_tiling_gpu(tiles, dith, n_pal, desired, palsize, active=active, use_count=use_count)
    assert all(np.array_equal(a, b) for a, b in zip(out, ref))


# ---- empty inputs ----
def test_no_tiles_and_no_active_tiles(gpu):
    out = gt.do_global_tiling_gpu(np.zeros((0, 64), np.uint8), np.zeros(0, np.int32), 4, 10, return_plan=True)
    assert [a.shape[0] for a in out[:4]] == [0, 0, 0, 0]
    assert out[4].tolist() == [0] * 4 and out[5]["bin_size"].tolist() == [0] * 4 and out[5]["start"].tolist() == [-7] * 4
    rng = np.random.default_rng(9)
    tiles = rng.integers(0, 16, (300, 64)).astype(np.uint8)
    dith = rng.integers(-3, 9, 300).astype(np.int32)
    uc = rng.integers(1, 9, 300).astype(np.int64)
    pp, act, uc2, mi, k, info = gt.do_global_tiling_gpu(tiles, dith, 4, 10, active=np.zeros(300, np.uint8),
                                                        use_count=uc, restart=3, return_plan=True)
    assert np.array_equal(pp, tiles) and not act.any() and np.array_equal(uc2, uc) and (mi == -1).all()
    assert k.tolist() == [0] * 4 and info["start"].tolist() == [-3] * 4


# ---- the device-array medoids ----
def test_medoids_batch_dev_equals_host_form(gpu):
    import torch
    from tiler_amd.kmodes import compute_kmodes_batch, medoids_batch
    (tiles, dith, n_pal, desired, palsize, active, _), plan, _, _ = _case("mixed_16")
    X = np.ascontiguousarray(np.concatenate([plan.lines[plan.bins[p]] for p in plan.run]))
    off = np.zeros(len(plan.run) + 1, np.int32)
    off[1:] = np.cumsum([plan.bins[p].size for p in plan.run])
    ks = np.array([plan.k_per_bin[p] for p in plan.run], np.int32)
    st = np.array([plan.starts[p] for p in plan.run], np.int32)
    labels, cent, _, _ = compute_kmodes_batch(X, off, ks, st, palsize)
    med, cnt = medoids_batch(X, off, ks, labels, cent)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(a).to(dev) for a in (X, labels, cent)]
    d_med = torch.full((int(ks.sum()),), -9, dtype=torch.int32, device=dev)
    d_cnt = torch.full((int(ks.sum()),), -9, dtype=torch.int32, device=dev)
    vp = ctypes.c_void_p
    rc = _lib.load().tiler_kmodes_medoids_batch_dev(vp(d[0].data_ptr()), off.ctypes.data_as(vp), len(plan.run),
                                                    ks.ctypes.data_as(vp), vp(d[1].data_ptr()), vp(d[2].data_ptr()),
                                                    vp(d_med.data_ptr()), vp(d_cnt.data_ptr()),
                                                    vp(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, _lib.last_error()
    assert np.array_equal(d_med.cpu().numpy(), med) and np.array_equal(d_cnt.cpu().numpy(), cnt)


# ---- the chain ----
def test_encoder_chain_with_the_flag(gpu):
    from tiler_amd.encoder import Encoder
    from tiler_amd.frame_tiling import FT_MEDIUM
    v = synth.video(52, 320, 240, kf_frames=(3, 3), n_palettes=8)
    a = Encoder(v)
    b = Encoder(v, gpu_global_tiling=True, gpu_unique=True, gpu_reindex=True)
    assert b.gpu_global_tiling and not a.gpu_global_tiling

    def same():
        for name in ("palpix", "thm", "tvm", "dith_pal", "active", "use_count", "tile", "pal", "hm", "vm"):
            x, y = getattr(a, name), getattr(b, name)
            assert x.shape == y.shape and np.array_equal(x, y), name

    steps = [lambda e: e.do_make_unique(), lambda e: e.do_global_tiling(700), lambda e: e.do_frame_tiling(FT_MEDIUM),
             lambda e: e.do_reindex(), lambda e: e.do_smooth(0.2)]
    for i, step in enumerate(steps):
        ra, rb = step(a), step(b)
        same()
        if i == 1:
            assert np.array_equal(ra, rb)  # k_per_bin
            gts = a.save_tileset()
            assert gts == b.save_tileset() and len(gts) > 1
    for name in ("tile", "pal", "hm", "vm", "smoothed"):
        assert np.array_equal(a.sm[name], b.sm[name]), name


def test_run_all_with_the_flag(gpu):
    from tiler_amd.encoder import Encoder
    v = synth.video(52, 320, 240, kf_frames=(3, 3), n_palettes=8)
    a = Encoder(v)
    b = Encoder(v, gpu_global_tiling=True, gpu_unique=True, gpu_reindex=True)
    a.run_all(700)
    b.run_all(700)
    for name in ("palpix", "use_count", "tile", "pal"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.save_tileset() == b.save_tileset()
