"""GlobalTiling step (btnDoGlobalTilingClick main.pas:837-856 -> DoGlobalTiling main.pas:4256-4370).

Host bookkeeping mirrors the reference procedures by name; the K-Modes reduction and the medoid choice
run on the GPU, all palette bins in one batch (tiler_kmodes_batch / tiler_kmodes_medoids_batch; the
reference runs the bins concurrently with ProcThreadPool, main.pas:4339):
  write_tile_dataset_line  WriteTileDatasetLine main.pas:4167-4183 (+ GetTilePalZoneThres 4142-4165)
  equal_quality_tile_count EqualQualityTileCount main.pas:722-725
  do_global_tiling         DoGlobalTiling 4256-4331 + DoKModes 4195-4254 + MergeTiles 3688-3712
  do_global_tiling_gpu     the same through one library call (tiler_global_tiling): the plan and the merges on the GPU too
  tile_dataset_lines_gpu / global_tiling_counts
                           its dataset-line kernel and its cluster counts alone
  make_tiles_unique        MakeTilesUnique 2555-2612 (stable order: lowest index represents duplicates)
  make_tiles_unique_gpu    the same on the GPU (tiler_make_tiles_unique), any number of chunks in one call
  reindex_tiles            ReindexTiles 4483-4527 (UseCount desc, old index asc)
  use_count_gpu / reindex_tiles_gpu / gather_tiles_gpu / remap_items_gpu
                           btnReindexClick's counts 1208-1221, ReindexTiles and the TileMap remap (also
                           FinishMergeTiles 3722-3734) on the GPU (tiler_tile_use_count, tiler_reindex_tiles, ...)
The reload branch (ReloadPreviousTiling main.pas:4372-4470) snaps every active tile to its closest tile of a saved
tileset instead; the matching runs on the GPU (tiler_tileset_load / tiler_tileset_match):
  write_tileset / read_tileset  the .gts file (main.pas:4359-4367 / 4420-4438)
  pal_signi                GetTilePalZoneThres' return value (main.pas:4142-4165)
  reload_previous_tiling   DoFindBest 4377-4410 over all tiles + MakeTilesUnique (4464)
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np

from ._lib import check, load
from .kmodes import compute_kmodes_batch, medoids_batch

CRANDOM_KMODES_COUNT = 7  # cRandomKModesCount main.pas:19


def write_tile_dataset_line(tiles: np.ndarray, palsize: int = 16) -> np.ndarray:
    """[T, 64] palette indices -> [T, 80] K-Modes rows: 64 indices + 16 zone flags
    (count(idx*16 div palsize == z) > palsize div 16)."""
    t = np.asarray(tiles, np.uint8).reshape(-1, 64)
    zone = (t.astype(np.int64) * 16) // palsize
    acc = np.stack([(zone == z).sum(1) for z in range(16)], 1)
    flags = (acc > (palsize // 16)).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([t, flags], 1))


FPC_INV_LN2 = 1.4426950408889634079  # FPC Math.log2(x) = ln(x) * 1.4426950408889634079


def equal_quality_tile_count(n: float) -> int:
    """round(sqrt(n) * log2(1 + n)) (main.pas:722-725) with FPC's banker's rounding (Python round is half-even)
    and FPC Math's log2 = ln(x) * (1 / ln 2)."""
    return int(round(math.sqrt(n) * (math.log(1.0 + n) * FPC_INV_LN2)))


def kmodes_medoids(X: np.ndarray, labels: np.ndarray, centroids: np.ndarray):
    lib = load()
    X = np.ascontiguousarray(X, np.uint8)
    labels = np.ascontiguousarray(labels, np.int32)
    centroids = np.ascontiguousarray(centroids, np.uint8)
    k = centroids.shape[0]
    medoid = np.zeros(k, np.int32)
    counts = np.zeros(k, np.int32)
    v = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(lib.tiler_kmodes_medoids(v(X), X.shape[0], v(labels), v(centroids), k, v(medoid), v(counts)),
          "tiler_kmodes_medoids")
    return medoid, counts


def merge_tiles(idx, best, palpix, active, use_count, merge_index):
    """MergeTiles main.pas:3688-3712 (NewTile = nil)."""
    for j in idx:
        if j == best:
            continue
        use_count[best] += use_count[j]
        active[j] = 0
        merge_index[j] = best
        palpix[j] = 0


@dataclass
class GTPlan:
    """DoGlobalTiling's binning (main.pas:4272-4331): the K-Modes rows, the active tiles of each palette bin,
    their StartingPoint and ClusterCount, and the bins that go through K-Modes (`run`)."""
    lines: np.ndarray
    bins: list
    starts: list
    k_per_bin: np.ndarray
    run: list


def plan_global_tiling(palpix, dith_pal, n_palettes: int, desired: int, palsize: int = 16,
                       restart: int = CRANDOM_KMODES_COUNT, active=None) -> GTPlan:
    palpix = np.asarray(palpix, np.uint8).reshape(-1, 64)
    T = palpix.shape[0]
    active = np.ones(T, np.uint8) if active is None else np.asarray(active, np.uint8)
    dith_pal = np.asarray(dith_pal, np.int64)
    lines = write_tile_dataset_line(palpix, palsize)
    act = np.nonzero(active)[0]
    bins = [act[dith_pal[act] == p] for p in range(n_palettes)]
    # StartingPoint: last row of the bin with minimal byte sum (acc <= best), -restart when empty
    starts = []
    for b in bins:
        if b.size == 0:
            starts.append(-restart)
            continue
        s = lines[b].astype(np.int64).sum(1)
        starts.append(int(b.size - 1 - np.argmin(s[::-1])))
    dis_cnt = sum(equal_quality_tile_count(b.size) for b in bins)
    share = desired / dis_cnt
    k_per_bin = np.zeros(n_palettes, np.int64)
    run = []  # bins that go through K-Modes (DoKModes, main.pas:4195-4254)
    for p, b in enumerate(bins):
        kc = math.ceil(equal_quality_tile_count(b.size) * share)
        k_per_bin[p] = int(round(kc))
        if b.size > kc:
            run.append(p)
    return GTPlan(lines, bins, starts, k_per_bin, run)


def kmodes_bins(plan: GTPlan, subset, palsize: int = 16) -> dict:
    """K-Modes + medoids of the listed bins in ONE GPU batch: {bin: (labels, medoid, counts)}, bin-local."""
    subset = list(subset)
    if not subset:
        return {}
    X = np.ascontiguousarray(np.concatenate([plan.lines[plan.bins[p]] for p in subset]))
    off = np.zeros(len(subset) + 1, np.int32)
    off[1:] = np.cumsum([plan.bins[p].size for p in subset])
    ks = np.array([plan.k_per_bin[p] for p in subset], np.int32)
    st = np.array([plan.starts[p] for p in subset], np.int32)
    labels, cent, _, _ = compute_kmodes_batch(X, off, ks, st, palsize)
    medoid, counts = medoids_batch(X, off, ks, labels, cent)
    koff = np.concatenate([[0], np.cumsum(ks)])
    return {p: (labels[off[i]:off[i + 1]], medoid[koff[i]:koff[i + 1]], counts[koff[i]:koff[i + 1]])
            for i, p in enumerate(subset)}


def kmodes_merge_map(plan: GTPlan, results: dict, T: int) -> np.ndarray:
    """DoKModes' merge decisions (main.pas:4231-4253) of the bins in `results` as one int32 map over all T tiles:
    merge_to[j] = the medoid tile j merges into, -1 = kept.  Bins own disjoint tiles, so maps of different bin
    sets combine with an element-wise max (the sharded path's all-reduce)."""
    merge_to = np.full(T, -1, np.int32)
    for p, (labels, medoid, counts) in results.items():
        b = plan.bins[p]
        best = np.where(counts >= 2, b[np.maximum(medoid, 0)], -1)[labels]
        sel = (best >= 0) & (b != best)
        merge_to[b[sel]] = best[sel]
    return merge_to


def apply_merge_map(merge_to, palpix, active, use_count):
    """MergeTiles for every merged tile (main.pas:3688-3712, NewTile = nil): UseCount summed into the medoid,
    Active := False, MergeIndex set, PalPixels zeroed.  Each medoid is kept (merge_to = -1), so the order of the
    reference's per-cluster loop does not change the result."""
    palpix = np.array(palpix, np.uint8, copy=True).reshape(-1, 64)
    T = palpix.shape[0]
    active = np.ones(T, np.uint8) if active is None else np.array(active, np.uint8, copy=True)
    use_count = np.ones(T, np.int64) if use_count is None else np.array(use_count, np.int64, copy=True)
    merge_to = np.asarray(merge_to, np.int64)
    src = np.nonzero(merge_to >= 0)[0]
    dst = merge_to[src]
    np.add.at(use_count, dst, use_count[src])
    active[src] = 0
    merge_index = np.full(T, -1, np.int64)
    merge_index[src] = dst
    palpix[src] = 0
    return palpix, active, use_count, merge_index


def apply_kmodes_merges(plan: GTPlan, results: dict, palpix, active, use_count):
    """MergeTiles for every cluster with >= 2 members (main.pas:4231-4253) of every K-Modes bin."""
    T = np.asarray(palpix).reshape(-1, 64).shape[0]
    return apply_merge_map(kmodes_merge_map(plan, results, T), palpix, active, use_count)


def do_global_tiling(palpix, dith_pal, n_palettes: int, desired: int, palsize: int = 16,
                     restart: int = CRANDOM_KMODES_COUNT, active=None, use_count=None):
    """Returns (palpix, active, use_count, merge_index, k_per_bin) after the K-Modes merge pass
    (the caller applies merge_index to tilemaps: FinishMergeTiles main.pas:3722-3734)."""
    plan = plan_global_tiling(palpix, dith_pal, n_palettes, desired, palsize, restart, active)
    res = kmodes_bins(plan, plan.run, palsize)
    pp, act, uc, mi = apply_kmodes_merges(plan, res, palpix, active, use_count)
    return pp, act, uc, mi, plan.k_per_bin


# ---- the K-Modes branch on the GPU (tiler_amd/csrc/global_tiling.hip): numpy arrays in and out ----
def global_tiling_counts(bin_size, desired: int):
    """plan_global_tiling's cluster counts alone (tiler_global_tiling_counts, host code): bin_size [n_palettes] ->
    (k int64 [n_palettes] = k_per_bin, run bool [n_palettes])."""
    b = np.asarray(bin_size)
    if b.ndim != 1 or b.size < 1:
        raise ValueError("global_tiling_counts: bin_size must be [n_palettes], n_palettes >= 1")
    if b.dtype.kind not in "iu":
        raise ValueError("global_tiling_counts: bin_size must hold integers")
    if int(b.min()) < 0 or int(b.max()) >= (1 << 31):
        raise ValueError("global_tiling_counts: a bin size outside [0, 2^31)")
    b = np.ascontiguousarray(b, np.int32)
    k = np.zeros(b.size, np.int32)
    run = np.zeros(b.size, np.uint8)
    check(load().tiler_global_tiling_counts(_vp(b), b.size, int(desired), _vp(k), _vp(run)),
          "tiler_global_tiling_counts")
    return k.astype(np.int64), run.astype(bool)


def tile_dataset_lines_gpu(tiles, palsize: int = 16, lines: bool = True, signi: bool = True):
    """write_tile_dataset_line and pal_signi on the GPU (tiler_tile_dataset_lines): (lines [T][80] u8, pal_signi [T]
    i32); an output switched off is None."""
    t = np.asarray(tiles)
    if t.dtype != np.uint8:
        raise ValueError("tile_dataset_lines_gpu: tiles must be uint8")
    if t.size % 64 or (t.ndim != 1 and t.shape[-1] != 64 and t.shape[-2:] != (8, 8)):
        raise ValueError("tile_dataset_lines_gpu: tiles must be [T][64]")
    t = np.ascontiguousarray(t).reshape(-1, 64)
    T = t.shape[0]
    out_l = np.zeros((T, 80), np.uint8) if lines else None
    out_s = np.zeros(T, np.int32) if signi else None
    check(load().tiler_tile_dataset_lines(_vp(t), T, int(palsize), _vp(out_l), _vp(out_s)),
          "tiler_tile_dataset_lines")
    return out_l, out_s


def do_global_tiling_gpu(palpix, dith_pal, n_palettes: int, desired: int, palsize: int = 16,
                         restart: int = CRANDOM_KMODES_COUNT, active=None, use_count=None, return_plan: bool = False):
    """do_global_tiling with the plan, the K-Modes batch, the medoids and the merges in one library call
    (tiler_global_tiling): the same (palpix, active, use_count, merge_index, k_per_bin).  return_plan: a sixth
    element {"bin_size", "k", "start"} (int32 [n_palettes] each: plan_global_tiling's bin sizes, k_per_bin and
    starts)."""
    pp = np.array(palpix, np.uint8, copy=True, order="C").reshape(-1, 64)
    T = pp.shape[0]
    act = np.ones(T, np.uint8) if active is None else np.array(active, np.uint8, copy=True, order="C")
    uc = np.ones(T, np.int64) if use_count is None else np.array(use_count, np.int64, copy=True, order="C")
    dp = np.asarray(dith_pal)
    if dp.dtype.kind not in "iu":
        raise ValueError("do_global_tiling_gpu: dith_pal must hold integers")
    if act.shape != (T,) or uc.shape != (T,) or dp.shape != (T,):
        raise ValueError("do_global_tiling_gpu: dith_pal, active and use_count must be [T]")
    if dp.dtype != np.int32 and T and (int(dp.min()) < -(1 << 31) or int(dp.max()) >= (1 << 31)):
        raise ValueError("do_global_tiling_gpu: a dith_pal value does not fit 32 bits")
    dp = np.ascontiguousarray(dp, np.int32)
    n_palettes = int(n_palettes)
    if n_palettes < 1:
        raise ValueError("do_global_tiling_gpu: n_palettes must be at least 1")
    mi = np.full(T, -1, np.int64)
    size = np.zeros(n_palettes, np.int32)
    k = np.zeros(n_palettes, np.int32)
    start = np.zeros(n_palettes, np.int32) if return_plan else None
    check(load().tiler_global_tiling(_vp(pp), _vp(dp), _vp(act), _vp(uc), _vp(mi), T, n_palettes, int(palsize),
                                     int(desired), int(restart), _vp(size), _vp(k), _vp(start)), "tiler_global_tiling")
    out = (pp, act, uc, mi, k.astype(np.int64))
    return out + ({"bin_size": size, "k": k, "start": start},) if return_plan else out


def make_tiles_unique(palpix, active, use_count):
    """MakeTilesUnique main.pas:2555-2612 over all tiles.  Active tiles sorted by CompareTilePalPixels
    (CompareDWord over 16 little-endian dwords, main.pas:2546-2553; equal keys by index: TFPList.Sort is
    unstable); each run of identical tiles merges into its first member.  The final
    DoOneMerge runs with i = Count - 1 (main.pas:2604-2605), so the last run never includes its last member
    and a 2-member last run does not merge: reproduced, not fixed."""
    palpix = np.array(palpix, np.uint8, copy=True)
    active = np.array(active, np.uint8, copy=True)
    use_count = np.array(use_count, np.int64, copy=True)
    merge_index = np.full(palpix.shape[0], -1, np.int64)
    idx = np.nonzero(active)[0]
    if idx.size:
        words = np.ascontiguousarray(palpix[idx]).view("<u4").reshape(-1, 16)
        order = idx[np.lexsort(words[:, ::-1].T)]  # dword 0 primary; stable: index order among equal keys
        w = np.ascontiguousarray(palpix[order]).view("<u4").reshape(-1, 16)
        starts = np.concatenate([[0], np.nonzero(np.any(w[1:] != w[:-1], axis=1))[0] + 1])
        ends = np.concatenate([starts[1:], [order.size]])
        ends[-1] -= 1  # the reference's final DoOneMerge: i := sortList.Count - 1
        for a, b in zip(starts, ends):
            if b - a >= 2:
                members = order[a:b]
                merge_tiles(members, int(members[0]), palpix, active, use_count, merge_index)
    return palpix, active, use_count, merge_index


def make_tiles_unique_gpu(palpix, active, use_count, seg_off=None):
    """make_tiles_unique on the GPU (tiler_make_tiles_unique): the same (palpix, active, use_count, merge_index).
    seg_off [nseg + 1] (non-decreasing from 0 to T): one MakeTilesUnique per segment [seg_off[s], seg_off[s+1]) in one
    call, as btnDoMakeUniqueClick runs one per chunk; merge_index keeps whole-list indices.  None = the whole list."""
    palpix = np.array(palpix, np.uint8, copy=True, order="C").reshape(-1, 64)
    T = palpix.shape[0]
    active = np.array(active, np.uint8, copy=True, order="C")
    use_count = np.array(use_count, np.int64, copy=True, order="C")
    if active.shape != (T,) or use_count.shape != (T,):
        raise ValueError("make_tiles_unique_gpu: active and use_count must be [T]")
    seg_off = np.ascontiguousarray([0, T] if seg_off is None else seg_off, np.int64).ravel()
    if seg_off.size < 2:
        raise ValueError("make_tiles_unique_gpu: seg_off must hold at least one segment")
    merge_index = np.full(T, -1, np.int64)
    v = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(load().tiler_make_tiles_unique(v(palpix), v(active), v(use_count), v(merge_index), T, v(seg_off),
                                         seg_off.size - 1), "tiler_make_tiles_unique")
    return palpix, active, use_count, merge_index


def reindex_tiles(active, use_count):
    """ReindexTiles main.pas:4483-4527: idx_map[old] = new, order (UseCount desc, old index asc)."""
    act = np.nonzero(active)[0]
    order = act[np.lexsort((act, -np.asarray(use_count)[act]))]
    idx_map = np.full(np.asarray(active).shape[0], -1, np.int64)
    idx_map[order] = np.arange(order.size)
    return idx_map


# ---- Reindex on the GPU (tiler_amd/csrc/reindex.hip): numpy arrays in and out, like make_tiles_unique_gpu ----
def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _items32(tile, who: str) -> np.ndarray:
    """TileMap items as the library takes them: flat, contiguous int32 (a value that does not fit is refused)."""
    t = np.asarray(tile)
    if t.dtype.kind not in "iu":
        raise ValueError(f"{who}: tilemap items must be integers")
    if t.dtype != np.int32 and t.size and (int(t.min()) < -(1 << 31) or int(t.max()) >= (1 << 31)):
        raise ValueError(f"{who}: a tilemap item does not fit 32 bits")
    return np.ascontiguousarray(t, np.int32).ravel()


def use_count_gpu(tile, T: int, use_count=None):
    """btnReindexClick's UseCount / Active (main.pas:1208-1221) on the GPU (tiler_tile_use_count): (use_count int64 [T]
    = np.bincount(tile, minlength=T), active uint8 [T] = use_count > 0).  use_count given ([T]): the items are
    counted on top of a copy of it (another keyframe's or rank's count), and active is that of the sum."""
    T = int(T)
    if T < 0:
        raise ValueError("use_count_gpu: T must not be negative")
    items = _items32(tile, "use_count_gpu")
    acc = use_count is not None
    uc = np.array(use_count, np.int64, copy=True, order="C") if acc else np.zeros(T, np.int64)
    if uc.shape != (T,):
        raise ValueError("use_count_gpu: use_count must be [T]")
    active = np.zeros(T, np.uint8)
    check(load().tiler_tile_use_count(_vp(items), items.size, T, _vp(uc), _vp(active), int(acc)),
          "tiler_tile_use_count")
    return uc, active


def reindex_tiles_gpu(active, use_count, return_order: bool = False):
    """reindex_tiles on the GPU (tiler_reindex_tiles): the same idx_map; return_order: (idx_map, order), order[new] =
    old over the active tiles."""
    active = np.asarray(active)
    use_count = np.asarray(use_count)
    if active.ndim != 1 or use_count.shape != active.shape:
        raise ValueError("reindex_tiles_gpu: active and use_count must be [T]")
    active = np.ascontiguousarray(active != 0, np.uint8)
    use_count = np.ascontiguousarray(use_count, np.int64)
    T = active.shape[0]
    idx_map = np.full(T, -1, np.int64)
    order = np.full(T, -1, np.int64)
    n = ctypes.c_int64(0)
    check(load().tiler_reindex_tiles(_vp(active), _vp(use_count), T, _vp(idx_map), _vp(order), ctypes.byref(n)),
          "tiler_reindex_tiles")
    return (idx_map, order[:n.value]) if return_order else idx_map


def gather_tiles_gpu(order, palpix=None, thm=None, tvm=None, dith_pal=None, use_count=None):
    """The tile list in a new order on the GPU (tiler_gather_tiles): a[order] for every array given, as a tuple in
    the order of the arguments (palpix [T][64] u8, thm / tvm [T] u8, dith_pal [T] i32, use_count [T] i64)."""
    order = np.asarray(order)
    if order.ndim != 1:
        raise ValueError("gather_tiles_gpu: order must be [n]")
    order = np.ascontiguousarray(order, np.int64)
    given = [(palpix, np.uint8, (64,)), (thm, np.uint8, ()), (tvm, np.uint8, ()), (dith_pal, np.int32, ()),
             (use_count, np.int64, ())]
    T = None
    ins, outs = [], []
    for a, dt, tail in given:
        if a is None:
            ins.append(None)
            outs.append(None)
            continue
        a = np.ascontiguousarray(a, dt)
        if a.ndim != 1 + len(tail) or a.shape[1:] != tail or (T is not None and a.shape[0] != T):
            raise ValueError("gather_tiles_gpu: the arrays must be [T] ([T][64] for palpix) with one T")
        T = a.shape[0]
        ins.append(a)
        outs.append(np.zeros((order.size,) + tail, dt))
    if T is None:
        raise ValueError("gather_tiles_gpu: nothing to gather")
    args = [x for pair in zip(ins, outs) for x in pair]
    check(load().tiler_gather_tiles(_vp(order), order.size, *[_vp(x) for x in args], T), "tiler_gather_tiles")
    return tuple(o for o in outs if o is not None)


def remap_items_gpu(tile, map, keep_unmapped: bool = False):  # noqa: A002 (the issue's name for the argument)
    """TileMap items through an index map on the GPU (tiler_remap_items), shape and dtype of `tile` kept:
    map[tile] (ReindexTiles; -1 where the tile was dropped), or with keep_unmapped np.where(map[tile] >= 0,
    map[tile], tile) (FinishMergeTiles)."""
    tile = np.asarray(tile)
    m = np.asarray(map)
    if m.ndim != 1:
        raise ValueError("remap_items_gpu: map must be [T]")
    if m.dtype.kind not in "iu":
        raise ValueError("remap_items_gpu: map must hold integers")
    items = np.array(_items32(tile, "remap_items_gpu"), copy=True)
    m = np.ascontiguousarray(m, np.int64)
    check(load().tiler_remap_items(_vp(items), items.size, _vp(m), m.shape[0], int(bool(keep_unmapped))),
          "tiler_remap_items")
    return items.reshape(tile.shape).astype(tile.dtype, copy=False)


# ---- the reload branch: .gts files and ReloadPreviousTiling (main.pas:4372-4470) ----
def pal_signi(tiles: np.ndarray, palsize: int = 16) -> np.ndarray:
    """[T, 64] palette indices -> [T] PalSigni, the return value of GetTilePalZoneThres with 16 zones
    (main.pas:4142-4165): min over zones z of 64 - count(idx*16 div palsize == z), 0..64.  ReloadPreviousTiling
    buckets by it; it is not the DitheringPalIndex DoGlobalTiling bins by."""
    t = np.asarray(tiles, np.uint8).reshape(-1, 64)
    zone = (t.astype(np.int64) * 16) // palsize
    acc = np.stack([(zone == z).sum(1) for z in range(16)], 1)
    return (64 - acc.max(1)).astype(np.int32)


def write_tileset(palpix, active, palsize: int = 16) -> bytes:
    """The .gts bytes DoGlobalTiling writes (main.pas:4359-4367): one byte FTilePaletteSize, then the 64 PalPixels of
    every Active tile in tile-index order."""
    palpix = np.asarray(palpix, np.uint8).reshape(-1, 64)
    act = np.nonzero(np.asarray(active))[0]
    return bytes([palsize & 255]) + np.ascontiguousarray(palpix[act]).tobytes()


def read_tileset(data, palsize: int = 16):
    """.gts bytes -> (rows [n][64] rescaled to the clip's palsize, the file's palette size), as ReloadPreviousTiling
    reads them (main.pas:4420-4438): n = size div 64; a size that is no multiple of 64 starts with the file's palette
    size, else the file is a header-less one of palette size 64; every byte becomes (v * palsize) div file_palsize,
    kept as a byte."""
    raw, file_palsize = _split_tileset(data)
    if file_palsize == 0:
        raise ValueError("read_tileset: the file's palette size is 0")
    rows = ((raw.astype(np.int64) * palsize) // file_palsize).astype(np.uint8)
    return rows, file_palsize


def _split_tileset(data):
    buf = np.frombuffer(bytes(data), np.uint8)
    n = buf.size // 64
    if buf.size % 64:
        return buf[1:1 + n * 64].reshape(n, 64), int(buf[0])
    return buf.reshape(n, 64), 64


class Tileset:
    """A saved tileset resident on the GPU (tiler_tileset_load): the file's tiles rescaled, as dataset lines bucketed
    by PalSigni.  close() frees it."""

    def __init__(self, data, palsize: int = 16):
        raw, self.file_palsize = _split_tileset(data)
        if self.file_palsize == 0:
            raise ValueError("Tileset: the file's palette size is 0")
        self.n, self.palsize = raw.shape[0], palsize
        raw = np.ascontiguousarray(raw)
        self._lib = load()
        self._h = self._lib.tiler_tileset_load(raw.ctypes.data_as(ctypes.c_void_p), self.n, self.file_palsize, palsize)
        if not self._h:
            check(-1, "tiler_tileset_load")

    def match(self, palpix, active):
        """DoFindBest over all tiles: (new palpix, idx [T] file-order row or -1, dis [T])."""
        pp = np.array(palpix, np.uint8, copy=True, order="C").reshape(-1, 64)
        act = np.ascontiguousarray(active, np.uint8)
        T = pp.shape[0]
        idx = np.full(T, -1, np.int32)
        dis = np.zeros(T, np.uint64)
        v = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        check(self._lib.tiler_tileset_match(self._h, v(pp), v(act), T, v(idx), v(dis)), "tiler_tileset_match")
        return pp, idx, dis

    def close(self):
        if self._h:
            self._lib.tiler_tileset_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def min_matching_dissim_groups(rows, grp_off, items, item_grp):
    """Batched GetMinMatchingDissim (tiler_min_matching_dissim_groups): rows [n][80] in groups [grp_off[g],
    grp_off[g+1]), items [m][80] each searched in its group (-1 or an empty group: all rows) -> (idx [m], dis [m])."""
    rows = np.ascontiguousarray(rows, np.uint8).reshape(-1, 80)
    items = np.ascontiguousarray(items, np.uint8).reshape(-1, 80)
    grp_off = np.ascontiguousarray(grp_off, np.int32)
    item_grp = np.ascontiguousarray(item_grp, np.int32)
    m = items.shape[0]
    idx = np.full(m, -1, np.int32)
    dis = np.zeros(m, np.uint64)
    v = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(load().tiler_min_matching_dissim_groups(v(rows), rows.shape[0], v(grp_off), grp_off.size - 1, v(items),
                                                  v(item_grp), m, v(idx), v(dis)), "tiler_min_matching_dissim_groups")
    return idx, dis


def reload_previous_tiling(palpix, active, use_count, tileset_bytes, palsize: int = 16, gpu_unique: bool = False):
    """ReloadPreviousTiling main.pas:4372-4470: every Active tile's PalPixels become those of its closest tile of the
    saved tileset (GPU), then MakeTilesUnique over all tiles (gpu_unique: on the GPU too); no K-Modes, no
    ReindexTiles.  Mirror flags, DitheringPalIndex and the tilemaps are not touched here (the caller applies
    merge_index to the tilemaps).  Returns (palpix, active, use_count, merge_index, idx, dis); idx / dis are the
    per-tile match."""
    with Tileset(tileset_bytes, palsize) as ts:
        pp, idx, dis = ts.match(palpix, active)
    pp, act, uc, mi = (make_tiles_unique_gpu if gpu_unique else make_tiles_unique)(pp, active, use_count)
    return pp, act, uc, mi, idx, dis
