#!/usr/bin/env python3
"""Reindex on MI355X: use counts, ReindexTiles' order, the tile-list gather and the TileMap remap, host numpy against
the GPU entry points.

The step (btnReindexClick main.pas:1199-1230 -> ReindexTiles 4483-4527) at three inputs:
  (a) the README's clip after FrameTiling: 1000 frames x 32,400 positions = 32.4 M items over 65,536 tiles whose use
      decays with their rank (bench_gtm.py's draw), the ranks scattered over the indices (nothing is sorted yet);
  (b) the same with one tile on 30 % of all items (a flat black tile): the contention case;
  (c) GlobalTiling's tail at C4: 1,048,576 tiles, one item each, merged down to about 65,536 active ones.
Per case: seconds of the host path in this process (np.bincount + global_tiling.reindex_tiles + the gathers and the
remap of Encoder.reindex_tiles), milliseconds of the four _dev calls with every array resident in HBM (after one
untimed call; median of --reps; kernel timers off) and their phases (one more call with the timers on), wall seconds of
the host-array entry points (copies included), the bytes moved / time of the count kernel (4 B read per item) and the
remap kernel (4 B read + 4 B written per item, plus the map), and whether the CRC-32 over all outputs is the same on
the three paths.

Prints one JSON line.  Not the headline metric (bench.py is).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PHASES = ("reindex_count", "reindex_active", "reindex_order", "reindex_gather", "reindex_remap")
LIST = (("palpix", np.uint8), ("thm", np.uint8), ("tvm", np.uint8), ("dith_pal", np.int32))


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--positions", type=int, default=32400)
    ap.add_argument("--tiles", type=int, default=65536)
    ap.add_argument("--hot", type=float, default=0.3, help="share of the items on one tile in case (b)")
    ap.add_argument("--c4-tiles", type=int, default=1 << 20)
    ap.add_argument("--c4-active", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    return ap


def digest(arrays) -> str:
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return "%08x" % c


def tile_list(rng, T):
    return {"palpix": rng.integers(0, 16, (T, 64)).astype(np.uint8), "thm": rng.integers(0, 2, T).astype(np.uint8),
            "tvm": rng.integers(0, 2, T).astype(np.uint8), "dith_pal": rng.integers(0, 128, T).astype(np.int32)}


def decaying_items(rng, n, T):
    """bench_gtm.py's draw (use ~ 1 / rank^0.9), the ranks at random indices."""
    w = 1.0 / np.arange(1, T + 1) ** 0.9
    cdf = np.cumsum(w / w.sum())
    rank = np.minimum(np.searchsorted(cdf, rng.random(n)), T - 1)
    return rng.permutation(T).astype(np.int32)[rank]


def run(args) -> dict:
    import torch
    import tiler_amd
    from tiler_amd import global_tiling as gt
    from tiler_amd._lib import check

    lib = tiler_amd.load()
    torch.cuda.init()
    check(lib.tiler_init(torch.cuda.current_device()), "tiler_init")
    dev = torch.device("cuda", torch.cuda.current_device())
    vp = ctypes.c_void_p
    stream = torch.cuda.current_stream(dev).cuda_stream
    dp = lambda t: vp(t.data_ptr())  # noqa: E731

    def host_path(tile, T, tl):
        uc = np.bincount(tile, minlength=T).astype(np.int64)
        active = (uc > 0).astype(np.uint8)
        idx_map = gt.reindex_tiles(active, uc)
        keep = np.nonzero(idx_map >= 0)[0]
        order = np.empty(keep.size, np.int64)
        order[idx_map[keep]] = keep
        out = [np.ascontiguousarray(tl[n][order]) for n, _ in LIST] + [uc[order]]
        return [uc, active, idx_map] + out + [idx_map[tile].astype(np.int32)]

    def array_path(tile, T, tl):
        uc, active = gt.use_count_gpu(tile, T)
        idx_map, order = gt.reindex_tiles_gpu(active, uc, return_order=True)
        out = gt.gather_tiles_gpu(order, *[tl[n] for n, _ in LIST], uc)
        return [uc, active, idx_map] + list(out) + [gt.remap_items_gpu(tile, idx_map)]

    def case(tile, T, tl):
        n = tile.size
        t0 = time.perf_counter()
        host = host_path(tile, T, tl)
        t_host = time.perf_counter() - t0
        # everything in HBM
        src = torch.from_numpy(tile).to(dev)
        d_tile = torch.empty_like(src)
        d_in = [torch.from_numpy(tl[name]).to(dev) for name, _ in LIST]
        d_uc = torch.empty(T, dtype=torch.int64, device=dev)
        d_act = torch.empty(T, dtype=torch.uint8, device=dev)
        d_map = torch.empty(T, dtype=torch.int64, device=dev)
        d_ord = torch.empty(T, dtype=torch.int64, device=dev)
        d_out = [torch.empty_like(x) for x in d_in] + [torch.empty_like(d_uc)]
        n_act = ctypes.c_int64(0)

        def once():
            d_tile.copy_(src)
            torch.cuda.synchronize(dev)
            t = time.perf_counter()
            check(lib.tiler_tile_use_count_dev(dp(d_tile), n, T, dp(d_uc), dp(d_act), 0, vp(stream)),
                  "tiler_tile_use_count_dev")
            check(lib.tiler_reindex_tiles_dev(dp(d_act), dp(d_uc), T, dp(d_map), dp(d_ord), ctypes.byref(n_act),
                                              vp(stream)), "tiler_reindex_tiles_dev")
            pairs = [dp(x) for io in zip(d_in + [d_uc], d_out) for x in io]
            check(lib.tiler_gather_tiles_dev(dp(d_ord), n_act.value, *pairs, T, vp(stream)), "tiler_gather_tiles_dev")
            check(lib.tiler_remap_items_dev(dp(d_tile), n, dp(d_map), T, 0, vp(stream)), "tiler_remap_items_dev")
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t) * 1e3

        once()  # untimed: module load, block cache
        ms = [once() for _ in range(args.reps)]
        lib.tiler_timing_reset()
        lib.tiler_timing_enable(1)
        once()
        lib.tiler_timing_enable(0)
        ph = {name: round(lib.tiler_timing_get(name.encode(), None), 4) for name in PHASES}
        lib.tiler_timing_reset()
        m = n_act.value
        dev_out = [d_uc.cpu().numpy(), d_act.cpu().numpy(), d_map.cpu().numpy()] + \
                  [x.cpu().numpy()[:m] for x in d_out] + [d_tile.cpu().numpy()]
        # host arrays in and out
        array_path(tile, T, tl)
        t0 = time.perf_counter()
        arr = array_path(tile, T, tl)
        t_arr = time.perf_counter() - t0
        dg = {"host": digest(host), "dev": digest(dev_out), "host_arrays": digest(arr)}
        med = float(np.median(ms))
        gbs = lambda b, t: round(b / (t * 1e-3) / 1e9, 1) if t > 0 else None  # noqa: E731
        return {"items": int(n), "tiles": int(T), "active": int(m), "top_tile_share": round(float(host[0].max()) / n, 4),
                "host_s": round(t_host, 4), "dev_ms": [round(x, 4) for x in ms], "dev_ms_median": round(med, 4),
                "phases_ms": ph, "host_arrays_wall_s": round(t_arr, 4), "host_over_dev": round(t_host * 1e3 / med, 1),
                "count_gb_s": gbs(4.0 * n, ph["reindex_count"]),
                "remap_gb_s": gbs(8.0 * n + 8.0 * T, ph["reindex_remap"]),
                "digest": dg, "digest_equal": len(set(dg.values())) == 1}

    rng = np.random.default_rng(args.seed)
    n, T = args.frames * args.positions, args.tiles
    tl = tile_list(rng, T)
    items = decaying_items(rng, n, T)
    ra = case(items, T, tl)
    hot = items.copy()
    hot[rng.random(n) < args.hot] = np.int32(T // 3)
    rb = case(hot, T, tl)
    del items, hot
    # (c): every tile of the C4 list holds one item; the K-Modes / MakeTilesUnique merges point it at a survivor
    T4 = args.c4_tiles
    surv = np.sort(rng.permutation(T4)[:args.c4_active]).astype(np.int32)
    merged = surv[decaying_items(rng, T4, surv.size)]
    merged[surv] = surv
    rc = case(merged, T4, tile_list(rng, T4))
    return {
        "metric": "Reindex ms (32.4 M items, 65,536 tiles, HBM-resident: count + order + gather + remap)",
        "value": ra["dev_ms_median"], "unit": "ms", "higher_is_better": False, "n_gpus": 1, "dtype": "i32",
        "data": "synthetic (seeded)",
        "config": {"frames": args.frames, "positions": args.positions, "tiles": T, "hot": args.hot,
                   "c4_tiles": T4, "c4_active": args.c4_active, "reps": args.reps},
        "after_frame_tiling": ra, "after_frame_tiling_hot_tile": rb, "global_tiling_tail": rc,
        "digests_equal": bool(ra["digest_equal"] and rb["digest_equal"] and rc["digest_equal"]),
    }


def main():
    print(json.dumps(run(parser().parse_args())))


if __name__ == "__main__":
    main()
