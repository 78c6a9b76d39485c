#!/usr/bin/env python3
"""Dither, PsyV and Smooth on MI355X at tile palette sizes 16, 32 and 64.

Dither: one 1080p frame's 32,400 tiles with 128 palettes, Thomas Knoll and Yliluoma mix 4, every array resident in
HBM (tiler_dither_tiles[_yliluoma]_dev); HIP events around one call, median of --reps after --warmup untimed calls.
The yardstick of the 32- and 64-entry kernels is the 16-entry kernel of the same run: the work per tile is
proportional to the palette size, so `expected_ms` = t16 * size / 16 and `ratio` = measured / expected.  Beside it:
the CPU restatement's one-thread rate on a --cpu-tiles sample (tiles per second), the PsyV-from-palette time of
--items DCT descriptors at 64 entries (tiler_psyv_batch_ps_dev, fp32 out) and one Smooth call at 64
(tiler_smooth_keyframe_ps_dev, --smooth-frames x 32,400 positions over a 65,536-tile set).

Prints one JSON line.  Not the headline metric (bench.py is).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=32400)
    ap.add_argument("--palettes", type=int, default=128)
    ap.add_argument("--mix", type=int, default=4)
    ap.add_argument("--cpu-tiles", type=int, default=200)
    ap.add_argument("--items", type=int, default=65536)
    ap.add_argument("--smooth-frames", type=int, default=8)
    ap.add_argument("--tileset", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    return ap


def run(args) -> dict:
    import torch
    import pyoracle
    import tiler_amd
    from tiler_amd import synth
    from tiler_amd._lib import check

    lib = tiler_amd.load()
    torch.cuda.init()
    check(lib.tiler_init(torch.cuda.current_device()), "tiler_init")
    dev = torch.device("cuda", torch.cuda.current_device())
    vp = ctypes.c_void_p
    stream = torch.cuda.current_stream(dev).cuda_stream
    dp = lambda t: vp(t.data_ptr())  # noqa: E731
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

    def timed(call):
        """Median milliseconds of `call` between two HIP events, after the warm-up calls."""
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), [round(m, 4) for m in ms]

    rng = np.random.default_rng(args.seed)
    n, P = args.tiles, args.palettes
    rgb = synth.frame_tiles(rng, n)
    pal_of = rng.integers(0, P, n).astype(np.int32)
    d_rgb, d_po = up(rgb), up(pal_of)
    d_px = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    d_hm = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_vm = torch.zeros(n, dtype=torch.uint8, device=dev)
    out = {"bench": "palsize", "device": torch.cuda.get_device_name(dev), "tiles": n, "palettes": P, "mix": args.mix,
           "reps": args.reps, "warmup": args.warmup, "dither": {}}
    sample = np.sort(rng.choice(n, min(args.cpu_tiles, n), replace=False))
    for name, mixed in (("thomas_knoll", 0), ("yliluoma", args.mix)):
        rows = {}
        for size in (16, 32, 64):
            pals = synth.palettes(np.random.default_rng(args.seed + size), P, size).astype(np.int32)
            d_pal = up(pals)

            def call():
                if mixed:
                    rc = lib.tiler_dither_tiles_yliluoma_dev(n, dp(d_rgb), dp(d_po), dp(d_pal), P, size, mixed,
                                                             dp(d_px), dp(d_hm), dp(d_vm), vp(stream))
                else:
                    rc = lib.tiler_dither_tiles_dev(n, dp(d_rgb), dp(d_po), dp(d_pal), P, size, dp(d_px), dp(d_hm),
                                                    dp(d_vm), vp(stream))
                check(rc, "tiler_dither_tiles_dev")

            med, all_ms = timed(call)
            t0 = time.perf_counter()
            if mixed:
                o = pyoracle.dither_tiles_yl(rgb[sample], pal_of[sample], pals, mixed)
            else:
                o = pyoracle.dither_tiles_tk(rgb[sample], pal_of[sample], pals)
            cpu_s = time.perf_counter() - t0
            same = bool(np.array_equal(d_px.cpu().numpy()[sample], o[0]))
            rows[str(size)] = {"ms": round(med, 4), "runs_ms": all_ms, "mtiles_per_s": round(n / med / 1e3, 3),
                               "cpu_one_thread_tiles_per_s": round(sample.size / cpu_s, 1),
                               "sample_equals_restatement": same}
        t16 = rows["16"]["ms"]
        for size in (32, 64):
            r = rows[str(size)]
            r["expected_ms"] = round(t16 * size / 16, 4)
            r["ratio"] = round(r["ms"] / r["expected_ms"], 3)
        out["dither"][name] = rows

    # PsyV from palettes at 64: DCT + Q-weighting descriptors of --items (tile, palette) items, fp32 out
    size, T = 64, args.tileset
    pp = rng.integers(0, size, (T, 64)).astype(np.uint8)
    pals = synth.palettes(rng, P, size).astype(np.int32)
    m = args.items
    d_pp, d_pal = up(pp), up(pals)
    d_t, d_p = up(rng.integers(0, T, m).astype(np.int32)), up(rng.integers(0, P, m).astype(np.int32))
    d_out = torch.zeros((m, 192), dtype=torch.float32, device=dev)
    med, all_ms = timed(lambda: check(lib.tiler_psyv_batch_ps_dev(m, None, dp(d_pp), dp(d_t), dp(d_pal), size, dp(d_p),
                                                                  None, 1 | 8, -1, None, dp(d_out), vp(stream)),
                                      "tiler_psyv_batch_ps_dev"))
    out["psyv_from_palette_64"] = {"items": m, "ms": round(med, 4), "runs_ms": all_ms}

    # Smooth at 64: coherent tilemaps (most positions keep the previous frame's item)
    F, Q = args.smooth_frames, args.tiles
    tile = np.zeros((F, Q), np.int32)
    tile[0] = rng.integers(0, T, Q)
    for f in range(1, F):
        tile[f] = np.where(rng.random(Q) < 0.7, tile[f - 1], rng.integers(0, T, Q))
    pal = np.repeat(rng.integers(0, P, (1, Q)), F, 0).astype(np.int32)
    src = [up(tile), up(pal), torch.zeros((F, Q), dtype=torch.uint8, device=dev),
           torch.zeros((F, Q), dtype=torch.uint8, device=dev), torch.zeros((F, Q), dtype=torch.uint8, device=dev)]
    work = [t.clone() for t in src]

    def smooth():
        for w, s in zip(work, src):
            w.copy_(s)
        check(lib.tiler_smooth_keyframe_ps_dev(F, Q, dp(work[0]), None, dp(work[1]), dp(work[2]), dp(work[3]),
                                               dp(work[4]), dp(d_pp), dp(d_pal), size, 0.02, vp(stream)),
              "tiler_smooth_keyframe_ps_dev")

    med, all_ms = timed(smooth)
    out["smooth_64"] = {"frames": F, "positions": Q, "ms": round(med, 4), "runs_ms": all_ms,
                        "note": "includes the device copies that reset the tilemaps"}
    return out


def main():
    print(json.dumps(run(parser().parse_args())))


if __name__ == "__main__":
    main()
