#!/usr/bin/env python3
"""Raster ingest on MI355X: pictures -> tile-major frames (load_frames_kernel) and back (store_frames_kernel).

At 1080p, F = 24 frames, for BGRA32, RGB24 and RGB24 with an odd pitch (rows at every byte alignment), per case:
  * frames in HBM, HIP-event timers on the launching stream, median of --reps after --warmup: milliseconds and GB/s
    moved (bytes read + bytes written) of the load and of the store;
  * the yardstick in the same run: one device-to-device hipMemcpyAsync (torch's copy_ of two contiguous uint8
    tensors) that moves the same byte count, read + written, and the ratios to it and to the 6.3 TB/s an MI355X
    sustains;
  * the host-array call (tiler_load_frames through frames_to_tiles), copies included, wall clock.
For RGB24 also the only path there was before: np.stack([synth.screen_to_tiles(img) ...]) on the host plus
tiler_interframe_correlation, against load_clip on the same pictures, and whether both give the same frames and
correlations.

Prints one JSON line.  Not the headline metric (bench.py is).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_WRITE_TB_S = 6.3


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    return ap


def run(args) -> dict:
    import torch
    import tiler_amd
    from tiler_amd import synth
    from tiler_amd._lib import check
    from tiler_amd.keyframes import interframe_correlation
    from tiler_amd.load import (_BPP, frames_to_tiles, frames_to_tiles_dev, load_clip, load_dims, tiles_to_frames,
                                tiles_to_frames_dev)

    lib = tiler_amd._lib.load()
    torch.cuda.init()
    check(lib.tiler_init(torch.cuda.current_device()), "tiler_init")
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream(dev).cuda_stream
    F, W, H = args.frames, args.width, args.height
    tm_w, tm_h = load_dims(W, H)
    rng = np.random.default_rng(args.seed)

    def event_ms(fn):
        """median of --reps HIP-event timings of fn() after --warmup untimed calls"""
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), [round(x, 4) for x in ms]

    def wall_s(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.reps):
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
        return float(np.median(ts))

    def rate(nbytes, ms):
        return round(nbytes / (ms * 1e-3) / 1e9, 1)

    def case(fmt, row_pad):
        bpp = _BPP[fmt]
        pitch = W * bpp + row_pad
        fs = H * pitch
        buf = rng.integers(0, 256, F * fs, dtype=np.uint8)
        images = np.lib.stride_tricks.as_strided(buf, (F, H, W, bpp), (fs, pitch, bpp, 1))
        d_src = torch.from_numpy(buf).to(dev)
        d_rgb = torch.empty((F, tm_w * tm_h, 64), dtype=torch.int32, device=dev)
        d_back = torch.zeros_like(d_src)
        used = F * tm_h * 8 * tm_w * 8 * bpp          # picture bytes the kernels touch
        moved = used + d_rgb.numel() * 4               # read + written, the same for load and store
        d_a = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        d_b = torch.empty_like(d_a)

        def load():
            frames_to_tiles_dev(d_src.data_ptr(), F, W, H, d_rgb.data_ptr(), fmt, pitch, fs, stream)

        def store():
            tiles_to_frames_dev(d_rgb.data_ptr(), F, tm_w, tm_h, d_back.data_ptr(), fmt, pitch, fs, stream)

        # alternate the three so that none of them owns the warm caches
        load_ms, load_all = event_ms(load)
        copy_ms, copy_all = event_ms(lambda: d_b.copy_(d_a))
        store_ms, store_all = event_ms(store)
        copy2_ms, _ = event_ms(lambda: d_b.copy_(d_a))
        copy_ms = min(copy_ms, copy2_ms)
        torch.cuda.synchronize(dev)
        got = d_rgb.cpu().numpy()
        back = np.lib.stride_tricks.as_strided(d_back.cpu().numpy(), (F, H, W, bpp), (fs, pitch, bpp, 1))
        want_back = images[:, :tm_h * 8, :tm_w * 8].copy()
        if bpp == 4:
            want_back[..., 3] = 0xFF
        round_trip = bool(np.array_equal(back[:, :tm_h * 8, :tm_w * 8], want_back))
        host_s = wall_s(lambda: frames_to_tiles(images, fmt))
        host_ok = bool(np.array_equal(frames_to_tiles(images, fmt)[0], got))
        host_back_s = wall_s(lambda: tiles_to_frames(got, tm_w, tm_h, fmt))
        out = {"fmt": fmt, "pitch": pitch, "bytes_moved": int(moved),
               "load_ms": round(load_ms, 4), "load_ms_all": load_all, "load_gb_s": rate(moved, load_ms),
               "store_ms": round(store_ms, 4), "store_ms_all": store_all, "store_gb_s": rate(moved, store_ms),
               "d2d_copy_ms": round(copy_ms, 4), "d2d_copy_ms_all": copy_all, "d2d_copy_gb_s": rate(moved, copy_ms),
               "load_over_d2d": round(copy_ms / load_ms, 3), "store_over_d2d": round(copy_ms / store_ms, 3),
               "load_over_hbm_write_rate": round(moved / (load_ms * 1e-3) / (HBM_WRITE_TB_S * 1e12), 3),
               "store_over_hbm_write_rate": round(moved / (store_ms * 1e-3) / (HBM_WRITE_TB_S * 1e12), 3),
               "host_arrays_load_s": round(host_s, 4), "host_arrays_store_s": round(host_back_s, 4),
               "round_trip_equal": round_trip, "host_equals_dev": host_ok}
        return out, images, got

    res = {}
    res["bgra32"], _, _ = case("bgra32", 0)
    res["rgb24_odd_pitch"], _, _ = case("rgb24", 1)
    res["rgb24"], images, got = case("rgb24", 0)

    # what a caller did before: tile on the host, then hand the frames over for the correlations
    t = time.perf_counter()
    frames = np.stack([synth.screen_to_tiles(img[:tm_h * 8, :tm_w * 8]) for img in images])
    t_tile = time.perf_counter() - t
    t = time.perf_counter()
    corr = interframe_correlation(frames, tm_w, tm_h)
    t_corr = time.perf_counter() - t
    load_clip(images, "rgb24")
    t = time.perf_counter()
    clip = load_clip(images, "rgb24")
    t_clip = time.perf_counter() - t
    same = bool(np.array_equal(frames, got) and np.array_equal(clip[0], frames) and
                np.array_equal(clip[5].view(np.uint64), corr.view(np.uint64)))
    res["load_step_rgb24"] = {"host_screen_to_tiles_s": round(t_tile, 4), "interframe_correlation_s": round(t_corr, 4),
                              "parent_path_s": round(t_tile + t_corr, 4), "load_clip_s": round(t_clip, 4),
                              "parent_over_load_clip": round((t_tile + t_corr) / t_clip, 1), "equal": same}
    ok = same and all(res[k]["round_trip_equal"] and res[k]["host_equals_dev"]
                      for k in ("bgra32", "rgb24", "rgb24_odd_pitch"))
    return {"metric": "raster ingest ms (24 frames 1080p BGRA32 -> tiles, HBM-resident)",
            "value": res["bgra32"]["load_ms"], "unit": "ms", "higher_is_better": False, "n_gpus": 1, "dtype": "u8/i32",
            "data": "synthetic (seeded)",
            "config": {"frames": F, "width": W, "height": H, "tm_w": tm_w, "tm_h": tm_h, "reps": args.reps,
                       "warmup": args.warmup},
            **res, "results_equal": bool(ok)}


def main():
    print(json.dumps(run(parser().parse_args())))


if __name__ == "__main__":
    main()
