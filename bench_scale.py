#!/usr/bin/env python3
"""Lanczos input scaling fused with the tile cut on MI355X (scale.hip: tiler_load_frames_scaled_dev).

RGB24 pictures in HBM, F = 24 frames, four cases: 3840 x 2160 at 0.5 and at 0.25, 1920 x 1080 at 0.5, 960 x 540 at 2.
Per case, in the same run, HIP-event timers on the launching stream, median of --reps after --warmup:
  * the scaled load;
  * the unscaled tiler_load_frames_dev over the same source bytes, no filtering (a source beyond ReframeUI's
    1920 x 1080 cap is handed over as that many 1920 x 1080 pictures of the same memory, so every byte is read;
    it then writes more tiles than the scaled load does -- both byte counts are reported);
  * one device-to-device copy of the source bytes;
  * the host way, where PIL imports: Image.resize(LANCZOS) of one picture on one thread plus the existing load of
    the resized picture, wall clock per picture; and whether the GPU's frame 0 equals it.
`floor_ms` is the least the scaled load could take: source bytes read once plus tiles written once at the 6.3 TB/s an
MI355X sustains.

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

HBM_TB_S = 6.3
CASES = (("4k_half", 3840, 2160, 0.5), ("4k_quarter", 3840, 2160, 0.25), ("1080p_half", 1920, 1080, 0.5),
         ("540p_double", 960, 540, 2.0))


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    return ap


def run(args) -> dict:
    import torch
    import tiler_amd
    from tiler_amd._lib import check
    from tiler_amd.load import frames_to_tiles, frames_to_tiles_dev, load_dims, scale_dims

    try:
        from PIL import Image
    except ImportError:
        Image = None

    lib = tiler_amd._lib.load()
    torch.cuda.init()
    check(lib.tiler_init(torch.cuda.current_device()), "tiler_init")
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream(dev).cuda_stream
    F = args.frames
    rng = np.random.default_rng(args.seed)

    def event_ms(fn):
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

    def case(W, H, factor):
        out_w, out_h = scale_dims(W, H, factor)
        tm_w, tm_h = load_dims(out_w, out_h)
        # smooth pictures under noise (what a resize is for), seeded
        lo = rng.integers(0, 256, (F, H // 32 + 2, W // 32 + 2, 3)).astype(np.uint8)
        pics = np.repeat(np.repeat(lo, 32, 1), 32, 2)[:, :H, :W]
        pics = np.ascontiguousarray(pics ^ rng.integers(0, 16, (F, H, W, 3), dtype=np.uint8))
        d_src = torch.from_numpy(pics.reshape(-1)).to(dev)
        d_rgb = torch.empty((F, tm_w * tm_h, 64), dtype=torch.int32, device=dev)
        # the unscaled load over the same memory: pictures within the cap
        uw, uh = min(W, 1920), min(H, 1080)
        assert W % uw == 0 and H % uh == 0
        uf = F * (W // uw) * (H // uh)
        utw, uth = load_dims(uw, uh)
        d_un = torch.empty((uf, utw * uth, 64), dtype=torch.int32, device=dev)
        d_copy = torch.empty_like(d_src)
        src_bytes = int(d_src.numel())

        def scaled():
            frames_to_tiles_dev(d_src.data_ptr(), F, W, H, d_rgb.data_ptr(), "rgb24", stream=stream,
                                size=(out_w, out_h))

        def unscaled():
            frames_to_tiles_dev(d_src.data_ptr(), uf, uw, uh, d_un.data_ptr(), "rgb24", stream=stream)

        scaled_ms, scaled_all = event_ms(scaled)
        un_ms, un_all = event_ms(unscaled)
        copy_ms, copy_all = event_ms(lambda: d_copy.copy_(d_src))
        scaled2_ms, _ = event_ms(scaled)
        scaled_ms = min(scaled_ms, scaled2_ms)
        torch.cuda.synchronize(dev)
        tile_bytes = int(d_rgb.numel()) * 4
        floor_ms = (src_bytes + tile_bytes) / (HBM_TB_S * 1e12) * 1e3
        out = {"src": [W, H], "factor": factor, "out": [out_w, out_h], "tilemap": [tm_w, tm_h], "frames": F,
               "src_bytes": src_bytes, "tile_bytes": tile_bytes,
               "scaled_ms": round(scaled_ms, 4), "scaled_ms_all": scaled_all,
               "scaled_src_gb_s": round(src_bytes / scaled_ms / 1e6, 1),
               "unscaled_ms": round(un_ms, 4), "unscaled_ms_all": un_all, "unscaled_tile_bytes": int(d_un.numel()) * 4,
               "unscaled_src_gb_s": round(src_bytes / un_ms / 1e6, 1),
               "scaled_over_unscaled_rate": round(un_ms / scaled_ms, 3),
               "d2d_copy_ms": round(copy_ms, 4), "d2d_copy_ms_all": copy_all,
               "floor_ms": round(floor_ms, 4), "scaled_over_floor": round(scaled_ms / floor_ms, 2)}
        if Image is not None:
            t = time.perf_counter()
            small = np.asarray(Image.fromarray(pics[0]).resize((out_w, out_h), Image.LANCZOS))
            t_pil = time.perf_counter() - t
            frames_to_tiles(small, "rgb24")
            t = time.perf_counter()
            host, _, _ = frames_to_tiles(small, "rgb24")
            t_load = time.perf_counter() - t
            out.update({"host_pil_resize_s_per_picture": round(t_pil, 4), "host_load_s_per_picture": round(t_load, 4),
                        "host_over_gpu_per_picture": round((t_pil + t_load) / (scaled_ms * 1e-3 / F), 1),
                        "equals_pil_frame0": bool(np.array_equal(host[0], d_rgb[0].cpu().numpy()))})
        return out

    res = {}
    for name, W, H, factor in CASES:
        if name in args.cases.split(","):
            res[name] = case(W, H, factor)
    first = next(iter(res.values()))
    ok = all(r.get("equals_pil_frame0", True) for r in res.values())
    return {"metric": "scaled raster ingest ms (24 frames RGB24 -> Lanczos -> tiles, HBM-resident)",
            "value": first["scaled_ms"], "unit": "ms", "higher_is_better": False, "n_gpus": 1, "dtype": "u8/i32",
            "data": "synthetic (seeded)", "config": {"frames": F, "reps": args.reps, "warmup": args.warmup},
            **res, "results_equal": bool(ok)}


def main():
    print(json.dumps(run(parser().parse_args())))


if __name__ == "__main__":
    main()
