"""Quality readout timings: Render of the tilemaps (tiler_render_frames_dev) and the lblCorrel figure + SSE
(tiler_frame_quality_dev) on 1080p frames (240 x 135 tiles) resident in HBM, at F = 24 and F = 240 frames.
Timed with the library's HIP-event timers (tiler_timing_get "render" / "quality": device time on the launch
stream); the median of --reps runs after --warmup runs.  The correlation is first re-checked bit for bit against
the sequential restatement (tests/test_quality.py) at the smallest test shape.  Prints one JSON line.

`python bench_quality.py [--frames 24,240] [--reps 3] [--warmup 1]`
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

TM_W, TM_H, T, P, KF_FRAMES = 240, 135, 65536, 128, 24


def timed(lib, family: str) -> float:
    n = ctypes.c_int(0)
    ms = lib.tiler_timing_get(family.encode(), ctypes.byref(n))
    if ms < 0 or n.value < 1:
        raise RuntimeError(f"no {family} timing recorded")
    return ms


def check_bit_exact(quality) -> bool:
    from test_quality import random_frames, ref_corr, ref_sse
    rng = np.random.default_rng(31)
    src, dst = random_frames(rng, 31, 12), random_frames(rng, 31, 12)
    corr, sse = quality.frame_quality(src, dst, 4, 3)
    return bool(np.array_equal(corr.view(np.uint64), ref_corr(src, dst, 4, 3).view(np.uint64))
                and np.array_equal(sse, ref_sse(src, dst)))


def run(lib, quality, torch, F: int, reps: int, warmup: int) -> dict:
    Q = TM_W * TM_H
    g = torch.Generator(device="cuda").manual_seed(F)
    ri = lambda hi, shape, dt: torch.randint(0, hi, shape, generator=g, device="cuda", dtype=dt)  # noqa: E731
    KF = (F + KF_FRAMES - 1) // KF_FRAMES
    src = ri(1 << 24, (F, Q, 64), torch.int32)
    out = torch.empty((F, Q, 64), dtype=torch.int32, device="cuda")
    invalid = torch.empty(F, dtype=torch.int32, device="cuda")
    tm = [ri(T, (F, Q), torch.int32), ri(P, (F, Q), torch.int32), ri(2, (F, Q), torch.uint8), ri(2, (F, Q), torch.uint8)]
    sm = [ri(T, (F, Q), torch.int32), ri(P, (F, Q), torch.int32), ri(2, (F, Q), torch.uint8), ri(2, (F, Q), torch.uint8),
          ri(2, (F, Q), torch.uint8)]
    palpix, thm, tvm = ri(16, (T, 64), torch.uint8), ri(2, (T,), torch.uint8), ri(2, (T,), torch.uint8)
    pals = ri(1 << 24, (KF * P, 16), torch.int32)
    row0 = (torch.arange(F, device="cuda", dtype=torch.int32) // KF_FRAMES * P).to(torch.int32)
    torch.cuda.synchronize()
    r_ms, q_ms, corr = [], [], None
    for i in range(warmup + reps):
        lib.tiler_timing_reset()
        quality.render_frames_dev(F, Q, *[t.data_ptr() for t in tm], T, palpix.data_ptr(), thm.data_ptr(),
                                  tvm.data_ptr(), KF * P, 16, pals.data_ptr(), row0.data_ptr(), P, out.data_ptr(),
                                  invalid.data_ptr(), *[t.data_ptr() for t in sm])
        corr, sse = quality.frame_quality_dev(src.data_ptr(), out.data_ptr(), F, TM_W, TM_H)
        torch.cuda.synchronize()
        if i >= warmup:
            r_ms.append(timed(lib, "render"))
            q_ms.append(timed(lib, "quality"))
    if int(invalid.sum()) != 0 or not np.isfinite(corr).all():
        raise RuntimeError("bench_quality: unexpected invalid items or correlation")
    return {"frames": F, "render_ms": round(statistics.median(r_ms), 3), "quality_ms": round(statistics.median(q_ms), 3),
            "render_ms_all": [round(x, 3) for x in r_ms], "quality_ms_all": [round(x, 3) for x in q_ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="24,240")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import tiler_amd
    from tiler_amd import quality
    from tiler_amd._lib import check
    lib = tiler_amd.load()
    check(lib.tiler_init(0), "tiler_init")
    exact = check_bit_exact(quality)
    lib.tiler_timing_enable(1)
    res = {"bench": "quality", "shape": f"{TM_W * 8}x{TM_H * 8}", "device": torch.cuda.get_device_name(0),
           "corr_sse_bit_exact_4x3_F31": exact,
           "runs": [run(lib, quality, torch, int(F), a.reps, a.warmup) for F in a.frames.split(",")]}
    lib.tiler_timing_enable(0)
    lib.tiler_timing_reset()
    print(json.dumps(res))
    if not exact:
        sys.exit(1)


if __name__ == "__main__":
    main()
