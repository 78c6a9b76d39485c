"""GTM playback timings on a C3-shape clip: 1080p (240 x 135 tiles), 24-frame keyframes, --keyframes keyframes, made
by the project's own writer (tiler_amd.gtm.save_stream) from synthetic SmoothedTileMaps (every later frame of a
keyframe keeps 60 % of the previous frame's items, so they are written as SkipBlock runs).

Host: open = tiler_gtm_open (header, LZMA decode of the keyframe streams on the default thread count, token walk);
lzma = the streams decoded one after the other (tiler_lzma_decode); walk = open on one thread minus lzma.
Device (the library's HIP-event timers on the launch stream, per played frame): play_stage (the dense items to HBM),
play_resolve, play_draw, for the tile-major and the raster layout, a keyframe (24 frames) per call; and in the same
process, alternating with them, tiler_render_frames_dev ("render") over the same SmoothedTileMaps of one keyframe --
it writes the same bytes as the tile-major draw, so it is that kernel's yardstick.  The tile-major frames are first
checked against the render kernel's, top byte masked.  Median and all values of --reps runs after --warmup runs.
GB/s = the bytes a kernel must move (draw: 256 B written + 8 B read per item; resolve: 10 B read + 8 B written) over
its time; hbm_write_fraction = the draw's written bytes per second over the 6.3 TB/s an MI355X sustains.
Prints one JSON line.

`python bench_play.py [--keyframes 3] [--reps 5] [--warmup 2]`
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time

import numpy as np

TM_W, TM_H, T, P, KF_FRAMES, KEEP = 240, 135, 65536, 128, 24, 0.6
HBM_SUSTAINED = 6.3e12


def make_clip(keyframes: int):
    rng = np.random.default_rng(2024)
    Q, F = TM_W * TM_H, keyframes * KF_FRAMES
    tile = rng.integers(0, T, (F, Q), dtype=np.int32)
    pal = rng.integers(0, P, (F, Q), dtype=np.int32)
    hm, vm = rng.integers(0, 2, (F, Q), dtype=np.uint8), rng.integers(0, 2, (F, Q), dtype=np.uint8)
    sm = np.zeros((F, Q), np.uint8)
    for f in range(F):
        if f % KF_FRAMES:
            keep = rng.random(Q) < KEEP
            for a in (tile, pal, hm, vm):
                a[f] = np.where(keep, a[f - 1], a[f])
            sm[f] = keep
    palpix = rng.integers(0, 16, (T, 64), dtype=np.uint8)
    thm, tvm = rng.integers(0, 2, T, dtype=np.uint8), rng.integers(0, 2, T, dtype=np.uint8)
    pals = rng.integers(0, 1 << 24, (keyframes, P, 16), dtype=np.int32)
    return dict(tile=tile, pal=pal, hm=hm, vm=vm, sm=sm, palpix=palpix, thm=thm, tvm=tvm, pals=pals,
                kf_start=np.arange(keyframes + 1) * KF_FRAMES)


def timed(lib, family: str) -> float:
    import ctypes
    n = ctypes.c_int(0)
    ms = lib.tiler_timing_get(family.encode(), ctypes.byref(n))
    if ms < 0 or n.value < 1:
        raise RuntimeError(f"no {family} timing recorded")
    return ms


def stats(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits),
            "max": round(max(xs), digits), "all": [round(x, digits) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import tiler_amd
    from tiler_amd import gtm, quality
    from tiler_amd._lib import check
    lib = tiler_amd.load()
    check(lib.tiler_init(0), "tiler_init")
    Q, F = TM_W * TM_H, a.keyframes * KF_FRAMES
    c = make_clip(a.keyframes)
    t0 = time.perf_counter()
    data = gtm.save_stream(c["palpix"], c["thm"], c["tvm"], c["kf_start"], c["pals"], c["tile"], c["pal"], c["hm"],
                           c["vm"], c["sm"], TM_W * 8, TM_H * 8, 24.0)
    save_s = time.perf_counter() - t0

    # host: open, LZMA alone, token walk
    open_ms, open1_ms, lzma_ms = [], [], []
    for _ in range(3):
        t0 = time.perf_counter()
        gtm.Stream(data).close()
        open_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        gtm.Stream(data, threads=1).close()
        open1_ms.append((time.perf_counter() - t0) * 1e3)
        at, t0, raw_bytes = int.from_bytes(data[8:12], "little"), time.perf_counter(), 0
        while at < len(data):
            raw, used = gtm.lzma_decode(data[at:])
            raw_bytes += len(raw)
            at += used
        lzma_ms.append((time.perf_counter() - t0) * 1e3)

    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dtype=dt)  # noqa: E731
    k0 = slice(0, KF_FRAMES)
    items = [dev(c["tile"][k0], torch.int32), dev(c["pal"][k0], torch.int32), dev(c["hm"][k0], torch.uint8),
             dev(c["vm"][k0], torch.uint8)]
    palpix, thm, tvm = dev(c["palpix"], torch.uint8), dev(c["thm"], torch.uint8), dev(c["tvm"], torch.uint8)
    pals = dev(c["pals"][0], torch.int32)
    row0 = torch.zeros(KF_FRAMES, dtype=torch.int32, device="cuda")
    invalid = torch.empty(KF_FRAMES, dtype=torch.int32, device="cuda")
    ref = torch.empty((KF_FRAMES, Q, 64), dtype=torch.int32, device="cuda")
    out = torch.empty((KF_FRAMES, Q, 64), dtype=torch.int32, device="cuda")
    undrawn = torch.empty(KF_FRAMES, dtype=torch.int32, device="cuda")

    def render():
        quality.render_frames_dev(KF_FRAMES, Q, *[t.data_ptr() for t in items], T, palpix.data_ptr(), thm.data_ptr(),
                                  tvm.data_ptr(), P, 16, pals.data_ptr(), row0.data_ptr(), P, ref.data_ptr(),
                                  invalid.data_ptr())

    st = gtm.Stream(data)
    lib.tiler_timing_enable(1)
    res = {"render": [], "tiles": {"stage": [], "resolve": [], "draw": []},
           "raster": {"stage": [], "resolve": [], "draw": []}}
    equal = None
    for i in range(a.warmup + a.reps):
        lib.tiler_timing_reset()
        render()
        torch.cuda.synchronize()
        if i >= a.warmup:
            res["render"].append(timed(lib, "render") / KF_FRAMES)
        for layout in ("tiles", "raster"):
            lib.tiler_timing_reset()
            st.rewind()
            for k in range(a.keyframes):
                if st.play_dev(KF_FRAMES, out.data_ptr(), layout, undrawn.data_ptr()) != KF_FRAMES:
                    raise RuntimeError("bench_play: short play")
                if equal is None:  # keyframe 0, tile-major: the render kernel's frames
                    torch.cuda.synchronize()
                    equal = bool(torch.equal(out & 0x00FFFFFF, ref)) and int(undrawn.sum()) == 0
            torch.cuda.synchronize()
            if i >= a.warmup:
                for fam in ("stage", "resolve", "draw"):
                    res[layout][fam].append(timed(lib, "play_" + fam) / F)
    lib.tiler_timing_enable(0)
    lib.tiler_timing_reset()
    st.close()

    def kernel(ms, bytes_per_frame, written_per_frame=None):
        s = stats(ms)
        s["gb_per_s"] = round(bytes_per_frame / (s["median"] * 1e-3) / 1e9, 1)
        if written_per_frame:
            s["hbm_write_fraction"] = round(written_per_frame / (s["median"] * 1e-3) / HBM_SUSTAINED, 3)
        return s

    draw_b, res_b = Q * (256 + 8), Q * 18
    report = {"bench": "play", "shape": f"{TM_W * 8}x{TM_H * 8}", "device": torch.cuda.get_device_name(0),
              "frames": F, "keyframes": a.keyframes, "file_bytes": len(data), "raw_bytes": raw_bytes,
              "save_stream_s": round(save_s, 2), "tiles_equal_render_masked": equal,
              "host_ms": {"open": stats(open_ms, 1), "open_1thread": stats(open1_ms, 1), "lzma": stats(lzma_ms, 1),
                          "walk": round(statistics.median(open1_ms) - statistics.median(lzma_ms), 1)},
              "per_frame_ms": {"render": kernel(res["render"], Q * (256 + 10), Q * 256)}}
    for layout in ("tiles", "raster"):
        report["per_frame_ms"][layout] = {"stage": kernel(res[layout]["stage"], Q * 10),
                                          "resolve": kernel(res[layout]["resolve"], res_b),
                                          "draw": kernel(res[layout]["draw"], draw_b, Q * 256)}
    print(json.dumps(report))
    if not equal:
        sys.exit(1)


if __name__ == "__main__":
    main()
