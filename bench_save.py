"""SaveStream timings on a 1080p clip (240 x 135 tiles): 3 keyframes of 24 frames, T = 70,000 tiles (so LongTileIdx
occurs), 128 palettes, at three smoothed fractions (0, about 0.5, about 0.9).  The smoothed flags come in runs --
geometric lengths, mean 24 positions, from fixed seeds -- as DoTemporalSmoothing leaves them along still areas, not
at independent random positions; a keyframe's first frame has none.

Per fraction, median and all values of --reps runs after --warmup runs:
  kernel_ms      the command words of the whole clip on the GPU, tiler_gtm_commands_dev from arrays in HBM: the
                 library's HIP-event timers gtm_count + gtm_scan + gtm_fixed + gtm_emit (per frame and in total),
                 and the call's wall time with its one wait;
  python_ms      gtm.keyframe_commands on the same arrays, per keyframe summed (host, one thread);
  lzma_ms        wall time of compressing the three raw streams on the default thread pool (gtm.compress_streams);
  write_ms       the whole tiler_gtm_write from host arrays (staging, kernels, copies back, LZMA, container);
  python_save_ms gtm.save_stream on the same arrays (once, not repeated);
  lzma_fraction  lzma_ms / write_ms: the share of a native save that is LZMA;
  files_equal    tiler_gtm_write's file == gtm.save_stream's, byte for byte.
No speed-up is claimed for the whole file: LZMA is host work in both writers.  Prints one JSON line.

`python bench_save.py [--reps 5] [--warmup 2]`
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
import time

import numpy as np

TM_W, TM_H, T, P, KF_FRAMES, KEYFRAMES, MEAN_RUN = 240, 135, 70000, 128, 24, 3, 24
FRACTIONS = (0.0, 0.5, 0.9)
FAMILIES = ("gtm_count", "gtm_scan", "gtm_fixed", "gtm_emit")


def run_flags(rng, Q: int, fraction: float) -> np.ndarray:
    """One frame's flags: alternating smoothed / live runs of geometric lengths whose means give `fraction`."""
    sm = np.zeros(Q, np.uint8)
    if fraction <= 0.0:
        return sm
    live_mean = MEAN_RUN * (1.0 - fraction) / fraction
    q = 0
    while q < Q:
        n = int(rng.geometric(1.0 / MEAN_RUN))
        sm[q:q + n] = 1
        q += n + int(rng.geometric(1.0 / max(live_mean, 1.0)))
    return sm


def make_clip(fraction: float):
    rng = np.random.default_rng(2025 + int(fraction * 100))
    Q, F = TM_W * TM_H, KEYFRAMES * KF_FRAMES
    sm = np.stack([run_flags(rng, Q, fraction if f % KF_FRAMES else 0.0) for f in range(F)])
    return dict(tile=rng.integers(0, T, (F, Q), dtype=np.int32), pal=rng.integers(0, P, (F, Q), dtype=np.int32),
                hm=rng.integers(0, 2, (F, Q), dtype=np.uint8), vm=rng.integers(0, 2, (F, Q), dtype=np.uint8), sm=sm,
                palpix=rng.integers(0, 16, (T, 64), dtype=np.uint8), thm=rng.integers(0, 2, T, dtype=np.uint8),
                tvm=rng.integers(0, 2, T, dtype=np.uint8), pals=rng.integers(0, 1 << 24, (KEYFRAMES, P, 16), dtype=np.int32),
                kf_start=np.arange(KEYFRAMES + 1) * KF_FRAMES)


def stats(xs, digits=3):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits),
            "max": round(max(xs), digits), "all": [round(x, digits) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import tiler_amd
    from tiler_amd import gtm
    from tiler_amd._lib import check
    lib = tiler_amd.load()
    check(lib.tiler_init(0), "tiler_init")
    Q, F = TM_W * TM_H, KEYFRAMES * KF_FRAMES
    W, H, fps = TM_W * 8, TM_H * 8, 24.0
    report = {"bench": "save", "shape": f"{W}x{H}", "device": torch.cuda.get_device_name(0), "frames": F,
              "keyframes": KEYFRAMES, "tiles": T, "cases": []}
    ok = True
    for fraction in FRACTIONS:
        c = make_clip(fraction)
        order = ("palpix", "thm", "tvm", "pals", "tile", "pal", "hm", "vm", "sm")
        host = [c["palpix"], c["thm"], c["tvm"], c["kf_start"], c["pals"], c["tile"], c["pal"], c["hm"], c["vm"], c["sm"]]
        dev = {k: torch.from_numpy(c[k]).cuda() for k in order}
        src, keep = gtm.gtm_source(dev["palpix"].data_ptr(), dev["thm"].data_ptr(), dev["tvm"].data_ptr(), c["kf_start"],
                                   dev["pals"].data_ptr(), dev["tile"].data_ptr(), dev["pal"].data_ptr(),
                                   dev["hm"].data_ptr(), dev["vm"].data_ptr(), dev["sm"].data_ptr(), width=W, height=H,
                                   fps=fps, tiles=T, n_palettes=P, frames=F, positions=Q)
        off = np.zeros(KEYFRAMES + 1, np.int64)
        check(lib.tiler_gtm_commands_dev(ctypes.byref(src), None, 0, off.ctypes.data_as(ctypes.c_void_p), None),
              "tiler_gtm_commands_dev")
        d_raw = torch.empty(int(off[-1]), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        kernel, call, py, lz, wr = [], [], [], [], []
        raws = None
        lib.tiler_timing_enable(1)
        for i in range(a.warmup + a.reps):
            lib.tiler_timing_reset()
            t0 = time.perf_counter()
            check(lib.tiler_gtm_commands_dev(ctypes.byref(src), ctypes.c_void_p(d_raw.data_ptr()), d_raw.numel(),
                                             off.ctypes.data_as(ctypes.c_void_p), None), "tiler_gtm_commands_dev")
            torch.cuda.synchronize()
            t_call = (time.perf_counter() - t0) * 1e3
            ms = 0.0
            for fam in FAMILIES:
                n = ctypes.c_int(0)
                v = lib.tiler_timing_get(fam.encode(), ctypes.byref(n))
                if v < 0 or n.value != 1:
                    raise RuntimeError(f"bench_save: {fam} was timed {n.value} times")
                ms += v
            lib.tiler_timing_enable(0)
            t0 = time.perf_counter()
            got = [gtm.keyframe_commands(*[c[k][f0:f1] for k in ("tile", "pal", "hm", "vm", "sm")], c["thm"], c["tvm"],
                                         c["pals"][k]) for k, (f0, f1) in enumerate(zip(c["kf_start"], c["kf_start"][1:]))]
            t_py = (time.perf_counter() - t0) * 1e3
            if raws is None:  # the kernel's words are the Python writer's (after keyframe 0's WriteTiles)
                raw = d_raw.cpu().numpy()
                raws = [raw[off[k]:off[k + 1]].tobytes() for k in range(KEYFRAMES)]
                ok = ok and raws[0][24 + 64 * T:] == got[0] and raws[1:] == got[1:]
            t0 = time.perf_counter()
            gtm.compress_streams(raws)
            t_lz = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            data = gtm.save_stream_gpu(*host, W, H, fps)
            t_wr = (time.perf_counter() - t0) * 1e3
            lib.tiler_timing_enable(1)
            if i >= a.warmup:
                kernel.append(ms), call.append(t_call), py.append(t_py), lz.append(t_lz), wr.append(t_wr)
        lib.tiler_timing_enable(0)
        lib.tiler_timing_reset()
        t0 = time.perf_counter()
        want = gtm.save_stream(*host, W, H, fps)
        t_save = (time.perf_counter() - t0) * 1e3
        equal = data == want
        ok = ok and equal
        report["cases"].append({
            "smoothed_fraction": round(float(c["sm"].mean()), 3), "raw_bytes": int(off[-1]), "file_bytes": len(data),
            "kernel_ms": stats(kernel), "kernel_ms_per_frame": round(statistics.median(kernel) / F, 5),
            "commands_call_ms": stats(call), "python_ms": stats(py, 1),
            "python_ms_per_frame": round(statistics.median(py) / F, 3), "lzma_ms": stats(lz, 1),
            "write_ms": stats(wr, 1), "python_save_ms": round(t_save, 1),
            "lzma_fraction": round(statistics.median(lz) / statistics.median(wr), 3), "files_equal": equal})
    report["words_equal"] = ok
    print(json.dumps(report))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
