#!/usr/bin/env python3
"""QuantizePalette's value-at-risk path (chkUseDL3 off) on MI355X, beside DLv3 and the CPU restatement.

One 8-frame 1080p keyframe (259,200 tiles, synth.keyframe_frames), 128 palettes -- the shape of bench.py's
secondary.palettes -- with the tiles assigned to palettes by mean luma (a stand-in for PrepareDitherTiles' k-means that
costs nothing here: similar tiles share a palette), pal_var 0.95.  tiler_quantize_palettes_var_dev with the tiles
resident in HBM: wall and HIP-event milliseconds of the whole call (after one untimed call; median of --reps; kernel
timers off), then one more call with the timers on for its stages -- var_usage (pixel keys, sort, run lengths,
segments), var_items (items, the two sorts, links, differences, prefix sums), var_prune (cut-off, tree, rounds, pick) --
and from the stats the largest pair, the most merges of a pair and the prune stage's microseconds per round of that
pair's chain (the stage is as long as its slowest pair).  In the same process: tiler_quantize_palettes_dev (DLv3, bpc 7)
on the same input, and the Python restatement (tests/var_palette_ref.py) on the --ref-pairs pairs that are cheapest
for it (it rescans a pair's whole list every round) on one host thread, its palettes and stats compared.

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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

STAGES = ("var_usage", "var_items", "var_prune")


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--tiles-per-frame", type=int, default=240 * 135)
    ap.add_argument("--palettes", type=int, default=128)
    ap.add_argument("--pal-var", type=float, default=0.95)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-pairs", type=int, default=3)
    return ap


def run(args) -> dict:
    import torch
    import tiler_amd
    import var_palette_ref as ref
    from tiler_amd import synth
    from tiler_amd._lib import check
    from tiler_amd.palette import var_acc0

    lib = tiler_amd.load()
    torch.cuda.init()
    check(lib.tiler_init(torch.cuda.current_device()), "tiler_init")
    dev = torch.device("cuda", torch.cuda.current_device())
    vp = ctypes.c_void_p
    hp = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    stream = torch.cuda.current_stream(dev).cuda_stream
    F, Q, P = args.frames, args.tiles_per_frame, args.palettes
    rgb = synth.keyframe_frames(np.random.default_rng(args.seed), F, Q).reshape(-1, 64)
    n = rgb.shape[0]
    luma = ((rgb & 255) * 2126 + ((rgb >> 8) & 255) * 7152 + ((rgb >> 16) & 255) * 722).sum(1)
    pal_of = np.empty(n, np.int32)
    pal_of[np.argsort(luma, kind="stable")] = (np.arange(n, dtype=np.int64) * P // n).astype(np.int32)
    acc0 = var_acc0([0, F], Q, P, args.pal_var)
    d_rgb, d_po = torch.from_numpy(rgb).to(dev), torch.from_numpy(pal_of).to(dev)
    pal, uc, stats = np.zeros((P, 16), np.int32), np.zeros(P, np.int32), np.zeros((P, 4), np.int32)

    def timed(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        a.record()
        call()
        b.record()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t) * 1e3, a.elapsed_time(b)

    var_call = lambda: check(lib.tiler_quantize_palettes_var_dev(  # noqa: E731
        n, vp(d_rgb.data_ptr()), vp(d_po.data_ptr()), None, P, 16, P, hp(acc0), hp(pal), hp(uc), hp(stats), vp(stream)),
        "tiler_quantize_palettes_var_dev")
    timed(var_call)  # untimed: module load
    t_var = [timed(var_call) for _ in range(args.reps)]
    lib.tiler_timing_reset()
    lib.tiler_timing_enable(1)
    var_call()
    lib.tiler_timing_enable(0)
    st = {name: round(lib.tiler_timing_get(name.encode(), None), 4) for name in STAGES}
    lib.tiler_timing_reset()
    big = int(np.argmax(stats[:, 2]))
    rounds = int(stats[big, 2]) + 1  # the round that stops the loop merges too, or finds nothing

    dpal, duc, dcol = np.zeros((P, 16), np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    dl3_call = lambda: check(lib.tiler_quantize_palettes_dev(  # noqa: E731
        n, vp(d_rgb.data_ptr()), vp(d_po.data_ptr()), None, P, 16, 7, hp(dpal), hp(duc), hp(dcol), vp(stream)),
        "tiler_quantize_palettes_dev")
    timed(dl3_call)
    t_dl3 = [timed(dl3_call) for _ in range(max(1, args.reps - 1))]

    # the restatement rescans the whole list every round: the pairs it can finish in about a minute, cheapest first
    cost = stats[:, 0].astype(np.int64) * (stats[:, 2] + 1)
    pairs = [int(p) for p in np.argsort(cost, kind="stable")[:args.ref_pairs] if cost[p] < 2e7] or \
        [int(np.argmin(cost))]
    t0 = time.perf_counter()
    rpal, ruc, rstats = ref.quantize_palettes_var(rgb, pal_of, P, P, acc0, 16, pairs=pairs)
    t_ref = time.perf_counter() - t0
    same = bool(np.array_equal(rpal[pairs], pal[pairs]) and np.array_equal(rstats[pairs], stats[pairs]) and
                np.array_equal(ruc, uc))
    med = lambda x: round(float(np.median(x)), 3)  # noqa: E731
    return {
        "metric": "value-at-risk QuantizePalette ms (8 frames of 1080p, 128 palettes, HBM-resident tiles)",
        "value": med([w for w, _ in t_var]), "unit": "ms", "higher_is_better": False, "n_gpus": 1, "dtype": "i32",
        "data": "synthetic (seeded, synth.keyframe_frames; palettes by mean luma)",
        "config": {"frames": F, "tiles_per_frame": Q, "palettes": P, "pal_var": args.pal_var, "pixels": int(n) * 64},
        "var_wall_ms": [round(w, 3) for w, _ in t_var], "var_event_ms": [round(e, 3) for _, e in t_var],
        "stages_ms": st,
        "colours": {"total": int(stats[:, 0].sum()), "largest_pair": int(stats[:, 0].max()),
                    "median_pair": int(np.median(stats[:, 0]))},
        "cml_pct_median": int(np.median(stats[:, 1])),
        "merges": {"max": int(stats[:, 2].max()), "median": int(np.median(stats[:, 2])),
                   "stopped_by_count": int((stats[:, 3] == 0).sum()), "stopped_by_repeat": int((stats[:, 3] == 1).sum())},
        "prune_us_per_round_of_slowest_pair": round(st["var_prune"] * 1e3 / rounds, 2),
        "dl3_wall_ms": [round(w, 3) for w, _ in t_dl3], "dl3_wall_ms_median": med([w for w, _ in t_dl3]),
        "restatement": {"pairs": pairs, "seconds": round(t_ref, 2), "host_threads": 1,
                        "note": "np.unique over every pixel, then the listed pairs only", "equal": same},
    }


def main():
    print(json.dumps(run(parser().parse_args())))


if __name__ == "__main__":
    main()
