#!/usr/bin/env python3
"""GlobalTiling's reload branch on MI355X: the C4 tile set matched against the tileset its own GlobalTiling saved.

ReloadPreviousTiling (main.pas:4372-4470) on the SURVEY.md 8(d) synthetic workload: 1,048,576 tiles (65,536
prototypes, 10 % per-byte perturbation) against the 65,536-tile .gts that DoGlobalTiling of the same seed writes.
The timed step is tiler_tileset_match_dev over the whole tile list, everything resident in HBM (after one untimed
call; kernel timers off), with the argmin kernel at 1 and at 2 queries per thread.  For comparison, in the same
process: the pairs/s of the K-Modes assignment kernel (kmb_assign16, from the GlobalTiling run that produced the
tileset, HIP-event busy time), and one oracle thread (pyoracle.km_get_min on the same buckets) on a sample of tiles,
which is also checked against the GPU's answer.

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


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--desired", type=int, default=65536)
    ap.add_argument("--bins", type=int, default=128)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--cpu-tiles", type=int, default=64, help="tiles of the one-thread oracle sample")
    ap.add_argument("--reps", type=int, default=3)
    return ap


def run(args) -> dict:
    import torch
    import tiler_amd
    from tiler_amd import global_tiling as gt
    from tiler_amd import synth
    from tiler_amd._lib import check

    lib = tiler_amd.load()
    torch.cuda.init()
    check(lib.tiler_init(torch.cuda.current_device()), "tiler_init")
    dev = torch.device("cuda", torch.cuda.current_device())
    vp = ctypes.c_void_p
    tiles, dith = synth.globaltiling_workload(args.seed, args.n, n_palettes=args.bins)

    # the tileset: DoGlobalTiling of the same tiles (K-Modes on the GPU, timers on for kmb_assign16's rate)
    t0 = time.perf_counter()
    lib.tiler_timing_reset()
    lib.tiler_timing_enable(1)
    pp, act, uc, _, _ = gt.do_global_tiling(tiles, dith, args.bins, args.desired)
    lib.tiler_timing_enable(0)
    n_l = ctypes.c_int(0)
    asg_ms = lib.tiler_timing_get(b"kmodes_assign", ctypes.byref(n_l))
    km_pairs = ctypes.c_int64(0)
    check(lib.tiler_kmodes_last_stats(ctypes.byref(km_pairs), None), "tiler_kmodes_last_stats")
    lib.tiler_timing_reset()
    pp, act, uc, _ = gt.make_tiles_unique(pp, act, uc)
    data = gt.write_tileset(pp, act, 16)
    t_gt = time.perf_counter() - t0
    kmb_rate = km_pairs.value / (asg_ms * 1e-3) if asg_ms > 0 else None

    active = np.ones(args.n, np.uint8)
    d_act = torch.from_numpy(active).to(dev)
    d_idx = torch.empty(args.n, dtype=torch.int32, device=dev)
    d_dis = torch.empty(args.n, dtype=torch.int64, device=dev)
    src = torch.from_numpy(tiles).to(dev)
    d_pix = torch.empty_like(src)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ts = gt.Tileset(data, 16)
    pairs = ctypes.c_int64(0)

    def match():
        d_pix.copy_(src)
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        check(lib.tiler_tileset_match_dev(ts._h, vp(d_pix.data_ptr()), vp(d_act.data_ptr()), args.n,
                                          vp(d_idx.data_ptr()), vp(d_dis.data_ptr()), vp(stream)),
              "tiler_tileset_match_dev")
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t

    ab = {}
    try:
        for qpt in (1, 2):
            check(lib.tiler_debug_reload(0, qpt, 0), "tiler_debug_reload")
            match()  # untimed: module load, scratch growth
            walls = [match() for _ in range(args.reps)]
            check(lib.tiler_reload_last_pairs(ctypes.byref(pairs)), "tiler_reload_last_pairs")
            lib.tiler_timing_reset()
            lib.tiler_timing_enable(1)
            match()
            lib.tiler_timing_enable(0)
            ph = {}
            for name in ("reload_rows", "reload_sort", "reload_match", "reload_gather"):
                ph[name] = round(lib.tiler_timing_get(name.encode(), None), 3)
            lib.tiler_timing_reset()
            idx = d_idx.cpu().numpy()
            ab[qpt] = {"wall_s": [round(w, 4) for w in walls], "wall_s_median": round(float(np.median(walls)), 4),
                       "phases_ms": ph, "match_pairs_per_s": round(pairs.value / (ph["reload_match"] * 1e-3), 1),
                       "digest": "%08x" % zlib.crc32(d_pix.cpu().numpy().tobytes(), zlib.crc32(idx.tobytes()))}
    finally:
        lib.tiler_debug_reload(0, 0, 0)
    check(lib.tiler_debug_reload(0, 0, 0), "tiler_debug_reload")
    wall = match()  # the shipped default once more: the reported value
    idx = d_idx.cpu().numpy()
    dis = d_dis.cpu().numpy().astype(np.uint64)

    # one oracle thread on a sample of tiles (and a check of the GPU's answer on them)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle
    rows64, _ = gt.read_tileset(data, 16)
    lines = gt.write_tile_dataset_line(rows64, 16)
    sg = gt.pal_signi(rows64, 16)
    buckets = {int(s): np.nonzero(sg == s)[0] for s in np.unique(sg)}
    sample = np.random.default_rng(1).choice(args.n, args.cpu_tiles, replace=False)
    q_lines = gt.write_tile_dataset_line(tiles[sample], 16)
    q_sg = gt.pal_signi(tiles[sample], 16)
    cpu_pairs, bad = 0, 0
    sub = {s: np.ascontiguousarray(lines[b]) for s, b in buckets.items()}
    tc = time.perf_counter()
    for k, i in enumerate(sample):
        s = int(q_sg[k])
        if s in sub:
            j, d = pyoracle.km_get_min(sub[s], q_lines[k])
            j = int(buckets[s][j])
            cpu_pairs += sub[s].shape[0]
        else:
            j, d = pyoracle.km_get_min(lines, q_lines[k])
            cpu_pairs += lines.shape[0]
        bad += int(j != idx[i] or d != dis[i])
    t_cpu = time.perf_counter() - tc
    ts.close()
    best = ab[min(ab, key=lambda q: ab[q]["wall_s_median"])]
    return {
        "metric": "GlobalTiling reload seconds (1M tiles against a 64k-tile .gts)", "value": round(wall, 4),
        "unit": "s", "higher_is_better": False, "n_gpus": 1, "dtype": "u8",
        "data": "synthetic (seeded, SURVEY.md 8(d))",
        "config": {"tiles": args.n, "tileset_rows": int(ts.n), "buckets": len(buckets),
                   "largest_bucket": int(max(b.size for b in buckets.values()))},
        "pairs": int(pairs.value), "pairs_per_s_wall": round(pairs.value / wall, 1),
        "queries_per_thread_ab": ab, "default_digest_equal": len({v["digest"] for v in ab.values()}) == 1,
        "kmb_assign16": {"pairs": int(km_pairs.value), "busy_ms": round(asg_ms, 2),
                         "pairs_per_s": round(kmb_rate, 1) if kmb_rate else None},
        "match_vs_kmb_assign16": round(best["match_pairs_per_s"] / kmb_rate, 3) if kmb_rate else None,
        "globaltiling_s": round(t_gt, 2),
        "cpu_one_thread": {"tiles": int(sample.size), "pairs": int(cpu_pairs), "seconds": round(t_cpu, 4),
                           "pairs_per_s": round(cpu_pairs / t_cpu, 1) if t_cpu else None,
                           "projected_s_all_tiles": round(t_cpu / sample.size * args.n, 1),
                           "mismatching_gpu": bad},
    }


def main():
    print(json.dumps(run(parser().parse_args())))


if __name__ == "__main__":
    main()
