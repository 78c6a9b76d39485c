#!/usr/bin/env python3
"""MakeTilesUnique on MI355X: the chain's three calls at the C4 size, host function against the GPU entry points.

MakeTilesUnique (main.pas:2555-2612) on the SURVEY.md 8(d) synthetic workload (1,048,576 tiles, 65,536 prototypes,
10 % per-byte perturbation, 128 palette bins: bench_reload.py's tile list), where the chain runs it:
  (a) the MakeUnique step (btnDoMakeUniqueClick main.pas:916-938): chunks of 810,000 tiles, all in one GPU call;
  (b) DoGlobalTiling's whole-list pass (main.pas:4347) over the tile list the K-Modes merges leave;
  (c) ReloadPreviousTiling's whole-list pass (main.pas:4464) after every tile was snapped to the .gts that (b) saves.
Each input is what the chain hands over at that point ((b) and (c) start from (a)'s output).  Per case: seconds of the
host function global_tiling.make_tiles_unique in this process, milliseconds of tiler_make_tiles_unique_dev with all
four arrays resident in HBM (after one untimed call; median of --reps; kernel timers off) and its four phases (one more
call with the timers on), wall seconds of the host-array entry point tiler_make_tiles_unique (copies included), and
whether the CRC-32 of the four outputs is the same on both paths.

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

PHASES = ("unique_insert", "unique_last", "unique_merge", "unique_zero")


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--desired", type=int, default=65536)
    ap.add_argument("--bins", type=int, default=128)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--chunk", type=int, default=810000, help="tiles per MakeUnique chunk of case (a)")
    ap.add_argument("--reps", type=int, default=3)
    return ap


def digest(pp, act, uc, mi) -> str:
    c = 0
    for a, dt in ((pp, np.uint8), (act, np.uint8), (uc, np.int64), (mi, np.int64)):
        c = zlib.crc32(np.ascontiguousarray(a, dt).tobytes(), c)
    return "%08x" % c


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
    stream = torch.cuda.current_stream(dev).cuda_stream

    def host_chunks(pp, act, uc, seg_off):
        """gt.make_tiles_unique segment by segment (Encoder.do_make_unique's loop)."""
        opp, oact, ouc = pp.copy(), act.copy(), uc.copy()
        omi = np.full(pp.shape[0], -1, np.int64)
        for a, b in zip(seg_off[:-1], seg_off[1:]):
            p, c, u, m = gt.make_tiles_unique(pp[a:b], act[a:b], uc[a:b])
            opp[a:b], oact[a:b], ouc[a:b] = p, c, u
            omi[a:b] = np.where(m >= 0, m + a, -1)
        return opp, oact, ouc, omi

    def case(pp, act, uc, seg_off):
        T = pp.shape[0]
        seg = np.ascontiguousarray(seg_off, np.int64)
        t0 = time.perf_counter()
        host = host_chunks(pp, act, uc, seg_off)
        t_host = time.perf_counter() - t0
        # everything in HBM
        src = [torch.from_numpy(a).to(dev) for a in (pp, act, uc)]
        d = [torch.empty_like(s) for s in src]
        d_mi = torch.empty(T, dtype=torch.int64, device=dev)

        def once():
            for x, s in zip(d, src):
                x.copy_(s)
            torch.cuda.synchronize(dev)
            t = time.perf_counter()
            check(lib.tiler_make_tiles_unique_dev(vp(d[0].data_ptr()), vp(d[1].data_ptr()), vp(d[2].data_ptr()),
                                                  vp(d_mi.data_ptr()), T, seg.ctypes.data_as(vp), seg.size - 1,
                                                  vp(stream)), "tiler_make_tiles_unique_dev")
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t) * 1e3

        once()  # untimed: module load, scratch growth
        ms = [once() for _ in range(args.reps)]
        lib.tiler_timing_reset()
        lib.tiler_timing_enable(1)
        once()
        lib.tiler_timing_enable(0)
        ph = {name: round(lib.tiler_timing_get(name.encode(), None), 4) for name in PHASES}
        lib.tiler_timing_reset()
        dev_out = [x.cpu().numpy() for x in d] + [d_mi.cpu().numpy()]
        # host arrays in and out
        gt.make_tiles_unique_gpu(pp, act, uc, seg)
        t0 = time.perf_counter()
        arr = gt.make_tiles_unique_gpu(pp, act, uc, seg)
        t_arr = time.perf_counter() - t0
        dg = {"host": digest(*host), "dev": digest(*dev_out), "host_arrays": digest(*arr)}
        res = {"tiles": int(T), "active_in": int(np.count_nonzero(act)), "segments": int(seg.size - 1),
               "merged": int((host[3] >= 0).sum()), "host_s": round(t_host, 3),
               "dev_ms": [round(m, 4) for m in ms], "dev_ms_median": round(float(np.median(ms)), 4),
               "phases_ms": ph, "host_arrays_wall_s": round(t_arr, 4),
               "host_over_dev": round(t_host * 1e3 / float(np.median(ms)), 1),
               "digest": dg, "digest_equal": len(set(dg.values())) == 1}
        return res, host

    tiles, dith = synth.globaltiling_workload(args.seed, args.n, n_palettes=args.bins)
    T = tiles.shape[0]
    seg_a = list(range(0, T, args.chunk)) + [T]
    ra, (pp, act, uc, _) = case(tiles, np.ones(T, np.uint8), np.ones(T, np.int64), seg_a)
    # (b): the K-Modes merges of DoGlobalTiling on (a)'s tile list, then the whole-list pass
    t0 = time.perf_counter()
    kpp, kact, kuc, _, _ = gt.do_global_tiling(pp, dith, args.bins, args.desired, active=act, use_count=uc)
    t_km = time.perf_counter() - t0
    rb, (bpp, bact, _, _) = case(kpp, kact, kuc, [0, T])
    # (c): (a)'s tile list snapped to the tileset (b) leaves, then the whole-list pass
    data = gt.write_tileset(bpp, bact, 16)
    t0 = time.perf_counter()
    with gt.Tileset(data, 16) as ts:
        mpp, _, _ = ts.match(pp, act)
    t_match = time.perf_counter() - t0
    rc, _ = case(mpp, act, uc, [0, T])
    return {
        "metric": "MakeTilesUnique ms (1M tiles, whole list after the K-Modes merges, HBM-resident)",
        "value": rb["dev_ms_median"], "unit": "ms", "higher_is_better": False, "n_gpus": 1, "dtype": "u8",
        "data": "synthetic (seeded, SURVEY.md 8(d))",
        "config": {"tiles": int(T), "chunk": args.chunk, "bins": args.bins, "desired": args.desired,
                   "tileset_rows": (len(data) - 1) // 64},
        "make_unique_step": ra, "after_kmodes": rb, "after_reload": rc,
        "digests_equal": bool(ra["digest_equal"] and rb["digest_equal"] and rc["digest_equal"]),
        "kmodes_wall_s": round(t_km, 2), "reload_match_wall_s": round(t_match, 3),
    }


def main():
    print(json.dumps(run(parser().parse_args())))


if __name__ == "__main__":
    main()
