#!/usr/bin/env python3
"""The whole GlobalTiling K-Modes step on MI355X through one library call (tiler_global_tiling_dev), against the host
plan around the same K-Modes kernels.

Workload: C4 (synth.globaltiling_workload: 1,048,576 tiles, 128 palette bins, desired 65,536), every array resident in
HBM.  Medians of --reps calls after --warmup untimed ones, kernel timers off; the inputs are restored from pristine
device copies before every call (outside the timed region).  Measured:
  dev            the whole tiler_global_tiling_dev call;
  phases         its parts by the library's HIP-event timers, in one more call with the timers on (an event pair
                 between dependent launches costs microseconds, so that call is not a timed one): validate + count,
                 partition, lines, K-Modes (kmodes_init + kmodes_assign + kmodes_seq + kmodes_apply), medoids, merge;
  host_arrays    tiler_global_tiling from numpy arrays, copies included;
  host_path      plan_global_tiling + kmodes_bins + apply_kmodes_merges on the same inputs (seconds, once; its parts);
  d2d_copy       a device-to-device copy of nt * (64 + 80) bytes: the floor of the non-K-Modes parts;
  kmodes_alone   tiler_kmodes_batch_dev on the same X (built by the host plan), same medians.
Checks: the CRC-32 over (palpix, active, use_count, merge_index, k_per_bin) is the same on the three paths; the
K-Modes time inside the call (whole call minus the other phases) against K-Modes alone and the spread of the runs.

Prints one JSON line and writes it to profiles/global_tiling/bench_gt_step.json.  Not the headline metric (bench.py is).
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

GT_PHASES = ("gt_validate", "gt_partition", "gt_lines", "gt_medoids", "gt_merge")
KM_PHASES = ("kmodes_init", "kmodes_assign", "kmodes_seq", "kmodes_apply")


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--desired", type=int, default=65536)
    ap.add_argument("--bins", type=int, default=128)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_tiling", "bench_gt_step.json"))
    return ap


def digest(arrays) -> str:
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return "%08x" % c


def stats(ms):
    return {"runs": [round(x, 3) for x in ms], "median": round(float(np.median(ms)), 3),
            "spread": round(float(max(ms) - min(ms)), 3)}


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
    dp = lambda t: vp(t.data_ptr())  # noqa: E731
    hp = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    nt, P, desired, palsize = args.n, args.bins, args.desired, 16

    tiles, dith = synth.globaltiling_workload(args.seed, nt, n_palettes=P)
    active = np.ones(nt, np.uint8)
    use_count = np.ones(nt, np.int64)

    # ---- the host path (the yardstick), timed in its parts ----
    t0 = time.perf_counter()
    plan = gt.plan_global_tiling(tiles, dith, P, desired, palsize, active=active)
    t_plan = time.perf_counter() - t0
    t0 = time.perf_counter()
    res = gt.kmodes_bins(plan, plan.run, palsize)
    t_bins = time.perf_counter() - t0
    t0 = time.perf_counter()
    host = gt.apply_kmodes_merges(plan, res, tiles, active, use_count) + (plan.k_per_bin,)
    t_apply = time.perf_counter() - t0

    # ---- everything in HBM ----
    src = [torch.from_numpy(a).to(dev) for a in (tiles, active, use_count)]
    d_pp, d_act, d_uc = (torch.empty_like(x) for x in src)
    d_dith = torch.from_numpy(dith).to(dev)
    d_mi = torch.empty(nt, dtype=torch.int64, device=dev)
    size, k, start = (np.zeros(P, np.int32) for _ in range(3))

    def once():
        for d, s in zip((d_pp, d_act, d_uc), src):
            d.copy_(s)
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        check(lib.tiler_global_tiling_dev(dp(d_pp), dp(d_dith), dp(d_act), dp(d_uc), dp(d_mi), nt, P, palsize, desired,
                                          gt.CRANDOM_KMODES_COUNT, hp(size), hp(k), hp(start), vp(stream)),
              "tiler_global_tiling_dev")
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t) * 1e3

    for _ in range(args.warmup):
        once()
    ms = [once() for _ in range(args.reps)]
    dev_out = [x.cpu().numpy() for x in (d_pp, d_act, d_uc, d_mi)] + [k.astype(np.int64)]
    lib.tiler_timing_reset()
    lib.tiler_timing_enable(1)
    ms_timers_on = once()
    lib.tiler_timing_enable(0)
    ph = {}
    for name in GT_PHASES + KM_PHASES:
        n = ctypes.c_int(0)
        v = lib.tiler_timing_get(name.encode(), ctypes.byref(n))
        ph[name] = {"ms": round(v, 4), "launches": n.value}
    lib.tiler_timing_reset()
    other_ms = sum(ph[n]["ms"] for n in GT_PHASES)
    km_timer_ms = sum(ph[n]["ms"] for n in KM_PHASES)

    # ---- K-Modes alone on the same X ----
    X = np.ascontiguousarray(np.concatenate([plan.lines[plan.bins[p]] for p in plan.run]))
    off = np.zeros(len(plan.run) + 1, np.int32)
    off[1:] = np.cumsum([plan.bins[p].size for p in plan.run])
    ks = np.array([plan.k_per_bin[p] for p in plan.run], np.int32)
    st = np.array([plan.starts[p] for p in plan.run], np.int32)
    d_X = torch.from_numpy(X).to(dev)
    d_lab = torch.empty(X.shape[0], dtype=torch.int32, device=dev)
    d_cent = torch.empty((int(ks.sum()), 80), dtype=torch.uint8, device=dev)

    def kmodes_once():
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        check(lib.tiler_kmodes_batch_dev(dp(d_X), hp(off), len(plan.run), hp(ks), hp(st), palsize, dp(d_lab), dp(d_cent),
                                         None, None, vp(stream)), "tiler_kmodes_batch_dev")
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t) * 1e3

    for _ in range(args.warmup):
        kmodes_once()
    km = [kmodes_once() for _ in range(args.reps)]
    km_digest = "%08x" % zlib.crc32(d_cent.cpu().numpy().tobytes(), zlib.crc32(d_lab.cpu().numpy().tobytes()))
    del d_X, d_lab, d_cent

    # ---- the copy floor ----
    a = torch.empty(nt * (64 + 80), dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)

    def copy_once():
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        b.copy_(a)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t) * 1e3

    for _ in range(args.warmup):
        copy_once()
    cp = [copy_once() for _ in range(args.reps)]
    del a, b

    # ---- host arrays in and out ----
    gt.do_global_tiling_gpu(tiles, dith, P, desired, palsize, active=active, use_count=use_count)
    arr_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        arr = gt.do_global_tiling_gpu(tiles, dith, P, desired, palsize, active=active, use_count=use_count)
        arr_s.append(time.perf_counter() - t0)

    dg = {"host_path": digest(host), "dev": digest(dev_out), "host_arrays": digest(arr)}
    med, km_med, cp_med = float(np.median(ms)), float(np.median(km)), float(np.median(cp))
    km_in_call = med - other_ms
    spread = max(max(ms) - min(ms), max(km) - min(km))
    host_s = t_plan + t_bins + t_apply
    out = {
        "metric": "GlobalTiling step ms (C4: 1M tiles, 128 bins, HBM-resident: plan + K-Modes + medoids + merges)",
        "value": round(med, 3), "unit": "ms", "higher_is_better": False, "n_gpus": 1, "dtype": "u8",
        "data": "synthetic (seeded, SURVEY.md 8(d))",
        "config": {"tiles": nt, "bins": P, "desired": desired, "bins_run": len(plan.run), "clusters": int(ks.sum()),
                   "reps": args.reps, "warmup": args.warmup},
        "dev_ms": stats(ms), "dev_ms_timers_on": round(ms_timers_on, 3), "phases": ph,
        "non_kmodes_ms": round(other_ms, 4), "kmodes_timer_ms": round(km_timer_ms, 3),
        "d2d_copy_ms": stats(cp), "non_kmodes_over_copy": round(other_ms / cp_med, 2) if cp_med > 0 else None,
        "kmodes_alone_ms": stats(km), "kmodes_alone_digest": km_digest,
        "kmodes_in_call_ms": round(km_in_call, 3),
        "kmodes_in_call_minus_alone_ms": round(km_in_call - km_med, 3), "runs_spread_ms": round(spread, 3),
        "kmodes_within_spread": bool(abs(km_in_call - km_med) <= spread),
        "host_arrays_wall_s": {"runs": [round(x, 4) for x in arr_s], "median": round(float(np.median(arr_s)), 4)},
        "host_path_s": {"plan_global_tiling": round(t_plan, 3), "kmodes_bins": round(t_bins, 3),
                        "apply_kmodes_merges": round(t_apply, 3), "total": round(host_s, 3)},
        "host_path_over_dev": round(host_s * 1e3 / med, 2),
        "merged_tiles": int((dev_out[3] >= 0).sum()), "active_after": int(dev_out[1].sum()),
        "digest": dg, "digests_equal": len(set(dg.values())) == 1,
    }
    return out


def main():
    args = parser().parse_args()
    res = run(args)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
