"""The LZMA match search on the GPU (tiler_gtm_set_gpu_matches) on bench_save.py's three 1080p clips (240 x 135
tiles, 3 keyframes of 24 frames, T = 70,000, smoothed fractions 0, about 0.5 and about 0.9).

Per clip, medians (and all values) of --reps runs after --warmup runs:
  table_kernel_ms  tiler_lzma_match_table_dev over the three raw streams in HBM, by the library's HIP-event timers
                   lzma_match_hash + lzma_match_sort + lzma_match_find (also each on its own);
  table_copy_ms    the three tables (4 bytes per raw byte) from HBM to host memory, wall time with the wait;
  lzma_ms / lzma_table_ms   per stream, one thread: tiler_lzma_encode, and tiler_lzma_encode_table with the table;
  host_table_ms    per stream, one thread: tiler_lzma_match_table (the search alone, on the host), once;
  write_off_ms / write_on_ms   the whole tiler_gtm_write from host arrays with the switch off and on, alternating;
  gain             whether write_on's slowest run beats write_off's fastest (a gain beyond the run-to-run spread);
  files_equal      the two files are the same bytes, and the GPU tables equal the host tables.
Prints one JSON line; exit status 1 if any file or table differs.

`python bench_lzma_match.py [--reps 5] [--warmup 2]`
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
import time

import numpy as np

from bench_save import FRACTIONS, KEYFRAMES, KF_FRAMES, P, T, TM_H, TM_W, make_clip, stats

FAMILIES = ("lzma_match_hash", "lzma_match_sort", "lzma_match_find")


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
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    report = {"bench": "lzma_match", "shape": f"{W}x{H}", "device": torch.cuda.get_device_name(0), "frames": F,
              "keyframes": KEYFRAMES, "tiles": T, "cases": []}
    ok = True
    for fraction in FRACTIONS:
        c = make_clip(fraction)
        host = [c["palpix"], c["thm"], c["tvm"], c["kf_start"], c["pals"], c["tile"], c["pal"], c["hm"], c["vm"], c["sm"]]
        dev = {k: torch.from_numpy(c[k]).cuda() for k in ("palpix", "thm", "tvm", "pals", "tile", "pal", "hm", "vm", "sm")}
        src, keep = gtm.gtm_source(dev["palpix"].data_ptr(), dev["thm"].data_ptr(), dev["tvm"].data_ptr(), c["kf_start"],
                                   dev["pals"].data_ptr(), dev["tile"].data_ptr(), dev["pal"].data_ptr(),
                                   dev["hm"].data_ptr(), dev["vm"].data_ptr(), dev["sm"].data_ptr(), width=W, height=H,
                                   fps=fps, tiles=T, n_palettes=P, frames=F, positions=Q)
        off = np.zeros(KEYFRAMES + 1, np.int64)
        check(lib.tiler_gtm_commands_dev(ctypes.byref(src), None, 0, vp(off), None), "tiler_gtm_commands_dev")
        d_raw = torch.empty(int(off[-1]), dtype=torch.uint8, device="cuda")
        d_tab = torch.empty(int(off[-1]), dtype=torch.int32, device="cuda")
        check(lib.tiler_gtm_commands_dev(ctypes.byref(src), ctypes.c_void_p(d_raw.data_ptr()), d_raw.numel(), vp(off),
                                         None), "tiler_gtm_commands_dev")
        torch.cuda.synchronize()
        raw = d_raw.cpu().numpy()
        raws = [raw[off[k]:off[k + 1]].tobytes() for k in range(KEYFRAMES)]
        kern = {f: [] for f in FAMILIES}
        kernel, copy, lz, lzt, w_off, w_on = [], [], [], [], [], []
        tables = None
        for i in range(a.warmup + a.reps):
            lib.tiler_timing_enable(1)
            lib.tiler_timing_reset()
            left = check(lib.tiler_lzma_match_table_dev(ctypes.c_void_p(d_raw.data_ptr()), vp(off), KEYFRAMES,
                                                        gtm.LZMA_DICT, ctypes.c_void_p(d_tab.data_ptr()), None),
                         "tiler_lzma_match_table_dev")
            torch.cuda.synchronize()
            if left:
                raise RuntimeError(f"bench_lzma_match: {left} streams were left to the host")
            ms = {}
            for fam in FAMILIES:
                n = ctypes.c_int(0)
                ms[fam] = lib.tiler_timing_get(fam.encode(), ctypes.byref(n))
                if ms[fam] < 0 or n.value != 1:
                    raise RuntimeError(f"bench_lzma_match: {fam} was timed {n.value} times")
            lib.tiler_timing_enable(0)
            t0 = time.perf_counter()
            tab = d_tab.cpu().numpy().view(np.uint32)
            t_copy = (time.perf_counter() - t0) * 1e3
            if tables is None:
                tables = [np.ascontiguousarray(tab[off[k]:off[k + 1]]) for k in range(KEYFRAMES)]
            t_lz, t_lzt = [], []
            for r, t in zip(raws, tables):
                t0 = time.perf_counter()
                plain = gtm.lzma_encode(r)
                t_lz.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                with_table = gtm.lzma_encode(r, matches=t)
                t_lzt.append((time.perf_counter() - t0) * 1e3)
                ok = ok and plain == with_table
            t0 = time.perf_counter()
            f_off = gtm.save_stream_gpu(*host, W, H, fps)
            t_off = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            f_on = gtm.save_stream_gpu(*host, W, H, fps, gpu_matches=True)
            t_on = (time.perf_counter() - t0) * 1e3
            ok = ok and f_off == f_on
            if i >= a.warmup:
                for fam in FAMILIES:
                    kern[fam].append(ms[fam])
                kernel.append(sum(ms.values())), copy.append(t_copy), lz.append(t_lz), lzt.append(t_lzt)
                w_off.append(t_off), w_on.append(t_on)
        lib.tiler_timing_reset()
        t_host, tables_equal = [], True
        for r, t in zip(raws, tables):
            t0 = time.perf_counter()
            ht = gtm.match_table(r)
            t_host.append(round((time.perf_counter() - t0) * 1e3, 1))
            tables_equal = tables_equal and np.array_equal(ht, t)
        ok = ok and tables_equal
        per = lambda xs: [stats([x[k] for x in xs], 1) for k in range(KEYFRAMES)]  # noqa: E731
        report["cases"].append({
            "smoothed_fraction": round(float(c["sm"].mean()), 3), "raw_bytes": [len(r) for r in raws],
            "file_bytes": len(f_on), "table_kernel_ms": stats(kernel), **{f + "_ms": stats(kern[f]) for f in FAMILIES},
            "table_copy_ms": stats(copy, 1), "lzma_ms": per(lz), "lzma_table_ms": per(lzt), "host_table_ms": t_host,
            "write_off_ms": stats(w_off, 1), "write_on_ms": stats(w_on, 1),
            "write_ratio": round(statistics.median(w_on) / statistics.median(w_off), 3),
            "gain": max(w_on) < min(w_off), "tables_equal": tables_equal, "files_equal": f_off == f_on})
    report["all_equal"] = ok
    print(json.dumps(report))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
