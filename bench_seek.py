"""GTM random-access timings on bench_play.py's clip: 1080p (240 x 135 tiles), 3 keyframes x 24 frames, written by
the project's own writer.  Each line stands beside the only way the sequential player has to show the same frames,
measured in the same run, alternating:

  index_build      the first tiler_gtm_frames_dev call of a fresh handle whose tileset is already uploaded (it builds
                   the checkpoint index: one walk over the items before the last checkpoint, then draws frame 0), and
                   the same call again (no build), to subtract;
  seek_play        seek(f) + play(1) for f = 30 and f = 54 -- both 6 frames into a keyframe, so both walk 6 frames
                   from a checkpoint -- beside rewind + play(f + 1);
  frames_8         frames() of 8 spread frames beside rewind + play of all 72;
  stream_frames    Encoder._stream_frames -- the playback inside verify_stream and quality(stream=...), host arrays in
                   and out, wall clock -- for an encoder that holds 9 of the 72 frames (every eighth), beside the
                   loop it replaced (play every frame in chunks, keep the held rows).  The render and the compare
                   that verify_stream adds are the same before and after and are not timed.

Device lines are HIP-event times around the calls on the null stream (ms); medians and all values of --reps runs
after --warmup runs.  Every frame compared is checked equal between the two ways first.  Prints one JSON line.

`python bench_seek.py [--reps 5] [--warmup 2]`
"""
from __future__ import annotations

import argparse
import json
import sys
import time

import numpy as np

from bench_play import KF_FRAMES, TM_H, TM_W, make_clip, stats

KEYFRAMES = 3
SEEKS = (30, 54)
SPREAD = (4, 13, 22, 31, 40, 49, 58, 67)


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
    from tiler_amd.encoder import Encoder
    lib = tiler_amd.load()
    check(lib.tiler_init(0), "tiler_init")
    Q, F = TM_W * TM_H, KEYFRAMES * KF_FRAMES
    c = make_clip(KEYFRAMES)
    data = gtm.save_stream(c["palpix"], c["thm"], c["tvm"], c["kf_start"], c["pals"], c["tile"], c["pal"], c["hm"],
                           c["vm"], c["sm"], TM_W * 8, TM_H * 8, 24.0)
    out = torch.empty((F, Q, 64), dtype=torch.int32, device="cuda")
    one = torch.empty((len(SPREAD), Q, 64), dtype=torch.int32, device="cuda")

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    runs = a.warmup + a.reps
    res = {"index_build": [], "indexed_same_call": [], "frames_8": [], "play_72": [],
           "seek": {f: [] for f in SEEKS}, "rewind_play": {f: [] for f in SEEKS}}

    # the index build: a fresh handle per run
    for i in range(runs):
        with gtm.Stream(data) as st:
            st.play_dev(1, out.data_ptr())  # the tileset and the palettes are uploaded by the first call of any kind
            torch.cuda.synchronize()
            build = timed(lambda: st.frames_dev([0], one.data_ptr()))
            again = timed(lambda: st.frames_dev([0], one.data_ptr()))
            if i >= a.warmup:
                res["index_build"].append(build)
                res["indexed_same_call"].append(again)

    st = gtm.Stream(data)
    equal = True
    for i in range(runs):
        for f in SEEKS:
            def seek_play():
                st.seek(f)
                st.play_dev(1, one.data_ptr())

            def rewind_play():
                st.rewind()
                st.play_dev(f + 1, out.data_ptr())
            ts, tr = timed(seek_play), timed(rewind_play)
            equal &= bool(torch.equal(one[0], out[f]))
            if i >= a.warmup:
                res["seek"][f].append(ts)
                res["rewind_play"][f].append(tr)

        def play_all():
            st.rewind()
            st.play_dev(F, out.data_ptr())
        t8, t72 = timed(lambda: st.frames_dev(SPREAD, one.data_ptr())), timed(play_all)
        equal &= bool(torch.equal(one, out[list(SPREAD)]))
        if i >= a.warmup:
            res["frames_8"].append(t8)
            res["play_72"].append(t72)
    st.close()
    del out, one
    torch.cuda.empty_cache()

    # the encoder's playback of a stream: 9 of the 72 frames held.  Only what _stream_frames reads is set up.
    e = Encoder.__new__(Encoder)
    e.n_frames, e.frame_idx = F, np.arange(0, F, 8)
    e.tile = np.zeros((e.frame_idx.size, Q), np.int64)

    def played_whole(enc, data):
        """_stream_frames before random access: every frame played and copied, the held rows kept."""
        with gtm.Stream(data) as s:
            rgb = np.zeros((enc.frames, Q, 64), np.int32)
            undrawn = np.zeros(enc.frames, np.int32)
            chunk = max(1, (1 << 27) // (Q * 256))
            for f0 in range(0, s.frames, chunk):
                got, und = s.play(chunk, "tiles", chunk)
                rows = np.nonzero((enc.frame_idx >= f0) & (enc.frame_idx < f0 + got.shape[0]))[0]
                rgb[rows] = (got[enc.frame_idx[rows] - f0] & 0x00FFFFFF).astype(np.int32)
                undrawn[rows] = und[enc.frame_idx[rows] - f0]
        return rgb, undrawn

    enc = {"frames": [], "play_all": []}
    for i in range(runs):
        t0 = time.perf_counter()
        new = e._stream_frames(data)
        t1 = time.perf_counter()
        old = played_whole(e, data)
        t2 = time.perf_counter()
        equal &= np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1])
        if i >= a.warmup:
            enc["frames"].append((t1 - t0) * 1e3)
            enc["play_all"].append((t2 - t1) * 1e3)

    report = {"bench": "seek", "shape": f"{TM_W * 8}x{TM_H * 8}", "device": torch.cuda.get_device_name(0),
              "frames": F, "keyframes": KEYFRAMES, "file_bytes": len(data), "equal": bool(equal),
              "ms": {"index_build": {"first_frames_call": stats(res["index_build"]),
                                     "same_call_indexed": stats(res["indexed_same_call"])},
                     "seek_play": {str(f): {"seek_play_1": stats(res["seek"][f]),
                                            "rewind_play_to_it": stats(res["rewind_play"][f])} for f in SEEKS},
                     "frames_8": {"frames": stats(res["frames_8"]), "play_72": stats(res["play_72"])},
                     "stream_frames_9_of_72": {"includes": "open (LZMA, token walk) and host copies; wall clock",
                                               "frames": stats(enc["frames"], 1),
                                               "play_all": stats(enc["play_all"], 1)}}}
    print(json.dumps(report))
    if not equal:
        sys.exit(1)


if __name__ == "__main__":
    main()
