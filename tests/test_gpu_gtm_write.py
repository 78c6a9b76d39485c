"""The native .gtm writer on the GPU (tiler_gtm_commands / _streams / _write over gtm_write.hip and gtm_write.cpp)
against the Python writer on the same arrays, byte for byte: gtm.keyframe_raw for the command words, gtm.save_stream
for the file (tests/test_gtm.py pins those to the reference's demo streams)."""
import ctypes
import struct

import numpy as np
import pytest

from tiler_amd import gtm
from tiler_amd._lib import TilerError

pytestmark = pytest.mark.gpu


def _clip(seed, W, H, T, P, kf_start, sm=None, p_run=0.5):
    """A seeded clip (W, H in tiles).  sm: the [F][Q] flags, or None for seeded runs of random lengths."""
    rng = np.random.default_rng(seed)
    Q, F, KF = W * H, int(kf_start[-1]), len(kf_start) - 1
    if sm is None:
        sm = np.zeros((F, Q), np.uint8)
        for f in range(F):
            q = 0
            while q < Q:
                n = int(rng.choice([1, 2, 3, 7, 64, 100, 1030]))
                if rng.random() < p_run:
                    sm[f, q:q + n] = rng.choice([1, 2, 255])
                q += n
    return dict(W=W * 8, H=H * 8, T=T, P=P, Q=Q, F=F, KF=KF, kf_start=np.asarray(kf_start, np.int64),
                palpix=rng.integers(0, 16, (T, 64)).astype(np.uint8), thm=rng.integers(0, 2, T).astype(np.uint8),
                tvm=rng.integers(0, 2, T).astype(np.uint8), pals=rng.integers(0, 1 << 24, (KF, P, 16)).astype(np.int32),
                tile=rng.integers(0, T, (F, Q)).astype(np.int32), pal=rng.integers(0, min(P, 256), (F, Q)).astype(np.int32),
                hm=rng.integers(0, 2, (F, Q)).astype(np.uint8), vm=rng.integers(0, 2, (F, Q)).astype(np.uint8),
                sm=np.asarray(sm, np.uint8), fps=24.0)


def _py_raws(c, first=True):
    out = []
    for k in range(c["KF"]):
        r = slice(int(c["kf_start"][k]), int(c["kf_start"][k + 1]))
        out.append(gtm.keyframe_raw(k if first else k + 1, c["palpix"], c["thm"], c["tvm"], c["pals"][k], c["tile"][r],
                                    c["pal"][r], c["hm"][r], c["vm"][r], c["sm"][r], width=c["W"], height=c["H"],
                                    fps=c["fps"]))
    return out


def _py_file(c):
    return gtm.save_stream(c["palpix"], c["thm"], c["tvm"], c["kf_start"], c["pals"], c["tile"], c["pal"], c["hm"],
                           c["vm"], c["sm"], c["W"], c["H"], c["fps"])


def _source(c, first=True):
    return gtm.gtm_source(c["palpix"], c["thm"], c["tvm"], c["kf_start"], c["pals"], c["tile"], c["pal"], c["hm"],
                          c["vm"], c["sm"], width=c["W"], height=c["H"], fps=c["fps"], first_keyframe=first)


def _dev_source(c, first=True):
    """The same source over HBM copies (torch tensors, returned to be kept alive)."""
    import torch
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda()
         for k in ("palpix", "thm", "tvm", "pals", "tile", "pal", "hm", "vm", "sm")}
    torch.cuda.synchronize()
    src, keep = gtm.gtm_source(t["palpix"].data_ptr(), t["thm"].data_ptr(), t["tvm"].data_ptr(), c["kf_start"],
                               t["pals"].data_ptr(), t["tile"].data_ptr(), t["pal"].data_ptr(), t["hm"].data_ptr(),
                               t["vm"].data_ptr(), t["sm"].data_ptr(), width=c["W"], height=c["H"], fps=c["fps"],
                               first_keyframe=first, tiles=c["T"], n_palettes=c["P"], frames=c["F"],
                               positions=c["Q"])
    return src, (keep, t)


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _commands_host(gpu, c, first=True):
    """tiler_gtm_commands -> (the streams, raw_off)."""
    lib = gpu.load()
    src, keep = _source(c, first)
    off = np.zeros(c["KF"] + 1, np.int64)
    assert lib.tiler_gtm_commands(ctypes.byref(src), None, 0, _vp(off)) == 0, gpu.last_error()
    raw = np.zeros(int(off[-1]), np.uint8)
    off2 = np.zeros_like(off)
    assert lib.tiler_gtm_commands(ctypes.byref(src), _vp(raw), raw.size, _vp(off2)) == 0, gpu.last_error()
    assert np.array_equal(off, off2) and off[0] == 0
    return [raw[off[k]:off[k + 1]].tobytes() for k in range(c["KF"])], off


def _commands_dev(gpu, c, first=True):
    import torch
    lib = gpu.load()
    src, keep = _dev_source(c, first)
    off = np.zeros(c["KF"] + 1, np.int64)
    assert lib.tiler_gtm_commands_dev(ctypes.byref(src), None, 0, _vp(off), None) == 0, gpu.last_error()
    d_raw = torch.zeros(int(off[-1]), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.tiler_gtm_commands_dev(ctypes.byref(src), ctypes.c_void_p(d_raw.data_ptr()), d_raw.numel(), _vp(off),
                                      None) == 0, gpu.last_error()
    torch.cuda.synchronize()
    raw = d_raw.cpu().numpy()
    return [raw[off[k]:off[k + 1]].tobytes() for k in range(c["KF"])], off


def _write(gpu, c, dev=False, threads=0):
    lib = gpu.load()
    src, keep = _dev_source(c) if dev else _source(c)
    n = ctypes.c_size_t(0)
    call = (lambda d, cap: lib.tiler_gtm_write_dev(ctypes.byref(src), threads, d, cap, ctypes.byref(n), None)) if dev \
        else (lambda d, cap: lib.tiler_gtm_write(ctypes.byref(src), threads, d, cap, ctypes.byref(n)))
    assert call(None, 0) == 0, gpu.last_error()
    out = np.zeros(n.value, np.uint8)
    assert call(_vp(out), out.size) == 0, gpu.last_error()
    assert n.value == out.size
    return out.tobytes()


def _frame_words(raw: bytes, Q: int):
    """The token walk of one keyframe stream (palsize 16): per frame the list of (cmd, arg), and the first command."""
    at, frames, cur, first = 0, [], [], None
    while at < len(raw):
        w, = struct.unpack_from("<H", raw, at)
        cmd, arg = w & 63, w >> 6
        first = cmd if first is None else first
        if cmd == gtm.GT_SET_DIMENSIONS:
            at += 2 + 12
        elif cmd == gtm.GT_TILE_SET:
            t0, t1 = struct.unpack_from("<II", raw, at + 2)
            at += 2 + 8 + 64 * (t1 - t0 + 1)
        elif cmd == gtm.GT_LOAD_PALETTE:
            at += 2 + 2 + 64
        else:
            cur.append((cmd, arg))
            at += {gtm.GT_SKIP_BLOCK: 2, gtm.GT_SHORT_TILE_IDX: 4, gtm.GT_LONG_TILE_IDX: 6, gtm.GT_FRAME_END: 2}[cmd]
            if cmd == gtm.GT_FRAME_END:
                frames.append(cur)
                cur = []
    assert not cur
    return frames, first


def _runs(Q, spans):
    sm = np.zeros(Q, np.uint8)
    for a, n in spans:
        assert a + n <= Q and not sm[a:a + n].any() and (a == 0 or not sm[a - 1])
        sm[a:a + n] = 1
    return sm


Q_RUNS = 4100  # 50 x 82
RUN_CLIPS = {
    # none | runs of 1, 1023, 1024, 1025 and one that reaches Q - 1 | begins smoothed: 2048, then 2049 | all
    "a": [[], [(3, 1), (5, 1023), (1029, 1024), (2054, 1025), (4000, 100)], [(0, 2048), (2049, 2049)], [(0, Q_RUNS)]],
    # 3073, 1, ends smoothed | begins smoothed with exactly 1024 | all | none
    "b": [[(10, 3073), (3084, 1), (4090, 10)], [(0, 1024)], [(0, Q_RUNS)], []],
}


@pytest.mark.parametrize("name", sorted(RUN_CLIPS))
@pytest.mark.parametrize("kf_start", [[0, 4], [0, 2, 4]])
def test_run_boundaries(gpu, name, kf_start):
    """F = 4, Q = 4100: runs of exactly 1, 1023, 1024, 1025, 2048, 2049 and 3073, a run that reaches Q - 1, a frame
    that ends smoothed before one that begins smoothed, an all-smoothed frame and one with none: the run restarts at
    every frame, within a keyframe and across two."""
    sm = np.stack([_runs(Q_RUNS, spans) for spans in RUN_CLIPS[name]])
    c = _clip(11, 50, 82, 300, 5, kf_start, sm)
    want = _py_raws(c)
    got, off = _commands_host(gpu, c)
    assert got == want and list(np.diff(off)) == [len(r) for r in want]
    skips = [[arg + 1 for cmd, arg in fr if cmd == gtm.GT_SKIP_BLOCK]
             for raw in got for fr in _frame_words(raw, Q_RUNS)[0]]
    expect = {"a": [[], [1, 1023, 1024, 1024, 1, 100], [1024, 1024, 1024, 1024, 1], [1024] * 4 + [4]],
              "b": [[1024, 1024, 1024, 1, 1, 10], [1024], [1024] * 4 + [4], []]}[name]
    assert skips == expect


@pytest.mark.parametrize("W, H", [(1, 1), (9, 7), (8, 8), (13, 5), (41, 25)])
def test_scan_seams(gpu, W, H):
    """Q in {1, 63, 64, 65, 1025}: the 64-lane seams and the 16 wave segments of a workgroup (Q = 1025: 9 segments of
    128, the last one position long), runs crossing them."""
    c = _clip(20 + W, W, H, 70000, 7, [0, 2, 3])
    if c["Q"] > 64:
        c["sm"][1, 60:70] = 1          # across the first 64-lane seam
        c["sm"][2, :] = 1
        c["sm"][2, 64] = 0             # a run ends at a seam, the next begins right after it
    if c["Q"] == 1025:
        c["sm"][0, 100:1025] = 1       # across every later segment, to the last position
        c["sm"][1, 127:129] = 1        # across a segment seam
    want = _py_raws(c)
    assert _commands_host(gpu, c)[0] == want and _commands_dev(gpu, c)[0] == want


def test_largest_tilemap(gpu):
    """Q = 32,400 (240 x 135), F = 3, the middle frame all smoothed: 31 SkipBlock words of 1024 and one of 656."""
    c = _clip(31, 240, 135, 300, 4, [0, 3], p_run=0.4)
    c["sm"][1, :] = 255
    want = _py_raws(c)
    got, off = _commands_dev(gpu, c)
    assert got == want and off[-1] == len(want[0])
    frames, _ = _frame_words(got[0], c["Q"])
    assert frames[1] == [(gtm.GT_SKIP_BLOCK, 1023)] * 31 + [(gtm.GT_SKIP_BLOCK, 655), (gtm.GT_FRAME_END, 0)]
    assert frames[2][-1] == (gtm.GT_FRAME_END, 1)


def test_index_and_attribute_edges(gpu):
    """Tiles 65,535 and 65,536 side by side (T = 70,000), pal 0 and 255, every (hm, vm) x (thm, tvm) combination,
    `smoothed` values 0, 1, 2 and 255."""
    c = _clip(41, 16, 4, 70000, 256, [0, 2])
    c["thm"][[65535, 65536, 7, 8]] = [0, 1, 0, 1]
    c["tvm"][[65535, 65536, 7, 8]] = [0, 0, 1, 1]
    q = 0
    for t in (65535, 65536, 7, 8):
        for h in (0, 1):
            for v in (0, 1):
                c["tile"][0, q], c["hm"][0, q], c["vm"][0, q], c["pal"][0, q] = t, h, v, (0, 255)[q & 1]
                q += 1
    c["tile"][1, :6] = [65535, 65536, 65535, 65536, 69999, 0]
    c["pal"][1, :6] = [255, 255, 0, 0, 255, 0]
    c["sm"][:] = 0
    c["sm"][1, 8:16] = [1, 0, 2, 0, 255, 0, 1, 2]
    c["sm"][0, 32:40] = [0, 1, 2, 255, 0, 0, 255, 1]
    want = _py_raws(c)
    assert _commands_host(gpu, c)[0] == want
    frames, _ = _frame_words(want[0], c["Q"])
    assert [cmd for cmd, _ in frames[1][:4]] == [gtm.GT_SHORT_TILE_IDX, gtm.GT_LONG_TILE_IDX] * 2
    assert {arg >> 2 for cmd, arg in frames[0][:16]} == {0, 255}


@pytest.mark.parametrize("first", [True, False])
def test_keyframes(gpu, first):
    """KF = 3 of 1, 2 and 5 frames: WriteTiles in stream 0 only, and only when it is the file's first keyframe;
    FrameEnd's data is 1 exactly on each keyframe's last frame; raw_off is the Python streams' lengths."""
    c = _clip(51, 9, 7, 500, 6, [0, 1, 3, 8])
    want = _py_raws(c, first)
    for got, off in (_commands_host(gpu, c, first), _commands_dev(gpu, c, first)):
        assert got == want
        assert list(off) == list(np.cumsum([0] + [len(r) for r in want]))
        for k, raw in enumerate(got):
            frames, cmd0 = _frame_words(raw, c["Q"])
            assert cmd0 == (gtm.GT_SET_DIMENSIONS if first and k == 0 else gtm.GT_LOAD_PALETTE)
            assert [fr[-1] for fr in frames] == [(gtm.GT_FRAME_END, 0)] * (len(frames) - 1) + [(gtm.GT_FRAME_END, 1)]
            assert len(frames) == (1, 2, 5)[k]
    # the Python wrapper, a keyframe at a time
    for k in range(3):
        r = slice(int(c["kf_start"][k]), int(c["kf_start"][k + 1]))
        assert gtm.keyframe_raw_gpu(k if first else k + 1, c["palpix"], c["thm"], c["tvm"], c["pals"][k],
                                    c["tile"][r], c["pal"][r], c["hm"][r], c["vm"][r], c["sm"][r], width=c["W"],
                                    height=c["H"], fps=c["fps"]) == want[k]


@pytest.mark.parametrize("W, H, T, P, kf_start, fps", [
    (7, 5, 50, 3, [0, 9], 24.0),
    (40, 30, 70000, 6, [0, 3, 4, 8], 29.97),
    (13, 5, 300, 256, [0, 1, 2, 3, 4, 5], 30.0),
])
def test_whole_file(gpu, W, H, T, P, kf_start, fps):
    """tiler_gtm_write is gtm.save_stream's file (the same LZMA encoder and parameters: the compressed bytes too), in
    the host-array and the _dev form and on one thread; read back, it holds the tilemaps with -1 where smoothed."""
    c = _clip(61 + W, W, H, T, P, kf_start)
    c["fps"] = fps
    c["sm"][c["kf_start"][:-1]] = 0  # a player has drawn every position by the end of a keyframe's first frame
    want = _py_file(c)
    assert _write(gpu, c) == want
    assert _write(gpu, c, dev=True) == want
    assert _write(gpu, c, threads=1) == want
    assert gtm.save_stream_gpu(c["palpix"], c["thm"], c["tvm"], c["kf_start"], c["pals"], c["tile"], c["pal"],
                               c["hm"], c["vm"], c["sm"], c["W"], c["H"], fps) == want
    with gtm.Stream(want) as st:
        tile, attrs, _ = st.items()
    live = c["sm"] == 0
    assert np.array_equal(tile, np.where(live, c["tile"], -1))
    t = c["tile"][live]
    assert np.array_equal(attrs[live], c["pal"][live] << 2 | (c["vm"][live] ^ c["tvm"][t]) << 1 |
                          (c["hm"][live] ^ c["thm"][t]))


def test_streams_of_a_keyframe_subset(gpu):
    """tiler_gtm_streams over keyframes 1 and 2 alone (first_keyframe off) and over keyframe 0 alone, in both forms:
    the compressed streams of the whole clip, so tiler_gtm_assemble over them is the file."""
    c = _clip(71, 9, 7, 400, 5, [0, 2, 5, 6])
    lib = gpu.load()
    want = [gtm.lzma_encode(r) for r in _py_raws(c)]

    def part(k0, k1, dev):
        f0, f1 = int(c["kf_start"][k0]), int(c["kf_start"][k1])
        sub = dict(c, kf_start=c["kf_start"][k0:k1 + 1] - f0, pals=c["pals"][k0:k1], KF=k1 - k0, F=f1 - f0,
                   **{a: c[a][f0:f1] for a in ("tile", "pal", "hm", "vm", "sm")})
        src, keep = (_dev_source if dev else _source)(sub, k0 == 0)
        lens, n = np.zeros(k1 - k0, np.uint64), ctypes.c_size_t(0)
        call = (lambda d, cap: lib.tiler_gtm_streams_dev(ctypes.byref(src), 0, d, cap, _vp(lens), ctypes.byref(n),
                                                         None)) if dev else \
            (lambda d, cap: lib.tiler_gtm_streams(ctypes.byref(src), 0, d, cap, _vp(lens), ctypes.byref(n)))
        assert call(None, 0) == 0, gpu.last_error()
        out = np.zeros(n.value, np.uint8)
        assert call(_vp(out), out.size) == 0 and int(lens.sum()) == n.value
        ends = np.cumsum(lens).astype(int)
        return [out[e - int(m):e].tobytes() for e, m in zip(ends, lens)]

    for dev in (False, True):
        got = part(0, 1, dev) + part(1, 3, dev)
        assert got == want
    assert gtm.assemble_stream_native(got, c["kf_start"], c["W"], c["H"], c["fps"]) == _py_file(c)


def test_encoder_chain_gpu_writer(gpu):
    """The small chain of test_gpu_gtm_play: Encoder.save_stream(gpu=True) is save_stream()'s file, and verify_stream
    over it reports no differing frame."""
    from tiler_amd import synth
    from tiler_amd.encoder import Encoder
    from tiler_amd.frame_tiling import FT_MEDIUM
    W, H = 320, 240
    e = Encoder(synth.video(51 + FT_MEDIUM, W, H, kf_frames=(3, 3), n_palettes=8))
    e.run_all(700, FT_MEDIUM, 0.2)
    data = e.save_stream(W, H, 24.0, gpu=True)
    assert e.sm["smoothed"].any() and data == e.save_stream(W, H, 24.0)
    res = e.verify_stream(data, width=W, height=H)
    assert (res["frames"], res["differing_frames"], res["undrawn"]) == (6, 0, 0)


def _error_clip():
    c = _clip(81, 9, 7, 200, 3, [0, 2, 4], p_run=0.3)
    c["sm"][:, 10:20] = 0
    return c


@pytest.mark.parametrize("field, value, P, word", [
    ("tile", -1, 3, "tile index -1"),
    ("tile", 200, 3, "tile index 200"),
    ("pal", 256, 300, "palette index 256"),
    ("pal", 3, 3, "palette index 3"),
])
def test_errors(gpu, field, value, P, word):
    """A tile outside [0, T) or a pal outside [0, min(n_palettes, 256)) at a non-smoothed position: -1, the message
    names the rule and (frame, position), nothing is written to the output -- in every entry point."""
    import torch
    lib = gpu.load()
    c = _error_clip()
    if P != 3:
        c = dict(c, P=P, pals=np.zeros((2, P, 16), np.int32))
    c[field][2, 13] = value
    where = "(frame 2, position 13)"
    src, keep = _source(c)
    off = np.full(3, -7, np.int64)
    raw = np.full(1 << 16, 0xAB, np.uint8)
    assert lib.tiler_gtm_commands(ctypes.byref(src), _vp(raw), raw.size, _vp(off)) == -1
    msg = gpu.last_error()
    assert word in msg and where in msg and (raw == 0xAB).all()
    n = ctypes.c_size_t(0)
    out = np.full(1 << 16, 0xAB, np.uint8)
    assert lib.tiler_gtm_write(ctypes.byref(src), 0, _vp(out), out.size, ctypes.byref(n)) == -1
    assert word in gpu.last_error() and where in gpu.last_error() and (out == 0xAB).all()
    dsrc, dkeep = _dev_source(c)
    d_raw = torch.full((1 << 16,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.tiler_gtm_commands_dev(ctypes.byref(dsrc), ctypes.c_void_p(d_raw.data_ptr()), d_raw.numel(), _vp(off),
                                      None) == -1
    assert word in gpu.last_error() and where in gpu.last_error()
    torch.cuda.synchronize()
    assert bool((d_raw == 0xAB).all())
    assert lib.tiler_gtm_write_dev(ctypes.byref(dsrc), 0, _vp(out), out.size, ctypes.byref(n), None) == -1
    assert where in gpu.last_error() and (out == 0xAB).all()
    with pytest.raises(TilerError, match="position 13"):
        gtm.save_stream_gpu(c["palpix"], c["thm"], c["tvm"], c["kf_start"], c["pals"], c["tile"], c["pal"], c["hm"],
                            c["vm"], c["sm"], c["W"], c["H"], 24.0)


def test_the_earlier_of_two_bad_items_is_reported(gpu):
    c = _error_clip()
    c["pal"][3, 11] = 99      # later frame, earlier position
    c["tile"][1, 17] = 5000   # the first in (frame, position) order
    c["tile"][1, 18] = -3
    src, keep = _source(c)
    off = np.zeros(3, np.int64)
    assert gpu.load().tiler_gtm_commands(ctypes.byref(src), None, 0, _vp(off)) == -1
    msg = gpu.last_error()
    assert "tile index 5000" in msg and "(frame 1, position 17)" in msg
    c["tile"][1, 17:19] = 0
    src, keep = _source(c)
    assert gpu.load().tiler_gtm_commands(ctypes.byref(src), None, 0, _vp(off)) == -1
    assert "palette index 99" in gpu.last_error() and "(frame 3, position 11)" in gpu.last_error()


def test_smoothed_position_holding_garbage(gpu):
    """A smoothed position's item is never read: tile and pal far out of range there are no error, same bytes."""
    c = _error_clip()
    c["sm"][1, 30:40] = 1
    c["sm"][3, 62] = 2
    c["tile"][1, 30:40] = [200, 1 << 30, 70000, 65536, 201, 999, 2 ** 31 - 1, 200, 200, 200]
    c["pal"][1, 30:40] = 999
    c["tile"][3, 62], c["pal"][3, 62] = 12345678, 256
    want = _py_raws(c)
    assert _commands_host(gpu, c)[0] == want and _commands_dev(gpu, c)[0] == want
    assert _write(gpu, c) == _py_file(c)


def test_size_query(gpu):
    """dst == NULL returns the exact size; a buffer one byte short fails, names the size needed and stays untouched."""
    import torch
    lib = gpu.load()
    c = _clip(91, 9, 7, 100, 4, [0, 2, 3])
    raws, want = _py_raws(c), _py_file(c)
    src, keep = _source(c)
    n, off = ctypes.c_size_t(0), np.zeros(3, np.int64)
    assert lib.tiler_gtm_write(ctypes.byref(src), 0, None, 0, ctypes.byref(n)) == 0 and n.value == len(want)
    out = np.full(len(want), 0xAB, np.uint8)
    n.value = 0
    assert lib.tiler_gtm_write(ctypes.byref(src), 0, _vp(out), len(want) - 1, ctypes.byref(n)) == -1
    assert n.value == len(want) and str(len(want)) in gpu.last_error() and (out == 0xAB).all()
    assert lib.tiler_gtm_write(ctypes.byref(src), 0, _vp(out), len(want), ctypes.byref(n)) == 0
    assert out.tobytes() == want
    total = sum(len(r) for r in raws)
    raw = np.full(total, 0xAB, np.uint8)
    assert lib.tiler_gtm_commands(ctypes.byref(src), None, 0, _vp(off)) == 0 and off[-1] == total
    off[:] = 0
    assert lib.tiler_gtm_commands(ctypes.byref(src), _vp(raw), total - 1, _vp(off)) == -1
    assert off[-1] == total and str(total) in gpu.last_error() and (raw == 0xAB).all()
    dsrc, dkeep = _dev_source(c)
    d_raw = torch.full((total,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    off[:] = 0
    assert lib.tiler_gtm_commands_dev(ctypes.byref(dsrc), ctypes.c_void_p(d_raw.data_ptr()), total - 1, _vp(off),
                                      None) == -1
    torch.cuda.synchronize()
    assert off[-1] == total and bool((d_raw == 0xAB).all())
    lens = np.zeros(2, np.uint64)
    comp = [gtm.lzma_encode(r) for r in raws]
    assert lib.tiler_gtm_streams(ctypes.byref(src), 0, None, 0, _vp(lens), ctypes.byref(n)) == 0
    assert n.value == sum(map(len, comp)) and list(lens) == [len(x) for x in comp]
    buf = np.full(n.value, 0xAB, np.uint8)
    need = n.value
    assert lib.tiler_gtm_streams(ctypes.byref(src), 0, _vp(buf), need - 1, _vp(lens), ctypes.byref(n)) == -1
    assert n.value == need and (buf == 0xAB).all()
