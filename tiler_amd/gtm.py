"""GTM bitstream writer (SaveStream main.pas:4529-4763) over libANN.so's LZMA-alone encoder, and the playback side:
`lzma_decode`, `Stream` (a .gtm file parsed by libANN.so's reader and played on the GPU, the reference player
decoders/htmljs/gtm.player.js) and `load_stream`.

`save_stream` follows the reference procedure step by step:
  header        TGTMHeader (main.pas:103-114) + one TGTMKeyFrameInfo per keyframe (116-124), rewritten at
                the end with the measured sizes (4753-4757);
  per keyframe  one LZMA-alone stream (LZCompress extern.pas:202-240: `lzma.exe e -lc8 -eos` ->
                tiler_lzma_encode(lc=8, lp=0, pb=2, eos)) of the command words (DoCmd 4565-4571: data << 6 | cmd):
                  first keyframe only: WriteTiles (4603-4622) = SetDimensions + TileSet + 64 B per tile,
                  WriteKFAttributes (4589-4601) = LoadPalette per palette,
                  per frame the SmoothedTileMap: runs of Smoothed items -> SkipBlock (count - 1, at most
                  2^10), others -> Short/LongTileIdx with (PalIdx << 2 | VMirror' << 1 | HMirror'), where the
                  mirrors are xored with the tile's canonical flags (4715), then FrameEnd(is last frame of KF).
`save_stream_gpu` / `keyframe_raw_gpu` / `keyframe_streams_gpu` are the same procedure in libANN.so (tiler_gtm_write,
tiler_gtm_commands, tiler_gtm_streams): the command words built by a kernel, LZMA and the container in native host
code.  The Python writer stays as the restatement they are held to, byte for byte.
The reference takes these bytes verbatim from lzma.exe; this build's encoder makes a different (valid)
parse, so the compressed bytes differ while everything a decoder returns is identical.
"""
from __future__ import annotations

import ctypes
import os
import struct
import weakref
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ._lib import GtmInfo, GtmSource, TilerError, check, last_error, load

GT_SKIP_BLOCK, GT_SHORT_TILE_IDX, GT_LONG_TILE_IDX, GT_LOAD_PALETTE = 0, 1, 2, 3
GT_FRAME_END, GT_TILE_SET, GT_SET_DIMENSIONS = 28, 29, 30
CMD_BITS = 6                      # round(ln(64) / ln(2)), main.pas:4532
ATTR_BITS = 16 - CMD_BITS         # 10
MAX_BLK_SKIP = 1 << ATTR_BITS     # CMaxBlkSkipCount main.pas:4535
LZMA_LC, LZMA_LP, LZMA_PB = 8, 0, 2
LZMA_DICT = 1 << 21             # the reference's lzma.exe streams (docs/demo/*.gtm headers)


def match_table(data: bytes, dict_size: int = LZMA_DICT, gpu: bool = False) -> np.ndarray:
    """The match table of `data` (include/tiler_ann.h): per position len | dist << 9 as uint32, what the encoder's
    match finder answers there.  gpu: computed on the device (tiler_lzma_match_table_gpu), else by the finder itself
    on the host (tiler_lzma_match_table, needs no GPU); the same entries either way.  dict_size <= 2^21."""
    lib = load()
    src = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    table = np.zeros(len(data), np.uint32)
    fn, what = ((lib.tiler_lzma_match_table_gpu, "tiler_lzma_match_table_gpu") if gpu else
                (lib.tiler_lzma_match_table, "tiler_lzma_match_table"))
    check(fn(src.ctypes.data_as(ctypes.c_void_p), len(data), dict_size, table.ctypes.data_as(ctypes.c_void_p)), what)
    return table


def lzma_encode(data: bytes, lc: int = LZMA_LC, lp: int = LZMA_LP, pb: int = LZMA_PB, dict_size: int = LZMA_DICT,
                eos: bool = True, matches=None) -> bytes:
    """LZCompress (extern.pas:202-240) on libANN.so: one LZMA-alone stream.  matches: None -- the encoder searches as
    it parses; "host" / "gpu" -- the search runs ahead of the parse (match_table) and the parse reads it
    (tiler_lzma_encode_table); a table (uint32 [len(data)]) is used as given, every entry checked.  The same bytes."""
    lib = load()
    src = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    if isinstance(matches, str):
        if matches not in ("host", "gpu"):
            raise ValueError("lzma_encode: matches is None, 'host', 'gpu' or a table")
        matches = match_table(data, dict_size, gpu=matches == "gpu")
    if matches is not None:
        matches = np.ascontiguousarray(matches, np.uint32)
        if matches.size != len(data):
            raise ValueError("lzma_encode: the match table has one entry per byte")
    t = matches.ctypes.data_as(ctypes.c_void_p) if matches is not None and matches.size else None
    n = ctypes.c_size_t(0)
    p = src.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros(len(data) + len(data) // 32 + 4096, np.uint8)  # LZMA expands incompressible data < 2 %
    if lib.tiler_lzma_encode_table(p, len(data), lc, lp, pb, dict_size, int(eos), t,
                                   out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(n)) != 0:
        if n.value <= out.size:
            raise TilerError(f"tiler_lzma_encode failed: {last_error()}")
        out = np.zeros(n.value, np.uint8)
        check(lib.tiler_lzma_encode_table(p, len(data), lc, lp, pb, dict_size, int(eos), t,
                                          out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(n)),
              "tiler_lzma_encode")
    return out[:n.value].tobytes()


class _GpuMatches:
    """tiler_gtm_set_gpu_matches for the length of a call (the switch is process-wide), restored afterwards."""

    def __init__(self, on: bool):
        self.on = bool(on)

    def __enter__(self):
        self.prev = load().tiler_gtm_set_gpu_matches(1) if self.on else None

    def __exit__(self, *exc):
        if self.on:
            load().tiler_gtm_set_gpu_matches(self.prev)


def fpc_round(x: float) -> int:
    """FPC Round: banker's rounding (Python's round)."""
    return int(round(x))


class _Z:
    def __init__(self):
        self.b = bytearray()

    def cmd(self, c: int, data: int):
        assert 0 <= data < (1 << ATTR_BITS) and 0 <= c < 64
        self.b += struct.pack("<H", (data << CMD_BITS) | c)

    def word(self, v):
        self.b += struct.pack("<H", v)

    def dword(self, v):
        self.b += struct.pack("<I", v & 0xFFFFFFFF)

    def byte(self, v):
        self.b.append(v & 0xFF)


def _frame_words(tile, pal, hm, vm, smb, thm, tvm, is_last: bool) -> np.ndarray:
    """One frame's command words in position order (main.pas:4675-4725), vectorised: every run of Smoothed
    items becomes SkipBlock words of at most 2^10 items, every other item Short/LongTileIdx + its index."""
    d = np.diff(np.concatenate([[0], smb.astype(np.int8), [0]]))
    starts, ends = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    nch = (ends - starts + MAX_BLK_SKIP - 1) // MAX_BLK_SKIP
    first = np.repeat(np.cumsum(nch) - nch, nch)
    cstart = np.repeat(starts, nch) + MAX_BLK_SKIP * (np.arange(int(nch.sum())) - first)
    clen = np.minimum(MAX_BLK_SKIP, np.repeat(ends, nch) - cstart)
    live = np.nonzero(~smb)[0]
    t = tile[live]
    attrs = (pal[live] << 2) | ((vm[live] ^ tvm[t]) << 1) | (hm[live] ^ thm[t])
    assert (attrs < (1 << ATTR_BITS)).all() and (pal >= 0).all()
    long_ = t >= (1 << 16)
    nc = cstart.size
    words = np.zeros((nc + live.size, 3), np.uint16)
    words[:nc, 0] = ((clen - 1) << CMD_BITS) | GT_SKIP_BLOCK
    words[nc:, 0] = (attrs << CMD_BITS) | np.where(long_, GT_LONG_TILE_IDX, GT_SHORT_TILE_IDX)
    words[nc:, 1] = t & 0xFFFF
    words[nc:, 2] = t >> 16
    nwords = np.concatenate([np.ones(nc, np.int64), np.where(long_, 3, 2)])
    order = np.argsort(np.concatenate([cstart, live]), kind="stable")
    words, nwords = words[order], nwords[order]
    out = words[np.arange(3)[None, :] < nwords[:, None]]  # row-major: each token's words in order
    end = np.array([(int(is_last) << CMD_BITS) | GT_FRAME_END], np.uint16)
    return np.concatenate([out, end]).astype("<u2")


def keyframe_commands(tile, pal, hm, vm, smoothed, thm, tvm, palettes, palsize: int = 16):
    """The command words of one keyframe's frames ([F][Q] SmoothedTileMap arrays), after WriteKFAttributes."""
    z = _Z()
    for j in range(palettes.shape[0]):  # WriteKFAttributes
        z.cmd(GT_LOAD_PALETTE, 0)
        z.byte(j)
        z.byte(0)
        for i in range(palsize):
            z.dword(int(palettes[j, i]) | 0xFF000000)
    F, Q = tile.shape
    thm = np.asarray(thm, np.int64)
    tvm = np.asarray(tvm, np.int64)
    for f in range(F):
        z.b += _frame_words(np.asarray(tile[f], np.int64), np.asarray(pal[f], np.int64), np.asarray(hm[f], np.int64),
                            np.asarray(vm[f], np.int64), np.asarray(smoothed[f]).astype(bool), thm, tvm,
                            f == F - 1).tobytes()
    return bytes(z.b)


def keyframe_raw(k: int, palpix, thm, tvm, palettes_k, tile, pal, hm, vm, smoothed, *, width: int, height: int,
                 fps: float, palsize: int = 16) -> bytes:
    """The uncompressed command bytes of keyframe k (SaveStream main.pas:4724-4734): WriteTiles for k = 0 only
    (SetDimensions + TileSet + 64 B per tile, 4603-4622), then WriteKFAttributes and the keyframe's frames
    (tile/pal/hm/vm/smoothed: its [f][Q] SmoothedTileMap rows)."""
    palpix = np.ascontiguousarray(palpix, np.uint8).reshape(-1, 64)
    T = palpix.shape[0]
    z = _Z()
    if k == 0:  # WriteTiles
        z.cmd(GT_SET_DIMENSIONS, 0)
        z.word(width // 8)
        z.word(height // 8)
        z.dword(fpc_round(1000 * 1000 * 1000 / fps))
        z.dword(T)
        z.cmd(GT_TILE_SET, palsize)
        z.dword(0)
        z.dword(T - 1)
        z.b += palpix.tobytes()
    z.b += keyframe_commands(tile, pal, hm, vm, smoothed, thm, tvm, palettes_k, palsize)
    return bytes(z.b)


def compress_streams(raws, threads: int | None = None) -> list:
    """LZCompress of independent keyframe streams, concurrently (the C encoder runs outside the GIL)."""
    if not raws:
        return []
    workers = max(1, min(len(raws), threads or min(16, len(os.sched_getaffinity(0)))))
    with ThreadPoolExecutor(workers) as ex:
        return list(ex.map(lzma_encode, raws))


def assemble_stream(comps, kf_start, width: int, height: int, fps: float) -> bytes:
    """The .gtm file from the keyframes' compressed streams (in keyframe order): TGTMHeader (main.pas:103-114),
    one TGTMKeyFrameInfo per keyframe (116-124) with the measured sizes (4735-4757), then the streams."""
    kf_start = np.asarray(kf_start, np.int64)
    KF = kf_start.size - 1
    F = int(kf_start[-1])
    header = {"AverageBytesPerSec": 0, "KFMaxBytesPerSec": 0}
    kfinfo = []
    for k in range(KF):
        kfinfo.append({"KFIndex": k, "FrameIndex": int(kf_start[k]), "RawSize": 0, "CompressedSize": 0,
                       "TimeCodeMillisecond": fpc_round(1000.0 * int(kf_start[k]) / fps)})
    body = bytearray()
    avg = 0
    last_kf = 0
    for k, comp in enumerate(comps):
        f1 = int(kf_start[k + 1])
        body += comp
        kf_count = (f1 - 1) - last_kf + 1
        last_kf = f1
        kfinfo[k]["RawSize"] = 0  # the reference reads ZStream.Size after ZStream.Clear (main.pas:4735-4739)
        kfinfo[k]["CompressedSize"] = len(comp)
        if k > 0 or KF == 1:
            header["KFMaxBytesPerSec"] = max(header["KFMaxBytesPerSec"], fpc_round(len(comp) * fps / kf_count))
        avg += len(comp)
    header["AverageBytesPerSec"] = fpc_round(avg * fps / F)
    h = b"GTMv" + struct.pack("<9I", 40 - 8, 40 + 28 * KF, 1, width, height, KF, F,
                              header["AverageBytesPerSec"] & 0xFFFFFFFF, header["KFMaxBytesPerSec"] & 0xFFFFFFFF)
    for ki in kfinfo:
        h += b"GTMk" + struct.pack("<6I", 28 - 8, ki["KFIndex"], ki["FrameIndex"], ki["RawSize"],
                                   ki["CompressedSize"], ki["TimeCodeMillisecond"])
    return h + bytes(body)


def save_stream(palpix, thm, tvm, kf_start, palettes, sm_tile, sm_pal, sm_hm, sm_vm, sm_smoothed, width: int,
                height: int, fps: float, palsize: int = 16, threads: int | None = None) -> bytes:
    """SaveStream main.pas:4529-4763.  palpix [T][64] (active tiles, reindexed), thm/tvm [T], kf_start [KF+1],
    palettes [KF][P][16], sm_* [F][Q] SmoothedTileMap; width/height in pixels.  Returns the .gtm bytes."""
    kf_start = np.asarray(kf_start, np.int64)
    raws = []
    for k in range(kf_start.size - 1):
        f0, f1 = int(kf_start[k]), int(kf_start[k + 1])
        raws.append(keyframe_raw(k, palpix, thm, tvm, palettes[k], sm_tile[f0:f1], sm_pal[f0:f1], sm_hm[f0:f1],
                                 sm_vm[f0:f1], sm_smoothed[f0:f1], width=width, height=height, fps=fps,
                                 palsize=palsize))
    return assemble_stream(compress_streams(raws, threads), kf_start, width, height, fps)


# ---- the native writer (tiler_amd/csrc/gtm_write.hip, gtm_write.cpp) ------------------------------------------------
def gtm_source(palpix, thm, tvm, kf_start, palettes, tile, pal, hm, vm, smoothed, *, width: int, height: int,
               fps: float, palsize: int = 16, first_keyframe: bool = True, tiles: int | None = None,
               n_palettes: int | None = None, frames: int | None = None, positions: int | None = None):
    """tiler_gtm_source_t over numpy arrays (converted to the ABI's types) or, given as integers, HBM pointers (then
    tiles, n_palettes, frames and positions must be given).  kf_start [KF + 1]: rows of the arrays, from 0.
    palettes [KF][P][>= palsize].  Returns (GtmSource, the arrays it points into: keep them alive)."""
    keep = []

    def ptr(a, dtype, shape=None):
        if a is None or isinstance(a, int):
            return a or None
        a = np.ascontiguousarray(a, dtype)
        keep.append(a)
        return a.ctypes.data

    kf = np.ascontiguousarray(kf_start, np.int32)
    keep.append(kf)
    if not isinstance(palettes, int):
        palettes = np.asarray(palettes)[..., :palsize].reshape(kf.size - 1, -1, palsize)
        n_palettes = palettes.shape[1]
    if not isinstance(tile, int):
        tile = np.asarray(tile)
        frames, positions = tile.shape
    if not isinstance(thm, int):
        tiles = np.asarray(thm).size
    if not isinstance(palpix, int) and palpix is not None:
        palpix = np.ascontiguousarray(palpix, np.uint8).reshape(-1, 64)
    as_flag = lambda a: a if isinstance(a, int) else np.asarray(a).astype(np.uint8, copy=False)  # noqa: E731
    src = GtmSource(ptr(tile, np.int32), ptr(pal, np.int32), ptr(as_flag(hm), np.uint8), ptr(as_flag(vm), np.uint8),
                    ptr(as_flag(smoothed), np.uint8), ptr(palpix if first_keyframe else None, np.uint8),
                    ptr(as_flag(thm), np.uint8), ptr(as_flag(tvm), np.uint8), ptr(palettes, np.int32), kf.ctypes.data,
                    int(frames), int(positions), int(tiles), kf.size - 1, int(n_palettes), int(palsize),
                    int(bool(first_keyframe)), int(width), int(height), float(fps))
    return src, keep


def _raw_bound(src: GtmSource) -> int:
    """No raw stream set is longer: the fixed parts + 6 Q + 2 bytes per frame."""
    return (src.first_keyframe * (24 + 64 * src.tiles) + src.keyframes * src.n_palettes * (4 + 4 * src.palsize) +
            src.frames * (6 * src.positions + 2))


def _sized_call(call, what: str, bound: int):
    """dst / cap / out_len by tiler_lzma_encode's rules: a buffer of `bound` bytes, grown once if the call asks."""
    n = ctypes.c_size_t(0)
    for _ in range(2):
        out = np.empty(max(bound, 1), np.uint8)
        if call(out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(n)) == 0:
            return out[:n.value]
        if n.value <= out.size:
            break
        bound = n.value
    raise TilerError(f"{what} failed: {last_error()}")


def keyframe_raw_gpu(k: int, palpix, thm, tvm, palettes_k, tile, pal, hm, vm, smoothed, *, width: int, height: int,
                     fps: float, palsize: int = 16) -> bytes:
    """keyframe_raw on the GPU (tiler_gtm_commands): the same bytes.  Raises TilerError where keyframe_raw asserts
    (a tile or palette index out of range at a non-smoothed position)."""
    F = np.asarray(tile).shape[0]
    src, keep = gtm_source(palpix, thm, tvm, [0, F], np.asarray(palettes_k)[None], tile, pal, hm, vm, smoothed,
                           width=width, height=height, fps=fps, palsize=palsize, first_keyframe=k == 0)
    raw = np.empty(_raw_bound(src), np.uint8)
    off = np.zeros(2, np.int64)
    check(load().tiler_gtm_commands(ctypes.byref(src), _vp(raw), raw.size, _vp(off)), "tiler_gtm_commands")
    return raw[:off[1]].tobytes()


def keyframe_streams_gpu(palpix, thm, tvm, kf_start, palettes, sm_tile, sm_pal, sm_hm, sm_vm, sm_smoothed, *,
                         width: int, height: int, fps: float, palsize: int = 16, first_keyframe: bool = True,
                         threads: int | None = None, gpu_matches: bool = False) -> list:
    """The LZCompress'd streams of the given keyframes (tiler_gtm_streams; kf_start: rows of the arrays, from 0;
    first_keyframe: the first of them is the file's keyframe 0) -- for a caller that holds only some keyframes and
    assembles the file later (assemble_stream / tiler_gtm_assemble).  gpu_matches: the LZMA match search on the GPU
    too (tiler_gtm_set_gpu_matches for this call); the same bytes."""
    src, keep = gtm_source(palpix, thm, tvm, kf_start, palettes, sm_tile, sm_pal, sm_hm, sm_vm, sm_smoothed,
                           width=width, height=height, fps=fps, palsize=palsize, first_keyframe=first_keyframe)
    lens = np.zeros(src.keyframes, np.uint64)
    raw = _raw_bound(src)
    lib = load()
    with _GpuMatches(gpu_matches):
        out = _sized_call(lambda d, cap, n: lib.tiler_gtm_streams(ctypes.byref(src), int(threads or 0), d, cap,
                                                                  _vp(lens), n),
                          "tiler_gtm_streams", raw + raw // 32 + 4096 * src.keyframes)
    ends = np.cumsum(lens).astype(np.int64)
    return [out[e - int(n):e].tobytes() for e, n in zip(ends, lens)]


def save_stream_gpu(palpix, thm, tvm, kf_start, palettes, sm_tile, sm_pal, sm_hm, sm_vm, sm_smoothed, width: int,
                    height: int, fps: float, palsize: int = 16, threads: int | None = None,
                    gpu_matches: bool = False) -> bytes:
    """save_stream in libANN.so (tiler_gtm_write): the command words on the GPU, LZMA on native threads, the
    container -- the same file, byte for byte.  gpu_matches: the LZMA match search on the GPU too
    (tiler_gtm_set_gpu_matches for this call); still the same file."""
    src, keep = gtm_source(palpix, thm, tvm, kf_start, palettes, sm_tile, sm_pal, sm_hm, sm_vm, sm_smoothed,
                           width=width, height=height, fps=fps, palsize=palsize)
    raw = _raw_bound(src)
    lib = load()
    with _GpuMatches(gpu_matches):
        out = _sized_call(lambda d, cap, n: lib.tiler_gtm_write(ctypes.byref(src), int(threads or 0), d, cap, n),
                          "tiler_gtm_write", raw + raw // 32 + 4096 * src.keyframes + 40 + 28 * src.keyframes)
    return out.tobytes()


def assemble_stream_native(comps, kf_start, width: int, height: int, fps: float) -> bytes:
    """assemble_stream in libANN.so (tiler_gtm_assemble; host code)."""
    kf = np.ascontiguousarray(kf_start, np.int32)
    lens = np.array([len(c) for c in comps], np.uint64)
    body = np.frombuffer(b"".join(comps), np.uint8) if lens.sum() else np.zeros(1, np.uint8)
    lib = load()
    out = _sized_call(lambda d, cap, n: lib.tiler_gtm_assemble(_vp(body), _vp(lens), _vp(kf), kf.size - 1, int(width),
                                                               int(height), float(fps), d, cap, n),
                      "tiler_gtm_assemble", int(lens.sum()) + 40 + 28 * max(kf.size - 1, 0))
    return out.tobytes()


# ---- playback -------------------------------------------------------------------------------------------------------
LZMA_GROW = 1                # TILER_LZMA_GROW
MAX_RAW_BYTES = 1 << 30      # per-stream output cap (decompression bombs)
LAYOUTS = {"tiles": 0, "raster": 1}


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def lzma_decode(data: bytes, max_raw_bytes: int = MAX_RAW_BYTES) -> tuple:
    """One LZMA-alone stream at the start of `data` (any lc / lp / pb; end-marker or known-size form) ->
    (raw bytes, compressed bytes consumed), so concatenated streams can be walked.  Corrupt or truncated input, or
    a stream that expands past max_raw_bytes, raises TilerError."""
    lib = load()
    src = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    cap = min(max_raw_bytes, max(1 << 16, 4 * len(data)))
    n, used = ctypes.c_size_t(0), ctypes.c_size_t(0)
    while True:
        out = np.empty(max(cap, 1), np.uint8)
        rc = lib.tiler_lzma_decode(_vp(src), len(data), _vp(out), cap, ctypes.byref(n), ctypes.byref(used))
        if rc == 0:
            return out[:n.value].tobytes(), used.value
        check(rc, "tiler_lzma_decode")
        if cap >= max_raw_bytes or n.value > max_raw_bytes:
            raise TilerError(f"tiler_lzma_decode: the stream expands past max_raw_bytes ({max_raw_bytes})")
        cap = min(max_raw_bytes, max(n.value, 4 * cap))


class _Frames(int):
    """Stream.frames: the stream's frame count -- an int, as it has always been -- which, called with a list of
    frame indices, draws those frames (Stream._frames has the contract).  One name serves both because the count
    was there first and `frames(indices)` is what a reader of the C ABI (tiler_gtm_frames) looks for."""

    def __new__(cls, count: int, draw):
        self = int.__new__(cls, count)
        self._draw = weakref.WeakMethod(draw)  # no cycle: an unreferenced Stream still closes at once
        return self

    def __call__(self, indices, layout: str = "tiles", chunk: int | None = None) -> tuple:
        draw = self._draw()
        if draw is None:
            raise TilerError("the stream is gone")
        return draw(indices, layout, chunk)


class Stream:
    """A .gtm file opened for playback: bytes, a path or a binary file.  Parsing (header, LZMA, command tokens) is
    host code and needs no GPU; `play`, `frames` and `frame` need the device.  Stricter than the reference JS player:
    malformed command streams raise TilerError naming the rule, the frame and the position (include/tiler_ann.h).
    `frames` is the frame count and, called with indices, random access: frames(indices, layout="tiles", chunk=None)
    -> (rgb, undrawn)."""

    def __init__(self, source, threads: int = 0, max_raw_bytes: int = MAX_RAW_BYTES):
        if isinstance(source, str) or hasattr(source, "__fspath__"):
            with open(source, "rb") as f:
                source = f.read()
        elif hasattr(source, "read"):
            source = source.read()
        data = bytes(source)
        self._lib = load()
        buf = np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8)
        self._h = self._lib.tiler_gtm_open(_vp(buf), len(data), int(threads), int(max_raw_bytes))
        if not self._h:
            raise TilerError(f"tiler_gtm_open failed: {last_error()}")
        info = GtmInfo()
        check(self._lib.tiler_gtm_info(self._h, ctypes.byref(info)), "tiler_gtm_info")
        self.width, self.height, self.frame_ns = info.width, info.height, info.frame_ns
        self.frames, self.keyframes, self.palsize = _Frames(info.frames, self._frames), info.keyframes, info.palsize
        self.n_tiles, self.pal_rows, self.n_streams = info.tiles, info.pal_rows, info.streams
        self.header = ({"AverageBytesPerSec": info.avg_bytes_per_sec, "KFMaxBytesPerSec": info.kf_max_bytes_per_sec}
                       if info.has_header else None)

    def close(self):
        if self._h:
            self._lib.tiler_gtm_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._h:
            raise TilerError("the stream is closed")
        return self._h

    @property
    def positions(self) -> int:
        return self.width * self.height

    @property
    def next_frame(self) -> int:
        info = GtmInfo()
        check(self._lib.tiler_gtm_info(self._handle(), ctypes.byref(info)), "tiler_gtm_info")
        return info.next_frame

    @property
    def kf_start(self) -> np.ndarray:
        """[KF + 1]: the first frame of every keyframe, then the frame count."""
        out = np.zeros(self.keyframes + 1, np.int32)
        check(self._lib.tiler_gtm_kf_start(self._handle(), _vp(out)), "tiler_gtm_kf_start")
        return out

    @property
    def tiles(self) -> np.ndarray:
        out = np.zeros((self.n_tiles, 64), np.uint8)
        check(self._lib.tiler_gtm_tiles(self._handle(), _vp(out)), "tiler_gtm_tiles")
        return out

    @property
    def palettes(self) -> np.ndarray:
        """[R][palsize] uint32 RGBA dwords as stored (0xAABBGGRR): one row per LoadPalette, in stream order."""
        out = np.zeros((self.pal_rows, self.palsize), np.uint32)
        check(self._lib.tiler_gtm_palettes(self._handle(), _vp(out)), "tiler_gtm_palettes")
        return out

    def frame_flags(self) -> tuple:
        """(kf_end [F] uint8, skipped [F] int32, undrawn [F] int32)."""
        e, s, u = np.zeros(self.frames, np.uint8), np.zeros(self.frames, np.int32), np.zeros(self.frames, np.int32)
        check(self._lib.tiler_gtm_frame_flags(self._handle(), _vp(e), _vp(s), _vp(u)), "tiler_gtm_frame_flags")
        return e, s, u

    def stream_sizes(self) -> tuple:
        """(raw [S], compressed [S]) bytes of every LZMA stream."""
        r, c = np.zeros(self.n_streams, np.uint64), np.zeros(self.n_streams, np.uint64)
        check(self._lib.tiler_gtm_stream_sizes(self._handle(), _vp(r), _vp(c)), "tiler_gtm_stream_sizes")
        return r, c

    def items(self, f0: int = 0, f1: int | None = None) -> tuple:
        """The dense items of frames [f0, f1): (tile [n][Q] int32, -1 = skipped; attrs [n][Q] uint16 = pal << 2 |
        V << 1 | H; palrow [n][Q] int32 = the row of `palettes` in effect when the item was drawn)."""
        f1 = self.frames if f1 is None else f1
        n, Q = f1 - f0, self.positions
        if n < 0:
            raise ValueError("items: f1 < f0")
        t, a, r = np.zeros((n, Q), np.int32), np.zeros((n, Q), np.uint16), np.zeros((n, Q), np.int32)
        check(self._lib.tiler_gtm_items(self._handle(), f0, n, _vp(t), _vp(a), _vp(r)), "tiler_gtm_items")
        return t, a, r

    def play(self, n: int | None = None, layout: str = "tiles", chunk: int | None = None) -> tuple:
        """The next n frames (default: to the end) as the reference player shows them, drawn on the GPU `chunk`
        frames per call (default: about 128 MiB of output).  layout "tiles": rgb [n][Q][64], the project's frames;
        "raster": rgb [n][8 height][8 width].  Pixels are uint32 0xAABBGGRR as stored in the stream (never drawn:
        0xFF000000); mask the top byte to compare with the project's 0x00BBGGRR frames.  Returns (rgb, undrawn [n]
        int32: positions nothing has drawn yet); fewer than n frames at the end of the stream."""
        if layout not in LAYOUTS:
            raise ValueError("play: layout is 'tiles' or 'raster'")
        Q = self.positions
        left = self.frames - self.next_frame
        n = left if n is None else min(int(n), left)
        if n < 0:
            raise ValueError("play: n < 0")
        chunk = max(1, (1 << 27) // (Q * 256)) if chunk is None else int(chunk)
        if chunk <= 0:
            raise ValueError("play: chunk must be positive")
        rgb = np.zeros((n, Q * 64), np.uint32)
        undrawn = np.zeros(n, np.int32)
        done = 0
        while done < n:
            m = min(chunk, n - done)
            got = check(self._lib.tiler_gtm_play(self._handle(), m, LAYOUTS[layout], _vp(rgb[done:]),
                                                 _vp(undrawn[done:])), "tiler_gtm_play")
            if got != m:
                raise TilerError(f"tiler_gtm_play produced {got} of {m} frames")
            done += m
        shape = (n, Q, 64) if layout == "tiles" else (n, self.height * 8, self.width * 8)
        return rgb.reshape(shape), undrawn

    def play_dev(self, n: int, d_rgb: int, layout: str = "tiles", d_undrawn: int = 0, stream=None) -> int:
        """The next n frames into HBM (device pointers; d_rgb 16-byte aligned), asynchronous on `stream`; returns
        the frames produced."""
        return check(self._lib.tiler_gtm_play_dev(self._handle(), int(n), LAYOUTS[layout],
                                                  ctypes.c_void_p(int(d_rgb)),
                                                  ctypes.c_void_p(int(d_undrawn)) if d_undrawn else None,
                                                  ctypes.c_void_p(int(stream)) if stream else None),
                     "tiler_gtm_play_dev")

    def rewind(self):
        check(self._lib.tiler_gtm_rewind(self._handle()), "tiler_gtm_rewind")

    def seek(self, frame: int):
        """The next play starts at `frame` (0 .. frames; frames = the end) and shows exactly what a play from frame 0
        shows there.  Needs no GPU itself; the play that follows walks at most a checkpoint stride of keyframes
        (include/tiler_ann.h), never the frames before.  Another frame raises TilerError and leaves the position."""
        check(self._lib.tiler_gtm_seek(self._handle(), int(frame)), "tiler_gtm_seek")

    def _frames(self, indices, layout: str = "tiles", chunk: int | None = None) -> tuple:
        """Stream.frames(indices, layout, chunk).  The frames `indices` (any order, repeats allowed) as play shows them, without moving next_frame: (rgb
        [len(indices)] + play's frame shape, undrawn [len(indices)]), row i = frame indices[i].  Drawn `chunk`
        requests per call (default: about 128 MiB of output).  An index outside the stream raises TilerError before
        anything is drawn."""
        if layout not in LAYOUTS:
            raise ValueError("frames: layout is 'tiles' or 'raster'")
        idx = np.ascontiguousarray(np.asarray(indices, np.int64).reshape(-1))
        n, Q = idx.size, self.positions
        chunk = max(1, (1 << 27) // max(Q * 256, 1)) if chunk is None else int(chunk)
        if chunk <= 0:
            raise ValueError("frames: chunk must be positive")
        if ((idx < 0) | (idx >= self.frames)).any():  # the ABI's error for the whole list: no earlier chunk is drawn
            check(self._lib.tiler_gtm_frames(self._handle(), _vp(idx), n, LAYOUTS[layout], None, None),
                  "tiler_gtm_frames")
        rgb = np.zeros((n, Q * 64), np.uint32)
        undrawn = np.zeros(n, np.int32)
        for at in range(0, n, chunk):
            m = min(chunk, n - at)
            got = check(self._lib.tiler_gtm_frames(self._handle(), _vp(idx[at:]), m, LAYOUTS[layout], _vp(rgb[at:]),
                                                   _vp(undrawn[at:])), "tiler_gtm_frames")
            if got != m:
                raise TilerError(f"tiler_gtm_frames produced {got} of {m} frames")
        shape = (n, Q, 64) if layout == "tiles" else (n, self.height * 8, self.width * 8)
        return rgb.reshape(shape), undrawn

    def frame(self, f: int, layout: str = "tiles") -> np.ndarray:
        """Frame f alone ([Q][64] or [8 height][8 width]); next_frame stays."""
        return self.frames([f], layout)[0][0]

    def frames_dev(self, indices, d_rgb: int, layout: str = "tiles", d_undrawn: int = 0, stream=None) -> int:
        """`frames` into HBM (device pointers; d_rgb 16-byte aligned, len(indices) frames), asynchronous on `stream`;
        the indices are host values.  Returns len(indices)."""
        idx = np.ascontiguousarray(np.asarray(indices, np.int64).reshape(-1))
        return check(self._lib.tiler_gtm_frames_dev(self._handle(), _vp(idx), idx.size, LAYOUTS[layout],
                                                    ctypes.c_void_p(int(d_rgb)) if d_rgb else None,
                                                    ctypes.c_void_p(int(d_undrawn)) if d_undrawn else None,
                                                    ctypes.c_void_p(int(stream)) if stream else None),
                     "tiler_gtm_frames_dev")


def load_stream(path) -> Stream:
    """Open a .gtm file (a path or a binary file) for playback."""
    return Stream(path)
