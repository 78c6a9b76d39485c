"""TEST INFRASTRUCTURE: GTM streams for the playback tests -- the SmoothedTileMap generator of
test_gtm.test_save_stream_roundtrip at any size, and command streams written token by token (gtm._Z) for the cases
the writer never produces (palette reloads under skipped positions, never-drawn positions, malformed streams)."""
from __future__ import annotations

import numpy as np

from tiler_amd import gtm


def smoothed_maps(rng, F, Q, T, P, long_run: int = 0, keep_p: float = 0.6):
    """[F][Q] SmoothedTileMap arrays: frame f keeps a random `keep_p` of frame f - 1's items (Smoothed set), plus
    one run of `long_run` kept items when given (longer than the 1024-item SkipBlock limit)."""
    tile = rng.integers(0, T, (F, Q))
    pal = rng.integers(0, P, (F, Q))
    hm = rng.integers(0, 2, (F, Q)).astype(np.uint8)
    vm = rng.integers(0, 2, (F, Q)).astype(np.uint8)
    sm = np.zeros((F, Q), np.uint8)
    for f in range(1, F):
        keep = rng.random(Q) < keep_p
        if long_run:
            s0 = int(rng.integers(0, Q - long_run))
            keep[s0:s0 + long_run] = True
        for a in (tile, pal, hm, vm):
            a[f] = np.where(keep, a[f - 1], a[f])
        sm[f] = keep
    return tile, pal, hm, vm, sm


def written_stream(seed, W, H, T, P, kf_start, long_run: int = 0, fps: float = 30.0):
    """gtm.save_stream of a seeded clip (W, H in pixels); the first frame of a keyframe is never smoothed.  Returns
    (data, dict of what went in)."""
    rng = np.random.default_rng(seed)
    Q = (W // 8) * (H // 8)
    kf_start = np.asarray(kf_start)
    F = int(kf_start[-1])
    palpix = rng.integers(0, 16, (T, 64)).astype(np.uint8)
    thm = rng.integers(0, 2, T).astype(np.uint8)
    tvm = rng.integers(0, 2, T).astype(np.uint8)
    pals = rng.integers(0, 1 << 24, (kf_start.size - 1, P, 16)).astype(np.int32)
    tile, pal, hm, vm, sm = smoothed_maps(rng, F, Q, T, P, long_run)
    sm[kf_start[:-1]] = 0
    data = gtm.save_stream(palpix, thm, tvm, kf_start, pals, tile, pal, hm, vm, sm, W, H, fps)
    return data, dict(palpix=palpix, thm=thm, tvm=tvm, pals=pals, tile=tile, pal=pal, hm=hm, vm=vm, sm=sm,
                      kf_start=kf_start, Q=Q, F=F)


def strip_header(data: bytes) -> bytes:
    """The same streams as a headerless file (the player's parseHeader fallback)."""
    assert data[:4] == b"GTMv"
    return data[int.from_bytes(data[8:12], "little"):]


class Z(gtm._Z):
    """Command tokens by name."""

    def dims(self, w, h, tiles, ns=41666667):
        self.cmd(gtm.GT_SET_DIMENSIONS, 0)
        self.word(w)
        self.word(h)
        self.dword(ns)
        self.dword(tiles)
        return self

    def tileset(self, tiles, palsize=16, first=0):
        tiles = np.ascontiguousarray(tiles, np.uint8).reshape(-1, 64)
        self.cmd(gtm.GT_TILE_SET, palsize)
        self.dword(first)
        self.dword(first + tiles.shape[0] - 1)
        self.b += tiles.tobytes()
        return self

    def palette(self, idx, colours):
        self.cmd(gtm.GT_LOAD_PALETTE, 0)
        self.byte(idx)
        self.byte(0)
        for c in colours:
            self.dword(int(c))
        return self

    def item(self, tile, pal=0, h=0, v=0, long=None):
        long = tile >= (1 << 16) if long is None else long
        self.cmd(gtm.GT_LONG_TILE_IDX if long else gtm.GT_SHORT_TILE_IDX, (pal << 2) | (v << 1) | h)
        (self.dword if long else self.word)(tile)
        return self

    def skip(self, n):
        self.cmd(gtm.GT_SKIP_BLOCK, n - 1)
        return self

    def end(self, last=0):
        self.cmd(gtm.GT_FRAME_END, last)
        return self


def assemble(raws, kf_start, w, h, fps=24.0) -> bytes:
    """A .gtm file from uncompressed keyframe streams (w, h in tiles)."""
    return gtm.assemble_stream([gtm.lzma_encode(bytes(r)) for r in raws], kf_start, w * 8, h * 8, fps)
