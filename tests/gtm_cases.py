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


def written_stream(seed, W, H, T, P, kf_start, long_run: int = 0, fps: float = 30.0, palsize: int = 16):
    """gtm.save_stream of a seeded clip (W, H in pixels); the first frame of a keyframe is never smoothed.  palsize:
    colours per palette (tile pixels use every index below it).  Returns (data, dict of what went in)."""
    rng = np.random.default_rng(seed)
    Q = (W // 8) * (H // 8)
    kf_start = np.asarray(kf_start)
    F = int(kf_start[-1])
    palpix = rng.integers(0, palsize, (T, 64)).astype(np.uint8)
    thm = rng.integers(0, 2, T).astype(np.uint8)
    tvm = rng.integers(0, 2, T).astype(np.uint8)
    pals = rng.integers(0, 1 << 24, (kf_start.size - 1, P, palsize)).astype(np.int32)
    tile, pal, hm, vm, sm = smoothed_maps(rng, F, Q, T, P, long_run)
    sm[kf_start[:-1]] = 0
    data = gtm.save_stream(palpix, thm, tvm, kf_start, pals, tile, pal, hm, vm, sm, W, H, fps, palsize=palsize)
    return data, dict(palpix=palpix, thm=thm, tvm=tvm, pals=pals, tile=tile, pal=pal, hm=hm, vm=vm, sm=sm,
                      kf_start=kf_start, Q=Q, F=F, W=W, H=H, fps=fps, palsize=palsize)


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


BLACK = 0xFF000000


def palette_reload_stream():
    """Hand-built (the writer never produces it): keyframe 1 reloads palette 0 with other colours and its first
    frame skips a block of positions.  Returns (data, W, H in tiles, the old and the new colours of palette 0)."""
    rng = np.random.default_rng(3)
    W, H, T = 4, 2, 6
    tiles = rng.integers(0, 16, (T, 64))
    old = rng.integers(0, 1 << 24, 16) | BLACK
    new = (old ^ 0x00FFFFFF)
    other = rng.integers(0, 1 << 24, 16) | BLACK
    k0 = Z().dims(W, H, T).tileset(tiles).palette(0, old).palette(1, other)
    for q in range(8):
        k0.item(q % T, pal=q & 1, h=q & 1, v=(q >> 1) & 1)
    k0.end(1)
    k1 = Z().palette(0, new).item(5, pal=0).skip(4).item(4, pal=0, h=1).item(3, pal=1).item(2, pal=0, v=1).end(0)
    k1.skip(2).item(1, pal=0).skip(5).end(1)
    return assemble([k0.b, k1.b], [0, 1, 3], W, H), W, H, old, new


def never_drawn_stream():
    """Hand-built: the first frame skips 5 of the 8 positions, frame 2 draws 2 of them (undrawn 5, 5, 3, 3).  Returns
    (data, W, H in tiles)."""
    rng = np.random.default_rng(4)
    W, H, T = 4, 2, 3
    pal = rng.integers(1, 1 << 24, 16) | BLACK
    z = Z().dims(W, H, T).tileset(rng.integers(0, 16, (T, 64))).palette(0, pal)
    z.item(0).skip(3).item(1).skip(2).item(2).end(0)
    z.skip(8).end(0)
    z.skip(2).item(1).skip(2).item(0, h=1).skip(2).end(0)
    z.skip(8).end(1)
    return assemble([z.b], [0, 4], W, H), W, H
