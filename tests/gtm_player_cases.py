"""TEST INFRASTRUCTURE: the .gtm files that the reference's own player (decoders/htmljs/gtm.player.js over its lzma.js,
driven by oracle/ref_player.js) has played, and what it drew: tests/golden/gtm_player.json, written by
tests/golden/make_gtm_player_golden.py where the reference tree is mounted.  Every case's bytes are rebuilt here on
the host (no GPU), deterministically, so the fixture holds digests and numbers only.

All cases are well formed.  The product reader (gtm_read.cpp) refuses streams that the player only logs, or plays on
through; those departures are deliberate and stay outside this fixture (tests/test_gtm_decode.py MALFORMED has them):
  - FrameEnd with an incomplete tilemap, and an unknown command: the player writes console.error and goes on;
  - a skip or an item past the end of the tilemap: the player writes outside its framebuffer, which a typed array
    ignores;
  - a tile index >= the tile count, or a palette index never loaded: the player throws from drawTilemapItem;
  - a second SetDimensions of another size, a TileSet after the first frame: the player takes them;
  - a truncated token or LZMA stream: the player reads `undefined` bytes / stalls.
"""
from __future__ import annotations

import functools
import hashlib
import json
import os

import numpy as np

from gtm_cases import BLACK, Z, assemble, never_drawn_stream, palette_reload_stream, strip_header, written_stream

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gtm_player.json")
DEMO_CLIPS = ("football_cif.gtm", "city_cif.gtm")

# name: written_stream's arguments.  Each is also written by the GPU paths (tests/test_gpu_gtm_ref_player.py).
WRITTEN = {
    # 7 x 5 tiles (Q = 35), 9 frames in 3 keyframes, 3 palettes, random skips, both mirrors
    "small": dict(seed=5, W=56, H=40, T=50, P=3, kf_start=[0, 3, 6, 9]),
    # 40 x 30 tiles, LongTileIdx (T = 70000), a kept run of 1,100 > the 1,024 SkipBlock limit in every later frame
    "long": dict(seed=70000, W=320, H=240, T=70000, P=6, kf_start=[0, 3, 4, 8], long_run=1100),
    # 32- and 64-colour tile sets: 5 x 3 tiles, 5 frames in 2 keyframes, 3 palettes
    "pal32": dict(seed=32, W=40, H=24, T=40, P=3, kf_start=[0, 2, 5], palsize=32),
    "pal64": dict(seed=64, W=40, H=24, T=40, P=3, kf_start=[0, 2, 5], palsize=64),
}
NAMES = ("small", "small_headerless", "long", "palette_reload", "never_drawn", "pal32", "pal64", "mirrors")
UNDRAWN = {"never_drawn": [5, 5, 3, 3]}  # every other case: zero in every frame


def mirrors_stream():
    """Hand-built, 4 x 4 tiles, 2 frames: two asymmetric tiles (no mirrored form equals another), each shown in all
    four mirror combinations through each of two palettes whose colours differ at every index; the second frame
    redraws two thirds of the positions with the mirror bits exchanged and the other palette.  An H/V swap, or a
    palette index taken from other bits, changes pixels.  Returns (data, W, H in tiles)."""
    rng = np.random.default_rng(8)
    W, H = 4, 4
    tiles = np.stack([np.arange(64) % 16, rng.integers(0, 16, 64)]).astype(np.uint8)
    for t in tiles.reshape(2, 8, 8):
        forms = [t, t[:, ::-1], t[::-1, :], t[::-1, ::-1]]
        assert all(not np.array_equal(forms[i], forms[j]) for i in range(4) for j in range(i))
    pal0 = rng.integers(0, 1 << 24, 16) | BLACK
    pal1 = (pal0 ^ 0x00FFFFFF)
    z = Z().dims(W, H, 2).tileset(tiles).palette(0, pal0).palette(1, pal1)
    for q in range(16):
        z.item(q >> 3, pal=(q >> 2) & 1, h=q & 1, v=(q >> 1) & 1)
    z.end(0)
    for q in range(16):
        if q % 3 == 0:
            z.skip(1)
        else:
            z.item(1 - (q >> 3), pal=1 - ((q >> 2) & 1), h=(q >> 1) & 1, v=q & 1)
    z.end(1)
    return assemble([z.b], [0, 2], W, H), W, H


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """data (the file), W, H (tiles), and for a written case `inputs`: written_stream's dict of what went in."""
    if name in WRITTEN:
        a = WRITTEN[name]
        data, c = written_stream(a["seed"], a["W"], a["H"], a["T"], a["P"], a["kf_start"], a.get("long_run", 0),
                                 palsize=a.get("palsize", 16))
        live = ~c["sm"].astype(bool)
        assert c["sm"].any() and c["hm"].any() and c["vm"].any() and (c["pal"][live] > 0).any()
        if name == "long":
            assert (c["tile"][live] >= 1 << 16).any()
        if c["palsize"] > 16:  # drawn tiles hold indices of the upper half, through palettes beyond 0
            assert (c["palpix"][c["tile"][live & (c["pal"] > 0)]] >= c["palsize"] // 2).any()
        return dict(data=data, W=a["W"] // 8, H=a["H"] // 8, inputs=c)
    if name == "small_headerless":
        full = case("small")
        return dict(data=strip_header(full["data"]), W=full["W"], H=full["H"], inputs=None)
    data, W, H = {"palette_reload": lambda: palette_reload_stream()[:3], "never_drawn": never_drawn_stream,
                  "mirrors": mirrors_stream}[name]()
    return dict(data=data, W=W, H=H, inputs=None)


@functools.lru_cache(maxsize=None)
def golden() -> dict:
    with open(FIXTURE) as f:
        return json.load(f)


def file_sha256(data: bytes) -> str:
    return hashlib.sha256(data).hexdigest()


def frame_digests(frames) -> list:
    """SHA-256 per frame of [F][8 H][8 W] RGBA pixels: uint8 [..., 4] in R,G,B,A order, or uint32 dwords (little
    endian: the same bytes)."""
    frames = np.ascontiguousarray(frames)
    assert frames.dtype in (np.uint8, np.dtype("<u4"))
    return [hashlib.sha256(f.tobytes()).hexdigest() for f in frames]


def check_file(name: str, data: bytes, what: str = "the registry"):
    """The bytes are the ones the reference player was given when the fixture was made."""
    want = golden()["cases"][name]
    assert (len(data), file_sha256(data)) == (want["file_bytes"], want["file_sha256"]), \
        f"case {name!r}: the file built by {what} is not the one in tests/golden/gtm_player.json; if the writer " \
        f"changed on purpose, regenerate it with tests/golden/make_gtm_player_golden.py"
