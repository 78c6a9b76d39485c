"""The GPU GTM player (tiler_amd.gtm.Stream.play over play.hip) against the test player tests/gtm_read.render: both
layouts, every chunking, long skip runs and long tile indices, pixels carried over a palette reload, never-drawn
positions, the ends of the stream, and the Encoder chain closed over the written bytes (verify_stream,
quality(stream=...))."""
import struct

import numpy as np
import pytest

import gtm_read
from gtm_cases import BLACK, never_drawn_stream, palette_reload_stream, strip_header, written_stream
from tiler_amd import gtm

pytestmark = pytest.mark.gpu


def _reference(oracle, data):
    """The test player's frames as [F][8 H][8 W] uint32 RGBA dwords."""
    img = gtm_read.render(gtm_read.read_gtm(oracle, data))
    return np.ascontiguousarray(img).view(np.uint32)[..., 0]


def _tiled(raster, W, H):
    F = raster.shape[0]
    return raster.reshape(F, H, 8, W, 8).transpose(0, 1, 3, 2, 4).reshape(F, W * H, 64)


def test_small_player_case(gpu, oracle):
    """7 x 5 tilemap (Q = 35: no multiple of 16 or 64), 9 frames in 3 keyframes, 3 palettes, random skips and
    mirrors: chunk 1, 4 and 9 give identical bytes, the raster layout is the test player's picture bit for bit, the
    tile-major layout is that picture re-tiled, nothing is left undrawn."""
    W, H = 7, 5
    data, c = written_stream(5, W * 8, H * 8, 50, 3, [0, 3, 6, 9])
    assert c["sm"].any() and c["hm"].any() and c["vm"].any()
    ref = _reference(oracle, data)
    with gtm.Stream(data) as st:
        assert (st.width, st.height, st.frames, st.keyframes) == (W, H, 9, 3)
        out = {}
        for layout in ("raster", "tiles"):
            for chunk in (1, 4, 9):
                st.rewind()
                rgb, undrawn = st.play(layout=layout, chunk=chunk)
                assert not undrawn.any() and rgb.dtype == np.uint32
                out[layout, chunk] = rgb
            assert np.array_equal(out[layout, 1], out[layout, 4]) and np.array_equal(out[layout, 1], out[layout, 9])
        assert out["raster", 1].shape == (9, H * 8, W * 8) and np.array_equal(out["raster", 1], ref)
        assert out["tiles", 1].shape == (9, W * H, 64) and np.array_equal(out["tiles", 1], _tiled(ref, W, H))


def test_long_runs_and_long_indices(gpu, oracle):
    """40 x 30 tilemap, a skip run over 1,024 in every later frame, T = 70000 so LongTileIdx occurs."""
    W, H = 40, 30
    data, c = written_stream(70000, W * 8, H * 8, 70000, 6, [0, 3, 4, 8], long_run=1100)
    assert (c["tile"][~c["sm"].astype(bool)] >= 1 << 16).any()
    ref = _reference(oracle, data)
    with gtm.Stream(data) as st:
        rgb, undrawn = st.play(layout="raster", chunk=3)
        assert not undrawn.any() and np.array_equal(rgb, ref)
        st.rewind()
        rgb, _ = st.play(layout="tiles")
        assert np.array_equal(rgb, _tiled(ref, W, H))


def test_carry_over_a_palette_reload(gpu, oracle):
    """Hand-built (the writer never produces it): keyframe 1 reloads palette 0 with other colours and its first
    frame skips a block of positions.  Those keep keyframe 0's pixels -- drawn through the old colours -- while the
    positions redrawn with palette 0 get the new ones."""
    data, W, H, old, new = palette_reload_stream()
    ref = _reference(oracle, data)
    with gtm.Stream(data) as st:
        assert st.pal_rows == 3 and np.array_equal(st.palettes[2], new.astype(np.uint32))
        rgb, undrawn = st.play(layout="raster", chunk=2)
        st.rewind()
        tl, _ = st.play(layout="tiles", chunk=1)
    assert np.array_equal(rgb, ref) and np.array_equal(tl, _tiled(ref, W, H)) and not undrawn.any()
    t = _tiled(rgb, W, H)
    assert np.array_equal(t[1, 1:5], t[0, 1:5]) and np.array_equal(t[2, 3:5], t[0, 3:5])  # carried, old colours
    assert np.isin(t[0, 2], old).all() and np.isin(t[1, 2], old).all()                    # palette 0, before
    for f, q in ((1, 0), (1, 5), (1, 7), (2, 2)):                                          # palette 0, after
        assert np.isin(t[f, q], new).all() and not np.isin(t[f, q], old).any()


def test_never_drawn_positions(gpu):
    """Hand-built: the first frame skips 5 positions -- opaque black, undrawn 5; a later frame draws 2 of them and
    undrawn is 3 from that frame on."""
    data, W, H = never_drawn_stream()
    with gtm.Stream(data) as st:
        assert list(st.frame_flags()[2]) == [5, 5, 3, 3]
        for chunk in (1, 4):
            st.rewind()
            rgb, undrawn = st.play(layout="tiles", chunk=chunk)
            assert list(undrawn) == [5, 5, 3, 3]
            never = np.ones((4, 8), bool)
            never[:, [0, 4, 7]] = False
            never[2:, [2, 5]] = False
            assert (rgb[never] == BLACK).all() and (rgb[~never] != BLACK).all()
            assert np.array_equal(rgb[1], rgb[0]) and np.array_equal(rgb[3], rgb[2])
        st.rewind()
        raster, _ = st.play(layout="raster")
        assert np.array_equal(_tiled(raster, W, H), rgb)


def test_stream_ends(gpu, oracle):
    """rewind() then play reproduces the first pass; play past the end returns fewer frames, then none; a
    headerless stream plays the same."""
    W, H = 7, 5
    data, _ = written_stream(6, W * 8, H * 8, 40, 3, [0, 2, 5])
    with gtm.Stream(data) as st:
        first, _ = st.play()
        assert first.shape[0] == 5 and st.next_frame == 5
        assert st.play()[0].shape[0] == 0
        st.rewind()
        a, _ = st.play(3)
        b, _ = st.play(3)
        c, _ = st.play(3)
        assert (a.shape[0], b.shape[0], c.shape[0]) == (3, 2, 0)
        assert np.array_equal(np.concatenate([a, b]), first)
        # the C entry point itself: asked for more than is left
        st.rewind()
        buf, und = np.zeros((8, W * H * 64), np.uint32), np.zeros(8, np.int32)
        lib = gpu.load()
        p = lambda x: x.ctypes.data  # noqa: E731
        assert lib.tiler_gtm_play(st._h, 4, 0, p(buf), p(und)) == 4
        assert lib.tiler_gtm_play(st._h, 4, 0, p(buf[4:]), p(und[4:])) == 1
        assert lib.tiler_gtm_play(st._h, 4, 0, p(buf[5:]), p(und[5:])) == 0
        assert np.array_equal(buf[:5].reshape(first.shape), first) and not buf[5:].any()
        assert lib.tiler_gtm_play(st._h, 1, 7, p(buf), p(und)) == -1 and "layout" in gpu.last_error()
    with gtm.Stream(strip_header(data)) as st:
        assert st.header is None and np.array_equal(st.play(chunk=2)[0], first)


def _item_offsets(raw: bytes, Q: int):
    """Offsets of the Short/LongTileIdx command words of a keyframe stream (palsize 16): {(frame, position): at}."""
    at, f, q, out = 0, 0, 0, {}
    while at < len(raw):
        w, = struct.unpack_from("<H", raw, at)
        cmd, arg = w & 63, w >> 6
        if cmd == gtm.GT_SET_DIMENSIONS:
            at += 2 + 12
        elif cmd == gtm.GT_TILE_SET:
            t0, t1 = struct.unpack_from("<II", raw, at + 2)
            at += 2 + 8 + 64 * (t1 - t0 + 1)
        elif cmd == gtm.GT_LOAD_PALETTE:
            at += 2 + 2 + 64
        elif cmd == gtm.GT_SKIP_BLOCK:
            q += arg + 1
            at += 2
        elif cmd in (gtm.GT_SHORT_TILE_IDX, gtm.GT_LONG_TILE_IDX):
            out[f, q] = at
            q += 1
            at += 4 if cmd == gtm.GT_SHORT_TILE_IDX else 6
        else:
            assert cmd == gtm.GT_FRAME_END and q == Q
            f, q = f + 1, 0
            at += 2
    return out


def test_encoder_chain(gpu):
    """Encoder.run_all on the suite's C1 video, then save_stream: verify_stream finds no differing frame, and
    quality(stream=...) returns quality()'s corr and sse bit for bit.  With one item's palette bits changed in the
    raw stream exactly the frames showing that item are reported, from the right (frame, position)."""
    from tiler_amd import synth
    from tiler_amd.encoder import Encoder
    from tiler_amd.frame_tiling import FT_MEDIUM
    W, H, Q = 320, 240, 1200
    e = Encoder(synth.video(51 + FT_MEDIUM, W, H, kf_frames=(3, 3), n_palettes=8))
    e.run_all(700, FT_MEDIUM, 0.2)
    data = e.save_stream(W, H, 24.0)
    res = e.verify_stream(data, width=W, height=H)
    assert (res["frames"], res["differing_frames"], res["differing"], res["first"], res["undrawn"]) == \
        (6, 0, [], None, 0)
    assert e.verify_stream(width=W, height=H)["differing_frames"] == 0  # default: its own save_stream
    q, qs = e.quality(width=W, height=H), e.quality(width=W, height=H, stream=data)
    assert np.array_equal(q["corr"].view(np.uint64), qs["corr"].view(np.uint64))
    assert np.array_equal(q["sse"], qs["sse"]) and np.array_equal(q["rgb"], qs["rgb"]) and not qs["invalid"].any()
    # keyframe 1 = frames 3..5: change the palette of an item of frame 4 that frame 5 skips (carries), if any
    sm = e.sm["smoothed"].astype(bool)
    assert sm.any()
    drawn4 = np.nonzero(~sm[4])[0]
    carried = drawn4[sm[5][drawn4]]
    pos = int(carried[0] if carried.size else drawn4[0])
    comps, at = [], int.from_bytes(data[8:12], "little")
    while at < len(data):
        raw, used = gtm.lzma_decode(data[at:])
        comps.append(bytearray(raw))
        at += used
    assert len(comps) == 2
    off = _item_offsets(bytes(comps[1]), Q)[1, pos]
    w, = struct.unpack_from("<H", comps[1], off)
    pal = w >> 8
    assert pal == e.sm["pal"][4, pos]
    rgb = q["rgb"]
    used = e.palpix[e.sm["tile"][4, pos]]  # a palette that shows this tile in other colours
    other = next(p for p in range(8) if (e.palettes[1, p][used] != e.palettes[1, pal][used]).any())
    struct.pack_into("<H", comps[1], off, (w & 0xFF) | (other << 8))
    bad = gtm.assemble_stream([gtm.lzma_encode(bytes(r)) for r in comps], e.kf_start, W, H, 24.0)
    res = e.verify_stream(bad, width=W, height=H)
    with gtm.Stream(bad) as st:
        played = st.play()[0] & 0x00FFFFFF
    want = [4, 5] if carried.size else [4]
    assert [f for f in range(6) if (played[f, pos] != rgb[f, pos].astype(np.uint32)).any()] == want
    assert res["differing"] == want and res["differing_frames"] == len(want) and res["first"] == (4, pos)
    assert not (played[:, np.arange(Q) != pos] != rgb[:, np.arange(Q) != pos].astype(np.uint32)).any()
