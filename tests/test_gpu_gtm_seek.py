"""GTM random access on the GPU (gtm.Stream.seek / frames / frame / frames_dev over play.hip's checkpoint index and
walk kernel): every frame of every case the reference's own player has played (tests/golden/gtm_player.json), reached
by seek and by frames(); a hand-built stream whose keyframes begin with skipped items, reload a palette index and
leave positions undrawn, against the test player with strided checkpoints and two-frame passes; the sequential state
beside frames(); frames_dev on a torch stream; and the Encoder's verify_stream / quality(stream=...) for an encoder
that holds every third frame."""

import numpy as np
import pytest

import gtm_player_cases as cases
import gtm_read
from gtm_cases import Z, assemble
from tiler_amd import TilerError, gtm

pytestmark = pytest.mark.gpu


def _tiled(raster, W, H):
    F = raster.shape[0]
    return raster.reshape(F, H, 8, W, 8).transpose(0, 1, 3, 2, 4).reshape(F, W * H, 64)


def _digests(rgb):
    return cases.frame_digests(rgb.astype("<u4", copy=False))


# ---- 1. against the reference player --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_seek_and_frames_show_the_reference_picture(gpu, name):
    """seek(f) + play for every f in 0..F: the reference player's digests from frame f on, undrawn from f on.
    palette_reload at f = 1, 2 and never_drawn at f = 1..3 differ for a seek that starts from an empty picture at the
    keyframe.  frames() backwards and with a repeat: the same digests in request order; tile-major = re-tiled."""
    c, want = cases.case(name), cases.golden()["cases"][name]
    cases.check_file(name, c["data"])
    W, H, F = want["width"], want["height"], want["frames"]
    sha, und = want["frame_sha256"], cases.UNDRAWN.get(name, [0] * F)
    with gtm.Stream(c["data"]) as st:
        for f in range(F + 1):
            st.seek(f)
            assert st.next_frame == f
            rgb, undrawn = st.play(layout="raster")
            assert rgb.shape == (F - f, H * 8, W * 8) and st.next_frame == F
            got = _digests(rgb)
            bad = [f + i for i in range(F - f) if got[i] != sha[f + i]]
            assert not bad, f"case {name!r}, seek({f}): frames {bad} differ from the reference player's"
            assert list(undrawn) == und[f:]
        st.seek(0)
        for idx in (list(range(F))[::-1], [F - 1, 0, F - 1]):
            raster, undrawn = st.frames(idx, "raster")
            assert raster.shape == (len(idx), H * 8, W * 8) and raster.dtype == np.uint32
            assert _digests(raster) == [sha[i] for i in idx], f"case {name!r}, frames({idx})"
            assert list(undrawn) == [und[i] for i in idx]
            tiles, undrawn = st.frames(idx, "tiles")
            assert np.array_equal(tiles, _tiled(raster, W, H)) and list(undrawn) == [und[i] for i in idx]
            assert st.next_frame == 0
        assert _digests(st.frame(F - 1, "raster")[None]) == [sha[F - 1]]


# ---- 2. strided checkpoints and pass boundaries ---------------------------------------------------------------------
SW, SH, SQ = 6, 4, 24
S_KF_START = [0, 2, 3, 6, 10, 11, 13, 16]  # 7 keyframes of 1-4 frames
S_LATE = (5, 17)                           # no frame before 14 draws these; frame 14 draws the first


def _sparse_stream():
    """Hand-built: every frame -- the first of a keyframe too -- draws about a third of the positions and skips the
    rest; palette index 1 is reloaded with other colours in keyframes 2 and 5.  Returns (data, row_of: per frame the
    palette row each of the three indices stands for)."""
    rng = np.random.default_rng(11)
    T, F = 10, S_KF_START[-1]
    tiles = rng.integers(0, 16, (T, 64))
    colours = lambda: rng.integers(0, 1 << 24, 16) | 0xFF000000  # noqa: E731
    raws, rows, row_of, n_rows = [], [0, 1, 2], [], 3
    for k in range(len(S_KF_START) - 1):
        z = Z()
        if k == 0:
            z.dims(SW, SH, T).tileset(tiles)
            for i in range(3):
                z.palette(i, colours())
        if k in (2, 5):
            z.palette(1, colours())
            rows[1], n_rows = n_rows, n_rows + 1
        for f in range(S_KF_START[k], S_KF_START[k + 1]):
            row_of.append(list(rows))
            draw = rng.random(SQ) < 1 / 3
            for q in S_LATE:
                draw[q] = False
            if f == 14:
                draw[S_LATE[0]] = True
            q = 0
            while q < SQ:
                if draw[q]:
                    z.item(int(rng.integers(0, T)), pal=int(rng.integers(0, 3)), h=int(rng.integers(0, 2)),
                           v=int(rng.integers(0, 2)))
                    q += 1
                else:
                    run = 1
                    while q + run < SQ and not draw[q + run]:
                        run += 1
                    z.skip(run)
                    q += run
            z.end(int(f == S_KF_START[k + 1] - 1))
        raws.append(z.b)
    return assemble(raws, S_KF_START, SW, SH), np.array(row_of)


@pytest.fixture(scope="module")
def sparse(oracle):
    data, row_of = _sparse_stream()
    img = gtm_read.render(gtm_read.read_gtm(oracle, data))
    ref = np.ascontiguousarray(img).view(np.uint32)[..., 0]
    ref.setflags(write=False)
    return data, row_of, ref


def test_sparse_stream_has_what_a_keyframe_reset_gets_wrong(sparse):
    """The generated items themselves: long-lived items, never-drawn positions and superseded palette rows are on
    screen at keyframe starts, so a seek must know more than the keyframe it lands in."""
    data, row_of, ref = sparse
    with gtm.Stream(data) as st:
        assert (st.width, st.height, st.frames, st.keyframes, st.pal_rows) == (SW, SH, 16, 7, 5)
        assert list(st.kf_start) == S_KF_START
        tile, attrs, palrow = st.items()
        undrawn = st.frame_flags()[2]
    F = tile.shape[0]
    drawn = tile >= 0
    frac = drawn.mean(axis=1)
    assert (frac > 0.1).all() and (frac < 0.6).all() and undrawn[0] > 0  # every frame skips most positions
    last = np.full((F + 1, SQ), -1)  # last[f]: the frame that drew what is on screen before frame f
    for f in range(F):
        last[f + 1] = np.where(drawn[f], f, last[f])
    at4 = last[S_KF_START[4]]
    assert ((at4 >= 0) & (at4 < S_KF_START[3])).any()          # on screen at keyframe 4, drawn >= 2 keyframes earlier
    assert (last[S_KF_START[6]] < 0).sum() == 2 and undrawn[S_KF_START[6]] == 2 and undrawn[-1] == 1
    stale = False
    for k in range(1, 7):
        f0 = S_KF_START[k]
        q = np.nonzero(last[f0] >= 0)[0]
        src = last[f0][q]
        stale |= bool((palrow[src, q] != row_of[f0][attrs[src, q] >> 2]).any())
    assert stale                                                 # on screen through a row its index no longer names
    assert ref.shape == (F, SH * 8, SW * 8)


@pytest.mark.parametrize("pass_items, index_bytes", [(2 * SQ, 0), (0, 2 * SQ * 8), (2 * SQ, 2 * SQ * 8)])
def test_strided_checkpoints_and_pass_boundaries(gpu, sparse, pass_items, index_bytes):
    """Two-frame passes, a two-row index (checkpoints at keyframes 3 and 6 only), and both: every seek(f) + play, and a
    shuffled frames() with repeats, equal the test player."""
    data, _, ref = sparse
    F = ref.shape[0]
    lib = gpu.load()
    rng = np.random.default_rng(pass_items + index_bytes)
    with gtm.Stream(data) as st:
        want_und = list(st.frame_flags()[2])
        try:
            assert lib.tiler_debug_gtm_seek(pass_items, index_bytes) == 0
            for f in list(rng.permutation(F + 1)):
                st.seek(int(f))
                rgb, undrawn = st.play(layout="raster")
                assert np.array_equal(rgb, ref[f:]), f"seek({f})"
                assert list(undrawn) == want_und[f:]
            idx = np.concatenate([rng.permutation(F), rng.integers(0, F, 9)])
            rng.shuffle(idx)
            raster, undrawn = st.frames(idx, "raster")
            assert np.array_equal(raster, ref[idx]) and list(undrawn) == [want_und[i] for i in idx]
            tiles, _ = st.frames(idx, "tiles", chunk=5)
            assert np.array_equal(tiles, _tiled(ref[idx], SW, SH))
            for f in (15, 12, 9, 1):
                assert np.array_equal(st.frame(f, "raster"), ref[f])
        finally:
            assert lib.tiler_debug_gtm_seek(0, 0) == 0


# ---- 3. the sequential state ----------------------------------------------------------------------------------------
def test_frames_leaves_sequential_play_alone(gpu):
    c = cases.case("small")
    with gtm.Stream(c["data"]) as st:
        F = st.frames
        full, _ = st.play()
        st.rewind()
        a, _ = st.play(2)
        got, _ = st.frames([F - 1, 0])
        assert st.next_frame == 2 and np.array_equal(got, full[[F - 1, 0]])
        b, _ = st.play()
        assert np.array_equal(np.concatenate([a, b]), full) and st.next_frame == F
        # a failed frames_dev: nothing of the sequential state is disturbed
        st.seek(3)
        a, _ = st.play(2)
        with pytest.raises(TilerError, match="null"):
            st.frames_dev([1, 2], 0)
        assert st.next_frame == 5
        b, _ = st.play()
        assert np.array_equal(np.concatenate([a, b]), full[3:])
        # seek after play: back, forth, to where it stands, to the end
        for f in (1, 7, 4):
            st.seek(f)
            assert np.array_equal(st.play(1)[0], full[f:f + 1]) and st.next_frame == f + 1
        st.seek(5)
        assert np.array_equal(st.play()[0], full[5:])
        st.seek(F)
        rgb, undrawn = st.play()
        assert rgb.shape[0] == 0 and undrawn.shape == (0,) and st.next_frame == F
        st.seek(0)
        assert np.array_equal(st.play()[0], full)


# ---- 4. frames_dev --------------------------------------------------------------------------------------------------
def test_frames_dev_on_a_torch_stream(gpu):
    import torch
    c = cases.case("small")
    idx = [8, 2, 2, 5, 0]
    with gtm.Stream(c["data"]) as st:
        Q = st.positions
        want, want_und = st.frames(idx, "raster")
        out = torch.zeros((len(idx), Q * 64), dtype=torch.int32, device="cuda")
        und = torch.full((len(idx),), -1, dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            assert st.frames_dev(idx, out.data_ptr(), "raster", und.data_ptr(), stream=s.cuda_stream) == len(idx)
        s.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(want.shape), want)
        assert np.array_equal(und.cpu().numpy(), want_und) and st.next_frame == 0


# ---- 5. the Encoder -------------------------------------------------------------------------------------------------
def test_encoder_scores_held_frames_only(gpu):
    """The chain of test_gpu_gtm_play.test_encoder_chain over keyframes of 1, 2, 1, 2, 1 frames; an encoder that
    holds frames 0, 3 and 6 (keyframes 0, 2 and 4, as a DistributedEncoder rank would) verifies the whole clip's file
    and scores it from those frames alone."""
    from tiler_amd import synth
    from tiler_amd.encoder import Encoder
    from tiler_amd.frame_tiling import FT_MEDIUM
    W, H = 320, 240
    v = synth.video(51 + FT_MEDIUM, W, H, kf_frames=(1, 2, 1, 2, 1), n_palettes=8)
    e = Encoder(v)
    e.run_all(700, FT_MEDIUM, 0.2)
    data = e.save_stream(W, H, 24.0)
    own = np.arange(0, 7, 3)
    part = Encoder(v, frames=own)  # the tileset and its own rows of the tilemaps, as after the chain
    part.palpix, part.thm, part.tvm = e.palpix, e.thm, e.tvm
    part.sm = {k: a[own].copy() for k, a in e.sm.items()}
    res = part.verify_stream(data, width=W, height=H)
    assert (res["frames"], res["differing_frames"], res["differing"], res["first"]) == (3, 0, [], None)
    with gtm.Stream(data) as st:
        played = st.play()[0]
    qs = part.quality(width=W, height=H, stream=data)
    assert qs["rgb"].shape == (3, 1200, 64) and not qs["invalid"].any()
    assert np.array_equal(qs["rgb"], (played[own] & 0x00FFFFFF).astype(np.int32))
    assert e.verify_stream(data, width=W, height=H)["differing_frames"] == 0
