"""The GPU GTM player (gtm.Stream.play over play.hip) and the GPU writer paths (tiler_gtm_write over gtm_write.hip,
with the LZMA match search on the host and on the GPU) against the reference's own player: the committed digests of
tests/golden/gtm_player.json, which oracle/ref_player.js recorded from decoders/htmljs/gtm.player.js for exactly the
files tests/gtm_player_cases.py rebuilds.  Nothing here runs the driver or reads the reference tree; the host side
(tests/test_gtm_ref_player.py) holds the test player and the live driver to the same fixture."""
import ctypes

import numpy as np
import pytest

import gtm_player_cases as cases
from tiler_amd import gtm

pytestmark = pytest.mark.gpu


def _tiled(raster, W, H):
    F = raster.shape[0]
    return raster.reshape(F, H, 8, W, 8).transpose(0, 1, 3, 2, 4).reshape(F, W * H, 64)


@pytest.mark.parametrize("name", cases.NAMES)
def test_gpu_player_draws_the_reference_picture(gpu, name):
    """Raster frames, drawn a frame per call and the whole clip in one call, digested over the little-endian RGBA
    dwords' bytes (the player's R,G,B,A order): the reference player's digests frame by frame.  The tile-major layout
    is that picture re-tiled; undrawn is zero, but [5, 5, 3, 3] where positions are never drawn."""
    c, want = cases.case(name), cases.golden()["cases"][name]
    cases.check_file(name, c["data"])
    W, H, F = want["width"], want["height"], want["frames"]
    undrawn_want = cases.UNDRAWN.get(name, [0] * F)
    with gtm.Stream(c["data"]) as st:
        assert (st.width, st.height, st.frames) == (W, H, F)
        raster = None
        for chunk in (1, F):
            st.rewind()
            rgb, undrawn = st.play(layout="raster", chunk=chunk)
            assert rgb.shape == (F, H * 8, W * 8) and rgb.dtype == np.uint32
            got = cases.frame_digests(rgb.astype("<u4", copy=False))
            bad = [f for f in range(F) if got[f] != want["frame_sha256"][f]]
            assert not bad, f"case {name!r}, chunk {chunk}: frames {bad} differ from the reference player's"
            assert list(undrawn) == undrawn_want
            raster = rgb
        st.rewind()
        tiles, undrawn = st.play(layout="tiles")
        assert np.array_equal(tiles, _tiled(raster, W, H)) and list(undrawn) == undrawn_want


def _tiler_gtm_write(gpu, c):
    """tiler_gtm_write itself over host arrays: the size query, then the file."""
    lib = gpu.load()
    src, keep = gtm.gtm_source(c["palpix"], c["thm"], c["tvm"], c["kf_start"], c["pals"], c["tile"], c["pal"],
                               c["hm"], c["vm"], c["sm"], width=c["W"], height=c["H"], fps=c["fps"],
                               palsize=c["palsize"])
    n = ctypes.c_size_t(0)
    assert lib.tiler_gtm_write(ctypes.byref(src), 0, None, 0, ctypes.byref(n)) == 0, gpu.last_error()
    out = np.zeros(n.value, np.uint8)
    assert lib.tiler_gtm_write(ctypes.byref(src), 0, out.ctypes.data_as(ctypes.c_void_p), out.size,
                               ctypes.byref(n)) == 0, gpu.last_error()
    assert n.value == out.size
    return out.tobytes()


@pytest.mark.parametrize("name", sorted(cases.WRITTEN))
def test_gpu_writers_make_the_file_the_reference_played(gpu, name):
    """The written cases' inputs through save_stream_gpu with the LZMA match search on the host and on the GPU, and
    through tiler_gtm_write: each file is, by SHA-256 and length, the one the reference player decoded with its own
    lzma.js and drew."""
    c = cases.case(name)["inputs"]
    args = (c["palpix"], c["thm"], c["tvm"], c["kf_start"], c["pals"], c["tile"], c["pal"], c["hm"], c["vm"], c["sm"],
            c["W"], c["H"], c["fps"])
    cases.check_file(name, gtm.save_stream_gpu(*args, palsize=c["palsize"], gpu_matches=False),
                     "save_stream_gpu, matches on the host")
    cases.check_file(name, gtm.save_stream_gpu(*args, palsize=c["palsize"], gpu_matches=True),
                     "save_stream_gpu, matches on the GPU")
    cases.check_file(name, _tiler_gtm_write(gpu, c), "tiler_gtm_write")
