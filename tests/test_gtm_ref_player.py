"""CPU tests that pin GTM playback and the written files to the reference's own player: decoders/htmljs/gtm.player.js
over its lzma.js, run under node by oracle/ref_player.js, is the ground truth for the picture, through the committed
digests of tests/golden/gtm_player.json everywhere and through the live driver where node and the reference tree are
present.  Held to it: the files the registry rebuilds (tests/gtm_player_cases.py: the Python writer over the library's
LZMA encoder), the test player tests/gtm_read.render, which the GPU player was judged against until now, and the two
LZMA decoders.  The GPU side is tests/test_gpu_gtm_ref_player.py."""
import hashlib
import os

import pytest

import gtm_player_cases as cases
import gtm_read
from tiler_amd import gtm

DEMO = os.path.join(os.environ.get("TILER_REFERENCE", "/root/reference"), "docs", "demo")


def test_fixture_is_whole():
    """Every case of the registry, and both demo clips, with one digest per frame and no player error."""
    g = cases.golden()
    assert sorted(g["cases"]) == sorted(cases.NAMES) and sorted(g["demo"]) == sorted(cases.DEMO_CLIPS)
    for v in list(g["cases"].values()) + list(g["demo"].values()):
        assert v["errors"] == [] and len(v["frame_sha256"]) == v["frames"] > 0
        assert all(len(d) == 64 for d in v["frame_sha256"])
    assert [g["cases"][n]["frames"] for n in cases.NAMES] == [9, 9, 8, 3, 4, 5, 5, 2]
    # the cases show what they are there for: the picture changes from frame to frame, or (skip-only frames) stays
    nd = g["cases"]["never_drawn"]["frame_sha256"]
    assert nd[0] == nd[1] != nd[2] == nd[3]
    for n in ("small", "long", "pal32", "pal64", "mirrors", "palette_reload"):
        d = g["cases"][n]["frame_sha256"]
        assert len(set(d)) == len(d), n
    assert g["cases"]["small"]["frame_sha256"] == g["cases"]["small_headerless"]["frame_sha256"]


@pytest.mark.parametrize("name", cases.NAMES)
def test_file_is_the_one_the_reference_played(name):
    cases.check_file(name, cases.case(name)["data"])


@pytest.mark.parametrize("name", cases.NAMES)
def test_test_player_draws_the_reference_picture(oracle, name):
    """gtm_read.render over gtm_read.read_gtm, frame by frame, is the reference player's framebuffer."""
    c, want = cases.case(name), cases.golden()["cases"][name]
    g = gtm_read.read_gtm(oracle, c["data"])
    assert (g.width, g.height, len(g.frames)) == (want["width"], want["height"], want["frames"])
    got = cases.frame_digests(gtm_read.render(g))
    bad = [f for f in range(len(got)) if got[f] != want["frame_sha256"][f]]
    assert not bad, f"case {name!r}: frames {bad} differ from the reference player's"


@pytest.mark.parametrize("name", cases.NAMES)
def test_library_lzma_decoder_equals_oracle_decoder(oracle, name):
    """Each keyframe stream through tiler_lzma_decode (host code of the library) and through oracle/lzma_dec.c: the
    same bytes and the same compressed length.  The reference player drawing the picture that these bytes describe
    ties both to its lzma.js."""
    data = cases.case(name)["data"]
    start = int.from_bytes(data[8:12], "little") if data[:4] == b"GTMv" else 0
    sizes = []
    raws, end = gtm_read.lzma_decode_all(oracle, data, start, sizes)
    assert end == len(data) and raws
    at = start
    for raw, n in zip(raws, sizes):
        assert gtm.lzma_decode(data[at:]) == (raw, n), (name, at)
        at += n


@pytest.mark.parametrize("name", cases.NAMES)
def test_live_reference_player(oracle, name):
    """Where node and the reference tree are here: the player itself, now, gives the committed numbers."""
    r = oracle.ref_player(cases.case(name)["data"])
    if r is None:
        pytest.skip("no node or no reference tree here: the committed fixture pins the reference player")
    want = cases.golden()["cases"][name]
    assert r["errors"] == want["errors"] == []
    assert (r["frames"], r["width"], r["height"]) == (want["frames"], want["width"], want["height"])
    assert r["frame_sha256"] == want["frame_sha256"]


@pytest.mark.skipif(not os.path.isdir(DEMO), reason="reference demo streams not present")
@pytest.mark.parametrize("name", cases.DEMO_CLIPS)
def test_test_player_on_the_demo_clips(oracle, name):
    """The reference encoder's own clips: the test player's frames are the reference player's, frame by frame."""
    want = cases.golden()["demo"][name]
    with open(os.path.join(DEMO, name), "rb") as f:
        data = f.read()
    assert (len(data), cases.file_sha256(data)) == (want["file_bytes"], want["file_sha256"])
    frames = gtm_read.render(gtm_read.read_gtm(oracle, data))
    assert cases.frame_digests(frames) == want["frame_sha256"]
    assert hashlib.sha256(frames.tobytes()).hexdigest() == want["clip_sha256"]
