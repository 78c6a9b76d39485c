"""GTM playback, host side (no GPU): libANN.so's LZMA-alone decoder (tiler_lzma_decode) against its encoder and the
oracle's decoder, and its .gtm reader (tiler_gtm_open and the getters) against the test reader tests/gtm_read.py,
the reference's demo streams and hand-built malformed command streams.  The plain-C++ sources behind both also run
under the host sanitizers as a stand-alone program (tools/gtm_read_check.cpp)."""
import ctypes
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from gtm_cases import Z, assemble, strip_header, written_stream
from gtm_read import lzma_decode_all, read_gtm
from tiler_amd import TilerError, gtm, load

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEMO = "/root/reference/docs/demo"
PROPS = [(8, 0, 2), (3, 0, 2), (0, 4, 0), (4, 2, 4), (8, 4, 4)]


def _inputs(seed):
    rng = np.random.default_rng(seed)
    return [b"", b"\x07", bytes(100000), rng.integers(0, 256, 30000, dtype=np.uint8).tobytes(),
            rng.integers(0, 4, 100000, dtype=np.uint8).tobytes(),
            np.tile(rng.integers(0, 256, 777, dtype=np.uint8), 200).tobytes()]


def _decode_raw(comp: bytes, cap: int):
    """tiler_lzma_decode once: (rc, output or None, out_len, consumed)."""
    src = np.frombuffer(comp, np.uint8) if comp else np.zeros(1, np.uint8)
    out = np.zeros(max(cap, 1), np.uint8)
    n, used = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = load().tiler_lzma_decode(src.ctypes.data_as(ctypes.c_void_p), len(comp), out.ctypes.data_as(ctypes.c_void_p),
                                  cap, ctypes.byref(n), ctypes.byref(used))
    return rc, (out[:n.value].tobytes() if rc == 0 else None), n.value, used.value


@pytest.mark.parametrize("props", PROPS)
def test_decoder_against_encoder_and_oracle(oracle, props):
    """Every prop set and input kind of test_lzma_roundtrip, end-marker and known-size form: the product decoder
    returns the input and the consumed byte count, both equal to the oracle decoder's on the same bytes -- also
    with bytes following the stream."""
    lc, lp, pb = props
    for data in _inputs(lc * 25 + lp * 5 + pb):
        for eos in (True, False):
            comp = gtm.lzma_encode(data, lc=lc, lp=lp, pb=pb, eos=eos)
            ref, end = lzma_decode_all(oracle, comp, 0)
            assert ref == [data] and end == len(comp)
            assert gtm.lzma_decode(comp) == (data, len(comp))
            assert gtm.lzma_decode(comp + b"\x5d\x00\x00tail") == (data, len(comp))
            sizes = []
            lzma_decode_all(oracle, comp + comp, 0, sizes)
            assert sizes == [len(comp)] * 2


def test_truncation():
    """A stream cut anywhere is an error: every one of the first 64 offsets, 20 seeded later ones; both forms."""
    rng = np.random.default_rng(7)
    data = rng.integers(0, 6, 50000, dtype=np.uint8).tobytes()
    for eos in (True, False):
        comp = gtm.lzma_encode(data, eos=eos)
        cuts = list(range(64)) + [int(c) for c in rng.integers(64, len(comp), 20)]
        for c in cuts:
            rc, out, _, _ = _decode_raw(comp[:c], len(data) + 64)
            assert rc == -1 and out is None, (eos, c)
            with pytest.raises(TilerError):
                gtm.lzma_decode(comp[:c])


def test_corruption():
    """200 seeded single-byte corruptions: an error or an output that differs, and the process survives.  The
    dictionary-size field (offsets 1..4) is left alone: it only bounds the distances a stream may use, so a changed
    value that is still large enough describes the same valid stream, which every LZMA decoder decodes alike."""
    rng = np.random.default_rng(11)
    data = rng.integers(0, 6, 50000, dtype=np.uint8).tobytes()
    comp = gtm.lzma_encode(data)
    errors = 0
    for _ in range(200):
        at = int(rng.integers(0, len(comp) - 4))
        at = at + 4 if at >= 1 else at
        bad = bytearray(comp)
        bad[at] ^= int(rng.integers(1, 256))
        rc, out, _, _ = _decode_raw(bytes(bad), len(data) + 4096)
        assert rc in (0, -1, gtm.LZMA_GROW), at
        assert rc != 0 or out != data, at
        errors += rc == -1
    assert errors > 0
    assert gtm.lzma_decode(comp) == (data, len(comp))  # still working


def test_buffer_and_bomb_limits():
    data = bytes(200000)  # compresses to a few dozen bytes
    for eos in (True, False):
        comp = gtm.lzma_encode(data, eos=eos)
        assert len(comp) < 1000
        rc, _, n, _ = _decode_raw(comp, 1000)
        assert rc == gtm.LZMA_GROW and (n == len(data) if not eos else n <= 1000)
        rc, out, n, used = _decode_raw(comp, len(data))  # exactly enough
        assert (rc, out, n, used) == (0, data, len(data), len(comp))
        assert gtm.lzma_decode(comp, max_raw_bytes=len(data)) == (data, len(comp))
        with pytest.raises(TilerError, match="max_raw_bytes"):
            gtm.lzma_decode(comp, max_raw_bytes=len(data) - 1)
    # the reader's per-stream cap
    z = Z().dims(2, 1, 1).tileset(np.zeros((1, 64))).palette(0, [0xFF000000] * 16)
    for _ in range(40000):
        z.item(0).item(0).end()
    file = assemble([z.b], [0, 40000], 2, 1)
    assert len(z.b) > 200000 and len(file) < 20000
    with gtm.Stream(file) as st:
        assert st.frames == 40000
    with pytest.raises(TilerError, match="max_raw_bytes"):
        gtm.Stream(file, max_raw_bytes=100000)
    with pytest.raises(TilerError, match="max_raw_bytes"):
        gtm.Stream(strip_header(file), max_raw_bytes=100000)


def _check_against_reader(oracle, st, data, Q):
    g = read_gtm(oracle, data)
    assert (st.width, st.height, st.frame_ns, st.palsize) == (g.width, g.height, g.frame_ns, g.palsize)
    assert st.frames == len(g.frames) and st.positions == Q
    assert np.array_equal(st.tiles, g.tiles)
    raw, comp = st.stream_sizes()
    assert list(raw) == [len(s) for s in g.streams] and list(comp) == g.stream_comp
    tile, attrs, palrow = st.items()
    kf_end, skipped, undrawn = st.frame_flags()
    versions = st.palettes
    assert list(kf_end) == [f[2] for f in g.frames]
    drawn = np.zeros(Q, bool)
    for f, (items, pal, _) in enumerate(g.frames):
        skip = items[:, 0] < 0
        assert np.array_equal(tile[f] < 0, skip) and skipped[f] == skip.sum()
        assert np.array_equal(tile[f][~skip], items[~skip, 0]) and np.array_equal(attrs[f][~skip], items[~skip, 1])
        assert (palrow[f][skip] == -1).all()
        # the palette version of every drawn item holds what that palette index held at this frame
        table = np.zeros((max(pal) + 1, st.palsize), np.uint32)
        for j, rgba in pal.items():
            table[j] = np.ascontiguousarray(rgba).view(np.uint32).ravel()
        assert np.array_equal(versions[palrow[f][~skip]], table[attrs[f][~skip] >> 2])
        drawn |= ~skip
        assert undrawn[f] == Q - drawn.sum()
    # items(f0, f1) is the same rows
    t2, a2, r2 = st.items(1, 3)
    assert np.array_equal(t2, tile[1:3]) and np.array_equal(a2, attrs[1:3]) and np.array_equal(r2, palrow[1:3])
    return g


@pytest.mark.parametrize("T", [300, 70000])
def test_reader_against_test_reader(oracle, T):
    """gtm.save_stream output (the generator of test_save_stream_roundtrip: skip runs over 1,024, LongTileIdx at
    T = 70000) read by the product reader and by tests/gtm_read.read_gtm: header fields, kf_start, tiles, palette
    versions, every frame's (tile, attrs), skipped sets and end flags; the same frames without the header."""
    W, H, P = 320, 240, 6
    kf_start = [0, 3, 4, 8]
    data, c = written_stream(T, W, H, T, P, kf_start, long_run=1100)
    if T == 70000:
        assert (c["tile"][~c["sm"].astype(bool)] >= 1 << 16).any()
    with gtm.Stream(data) as st:
        g = _check_against_reader(oracle, st, data, c["Q"])
        assert st.header == {k: g.header[k] for k in ("AverageBytesPerSec", "KFMaxBytesPerSec")}
        assert (g.header["KFCount"], g.header["FrameCount"]) == (st.keyframes, st.frames) == (3, 8)
        assert list(st.kf_start) == kf_start == [k["FrameIndex"] for k in g.kfinfo] + [8]
        assert st.pal_rows == 3 * P
        full = st.items()
    bare = strip_header(data)
    with gtm.Stream(bare, threads=1) as st:
        assert st.header is None and list(st.kf_start) == kf_start
        _check_against_reader(oracle, st, bare, c["Q"])
        for a, b in zip(full, st.items()):
            assert np.array_equal(a, b)
    # the header is cross-checked against the streams
    for off, what in ((24, "KFCount"), (28, "FrameCount"), (16, "pixels")):
        bad = bytearray(data)
        bad[off] += 8
        with pytest.raises(TilerError, match=what):
            gtm.Stream(bytes(bad))
    bad = bytearray(data)
    bad[40 + 20] += 1  # the first record's CompressedSize
    with pytest.raises(TilerError):
        gtm.Stream(bytes(bad))


@pytest.mark.skipif(not os.path.isdir(DEMO), reason="reference demo streams not present")
def test_reference_demo_streams():
    """The reference encoder's own streams (headerless, lzma.exe -lc8) through the product decoder and reader."""
    golden = json.load(open(os.path.join(HERE, "golden", "gtm_demo.json")))
    for name, want in golden.items():
        data = open(os.path.join(DEMO, name), "rb").read()
        raws, pos = [], 0
        while pos < len(data):
            raw, used = gtm.lzma_decode(data[pos:])
            raws.append(raw)
            pos += used
        assert [len(r) for r in raws] == want["streams_raw_bytes"]
        assert [hashlib.sha256(r).hexdigest() for r in raws] == want["streams_sha256"]
        with gtm.load_stream(os.path.join(DEMO, name)) as st:
            raw, comp = st.stream_sizes()
            assert list(raw) == want["streams_raw_bytes"] and list(comp) == want["streams_compressed_bytes"]
            assert (st.width, st.height, st.frame_ns, st.n_tiles, st.palsize, st.frames) == \
                (want["width"], want["height"], want["frame_ns"], want["tiles"], want["palsize"], want["frames"])
            kf_end, skipped, _ = st.frame_flags()
            assert int(skipped.sum()) == want["skipped_items"] and int(kf_end.sum()) == want["keyframe_ends"]
            assert st.header is None


def _valid(z=None):
    """A 3 x 2 tilemap, 4 tiles, one palette, and (z given) the tokens of its single keyframe after that."""
    head = Z().dims(3, 2, 4).tileset(np.arange(256).reshape(4, 64) % 16).palette(0, range(0xFF000000, 0xFF000010))
    head.b += z.b if z is not None else Z().item(0).item(1).item(2).skip(2).item(3).end(1).b
    return head


def _dangling(z, cmd, *words):
    """z followed by a command word and some of its operand words."""
    z.cmd(cmd, 0)
    for w in words:
        z.word(w)
    return z


MALFORMED = {
    "FrameEnd with an incomplete tilemap": lambda: Z().item(0).item(1).item(2).item(3).item(0).end(1),
    "skip past the end of the tilemap": lambda: Z().item(0).skip(6).end(1),
    "item past the end of the tilemap": lambda: Z().skip(6).item(0).end(1),
    "tile index 4 >= the tile count": lambda: Z().item(4).skip(5).end(1),
    "palette index 5 was never loaded": lambda: Z().item(0, pal=5).skip(5).end(1),
    "unknown command 17": lambda: _dangling(Z().skip(6).end(0), 17),
    "truncated token": lambda: _dangling(Z().skip(6).end(1), gtm.GT_LONG_TILE_IDX, 1),
    "second SetDimensions changes the size": lambda: Z().skip(6).end(0).dims(2, 3, 4).skip(6).end(1),
    "TileSet after the first frame": lambda: Z().skip(6).end(0).tileset(np.zeros((1, 64))).skip(6).end(1),
}


@pytest.mark.parametrize("rule", list(MALFORMED))
def test_malformed_command_streams(rule):
    """One hand-built stream per strict rule: each is refused with a message naming the rule, the frame and the
    position, with and without the header, and a valid open afterwards works."""
    z = _valid(MALFORMED[rule]())
    file = assemble([z.b], [0, 2], 3, 2)
    for data in (file, strip_header(file)):
        with pytest.raises(TilerError, match=rule) as e:
            gtm.Stream(data)
        assert "frame " in str(e.value) and "position " in str(e.value)
    with gtm.Stream(assemble([_valid().b], [0, 1], 3, 2)) as st:
        assert (st.frames, st.keyframes, st.n_tiles, st.pal_rows) == (1, 1, 4, 1)
        assert list(st.items()[0][0]) == [0, 1, 2, -1, -1, 3] and list(st.frame_flags()[2]) == [2]


def test_parsing_needs_no_device():
    """tiler_gtm_open and the getters are host code: they work where no GPU is, as tiler_lzma_encode does; only the
    play calls need the device (tests/test_gpu_gtm_play.py)."""
    with gtm.Stream(assemble([_valid().b], [0, 1], 3, 2)) as st:
        assert st.next_frame == 0 and st.positions == 6
    with pytest.raises(TilerError):
        gtm.Stream(b"")
    with pytest.raises(TilerError):
        gtm.Stream(b"GTMv" + bytes(10))


def test_sanitized_standalone_reader(tmp_path):
    """tools/gtm_read_check.cpp: the plain-C++ decoder and reader with a main of their own, built with
    -fsanitize=address,undefined and run on the CPU: its truncation and corruption sweeps end without a report."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    base = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for san in (base + ["-static-libasan"], base):  # the runtime inside the program where the compiler can
        r = subprocess.run([cxx, *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True)
        if r.returncode == 0 and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip("the compiler has no sanitizer runtime")
    csrc = os.path.join(ROOT, "tiler_amd", "csrc")
    exe = str(tmp_path / "gtm_read_check")
    srcs = [os.path.join(ROOT, "tools", "gtm_read_check.cpp")] + \
        [os.path.join(csrc, f) for f in ("lzma_alone.cpp", "lzma_dec.cpp", "gtm_read.cpp")]
    objs = [str(tmp_path / (os.path.basename(f) + ".o")) for f in srcs]
    jobs = [subprocess.Popen([cxx, "-std=c++17", "-O1", *san, "-I", os.path.join(ROOT, "include"), "-c", f, "-o", o])
            for f, o in zip(srcs, objs)]  # the four sources side by side
    assert [j.wait() for j in jobs] == [0] * 4
    subprocess.run([cxx, *san, *objs, "-lpthread", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "gtm_read_check ok" in r.stdout, r.stdout + r.stderr
