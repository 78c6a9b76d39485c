"""The native .gtm writer, host side (no GPU): tiler_gtm_assemble against gtm.assemble_stream on hand-made compressed
blobs, its argument checks, and the plain-C++ half (the compressor pool and the container, gtm_write.cpp) as a
stand-alone program under the host sanitizers (tools/gtm_write_check.cpp)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import tiler_amd
from tiler_amd import gtm
from tiler_amd._lib import TilerError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blobs(seed, sizes):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]


@pytest.mark.parametrize("fps", [24.0, 29.97])
@pytest.mark.parametrize("kf_start, sizes", [
    ([0, 7], [1234]),                         # KF = 1: its own rate is KFMaxBytesPerSec
    ([0, 1, 3, 8], [5000, 777, 31]),          # KF = 3: keyframe 0 is left out of KFMaxBytesPerSec
    ([0, 24, 48, 49], [13, 0, 99991]),        # an empty stream, a one-frame keyframe
])
def test_assemble_matches_python(kf_start, sizes, fps):
    comps = _blobs(len(sizes), sizes)
    want = gtm.assemble_stream(comps, kf_start, 1920, 1080, fps)
    assert gtm.assemble_stream_native(comps, kf_start, 1920, 1080, fps) == want


def test_assemble_rounding_ties():
    """FPC Round is ties-to-even: 5 bytes over 2 frames at 1 fps is 2.5 -> 2, 7 over 2 is 3.5 -> 4, 1000 * 1 / 16
    = 62.5 ms -> 62 and 1000 * 3 / 16 = 187.5 -> 188; the same fields from the Python writer."""
    for comps, kf_start, fps in (([b"12345"], [0, 2], 1.0), ([b"1234567"], [0, 2], 1.0),
                                 ([b"a", b"bcdefgh", b"ijklm"], [0, 1, 3, 5], 16.0)):
        want = gtm.assemble_stream(comps, kf_start, 64, 32, fps)
        got = gtm.assemble_stream_native(comps, kf_start, 64, 32, fps)
        assert got == want
    one = gtm.assemble_stream_native([b"12345"], [0, 2], 64, 32, 1.0)
    assert int.from_bytes(one[32:36], "little") == 2 and int.from_bytes(one[36:40], "little") == 2
    one = gtm.assemble_stream_native([b"1234567"], [0, 2], 64, 32, 1.0)
    assert int.from_bytes(one[32:36], "little") == 4
    three = gtm.assemble_stream_native([b"a", b"bcdefgh", b"ijklm"], [0, 1, 3, 5], 64, 32, 16.0)
    ms = [int.from_bytes(three[40 + 28 * k + 24:40 + 28 * k + 28], "little") for k in range(3)]
    assert ms == [0, 62, 188]
    # 7 * 16 / 2 = 56, 5 * 16 / 2 = 40; keyframe 0 (16 bytes a second) does not count
    assert int.from_bytes(three[36:40], "little") == 56


def test_assemble_size_query_and_errors():
    lib = tiler_amd.load()
    comps = _blobs(9, [40, 50])
    body = np.frombuffer(b"".join(comps), np.uint8)
    lens = np.array([40, 50], np.uint64)
    kf = np.array([0, 2, 5], np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    n = ctypes.c_size_t(0)
    assert lib.tiler_gtm_assemble(p(body), p(lens), p(kf), 2, 64, 32, 24.0, None, 0, ctypes.byref(n)) == 0
    want = gtm.assemble_stream(comps, kf, 64, 32, 24.0)
    assert n.value == len(want) == 40 + 56 + 90
    out = np.full(n.value + 8, 0xAB, np.uint8)
    n2 = ctypes.c_size_t(0)
    assert lib.tiler_gtm_assemble(p(body), p(lens), p(kf), 2, 64, 32, 24.0, p(out), n.value - 1,
                                  ctypes.byref(n2)) == -1
    assert n2.value == n.value and str(n.value) in tiler_amd.last_error() and (out == 0xAB).all()
    assert lib.tiler_gtm_assemble(p(body), p(lens), p(kf), 2, 64, 32, 24.0, p(out), n.value, ctypes.byref(n2)) == 0
    assert out[:n.value].tobytes() == want and (out[n.value:] == 0xAB).all()
    for bad_kf, fps, word in (([1, 2, 5], 24.0, "kf_start[0]"), ([0, 2, 2], 24.0, "increase"), ([0, 2, 5], 0.0, "fps")):
        with pytest.raises(TilerError, match=word.replace("[", r"\[").replace("]", r"\]")):
            gtm.assemble_stream_native(comps, bad_kf, 64, 32, fps)


def test_sanitized_standalone_writer(tmp_path):
    """tools/gtm_write_check.cpp: the compressor pool and the container with a main of their own, built with
    -fsanitize=address,undefined on the host sources only and run on the CPU; the file it writes is read back with
    the host reader."""
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
    exe = str(tmp_path / "gtm_write_check")
    srcs = [os.path.join(ROOT, "tools", "gtm_write_check.cpp")] + \
        [os.path.join(csrc, f) for f in ("lzma_alone.cpp", "lzma_dec.cpp", "gtm_read.cpp", "gtm_write.cpp")]
    objs = [str(tmp_path / (os.path.basename(f) + ".o")) for f in srcs]
    jobs = [subprocess.Popen([cxx, "-std=c++17", "-O1", *san, "-I", os.path.join(ROOT, "include"), "-c", f, "-o", o])
            for f, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0] * len(srcs)
    subprocess.run([cxx, *san, *objs, "-lpthread", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "gtm_write_check ok" in r.stdout, r.stdout + r.stderr
