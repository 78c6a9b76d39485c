"""LZMA match tables on the host (no GPU): tiler_lzma_match_table against a pure-Python restatement of the finder's
rule (include/tiler_ann.h) kept here, tiler_lzma_encode_table against tiler_lzma_encode byte for byte, the table
encoder's refusal of every kind of wrong entry, and the stand-alone sanitizer program (tools/lzma_table_check.cpp)."""
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
HASH_BITS, DEPTH, NICE, MAX_LEN = 18, 24, 128, 273


def py_hash(b, p):
    m = 0xFFFFFFFF
    return (((b[p] * 0x9E3779B1) & m) ^ ((b[p + 1] * 0x85EBCA77) & m) ^ ((b[p + 2] * 0xC2B2AE3D) & m)) >> (32 - HASH_BITS)


def py_table(data: bytes, dict_size: int) -> np.ndarray:
    """The rule, written out without chains: all earlier positions of the same hash, nearest first."""
    n = len(data)
    out = np.zeros(n, np.uint32)
    buckets = {}
    for p in range(n):
        if p + 3 > n:
            continue
        h = py_hash(data, p)
        lim = min(MAX_LEN, n - p)
        best, dist = 0, 0
        for q in reversed(buckets.get(h, [])[-DEPTH:]):  # at most 24, whatever their bytes
            if p - q > dict_size:
                break
            l = 0
            while l < lim and data[q + l] == data[p + l]:
                l += 1
            if l > best:
                best, dist = l, p - q - 1
                if l >= NICE or l == lim:
                    break
        if best >= 2:
            out[p] = best | dist << 9
        buckets.setdefault(h, []).append(p)
    return out


def _inputs():
    rng = np.random.default_rng(7)
    words = rng.integers(0, 8, 1500).astype("<u2")
    block = rng.integers(0, 256, 300, dtype=np.uint8)
    near = block.copy()
    near[200] ^= 0x55
    return {
        "empty": b"",
        "one": b"a",
        "two": b"ab",
        "three": b"aaa",
        "five": b"abcab",
        "equal": bytes(1000),
        "random": rng.integers(0, 256, 4096, dtype=np.uint8).tobytes(),
        "words8": words.tobytes(),                                    # deep buckets: depth matters
        "text": (b"the quick brown fox jumps over the lazy dog. " * 60)[:2500],
        "nice": block.tobytes() + bytes(10) + near.tobytes() + bytes(10) + block.tobytes(),
        "period": (rng.integers(0, 256, 700, dtype=np.uint8).tobytes() * 6)[:4000],
    }


INPUTS = _inputs()
_TABLES = {}


def host_table(name):
    if name not in _TABLES:
        _TABLES[name] = gtm.match_table(INPUTS[name])
    return _TABLES[name]


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_host_table_is_the_rule(name):
    data = INPUTS[name]
    assert len(data) <= 4096
    got = host_table(name)
    want = py_table(data, gtm.LZMA_DICT)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    ln = got & 511
    assert ((ln == 0) | ((ln >= 2) & (ln <= MAX_LEN))).all() and (got[ln == 0] == 0).all()


def test_inputs_reach_the_rule_edges():
    """The inputs above do hit what they are there for: a walk ended by the nice length with a longer match behind
    it, a bucket deeper than 24, and a match that ends at the end of the buffer."""
    t = host_table("nice")
    p = 300 + 10 + 300 + 10
    assert (t[p] & 511) == 200 and (t[p] >> 9) == 310 - 1          # the nearest copy ends the walk at 200 >= 128
    data = INPUTS["words8"]
    full = py_table(data, gtm.LZMA_DICT)
    assert max(np.bincount([py_hash(data, p) for p in range(len(data) - 2)])) > DEPTH + 1
    assert np.array_equal(host_table("words8"), full)
    t = host_table("equal")
    assert (t[1] & 511) == MAX_LEN and (t[900] & 511) == 100 and t[998] == 0 and t[999] == 0


def test_small_dictionary():
    """dict 4096: a copy at back distance exactly dict is a match, one at dict + 1 is none."""
    rng = np.random.default_rng(11)
    unit = rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()
    at, beyond = unit + unit[:50], unit + b"\x00" + unit[:50]
    t = gtm.match_table(at, 4096)
    assert (t[4096] & 511) == 50 and (t[4096] >> 9) == 4095 and np.array_equal(t, py_table(at, 4096))
    t = gtm.match_table(beyond, 4096)
    assert t[4097] == 0 and np.array_equal(t, py_table(beyond, 4096))
    assert (gtm.match_table(beyond, 8192)[4097] & 511) == 50


@pytest.mark.parametrize("lc, lp, pb", [(8, 0, 2), (3, 0, 2), (0, 2, 0)])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_table_encoder_writes_the_same_stream(name, lc, lp, pb):
    data = INPUTS[name]
    want = gtm.lzma_encode(data, lc, lp, pb)
    got = gtm.lzma_encode(data, lc, lp, pb, matches=host_table(name))
    assert got == want
    assert gtm.lzma_decode(got) == (data, len(got))
    if name == "text":
        assert gtm.lzma_encode(data, lc, lp, pb, eos=False, matches="host") == gtm.lzma_encode(data, lc, lp, pb, eos=False)


def _first_read_match(table):
    """A position whose entry the parse certainly reads: the first non-zero one (everything before it is literals)."""
    return int(np.nonzero(table)[0][0])


@pytest.mark.parametrize("kind", ["len_past_end", "dist_past_start", "dist_past_dict", "bytes_differ", "len_one",
                                  "len_274"])
def test_wrong_entries_are_refused(kind):
    data = INPUTS["text"]
    t = host_table("text").copy()
    dict_size = gtm.LZMA_DICT
    if kind == "len_past_end":
        data = data[:200]
        t = gtm.match_table(data).copy()
        p = _first_read_match(t)
        t[p] = (len(data) - p + 1) | (t[p] >> 9) << 9                           # one byte past the buffer
        assert (t[p] & 511) <= MAX_LEN
    elif kind == "dist_past_start":
        p = _first_read_match(t)
        t[p] = (t[p] & 511) | p << 9                                            # back distance p + 1
    elif kind == "dist_past_dict":
        unit = np.random.default_rng(5).integers(0, 256, 4300, dtype=np.uint8).tobytes()
        data = unit + unit[:300]                                                # a match 4,300 back
        t = gtm.match_table(data).copy()
        far = np.nonzero((t >> 9) >= 4096)[0]
        assert far.size
        t[:] = 0                                                                # literals up to one far match
        p = int(far[0])
        t[p] = gtm.match_table(data)[p]
        dict_size = 4096
    elif kind == "bytes_differ":
        p = _first_read_match(t)
        d = next(d for d in range(p) if data[p - d - 1] != data[p])
        t[p] = 2 | d << 9
    elif kind == "len_one":
        p = _first_read_match(t)
        t[p] = 1 | (t[p] >> 9) << 9
    else:
        p = _first_read_match(t)
        t[p] = 274
    with pytest.raises(TilerError, match=rf"position {p}\b"):
        gtm.lzma_encode(data, dict_size=dict_size, matches=t)
    # the same call without the bad entry goes through, and the untouched table still gives the encoder's stream
    t[p] = 0
    assert gtm.lzma_decode(gtm.lzma_encode(data, dict_size=dict_size, matches=t))[0] == data


def test_any_valid_table_decodes_to_the_input():
    """A table that is valid but not the finder's (only every third match kept, lengths cut) still gives a stream
    that decodes to the input: the checks are what makes a table safe, not where it came from."""
    data = INPUTS["text"]
    t = host_table("text").copy()
    nz = np.nonzero(t)[0]
    t[nz[::3]] = 0
    cut = nz[1::3]
    t[cut] = np.maximum(2, (t[cut] & 511) // 2) | (t[cut] >> 9) << 9
    assert gtm.lzma_decode(gtm.lzma_encode(data, matches=t))[0] == data


def test_dictionary_above_the_packing_is_refused():
    lib = tiler_amd.load()
    data = np.frombuffer(INPUTS["text"], np.uint8)
    t = np.zeros(data.size, np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    n = ctypes.c_size_t(0)
    out = np.zeros(8192, np.uint8)
    big = (1 << 21) + 1
    assert lib.tiler_lzma_match_table(p(data), data.size, big, p(t)) == -1 and "2^21" in tiler_amd.last_error()
    assert lib.tiler_lzma_encode_table(p(data), data.size, 8, 0, 2, big, 1, p(t), p(out), out.size,
                                       ctypes.byref(n)) == -1
    assert "2^21" in tiler_amd.last_error()
    # table == NULL is tiler_lzma_encode, which keeps taking any dictionary
    assert lib.tiler_lzma_encode_table(p(data), data.size, 8, 0, 2, 1 << 24, 1, None, p(out), out.size,
                                       ctypes.byref(n)) == 0
    assert out[:n.value].tobytes() == gtm.lzma_encode(INPUTS["text"], dict_size=1 << 24)
    assert lib.tiler_lzma_match_table(p(data), data.size, 1 << 21, p(t)) == 0


def test_sanitized_standalone_table_check(tmp_path):
    """tools/lzma_table_check.cpp with a main of its own, built with -fsanitize=address,undefined against
    lzma_alone.cpp (and the decoder) alone and run on the CPU."""
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
    exe = str(tmp_path / "lzma_table_check")
    srcs = [os.path.join(ROOT, "tools", "lzma_table_check.cpp"), os.path.join(csrc, "lzma_alone.cpp"),
            os.path.join(csrc, "lzma_dec.cpp")]
    objs = [str(tmp_path / (os.path.basename(f) + ".o")) for f in srcs]
    jobs = [subprocess.Popen([cxx, "-std=c++17", "-O1", "-g", *san, "-I", os.path.join(ROOT, "include"), "-c", f,
                              "-o", o]) for f, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0] * len(srcs)
    subprocess.run([cxx, *san, *objs, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "lzma_table_check ok" in r.stdout, r.stdout + r.stderr
