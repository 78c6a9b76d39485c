"""LZMA match tables on the GPU (lzma_match.hip): tiler_lzma_match_table_gpu / _dev against the host finder's table
(tiler_lzma_match_table; tests/test_lzma_match_host.py holds that to the rule), entry for entry, on the smallest
inputs that can still go wrong; each case asserts with numpy that its input has the property it is there for.  Then
the encoders and the .gtm writer with the search on the GPU against the ones without, byte for byte."""
import ctypes

import numpy as np
import pytest

import gtm_cases
from tiler_amd import gtm

pytestmark = pytest.mark.gpu

DICT = gtm.LZMA_DICT
HASH_BITS, DEPTH = 18, 24


def _hashes(data: bytes) -> np.ndarray:
    b = np.frombuffer(data, np.uint8).astype(np.uint64)
    h = (b[:-2] * 0x9E3779B1 ^ b[1:-1] * 0x85EBCA77 ^ b[2:] * 0xC2B2AE3D) & 0xFFFFFFFF
    return (h >> (32 - HASH_BITS)).astype(np.int64)


def _longest_over_all(data: bytes, p: int) -> int:
    """The longest match at p over every earlier position (no depth limit), at most 273."""
    n, best = len(data), 0
    for q in range(p):
        l = 0
        while l < min(273, n - p) and data[q + l] == data[p + l]:
            l += 1
        best = max(best, l)
    return best


def _cases():
    rng = np.random.default_rng(2024)
    c = {f"len{n}": bytes(rng.integers(0, 2, n, dtype=np.uint8)) for n in range(6)}
    c["len5"] = b"ababa"
    c["equal"] = bytes(1000)
    c["random"] = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    c["words8"] = rng.integers(0, 8, 10000).astype("<u2").tobytes()
    block = rng.integers(0, 256, 300, dtype=np.uint8)
    near = block.copy()
    near[200] ^= 0x55
    c["nice"] = block.tobytes() + bytes(7) + near.tobytes() + bytes(7) + block.tobytes()
    tail = rng.integers(0, 256, 500, dtype=np.uint8).tobytes()
    c["tail"] = tail + b"xyz" + tail[:100]                      # the last match runs into the end of the buffer
    return c


CASES = _cases()
_HOST = {}


def host_table(name, dict_size=DICT):
    key = (name, dict_size)
    if key not in _HOST:
        _HOST[key] = gtm.match_table(CASES[name], dict_size)
    return _HOST[key]


def _pre_len(name):
    assert len(CASES[name]) == int(name[3:])


def _pre_equal(name):
    t = host_table(name)
    ln = t & 511
    assert (ln[1:-2] == np.minimum(273, 1000 - np.arange(1, 998))).all()   # every walk ends at its first candidate
    assert (t[1:-2] >> 9 == 0).all() and np.bincount(_hashes(CASES[name])).max() > DEPTH


def _pre_random(name):
    data = CASES[name]
    h = _hashes(data)
    b = np.frombuffer(data, np.uint8).astype(np.int64)
    tri = b[:-2] << 16 | b[1:-1] << 8 | b[2:]
    order = np.argsort(h, kind="stable")
    same_h = h[order][1:] == h[order][:-1]
    assert (same_h & (tri[order][1:] != tri[order][:-1])).any()           # a bucket holds two different strings


def _pre_words8(name):
    data, t = CASES[name], host_table(name)
    h = _hashes(data)
    assert np.bincount(h).max() > DEPTH + 1                               # more than 24 predecessors (all in window)
    ps = [p for p in range(len(data) - 400, len(data) - 3) if 2 <= (t[p] & 511) < 100][:40]
    assert any(_longest_over_all(data, p) > (t[p] & 511) for p in ps)     # the depth limit changes the answer


def _pre_nice(name):
    t = host_table(name)
    p = 2 * 307
    assert (t[p] & 511) == 200 and (t[p] >> 9) == 306                     # not the exact copy 614 back (273)
    assert CASES[name][p:p + 273] == CASES[name][:273]


def _pre_tail(name):
    t = host_table(name)
    assert (t[503] & 511) == 100 and (t[550] & 511) == 53 and t[601] == 0 and t[602] == 0


PRE = {"equal": _pre_equal, "random": _pre_random, "words8": _pre_words8, "nice": _pre_nice, "tail": _pre_tail}


@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_table_is_the_host_table(gpu, name):
    PRE.get(name, _pre_len)(name)
    got = gtm.match_table(CASES[name], gpu=True)
    assert got.dtype == np.uint32 and np.array_equal(got, host_table(name))


def _dict_case(kind):
    rng = np.random.default_rng(len(kind))
    if kind == "edge":  # a copy of the first 64 bytes 4,096 after them, and another 4,097 after that one
        data = rng.integers(0, 256, 20000, dtype=np.uint8)
        data[4096:4096 + 64] = data[:64]
        data[8193:8193 + 64] = data[:64]
        return data.tobytes()
    period = int(kind[1:])
    return np.tile(rng.integers(0, 256, period, dtype=np.uint8), 20000 // period).tobytes()


@pytest.mark.parametrize("kind", ["p4000", "p5000", "edge"])
def test_small_dictionary(gpu, kind):
    """dict 4096 on 20,000 bytes: period 4,000 matches one period back, period 5,000 is out of reach (only chance
    matches of random bytes are left); "edge": back distances of exactly dict (a match) and dict + 1 (none)."""
    data = _dict_case(kind)
    want = gtm.match_table(data, 4096)
    if kind == "p4000":
        assert (want[4000:-300] == (273 | 3999 << 9)).all() and (want[:4000] & 511).max() < 8
    elif kind == "p5000":
        assert (want & 511).max() < 8 and (gtm.match_table(data, 8192)[5000:-300] == (273 | 4999 << 9)).all()
    else:
        assert (want[4096] & 511) == 64 and (want[4096] >> 9) == 4095     # back distance exactly dict
        assert (want[8193] & 511) < 8                                     # the copies are 4,097 and 8,193 back
        assert (gtm.match_table(data, 8192)[8193] & 511) == 64 and (gtm.match_table(data, 8192)[8193] >> 9) == 4096
    assert np.array_equal(gtm.match_table(data, 4096, gpu=True), want)


def _dev_tables(gpu, streams, dict_size=DICT, shift=0):
    """tiler_lzma_match_table_dev over the streams back to back, `shift` bytes into an allocation."""
    import torch
    lib = gpu.load()
    raw = b"".join(streams)
    off = np.cumsum([0] + [len(s) for s in streams]).astype(np.int64)
    d_src = torch.zeros(len(raw) + shift + 1, dtype=torch.uint8, device="cuda")
    d_src[shift:shift + len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    d_tab = torch.full((max(len(raw), 1),), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = lib.tiler_lzma_match_table_dev(ctypes.c_void_p(d_src.data_ptr() + shift), off.ctypes.data_as(ctypes.c_void_p),
                                        len(streams), dict_size, ctypes.c_void_p(d_tab.data_ptr()), None)
    assert rc >= 0, gpu.last_error()
    torch.cuda.synchronize()
    t = d_tab.cpu().numpy().view(np.uint32)[:len(raw)]
    return rc, [t[off[k]:off[k + 1]] for k in range(len(streams))]


@pytest.mark.parametrize("budget", [0, 16 * 3000, 16 * 6000])
def test_three_streams_and_batches(gpu, budget):
    """[A, empty, A], A 3,000 bytes of a small alphabet: the third table is the first, so nothing crosses a border;
    with a budget of one stream per batch (and of two) the call is split and the tables stay the same; with a budget
    below A the streams are left to the host: their tables are not written."""
    lib = gpu.load()
    A = np.random.default_rng(3).integers(0, 4, 3000, dtype=np.uint8).tobytes()
    want = gtm.match_table(A)
    assert np.count_nonzero(want) > 2900 and np.count_nonzero(gtm.match_table(A + A)[3000:] != want) > 0
    prev = lib.tiler_debug_lzma_match(budget)
    try:
        assert prev == 1 << 30
        rc, tabs = _dev_tables(gpu, [A, b"", A])
        assert rc == 0 and tabs[1].size == 0
        assert np.array_equal(tabs[0], want) and np.array_equal(tabs[2], want)
        lib.tiler_debug_lzma_match(16 * 2999)
        rc, tabs = _dev_tables(gpu, [A, b"ab", A])
        assert rc == 2 and (tabs[0] == 0x7FFFFFFF).all() and (tabs[2] == 0x7FFFFFFF).all() and (tabs[1] == 0).all()
        assert np.array_equal(gtm.match_table(A, gpu=True), want)         # the host form falls back to the host finder
    finally:
        assert lib.tiler_debug_lzma_match(0) >= 0
    assert lib.tiler_debug_lzma_match(0) == 1 << 30


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_odd_source_alignment(gpu, shift):
    names = ("nice", "tail", "words8")
    rc, tabs = _dev_tables(gpu, [CASES[n] for n in names], shift=shift)
    assert rc == 0
    for n, t in zip(names, tabs):
        assert np.array_equal(t, host_table(n)), n


def test_dictionary_above_the_packing_is_refused(gpu):
    lib = gpu.load()
    off = np.array([0, 10], np.int64)
    assert lib.tiler_lzma_match_table_dev(None, off.ctypes.data_as(ctypes.c_void_p), 1, (1 << 21) + 1, None, None) == -1
    assert "2^21" in gpu.last_error()
    with pytest.raises(gtm.TilerError, match="2\\^21"):
        gtm.match_table(b"abcabcabc", (1 << 21) + 1, gpu=True)


@pytest.mark.parametrize("name", sorted(CASES))
def test_encode_with_gpu_matches(gpu, name):
    data = CASES[name]
    assert gtm.lzma_encode(data, matches="gpu") == gtm.lzma_encode(data)


def _clip(seed, W, H, T, P, kf_start):
    _, c = gtm_cases.written_stream(seed, W, H, T, P, kf_start)
    return c


@pytest.mark.parametrize("W, H, T, P, kf_start", [(64, 40, 300, 4, [0, 5]), (72, 48, 70000, 6, [0, 3, 7])])
def test_save_stream_with_gpu_matches(gpu, W, H, T, P, kf_start):
    """save_stream_gpu(gpu_matches=True) is gtm.save_stream's file, one keyframe and two; the switch reads 0 after."""
    lib = gpu.load()
    want, c = gtm_cases.written_stream(90 + W, W, H, T, P, kf_start)
    args = (c["palpix"], c["thm"], c["tvm"], c["kf_start"], c["pals"], c["tile"], c["pal"], c["hm"], c["vm"], c["sm"],
            W, H, 30.0)
    assert gtm.save_stream_gpu(*args, gpu_matches=True) == want
    assert gtm.save_stream_gpu(*args, gpu_matches=True, threads=1) == want
    streams = gtm.keyframe_streams_gpu(*args[:10], width=W, height=H, fps=30.0, gpu_matches=True)
    assert gtm.assemble_stream(streams, c["kf_start"], W, H, 30.0) == want
    # the switch by hand around tiler_gtm_write: its previous value comes back, and it reads 0 afterwards
    assert lib.tiler_gtm_set_gpu_matches(1) == 0
    try:
        assert lib.tiler_gtm_set_gpu_matches(1) == 1
        assert gtm.save_stream_gpu(*args) == want
    finally:
        assert lib.tiler_gtm_set_gpu_matches(0) == 1
    assert lib.tiler_gtm_set_gpu_matches(0) == 0


def test_table_kernels_are_timed(gpu):
    """With the switch on, the tiler_timing_* counters hold the table kernels and the table copy."""
    lib = gpu.load()
    want, c = gtm_cases.written_stream(7, 64, 40, 300, 4, [0, 2, 4])
    lib.tiler_timing_reset()
    lib.tiler_timing_enable(1)
    try:
        got = gtm.save_stream_gpu(c["palpix"], c["thm"], c["tvm"], c["kf_start"], c["pals"], c["tile"], c["pal"],
                                  c["hm"], c["vm"], c["sm"], 64, 40, 30.0, gpu_matches=True)
        n = ctypes.c_int(0)
        for name, launches in ((b"lzma_match_hash", 1), (b"lzma_match_sort", 1), (b"lzma_match_find", 1),
                               (b"gtm_table_copy", 2)):
            assert lib.tiler_timing_get(name, ctypes.byref(n)) >= 0.0 and n.value == launches, name
    finally:
        lib.tiler_timing_enable(0)
        lib.tiler_timing_reset()
    assert got == want and lib.tiler_gtm_set_gpu_matches(0) == 0


def test_encoder_chain_with_gpu_matches(gpu):
    """Encoder.save_stream(gpu=True, gpu_matches=True) is save_stream()'s file (two keyframes)."""
    from tiler_amd import synth
    from tiler_amd.encoder import Encoder
    from tiler_amd.frame_tiling import FT_MEDIUM
    W, H = 160, 96
    e = Encoder(synth.video(77, W, H, kf_frames=(2, 2), n_palettes=4))
    e.run_all(300, FT_MEDIUM, 0.2)
    data = e.save_stream(W, H, 24.0, gpu=True, gpu_matches=True)
    assert data == e.save_stream(W, H, 24.0) and data == e.save_stream(W, H, 24.0, gpu=True)
    assert gpu.load().tiler_gtm_set_gpu_matches(0) == 0
    with pytest.raises(ValueError):
        e.save_stream(W, H, 24.0, gpu_matches=True)
