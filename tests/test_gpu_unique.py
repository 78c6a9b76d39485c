"""GPU tests of MakeTilesUnique (tiler_amd/csrc/unique.hip): all four outputs of tiler_make_tiles_unique against
oracle.make_tiles_unique (or_make_tiles_unique, the restatement of main.pas:2555-2612) bit for bit -- the last-member
quirk, the full 64-byte compare, forced hash collisions, segments -- and the Encoder chain with gpu_unique on."""
import ctypes

import numpy as np
import pytest

from tiler_amd import global_tiling as gt
from tiler_amd import synth
from tiler_amd._lib import TilerError

pytestmark = pytest.mark.gpu

NAMES = ("palpix", "active", "use_count", "merge_index")


def proto_tiles(seed, T, protos, inactive=0.1):
    """T 4-bit tiles drawn from `protos` prototypes, a share of them inactive (copies of active ones among them),
    UseCount 1..1000."""
    rng = np.random.default_rng(seed)
    P = rng.integers(0, 16, (protos, 64)).astype(np.uint8)
    pp = P[rng.integers(0, protos, T)]
    act = (rng.random(T) >= inactive).astype(np.uint8)
    uc = rng.integers(1, 1001, T).astype(np.int64)
    return pp, act, uc


def oracle_segments(oracle, pp, act, uc, seg_off=None):
    """oracle.make_tiles_unique on every segment by itself; merge_index in whole-list indices."""
    T = pp.shape[0]
    seg_off = [0, T] if seg_off is None else list(seg_off)
    opp, oact = pp.copy(), act.copy()
    ouc, omi = np.asarray(uc, np.int64).copy(), np.full(T, -1, np.int64)
    for a, b in zip(seg_off[:-1], seg_off[1:]):
        p, c, u, m = oracle.make_tiles_unique(pp[a:b], act[a:b], uc[a:b].astype(np.int32))
        opp[a:b], oact[a:b], ouc[a:b] = p, c, u
        omi[a:b] = np.where(m >= 0, m.astype(np.int64) + a, -1)
    return opp, oact, ouc, omi


def assert_same(got, want):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, name
        if name in ("use_count", "merge_index"):
            assert np.array_equal(g.astype(np.int64), w.astype(np.int64)), name  # compared as integers
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), name


def check_oracle(oracle, pp, act, uc, seg_off=None):
    got = gt.make_tiles_unique_gpu(pp, act, uc, seg_off)
    assert_same(got, oracle_segments(oracle, pp, act, uc, seg_off))
    return got


@pytest.fixture(scope="module")
def case1():
    return proto_tiles(101, 5000, 700)


# ---- 1. random duplicates ----
def test_random_duplicates(gpu, oracle, case1):
    pp, act, uc = case1
    on = act.astype(bool)
    keys = {bytes(t) for t in pp[on]}
    assert 400 <= (~on).sum() <= 600 and sum(bytes(t) in keys for t in pp[~on]) >= 100
    _, gact, guc, gmi = check_oracle(oracle, pp, act, uc)
    assert (gmi >= 0).sum() >= 3000 and guc[gact.astype(bool)].sum() == uc[on].sum()
    assert np.array_equal(gact[~on], act[~on]) and (gmi[~on] == -1).all()  # inactive tiles untouched


# ---- 2. the quirk ----
def quirk_case(members, seed=7):
    """600 tiles whose byte 3 (the top byte of dword 0) is < 15, with duplicates, and `members` copies of one tile of
    byte 3 = 15: the greatest-key group.  Returns the copies' indices too."""
    pp, _, uc = proto_tiles(seed, 600, 150, 0.0)
    pp[:, 3] %= 15
    top = pp[17].copy()
    top[3] = 15
    at = np.array([590, 31, 310, 2, 455][:members])
    pp[at] = top
    return pp, np.ones(600, np.uint8), uc, np.sort(at)


@pytest.mark.parametrize("members", [1, 2, 3, 5])
def test_quirk_last_group(gpu, oracle, members):
    pp, act, uc, at = quirk_case(members)
    _, gact, guc, gmi = check_oracle(oracle, pp, act, uc)
    # the group's highest index is the sorted list's last entry and never merges; the others merge into the lowest
    assert gact[at[-1]] == 1 and gmi[at[-1]] == -1 and guc[at[-1]] == uc[at[-1]]
    assert gact[at[0]] == 1 and (gmi[at[1:-1]] == at[0]).all() and not gact[at[1:-1]].any()
    assert (gmi[at] >= 0).sum() == max(0, members - 2)  # 2 members: no merge, 3: one


@pytest.mark.parametrize("T", [0, 1, 2])
def test_quirk_tiny(gpu, oracle, T):
    for same in (False, True):
        pp = np.full((T, 64), 3, np.uint8)
        if not same:
            pp[:, 0] = np.arange(T)
        got = check_oracle(oracle, pp, np.ones(T, np.uint8), np.arange(1, T + 1, dtype=np.int64))
        assert (got[3] == -1).all() and got[1].all()  # (two identical tiles are a 2-member last group: no merge)


def test_quirk_all_identical(gpu, oracle):
    pp = np.full((300, 64), 9, np.uint8)
    uc = np.arange(1, 301, dtype=np.int64)
    _, gact, guc, gmi = check_oracle(oracle, pp, np.ones(300, np.uint8), uc)
    assert gact.sum() == 2 and gact[0] and gact[299] and (gmi[1:299] == 0).all()
    assert guc[0] == uc[:299].sum() and guc[299] == 300


def test_quirk_all_inactive(gpu, oracle):
    pp, _, uc = proto_tiles(8, 400, 50)
    got = check_oracle(oracle, pp, np.zeros(400, np.uint8), uc)
    assert np.array_equal(got[0], pp) and (got[3] == -1).all()


def test_quirk_greatest_key_inactive(gpu, oracle):
    """The greatest key belongs to inactive tiles: the last entry is the greatest ACTIVE tile."""
    pp, act, uc, at = quirk_case(3)
    act[at] = 0
    pp[:, 2] %= 15
    second = pp[17].copy()
    second[:4] = (15, 15, 15, 14)  # below the inactive copies (byte 3 = 15), above every other tile
    pp[[40, 200, 577]] = second  # the greatest active key, three times
    _, gact, _, gmi = check_oracle(oracle, pp, act, uc)
    assert gmi[200] == 40 and gmi[577] == -1 and gact[577] == 1 and (gmi[at] == -1).all()


# ---- 3. full-key compare ----
def test_full_key_compare(gpu, oracle):
    rng = np.random.default_rng(9)
    pp = rng.integers(0, 16, (400, 64)).astype(np.uint8)  # distinct tiles
    uc = rng.integers(1, 1001, 400).astype(np.int64)
    pp[350:360] = pp[100:110]  # and ten true duplicates
    pairs = []
    for k, (byte, bit) in enumerate([(63, 1), (0, 1), (7 * 4 + 2, 16), (63, 128), (0, 128), (7 * 4, 1)]):
        a, b = 10 + 2 * k, 300 + 7 * k
        pp[b] = pp[a]
        pp[b, byte] ^= bit  # differ only in byte 63, only in byte 0, or only in one bit of dword 7
        pairs.append((a, b))
    _, gact, _, gmi = check_oracle(oracle, pp, np.ones(400, np.uint8), uc)
    assert (gmi >= 0).sum() >= 9
    for a, b in pairs:
        assert gact[a] and gact[b] and gmi[a] == -1 and gmi[b] == -1


def test_dword_order_not_byte_order(gpu, oracle):
    """Two keys whose dword order and byte order disagree: bytes 2, 3 of dword 0 are (0x00, 0x01) in A and (0x01, 0x00)
    in B, so A > B as little-endian dwords and A < B as bytes.  The last entry must be A's highest index."""
    pp, _, uc = proto_tiles(10, 300, 80, 0.0)
    pp[:, 2:4] = 0  # every other tile's dword 0 is below both
    A, B = pp[0].copy(), pp[0].copy()
    A[2:4] = (0, 1)
    B[2:4] = (1, 0)
    ia, ib = [20, 150, 260], [5, 90, 299]
    pp[ia], pp[ib] = A, B
    _, gact, _, gmi = check_oracle(oracle, pp, np.ones(300, np.uint8), uc)
    assert gmi[150] == 20 and gmi[260] == -1 and gact[260] == 1  # A: one merge, its last member left out
    assert gmi[90] == 5 and gmi[299] == 5                         # B: both merge
    # the same with the disagreement in the last dword (dword 15 is the least significant)
    pp2, _, _ = proto_tiles(11, 300, 80, 0.0)
    pp2[:, :60] = 15  # all keys equal up to dword 14
    pp2[:, 62:64] = 0
    A, B = pp2[0].copy(), pp2[0].copy()
    A[62:64] = (0, 1)
    B[62:64] = (1, 0)
    pp2[ia], pp2[ib] = A, B
    _, gact, _, gmi = check_oracle(oracle, pp2, np.ones(300, np.uint8), uc)
    assert gmi[150] == 20 and gmi[260] == -1 and gmi[90] == 5 and gmi[299] == 5


# ---- 4. forced collisions ----
@pytest.mark.parametrize("bits", [0, 3])
def test_forced_collisions(gpu, oracle, case1, bits):
    pp, act, uc = (a[:2000] for a in case1)
    want = gt.make_tiles_unique_gpu(pp, act, uc)
    assert_same(want, oracle_segments(oracle, pp, act, uc))
    lib = gpu.load()
    assert lib.tiler_debug_unique(bits) == 0
    try:
        got = gt.make_tiles_unique_gpu(pp, act, uc)
    finally:
        lib.tiler_debug_unique(-1)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert lib.tiler_debug_unique(33) == -1 and lib.tiler_debug_unique(-2) == -1


# ---- 5. segments ----
SEG_OFF = [0, 2500, 2500, 6000]  # the middle segment is empty


@pytest.fixture(scope="module")
def seg_case():
    pp, act, uc = proto_tiles(12, 6000, 900)
    act[[10, 2498, 2499, 2500, 2501, 5990]] = 1
    pp[10] = np.arange(64) % 16  # a tile of its own, with a small dword 0
    pp[10, 3] = 0
    pp[[2499, 2500, 5990]] = pp[10]  # duplicates straddle the boundaries (both lie at tile 2500)
    pp[2501] = pp[2498]
    return pp, act, uc


def test_segments(gpu, oracle, seg_case):
    pp, act, uc = seg_case
    _, gact, guc, gmi = check_oracle(oracle, pp, act, uc, SEG_OFF)
    src = np.nonzero(gmi >= 0)[0]
    assert src.size >= 3000 and np.array_equal(src < 2500, gmi[src] < 2500)  # no merge crosses a boundary
    assert gmi[2499] == 10 and gact[2500] == 1 and gmi[2500] == -1 and gmi[5990] == 2500
    assert gmi[2501] < 0 or gmi[2501] >= 2500
    # the whole list as one segment merges across: another result
    whole = check_oracle(oracle, pp, act, uc)
    assert whole[3][2500] == 10 and not np.array_equal(whole[3], gmi)
    # one segment per call equals the segments of one call
    for a, b in ((0, 2500), (2500, 6000)):
        part = gt.make_tiles_unique_gpu(pp[a:b], act[a:b], uc[a:b])
        assert np.array_equal(part[1], gact[a:b]) and np.array_equal(part[2], guc[a:b])
        assert np.array_equal(np.where(part[3] >= 0, part[3] + a, -1), gmi[a:b])


@pytest.mark.parametrize("bad", [[0, 3000, 2000, 6000], [1, 6000], [0, 5000], [0, 6001], [-1, 6000], [0, 7000, 6000]])
def test_bad_seg_off(gpu, oracle, seg_case, bad):
    pp, act, uc = seg_case
    with pytest.raises(TilerError, match="seg_off"):
        gt.make_tiles_unique_gpu(pp, act, uc, bad)
    check_oracle(oracle, pp[:500], act[:500], uc[:500], [0, 100, 500])  # and the next call is served


# ---- 6. large counts ----
def test_large_use_counts(gpu):
    pp, act, _ = proto_tiles(13, 3000, 200)
    rng = np.random.default_rng(14)
    uc = (1 << 40) + rng.integers(-1000, 1000, 3000).astype(np.int64)
    got = gt.make_tiles_unique_gpu(pp, act, uc)
    assert_same(got, gt.make_tiles_unique(pp, act, uc))  # (the oracle's UseCount is int32)
    assert got[2].dtype == np.int64 and got[2].max() > 5 << 40


# ---- 7. size ----
def test_size_and_repeatability(gpu):
    pp, act, uc = proto_tiles(15, 200_000, 20_000)
    want = gt.make_tiles_unique(pp, act, uc)
    a = gt.make_tiles_unique_gpu(pp, act, uc)
    b = gt.make_tiles_unique_gpu(pp, act, uc)
    assert_same(a, want)
    for x, y in zip(a, b):  # the result does not depend on the order threads ran in
        assert x.tobytes() == y.tobytes()


# ---- 8. the _dev entry ----
def test_dev_entry_on_side_stream(gpu, case1):
    import torch
    pp, act, uc = case1
    seg = np.array([0, 1234, 5000], np.int64)
    want = gt.make_tiles_unique_gpu(pp, act, uc, seg)
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.Stream(dev)
    assert st.cuda_stream != 0
    with torch.cuda.stream(st):
        d_pp, d_act, d_uc = (torch.from_numpy(a).to(dev) for a in (pp, act, uc))
        d_mi = torch.zeros(5000, dtype=torch.int64, device=dev)
    st.synchronize()
    vp = ctypes.c_void_p
    rc = gpu.load().tiler_make_tiles_unique_dev(vp(d_pp.data_ptr()), vp(d_act.data_ptr()), vp(d_uc.data_ptr()),
                                                vp(d_mi.data_ptr()), 5000, seg.ctypes.data_as(vp), 2,
                                                vp(st.cuda_stream))
    assert rc == 0, gpu.last_error()
    assert_same([t.cpu().numpy() for t in (d_pp, d_act, d_uc, d_mi)], want)


# ---- 9. the Encoder ----
@pytest.fixture(scope="module")
def clip():
    return synth.video(50, 160, 120, kf_frames=(30,), n_palettes=4)


def test_encoder_make_unique_step(gpu, clip):
    from tiler_amd.encoder import Encoder
    a, b = Encoder(clip), Encoder(clip, gpu_unique=True)
    assert a.palpix.shape[0] > a.tiles_per_frame * 25  # more than one chunk
    a.do_make_unique()
    b.do_make_unique()
    assert (a.active == 0).any()
    for n in ("palpix", "active", "use_count", "tile"):
        x, y = getattr(a, n), getattr(b, n)
        assert x.dtype == y.dtype and np.array_equal(x, y), n


def test_encoder_run_all(gpu, clip):
    from tiler_amd.encoder import Encoder
    from tiler_amd.frame_tiling import FT_MEDIUM
    a, b = Encoder(clip), Encoder(clip, gpu_unique=True)
    sa = a.run_all(700, FT_MEDIUM, 0.2)
    sb = b.run_all(700, FT_MEDIUM, 0.2)
    assert sorted(sa) == sorted(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and np.array_equal(sa[k], sb[k]), k
    assert a.save_stream(160, 120, 24.0) == b.save_stream(160, 120, 24.0)
