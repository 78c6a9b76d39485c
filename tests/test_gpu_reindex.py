"""GPU tests of Reindex (tiler_amd/csrc/reindex.hip): the use counts under every counting strategy (uniform and skewed
items, accumulation, out-of-range items beside guarded memory), the order against global_tiling.reindex_tiles and
oracle.reindex, the tile-list gather, the TileMap remap in both modes, the host-array forms against the _dev forms,
and the Encoder / DistributedEncoder chain with gpu_reindex on against the host chain, step by step."""
import ctypes

import numpy as np
import pytest

from tiler_amd import global_tiling as gt
from tiler_amd import synth
from tiler_amd._lib import TilerError

pytestmark = pytest.mark.gpu

STRATEGIES = [0, 1]  # tiler_debug_reindex: LDS windows, global atomics
vp = ctypes.c_void_p


@pytest.fixture
def strategy(gpu, request):
    lib = gpu.load()
    assert lib.tiler_debug_reindex(request.param) == 0
    yield request.param
    lib.tiler_debug_reindex(-1)


def want_counts(tile, nt):
    uc = np.bincount(np.asarray(tile).ravel(), minlength=nt).astype(np.int64)
    return uc, (uc > 0).astype(np.uint8)


def check_counts(tile, nt):
    uc, act = gt.use_count_gpu(tile, nt)
    wuc, wact = want_counts(tile, nt)
    assert uc.dtype == np.int64 and act.dtype == np.uint8
    assert np.array_equal(uc, wuc) and np.array_equal(act, wact), (np.asarray(tile).size, nt)


# ---- 1. counts ----
@pytest.mark.parametrize("strategy", STRATEGIES, indirect=True)
def test_counts_uniform(gpu, strategy):
    rng = np.random.default_rng(1)
    for nt in (1, 2, 255, 4096, 70_001):
        for n in (0, 1, 63, 64, 65, 1000, 100_003):
            check_counts(rng.integers(0, nt, n).astype(np.int32), nt)


def test_debug_hook_range(gpu):
    lib = gpu.load()
    assert lib.tiler_debug_reindex(2) == -1 and lib.tiler_debug_reindex(-2) == -1
    assert lib.tiler_debug_reindex(-1) == 0
    check_counts(np.random.default_rng(2).integers(0, 300, 5000).astype(np.int32), 300)  # the default choice


# ---- 2. counts under skew: more than 65,535 hits on one tile, which a 16-bit counter could not hold ----
@pytest.mark.parametrize("strategy", STRATEGIES, indirect=True)
def test_counts_skewed(gpu, strategy):
    for nt in (1, 70_001):
        check_counts(np.zeros(200_000, np.int32), nt)
        rng = np.random.default_rng(3 + nt)
        tile = rng.integers(0, nt, 200_000).astype(np.int32)
        tile[rng.permutation(200_000)[:100_000]] = nt - 1
        check_counts(tile, nt)
    # an odd and an even tile of one LDS dword, both beyond 16 bits, in one workgroup's reach and beyond
    check_counts(np.repeat(np.array([6, 7], np.int32), 150_000), 8)
    check_counts(np.tile(np.array([6, 7], np.int32), 150_000), 70_001)


# ---- 3. accumulate ----
@pytest.mark.parametrize("strategy", STRATEGIES, indirect=True)
def test_counts_accumulate(gpu, strategy):
    rng = np.random.default_rng(4)
    nt = 5000
    tile = rng.integers(0, nt // 2, 100_003).astype(np.int32)  # the upper half of the tiles stays unused
    tile[40_000:] %= nt // 4  # and the second call sees the lowest quarter alone
    a, _ = gt.use_count_gpu(tile[:40_000], nt)
    uc, act = gt.use_count_gpu(tile[40_000:], nt, use_count=a)
    wuc, wact = want_counts(tile, nt)
    assert np.array_equal(uc, wuc) and np.array_equal(act, wact)
    # active is that of the accumulated count: a tile only the first call saw stays active
    only_first = np.setdiff1d(tile[:40_000], tile[40_000:])
    assert only_first.size and act[only_first].all()
    # accumulate = 0 clears what the array held
    lib = gpu.load()
    dirty = np.full(nt, 77, np.int64)
    act2 = np.full(nt, 9, np.uint8)
    assert lib.tiler_tile_use_count(vp(tile.ctypes.data), tile.size, nt, vp(dirty.ctypes.data), vp(act2.ctypes.data),
                                    0) == 0, gpu.last_error()
    assert np.array_equal(dirty, wuc) and np.array_equal(act2, wact)
    assert lib.tiler_tile_use_count(vp(tile.ctypes.data), tile.size, nt, vp(dirty.ctypes.data), None, 1) == 0
    assert np.array_equal(dirty, 2 * wuc)  # active may be NULL


# ---- 4. bad items ----
GUARD = 4096


@pytest.mark.parametrize("strategy", STRATEGIES, indirect=True)
def test_counts_bad_items(gpu, strategy):
    import torch
    lib = gpu.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(5)
    for nt, n, at, bad in ((300, 1000, 417, -1), (300, 1000, 3, 300), (70_001, 100_003, 100_002, 70_001),
                           (70_001, 100_003, 100_002, -(1 << 31)), (1, 5, 0, 1 << 30)):
        tile = rng.integers(0, nt, n).astype(np.int32)
        tile[at] = bad
        if at > 10:
            tile[at + 1:] = -7  # later offenders do not change the one that is named
        with pytest.raises(TilerError, match=rf"item {at} is tile {bad}\b"):
            gt.use_count_gpu(tile, nt)
        # the _dev form beside guarded memory: nothing outside the nt counts and flags is written
        d_tile = torch.from_numpy(tile).to(dev)
        d_uc = torch.full((GUARD + nt + GUARD,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
        d_act = torch.full((GUARD + nt + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        rc = lib.tiler_tile_use_count_dev(vp(d_tile.data_ptr()), n, nt, vp(d_uc.data_ptr() + GUARD * 8),
                                          vp(d_act.data_ptr() + GUARD), 0, None)
        assert rc == -1 and f"item {at} is tile {bad}" in gpu.last_error()
        uc, act = d_uc.cpu().numpy(), d_act.cpu().numpy()
        for g in (uc[:GUARD], uc[GUARD + nt:]):
            assert (g == 0x5A5A5A5A5A5A5A5A).all()
        for g in (act[:GUARD], act[GUARD + nt:]):
            assert (g == 0xA5).all()
    with pytest.raises(TilerError, match="item 0 is tile 0"):  # no tile at all: every item is outside
        gt.use_count_gpu(np.zeros(3, np.int32), 0)
    check_counts(rng.integers(0, 300, 1000).astype(np.int32), 300)  # and the next call is served


def test_counts_refused_sizes(gpu):
    lib = gpu.load()
    one = np.zeros(1, np.int64)
    for n, nt in ((1 << 31, 1), (1, 1 << 31), (-1, 1), (1, -1)):
        assert lib.tiler_tile_use_count_dev(vp(one.ctypes.data), n, nt, vp(one.ctypes.data), None, 0, None) == -1
        assert "2^31" in gpu.last_error()
    uc, act = gt.use_count_gpu(np.zeros(0, np.int32), 0)
    assert uc.shape == (0,) and act.shape == (0,)


# ---- 5. the order ----
@pytest.fixture(scope="module")
def order_case():
    rng = np.random.default_rng(6)
    nt = 50_000
    active = (rng.random(nt) >= 1 / 3).astype(np.uint8)
    uc = np.ones(nt, np.int64)
    some = rng.permutation(nt)[:20_000]
    uc[some] = rng.integers(2, 300, some.size)  # a few hundred distinct counts, each shared by many tiles
    uc[rng.permutation(nt)[:50]] = rng.integers(300, 1 << 30, 50)
    active[[11, 12, 13, 14, 15]] = (1, 0, 1, 1, 1)
    uc[[11, 12, 13, 14, 15]] = (0, 1 << 30, (1 << 31) - 1, 70_000, 70_000)
    return active, uc


def test_order(gpu, oracle, order_case):
    active, uc = order_case
    on = active.astype(bool)
    assert 0.3 < 1 - on.mean() < 0.37 and (uc[on] == 1).sum() >= on.sum() / 2
    idx_map, order = gt.reindex_tiles_gpu(active, uc, return_order=True)
    assert idx_map.dtype == np.int64 and order.dtype == np.int64
    assert np.array_equal(idx_map, gt.reindex_tiles(active, uc))
    assert np.array_equal(idx_map, oracle.reindex(active, uc).astype(np.int64))
    assert order.size == on.sum() and np.array_equal(idx_map[order], np.arange(order.size))
    assert (idx_map[~on] == -1).all() and idx_map[13] == 0 and idx_map[11] == order.size - 1
    assert idx_map[15] == idx_map[14] + 1  # equal counts: by index


def test_order_edges(gpu, oracle):
    idx_map, order = gt.reindex_tiles_gpu(np.zeros(0, np.uint8), np.zeros(0, np.int64), return_order=True)
    assert idx_map.shape == (0,) and order.shape == (0,)
    idx_map, order = gt.reindex_tiles_gpu(np.zeros(777, np.uint8), np.arange(777), return_order=True)
    assert (idx_map == -1).all() and order.size == 0
    for nt in (1, 64, 1000, 70_001):  # all active, equal counts: the identity
        idx_map, order = gt.reindex_tiles_gpu(np.ones(nt, np.uint8), np.full(nt, 5, np.int64), return_order=True)
        assert np.array_equal(idx_map, np.arange(nt)) and np.array_equal(order, np.arange(nt))
    # the whole order array: -1 past n_active
    lib = gpu.load()
    act = np.array([1, 0, 1, 1], np.uint8)
    uc = np.array([3, 9, 3, 8], np.int64)
    m, o, n = np.zeros(4, np.int64), np.zeros(4, np.int64), ctypes.c_int64(-5)
    assert lib.tiler_reindex_tiles(vp(act.ctypes.data), vp(uc.ctypes.data), 4, vp(m.ctypes.data), vp(o.ctypes.data),
                                   ctypes.byref(n)) == 0, gpu.last_error()
    assert n.value == 3 and m.tolist() == [1, -1, 2, 0] and o.tolist() == [3, 0, 2, -1]
    for bad in (1 << 31, -1):
        uc = np.full(1000, 4, np.int64)
        uc[[321, 900]] = bad
        with pytest.raises(TilerError, match=rf"use_count\[321\] is {bad}\b"):
            gt.reindex_tiles_gpu(np.ones(1000, np.uint8), uc)
    assert np.array_equal(gt.reindex_tiles_gpu(act, np.array([3, 9, 3, 8])), [1, -1, 2, 0])  # the next call is served


# ---- 6. gather ----
def tile_list(seed, nt):
    rng = np.random.default_rng(seed)
    return {"palpix": rng.integers(0, 256, (nt, 64)).astype(np.uint8), "thm": rng.integers(0, 2, nt).astype(np.uint8),
            "tvm": rng.integers(0, 2, nt).astype(np.uint8),
            "dith_pal": rng.integers(-5, 1 << 20, nt).astype(np.int32),
            "use_count": rng.integers(0, 1 << 40, nt).astype(np.int64)}


@pytest.mark.parametrize("n", [0, 1, 65, 50_000])
def test_gather(gpu, n):
    nt = 60_001
    tl = tile_list(7, nt)
    order = np.random.default_rng(8).integers(0, nt, n).astype(np.int64)
    if n:
        order[0], order[-1] = nt - 1, 0
    got = gt.gather_tiles_gpu(order, **tl)
    assert len(got) == 5
    for (name, a), g in zip(tl.items(), got):
        assert g.dtype == a.dtype and np.array_equal(g, a[order]), name
    for name, a in tl.items():  # each pair alone
        (g,) = gt.gather_tiles_gpu(order, **{name: a})
        assert g.dtype == a.dtype and np.array_equal(g, a[order]), name


def test_gather_refusals(gpu):
    lib = gpu.load()
    tl = tile_list(9, 100)
    order = np.arange(50, dtype=np.int64)
    p = lambda a: vp(a.ctypes.data)  # noqa: E731
    nul = [None] * 10
    thm_out = np.zeros(50, np.uint8)
    args = list(nul)
    args[2], args[3] = p(tl["thm"]), p(tl["thm"])  # out = in
    assert lib.tiler_gather_tiles(p(order), 50, *args, 100) == -1 and "must not be the input" in gpu.last_error()
    args[3] = None  # half a pair
    assert lib.tiler_gather_tiles(p(order), 50, *args, 100) == -1 and "both arrays" in gpu.last_error()
    for at, bad in ((17, 100), (49, -1)):
        o = order.copy()
        o[at] = bad
        with pytest.raises(TilerError, match=rf"order\[{at}\] is {bad}\b"):
            gt.gather_tiles_gpu(o, **tl)
    args[3] = p(thm_out)
    assert lib.tiler_gather_tiles(p(order), 50, *args, 100) == 0, gpu.last_error()
    assert np.array_equal(thm_out, tl["thm"][:50])


# ---- 7. remap ----
def test_remap(gpu):
    rng = np.random.default_rng(10)
    nt = 70_001
    active = (rng.random(nt) >= 0.3).astype(np.uint8)
    idx_map = gt.reindex_tiles(active, rng.integers(1, 50, nt))
    assert (idx_map == -1).sum() > 10_000
    for shape in ((0,), (1,), (63,), (7, 9), (3, 33_335)):
        tile = rng.integers(0, nt, shape).astype(np.int64)
        assert tile.size == 0 or tile.size < 10 or (idx_map[tile] == -1).any()  # items point at dropped tiles
        got = gt.remap_items_gpu(tile, idx_map)
        assert got.dtype == tile.dtype and got.shape == tile.shape and np.array_equal(got, idx_map[tile])
        got = gt.remap_items_gpu(tile, idx_map, keep_unmapped=True)
        assert np.array_equal(got, np.where(idx_map[tile] >= 0, idx_map[tile], tile))
        t32 = tile.astype(np.int32)
        got = gt.remap_items_gpu(t32[..., 1:], idx_map)  # int32 in, int32 out; a view
        assert got.dtype == np.int32 and np.array_equal(got, idx_map[t32[..., 1:]])


def test_remap_merge_index_of_make_tiles_unique(gpu):
    rng = np.random.default_rng(11)
    protos = rng.integers(0, 16, (300, 64)).astype(np.uint8)
    pp = protos[rng.integers(0, 300, 4000)]
    _, act, _, mi = gt.make_tiles_unique_gpu(pp, np.ones(4000, np.uint8), np.ones(4000, np.int64))
    assert mi.dtype == np.int64 and (mi >= 0).sum() > 3000
    tile = rng.integers(0, 4000, (5, 1200)).astype(np.int64)
    got = gt.remap_items_gpu(tile, mi, keep_unmapped=True)  # FinishMergeTiles, the map applied as it came
    m = mi[tile]
    assert np.array_equal(got, np.where(m >= 0, m, tile)) and act[got].all()


def test_remap_bad_item(gpu):
    rng = np.random.default_rng(12)
    idx_map = rng.permutation(500).astype(np.int64)
    for at, bad in ((0, 500), (1233, -1), (4999, 1 << 20)):
        tile = rng.integers(0, 500, 5000).astype(np.int32)
        tile[at] = bad
        for keep in (False, True):
            with pytest.raises(TilerError, match=rf"item {at} is tile {bad}\b"):
                gt.remap_items_gpu(tile, idx_map, keep)
    tile = rng.integers(0, 500, 5000)
    assert np.array_equal(gt.remap_items_gpu(tile, idx_map), idx_map[tile])


# ---- 8. host forms = _dev forms ----
def test_dev_forms_on_side_stream(gpu, order_case):
    import torch
    lib = gpu.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.Stream(dev)
    s = vp(st.cuda_stream)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    dp = lambda t: vp(t.data_ptr())  # noqa: E731
    rng = np.random.default_rng(13)
    # counts (test 1's largest case)
    nt, n = 70_001, 100_003
    tile = rng.integers(0, nt, n).astype(np.int32)
    with torch.cuda.stream(st):
        d_tile, d_uc, d_act = up(tile), up(np.full(nt, -3, np.int64)), up(np.full(nt, 7, np.uint8))
    st.synchronize()
    assert lib.tiler_tile_use_count_dev(dp(d_tile), n, nt, dp(d_uc), dp(d_act), 0, s) == 0, gpu.last_error()
    h_uc, h_act = gt.use_count_gpu(tile, nt)
    assert np.array_equal(d_uc.cpu().numpy(), h_uc) and np.array_equal(d_act.cpu().numpy(), h_act)
    # the order (test 5's case)
    active, uc = order_case
    T = active.size
    with torch.cuda.stream(st):
        d_a, d_c = up(active), up(uc)
        d_map, d_ord = up(np.zeros(T, np.int64)), up(np.zeros(T, np.int64))
    st.synchronize()
    n_act = ctypes.c_int64(0)
    assert lib.tiler_reindex_tiles_dev(dp(d_a), dp(d_c), T, dp(d_map), dp(d_ord), ctypes.byref(n_act), s) == 0
    h_map, h_ord = gt.reindex_tiles_gpu(active, uc, return_order=True)
    assert n_act.value == h_ord.size and np.array_equal(d_map.cpu().numpy(), h_map)
    assert np.array_equal(d_ord.cpu().numpy()[:h_ord.size], h_ord) and (d_ord.cpu().numpy()[h_ord.size:] == -1).all()
    # the gather, from the order in HBM (test 6's list)
    tl = tile_list(7, T)
    m = h_ord.size
    with torch.cuda.stream(st):
        d_in = [up(a) for a in tl.values()]
        d_out = [torch.zeros((m,) + a.shape[1:], dtype=t.dtype, device=dev) for a, t in zip(tl.values(), d_in)]
    st.synchronize()
    pairs = [x for io in zip(d_in, d_out) for x in io]
    assert lib.tiler_gather_tiles_dev(dp(d_ord), m, *[dp(x) for x in pairs], T, s) == 0, gpu.last_error()
    for a, g, o in zip(tl.values(), gt.gather_tiles_gpu(h_ord, **tl), d_out):
        assert np.array_equal(o.cpu().numpy(), g) and np.array_equal(g, a[h_ord])
    assert lib.tiler_gather_tiles_dev(dp(d_ord), m, dp(d_in[0]), dp(d_in[0]), *([None] * 8), T, s) == -1
    # the remap, with the map in HBM (test 7's shapes)
    items = rng.integers(0, T, (3, 33_335)).astype(np.int32)
    for keep in (0, 1):
        with torch.cuda.stream(st):
            d_items = up(items)
        st.synchronize()
        assert lib.tiler_remap_items_dev(dp(d_items), items.size, dp(d_map), T, keep, s) == 0, gpu.last_error()
        assert np.array_equal(d_items.cpu().numpy(), gt.remap_items_gpu(items, h_map, bool(keep)))
    # arrays that start 4 bytes past a 16-byte boundary: the kernels' scalar paths
    for forced in STRATEGIES:
        assert lib.tiler_debug_reindex(forced) == 0
        try:
            rc = lib.tiler_tile_use_count_dev(vp(d_tile.data_ptr() + 4), n - 1, nt, dp(d_uc), dp(d_act), 0, s)
        finally:
            lib.tiler_debug_reindex(-1)
        assert rc == 0, gpu.last_error()
        assert np.array_equal(d_uc.cpu().numpy(), want_counts(tile[1:], nt)[0])
    with torch.cuda.stream(st):
        d_items = up(items)
    st.synchronize()
    assert lib.tiler_remap_items_dev(vp(d_items.data_ptr() + 4), items.size - 1, dp(d_map), T, 0, s) == 0
    got = d_items.cpu().numpy().ravel()
    assert got[0] == items.ravel()[0] and np.array_equal(got[1:], h_map[items.ravel()[1:]])


# ---- 9. the chain ----
DESIRED, STRENGTH = 700, 0.2
TILE_LIST = ("palpix", "thm", "tvm", "dith_pal", "use_count", "active", "tile")


def chain_video():
    return synth.video(51, 320, 240, kf_frames=(3, 3), n_palettes=8)


def run_chain(e):
    """The steps of run_all one by one: the state after each, then the smoothed maps and the file."""
    from tiler_amd.frame_tiling import FT_MEDIUM
    out = {}

    def snap(step):
        out[step] = {n: np.array(getattr(e, n), copy=True) for n in TILE_LIST}
    e.do_make_unique()
    snap("unique")
    e.do_global_tiling(DESIRED)
    snap("global")
    e.do_frame_tiling(FT_MEDIUM)
    snap("ft")
    e.do_reindex()
    snap("reindex")
    out["smooth"] = {k: np.array(a, copy=True) for k, a in e.do_smooth(STRENGTH).items()}
    out["gtm"] = e.save_stream(320, 240, 24.0)
    return out


@pytest.fixture(scope="module")
def host_chain(gpu):
    from tiler_amd.encoder import Encoder
    e = Encoder(chain_video())
    out = run_chain(e)
    out["encoder"] = e  # copied, never changed, by the tests
    return out


def assert_same_chain(got, want):
    assert list(got) == [k for k in want if k != "encoder"]
    for step in want:
        if step in ("gtm", "encoder"):
            continue
        for name, w in want[step].items():
            g = got[step][name]
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (step, name)
    assert got["gtm"] == want["gtm"]


@pytest.mark.parametrize("gpu_unique", [False, True])
def test_encoder_chain(gpu, host_chain, gpu_unique):
    from tiler_amd.encoder import Encoder
    e = Encoder(chain_video(), gpu_reindex=True, gpu_unique=gpu_unique)
    assert e.gpu_reindex and not Encoder(chain_video()).gpu_reindex
    got = run_chain(e)
    assert_same_chain(got, host_chain)
    w = host_chain["reindex"]
    assert w["palpix"].shape[0] < host_chain["ft"]["palpix"].shape[0]  # FrameTiling left tiles unused: Reindex dropped them
    assert (np.diff(w["use_count"]) <= 0).all() and host_chain["smooth"]["smoothed"].sum() > 0
    # a second Reindex after Smooth remaps the SmoothedTileMaps too
    import copy
    h = copy.deepcopy(host_chain["encoder"])
    for x in (e, h):
        x.use_count[::3] += 5  # another order
        x.reindex_tiles()
    assert np.array_equal(e.sm["tile"], h.sm["tile"]) and np.array_equal(e.tile, h.tile)
    assert np.array_equal(e.palpix, h.palpix) and np.array_equal(e.use_count, h.use_count)


def _dist_worker(rank, world, port, out, backend="gloo"):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group(backend, rank=rank, world_size=world)
    import tiler_amd
    from tiler_amd._lib import check
    from tiler_amd.encoder import DistributedEncoder
    from tiler_amd.frame_tiling import FT_MEDIUM
    check(tiler_amd.load().tiler_init(0), "tiler_init")
    e = DistributedEncoder(chain_video(), device=0, gpu_reindex=True)
    assert e.gpu_reindex
    sm = e.run_all(DESIRED, FT_MEDIUM, STRENGTH)
    data = e.save_stream(320, 240, 24.0)
    np.savez(out + f".{rank}.npz", frame_idx=e.frame_idx, gtm=np.frombuffer(data, np.uint8),
             **{n: getattr(e, n) for n in TILE_LIST}, **{"sm_" + k: a for k, a in sm.items()})
    dist.barrier()
    dist.destroy_process_group()


def test_distributed_encoder_world_1(gpu, host_chain, tmp_path):
    import socket

    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "r")
    mp.spawn(_dist_worker, args=(1, port, out), nprocs=1, join=True)
    z = np.load(out + ".0.npz")
    assert np.array_equal(z["frame_idx"], np.arange(6))
    for n in TILE_LIST:
        w = host_chain["reindex"][n]
        assert z[n].dtype == w.dtype and np.array_equal(z[n], w), n
    for k, w in host_chain["smooth"].items():
        assert np.array_equal(z["sm_" + k], w), k
    assert z["gtm"].tobytes() == host_chain["gtm"]
