"""Every tier of the exact search publishes its answer through one sink (tiler_amd/csrc/result_sink.hpp): the result
slot and, for FrameTiling, the tilemap item looked up through the handle's tr_tile / tr_pal / tr_attr maps.  A tier
whose sink misses the maps, or looks them up with the wrong candidate, still returns a plausible item, so each
delivery path is driven here with maps of distinct random values and its items are checked against the lookup of the
winner's index.

No entry point returns the index together with the item (tiler_frame_tiling returns items and distances,
ann_kdtree_search_batch indices and distances), so for every path the index is ANN's kd-tree search restated on the
host (oracle.KDTree over the oracle's own query descriptors): tile == tr_tile[idx], pal == tr_pal[idx],
hm == tr_attr[idx] & 1, vm == (tr_attr[idx] >> 1) & 1 and the distance bit for bit, for every query.  tr_tile is
injective, so the item also names the index the GPU found, and that must be the oracle's.  ann_kdtree_get_stats then
tells that the intended path ran.  Two things the stats cannot tell: the orbit rescore's own exit from its pair pass
(the orbit case reaches both: a query with more than 4 queued candidates ends in the rescore, the usual one in the
pair pass), and the small-batch merge's in-place replay, which leaves no count (the forced-replay scan case has the
switch set and must return the same items)."""
import ctypes

import numpy as np
import pytest

from tiler_amd import synth

pytestmark = pytest.mark.gpu


def _desc(oracle, rgb):
    rgb = np.ascontiguousarray(rgb, np.int32).reshape(-1, 64)
    return oracle.psyv_batch(rgb.shape[0], rgb=rgb, flags=2).astype(np.float32)


def _rows(oracle, rng, n):
    """Descriptors of n noisy tiles of random mean colour: float rows without mirror orbits, near enough to frame
    tiles that the queries' winners differ."""
    px = np.clip(rng.integers(0, 256, (n, 1, 3)) + rng.integers(-24, 25, (n, 64, 3)), 0, 255)
    return _desc(oracle, synth.rgb_pack(px[..., 0], px[..., 1], px[..., 2]))


def _plain(oracle, rng):
    """2,500 candidates: no multiple of a 16- or 32-row block."""
    return _rows(oracle, rng, 2500), synth.frame_tiles(rng, 300)


def _copies(copies):
    """700 such rows and `copies` identical ones, the descriptor of the first query tile: every lane list
    fills with that distance (tier 2: 300 copies; 1,500 overflow the tier-2 buffer too: tier 3)."""
    def make(oracle, rng):
        q = synth.frame_tiles(rng, 100)
        q[0] = rng.integers(0, 1 << 24, 64)  # textured: no mirror of it equals it
        data = np.concatenate([_rows(oracle, rng, 700), np.repeat(_desc(oracle, q[:1]), copies, 0)])
        return data, q
    return make


def _orbit(dups):
    """A keyframe dataset in its 4 orientations (mirror orbits); dups: that many tiles repeat tile 0, whose rendering
    is the first query (equal-distance groups larger than the shortlist's lists: orbit tier 2)."""
    def make(oracle, rng):
        T = 600
        tiles, thm, tvm = synth.tileset(rng, T)
        if dups:
            tiles[T - dups:], thm[T - dups:], tvm[T - dups:] = tiles[0], thm[0], tvm[0]
        pals = synth.palettes(rng, 2)
        used = np.zeros((2, T, 4), np.uint8)
        used[0] = 1
        ods = oracle.build_ft_dataset(used, tiles, thm, tvm, pals)[0]
        q = synth.frame_tiles(rng, 300)
        q[0] = pals[0][tiles[0].astype(np.int64)]
        return np.ascontiguousarray(ods, np.float32), q
    return make


def _shortlist(st):  # the MFMA shortlist ran (not the scan, not the k > 8 exhaustive kernel)
    return st["splits"] > 0


def _scan(st):  # the small-batch scan ran: no shortlist, and no query left to the exhaustive kernel
    return st["splits"] == 0 and st["fallback_queries"] + st["exhaustive_queries"] == 0


CASES = {
    # name: (dataset and query tiles, queries searched (<= 64: the small-batch scan), forced replay, what the stats
    # must show)
    "generic-rescore": (_plain, 300, 0, lambda st, nq: _shortlist(st) and st["orbit_search"] == 0 and
                        st["fallback_queries"] + st["exhaustive_queries"] < nq),
    "generic-tier2": (_copies(300), 100, 0, lambda st, nq: _shortlist(st) and st["orbit_search"] == 0 and
                      st["fallback_queries"] >= 1),
    "generic-tier3": (_copies(1500), 100, 0, lambda st, nq: _shortlist(st) and st["orbit_search"] == 0 and
                      st["exhaustive_queries"] >= 1),
    "scan": (_plain, 37, 0, lambda st, nq: _scan(st)),
    "scan-forced-replay": (_plain, 37, 1, lambda st, nq: _scan(st)),
    "orbit-rescore-and-pairs": (_orbit(0), 300, 0, lambda st, nq: st["orbit_search"] == 1 and st["orbit_groups"] > 0 and
                                st["fallback_queries"] + st["exhaustive_queries"] < nq),
    "orbit-tier2": (_orbit(300), 300, 0, lambda st, nq: st["orbit_search"] == 1 and
                    st["fallback_queries"] + st["exhaustive_queries"] >= 1),
    "kd-replay": (_plain, 300, 1, lambda st, nq: _shortlist(st) and st["kd_replayed"] == nq),
}


@pytest.mark.parametrize("name", list(CASES))
def test_every_tier_delivers_through_the_maps(gpu, oracle, name):
    make, nq, force, ran = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 900)
    data, q_rgb = make(oracle, rng)
    q_rgb = np.ascontiguousarray(q_rgb[:nq], np.int32)
    n = data.shape[0]
    tr_tile = (rng.permutation(n) * 7 + 1000003).astype(np.int32)  # injective
    tr_pal = rng.integers(0, 1 << 20, n).astype(np.int32)
    tr_attr = rng.integers(0, 256, n).astype(np.uint8)  # the bits above H and V must not leak into the flags
    okd = oracle.KDTree(data)
    oi, oe = okd.search_batch(_desc(oracle, q_rgb))
    okd.close()
    oi = oi.reshape(-1)

    lib = gpu.load()
    v = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    tile, pal = np.full(nq, -7, np.int32), np.full(nq, -7, np.int32)
    hm, vm, err = np.full(nq, 9, np.uint8), np.full(nq, 9, np.uint8), np.zeros(nq, np.float32)
    try:
        assert lib.tiler_debug_force_replay(force) == 0
        with gpu.KDTree(data) as kdt:
            assert lib.tiler_ft_set_maps(kdt.handle, v(tr_tile), v(tr_pal), v(tr_attr)) == 0
            rc = lib.tiler_frame_tiling(kdt.handle, v(q_rgb), nq, 1, -1, v(tile), v(pal), v(hm), v(vm), v(err))
            assert rc == 0, gpu.last_error()
            st = kdt.stats()
    finally:
        lib.tiler_debug_force_replay(0)

    assert np.array_equal(tile, tr_tile[oi]), f"{np.count_nonzero(tile != tr_tile[oi])} of {nq} tiles differ"
    assert np.array_equal(pal, tr_pal[oi])
    assert np.array_equal(hm, tr_attr[oi] & 1)
    assert np.array_equal(vm, (tr_attr[oi] >> 1) & 1)
    assert np.array_equal(err.view(np.uint32), oe.reshape(-1).view(np.uint32))
    assert st["tie_order"] == 0 and ran(st, nq), (name, st)
