"""Regenerate the committed fixtures in tests/golden/ (run here, where /root/reference is mounted).

kmodes_asm_kat.npz  -- K-Modes dissimilarity / argmin / min-distance vectors computed by the
                       REFERENCE's own x86-64 asm (kmodes.pas:316-596, assembled by
                       oracle/build_ref_asm.sh into oracle/_ref/).  Pins the oracle on the GPU box,
                       where the reference is absent.
psyv_kat.npz        -- descriptor known-answer vectors from the oracle (regression pin; the formulas
                       themselves are checked analytically in tests/test_oracle_kats.py).
dl3_ref_kat.npz     -- DLv3 palettes computed by the REFERENCE's own dlquant/quantizer.c (built by
                       oracle/build_ref_dlquant.sh into oracle/_ref/): pixel sets as histograms and
                       the raw dl3quant palette of each at quant_to 16 / 32 / 64 and lookup_bpc 4..8,
                       plus flat-tile cases that wrap the 32-bit colour sums.  Pins oracle/palette.c
                       and palette.hip; read through tests/dl3_kat.py.
Data only: inputs and expected outputs.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import pyoracle  # noqa: E402


def kmodes_asm_kat():
    ref = pyoracle.ref_kmodes_lib()
    if ref is None:
        raise SystemExit("oracle/_ref/libkmodes_ref.so missing: run `make -C oracle` with /root/reference mounted")
    rng = np.random.default_rng(4242)
    rows_all, items, counts, best_idx, best_dis, md_in, md_out = [], [], [], [], [], [], []
    for trial in range(96):
        n = int(rng.integers(1, 40))
        mode = trial % 6
        if mode == 0:
            rows = rng.integers(0, 16, (n, 80), dtype=np.uint8)
            rows[:, 64:] = rng.integers(0, 2, (n, 16))
        elif mode == 1:
            rows = rng.integers(0, 256, (n, 80), dtype=np.uint8)
        elif mode == 2:
            rows = rng.choice(np.array([0, 1, 127, 128, 129, 255], np.uint8), (n, 80))
        elif mode == 3:
            rows = np.repeat(rng.integers(0, 16, (1, 80), dtype=np.uint8), n, 0)
        elif mode == 4:
            rows = np.full((n, 80), 255, np.uint8)
            rows[:, 1] = rng.integers(0, 256, n)
            rows[:, 9] = rng.integers(0, 256, n)
        else:
            rows = rng.integers(0, 256, (n, 80), dtype=np.uint8)
        item = rows[rng.integers(0, n)].copy() if trial % 3 == 0 else rng.integers(0, 256, 80, dtype=np.uint8)
        ptrs = (ctypes.c_void_p * n)(*[rows[i].ctypes.data for i in range(n)])
        best = ctypes.c_uint64()
        bi = ref.ref_get_min(item.ctypes.data_as(ctypes.c_void_p), ptrs, ctypes.c_uint64(n), ctypes.byref(best))
        md = np.full(n, np.iinfo(np.uint64).max, np.uint64)
        md[::2] = rng.integers(0, 70000, md[::2].size)
        md0 = md.copy()
        used = rng.integers(0, 2, n).astype(np.uint8)
        ref.ref_update_min_distance(item.ctypes.data_as(ctypes.c_void_p), ptrs, used.ctypes.data_as(ctypes.c_void_p),
                                    md.ctypes.data_as(ctypes.c_void_p), n)
        pad = np.zeros((40, 80), np.uint8)
        pad[:n] = rows
        rows_all.append(pad)
        items.append(item)
        counts.append(n)
        best_idx.append(bi)
        best_dis.append(best.value)
        m_in = np.zeros(40, np.uint64)
        m_out = np.zeros(40, np.uint64)
        m_in[:n] = md0
        m_out[:n] = md
        md_in.append(m_in)
        md_out.append(m_out)
    np.savez_compressed(os.path.join(HERE, "kmodes_asm_kat.npz"), rows=np.stack(rows_all), items=np.stack(items),
                        counts=np.array(counts, np.int32), best_idx=np.array(best_idx, np.int64),
                        best_dis=np.array(best_dis, np.uint64), md_in=np.stack(md_in), md_out=np.stack(md_out))


def psyv_kat():
    rng = np.random.default_rng(777)
    from tiler_amd import synth
    rgb = synth.frame_tiles(rng, 24)
    pp = rng.integers(0, 16, (8, 64)).astype(np.uint8)
    pal = synth.palettes(rng, 1)[0]
    flags_rgb = np.array([2, 0, 8, 2 | 16 | 32], np.int32)
    flags_pal = np.array([1 | 2, 1 | 8 | 16, 1 | 32], np.int32)
    out_rgb = np.stack([[pyoracle.psyv(rgb=t, flags=int(f)) for t in rgb] for f in flags_rgb])
    out_pal = np.stack([[pyoracle.psyv(palpix=t, pal=pal, flags=int(f)) for t in pp] for f in flags_pal])
    np.savez_compressed(os.path.join(HERE, "psyv_kat.npz"), rgb=rgb, palpix=pp, pal=pal, flags_rgb=flags_rgb,
                        flags_pal=flags_pal, out_rgb=out_rgb, out_pal=out_pal)


def _hist(px):
    """pixels [n][3] -> (distinct colours 0x00BBGGRR ascending, their counts); whole 64-pixel tiles only."""
    px = np.asarray(px, np.int64).reshape(-1, 3)
    assert px.shape[0] % 64 == 0 and px.min() >= 0 and px.max() <= 255
    col, cnt = np.unique(px[:, 0] | (px[:, 1] << 8) | (px[:, 2] << 16), return_counts=True)
    return col.astype(np.int32), cnt.astype(np.int32)


def _grid_colours(rng, n):
    """n colours in n different cells at every lookup_bpc >= 4: components 8 + 17 k (k < 15) are 17 apart, and a
    cell is at most 255 / 15 = 17 wide at bpc 4 and narrower above."""
    cells = rng.choice(15 ** 3, n, replace=False)
    return np.stack([8 + 17 * (cells % 15), 8 + 17 * (cells // 15 % 15), 8 + 17 * (cells // 225)], 1)


def _with_counts(rng, colours, tiles):
    """every colour at least once, tiles * 64 pixels in all"""
    n = colours.shape[0]
    extra = rng.multinomial(tiles * 64 - n, rng.dirichlet(np.ones(n)))
    return np.repeat(colours, 1 + extra, 0)


def _dl3_cases():
    from tiler_amd import synth
    rng = np.random.default_rng(20240)
    cases = [("one_colour", np.tile([[10, 20, 30]], (192, 1)))]
    for q in (16, 32, 64):
        cases.append((f"exact_{q}", _with_counts(rng, _grid_colours(rng, q), 4)))
        cases.append((f"exact_{q}_plus_1", _with_counts(rng, _grid_colours(rng, q + 1), 4)))
    cases.append(("fewer_5", _with_counts(rng, _grid_colours(rng, 5), 5)))
    cases.append(("two_equal_counts", np.repeat(_grid_colours(rng, 2), 96, 0)))
    # gradients with one pixel in every cell: many calc_err values tie, the strict < keeps the first
    i, j, k = np.mgrid[0:8, 0:8, 0:4]
    cases.append(("grad_1px_cells_all_bpc", np.stack([8 + 34 * i, 8 + 34 * j, 8 + 51 * k], -1)))
    first = np.array([min(v for v in range(256) if v * 127 // 255 == k) for k in range(128)])
    i, j = np.mgrid[40:72, 50:82]
    cases.append(("grad_1px_cells_bpc7", np.stack([first[i], first[j], np.full_like(i, 90)], -1)))
    v = np.arange(256)
    cases.append(("grey_ramp", np.stack([v, v, v], 1)))
    # a few dominant colours, counts in the tens of thousands (sqrtf(d) * P rounds in float), noise of +-10 round
    # them (long recount lists)
    base = rng.integers(30, 226, (4, 3))
    heavy = np.repeat(base, [30000, 41000, 23000, 52000], 0)
    noisy = base[rng.integers(0, 4, 2352)] + rng.integers(-10, 11, (2352, 3))
    cases.append(("dominant_exact_plus_noise", np.concatenate([heavy, noisy])))
    base = rng.integers(30, 226, (3, 3))
    off = np.clip(np.rint(rng.normal(0, 1.5, (92160, 3))), -10, 10).astype(np.int64)
    cases.append(("dominant_peaked_noise", base[rng.integers(0, 3, 92160)] + off))
    for n in (10, 48):  # textured / gradient / flat tiles
        t = synth.frame_tiles(rng, n).reshape(-1)
        cases.append((f"synth_{n}_tiles", np.stack([t & 255, (t >> 8) & 255, (t >> 16) & 255], 1)))
    cases.append(("noise_320", rng.integers(0, 256, (320, 3))))
    cases.append(("near_flat", np.clip(np.array([[200, 100, 50]]) + rng.integers(-1, 2, (640, 3)), 0, 255)))
    base = rng.integers(0, 256, (12, 3))
    cases.append(("clustered_12", np.clip(base[rng.integers(0, 12, 640)] + rng.integers(-6, 7, (640, 3)), 0, 255)))
    return [(name, *_hist(px)) for name, px in cases]


# flat tiles that carry a colour sum past 2^32: 263,200 tiles of 0xFFFFFF are 16,844,800 pixels, 255 each =
# 4,295,424,000 > 2^32 (the count stays below 2^31); (name, [(colour, tiles)], quant_to, bpc)
DL3_WRAP = [
    ("white_wraps", [(0xFFFFFF, 263200)], 16, 7),
    ("white_wraps_then_merges", [(0xFFFFFF, 263200), (0x3060C0, 1000)], 1, 7),  # quant_to 1: the two must merge
    ("white_wraps_among_20", [(0xFFFFFF, 263200)] + [(0x0A0B0C * (k + 1) & 0xFFFFFF, 1 + 37 * k) for k in range(20)],
     16, 7),
]


def dl3_ref_kat():
    ref = pyoracle.ref_dlquant_lib()
    if ref is None:
        raise SystemExit("oracle/_ref/libdlquant_ref.so missing: run `make -C oracle` with the reference tree present")
    sys.path.insert(0, os.path.dirname(HERE))
    import dl3_kat
    cases = _dl3_cases()
    pal = np.zeros((len(cases), len(dl3_kat.QUANT_TO), len(dl3_kat.BPC), 64), np.int32)
    for c, (name, col, cnt) in enumerate(cases):
        k = dl3_kat.Case(name, col, cnt, None)
        assert max(k.cells(b) for b in dl3_kat.BPC) < 3000, name
        for qi, q in enumerate(dl3_kat.QUANT_TO):
            for bi, b in enumerate(dl3_kat.BPC):
                pal[c, qi, bi, :q] = pyoracle.ref_dl3quant(ref, k.pixels, q, b)
        print(name, int(cnt.sum()), "pixels, cells at bpc 4..8:", [k.cells(b) for b in dl3_kat.BPC])
    wpal = np.zeros((len(DL3_WRAP), 64), np.int32)
    for w, (name, parts, q, b) in enumerate(DL3_WRAP):
        c = np.repeat(np.array([p[0] for p in parts], np.int64), [p[1] * 64 for p in parts])
        px = np.stack([c & 255, (c >> 8) & 255, (c >> 16) & 255], 1).astype(np.uint8)
        wpal[w, :q] = pyoracle.ref_dl3quant(ref, px, q, b)
        print(name, [hex(x) for x in wpal[w, :q]])
    np.savez_compressed(
        os.path.join(HERE, "dl3_ref_kat.npz"), names=np.array([c[0] for c in cases]),
        col=np.concatenate([c[1] for c in cases]), cnt=np.concatenate([c[2] for c in cases]),
        off=np.cumsum([0] + [c[1].size for c in cases]).astype(np.int64),
        quant_to=np.array(dl3_kat.QUANT_TO, np.int32), bpc=np.array(dl3_kat.BPC, np.int32), pal=pal,
        wrap_names=np.array([w[0] for w in DL3_WRAP]),
        wrap_col=np.array([p[0] for w in DL3_WRAP for p in w[1]], np.int32),
        wrap_tiles=np.array([p[1] for w in DL3_WRAP for p in w[1]], np.int32),
        wrap_off=np.cumsum([0] + [len(w[1]) for w in DL3_WRAP]).astype(np.int64),
        wrap_quant_to=np.array([w[2] for w in DL3_WRAP], np.int32),
        wrap_bpc=np.array([w[3] for w in DL3_WRAP], np.int32), wrap_pal=wpal)


if __name__ == "__main__":
    kmodes_asm_kat()
    psyv_kat()
    dl3_ref_kat()
    print("fixtures written to", HERE)
