"""CPU tests of the GlobalTiling reload branch (ReloadPreviousTiling main.pas:4372-4470): the .gts file format,
PalSigni, and the plain restatement of the matching step that the GPU tests (test_gpu_reload.py) compare with.

The restatement is written here from the reference text alone (loops, pyoracle.km_get_min for the argmin) and shares
no code with tiler_amd.global_tiling; a 40-tile case worked out by hand pins it."""
import numpy as np

from tiler_amd import global_tiling as gt


# ---- the restatement (also imported by test_gpu_reload.py) ----
def dataset_line(tile, palsize):
    """WriteTileDatasetLine + GetTilePalZoneThres (main.pas:4142-4183) of one tile: (line [80], PalSigni)."""
    acc = [0] * 64
    for b in tile:
        z = int(b) * 16 // palsize
        if z < 64:  # the reference's acc has 64 entries; only the first 16 are read
            acc[z] += 1
    line = np.zeros(80, np.uint8)
    line[:64] = tile
    signi = 64
    for z in range(16):
        signi = min(signi, 64 - acc[z])
        line[64 + z] = 1 if acc[z] > palsize // 16 else 0
    return line, signi


def parse_gts(data, palsize):
    """main.pas:4420-4438: (rescaled rows [n][64], file palette size)."""
    data = bytes(data)
    n = len(data) // 64
    file_palsize, off = 64, 0
    if len(data) % 64:
        file_palsize, off = data[0], 1
    raw = np.frombuffer(data, np.uint8, n * 64, off).reshape(n, 64).astype(np.int64)
    return ((raw * palsize) // file_palsize).astype(np.uint8), file_palsize


def restate_match(oracle, palpix, active, rows64, palsize):
    """DoFindBest (main.pas:4377-4410) over every tile against the loaded, rescaled rows: (palpix, idx, dis)."""
    n = rows64.shape[0]
    lines = np.zeros((n, 80), np.uint8)
    buckets = {}
    for i in range(n):
        lines[i], s = dataset_line(rows64[i], palsize)
        buckets.setdefault(s, []).append(i)
    buckets = {s: np.array(b) for s, b in buckets.items()}
    out = np.array(palpix, np.uint8, copy=True).reshape(-1, 64)
    idx = np.full(out.shape[0], -1, np.int32)
    dis = np.full(out.shape[0], np.iinfo(np.uint64).max, np.uint64)
    for i in range(out.shape[0]):
        if not active[i]:
            continue
        line, s = dataset_line(out[i], palsize)
        if s in buckets:
            j, d = oracle.km_get_min(lines[buckets[s]], line)
            j = int(buckets[s][j])
        else:
            j, d = oracle.km_get_min(lines, line)
        idx[i], dis[i] = j, d
        out[i] = lines[j, :64]
    return out, idx, dis


def restate_reload(oracle, palpix, active, use_count, data, palsize):
    """ReloadPreviousTiling: the match, then MakeTilesUnique over all tiles."""
    rows64, _ = parse_gts(data, palsize)
    pp, idx, dis = restate_match(oracle, palpix, active, rows64, palsize)
    pp, act, uc, mi = oracle.make_tiles_unique(pp, active, use_count)
    return pp, act, uc, mi, idx, dis


# ---- file format ----
def test_tileset_round_trip():
    rng = np.random.default_rng(1)
    palpix = rng.integers(0, 16, (37, 64)).astype(np.uint8)
    active = (rng.random(37) < 0.7).astype(np.uint8)
    data = gt.write_tileset(palpix, active, 16)
    assert len(data) == 1 + 64 * int(active.sum()) and data[0] == 16  # the header byte, active tiles only
    rows, fps = gt.read_tileset(data, 16)
    assert fps == 16 and np.array_equal(rows, palpix[active.astype(bool)])  # in index order
    r2, f2 = parse_gts(data, 16)
    assert f2 == 16 and np.array_equal(r2, rows)


def test_headerless_file_is_palette_size_64():
    rng = np.random.default_rng(2)
    raw = rng.integers(0, 64, (5, 64)).astype(np.uint8)
    rows, fps = gt.read_tileset(raw.tobytes(), 64)
    assert fps == 64 and np.array_equal(rows, raw)
    # a 16-colour clip reading the 64-colour file: (v * 16) div 64
    rows, fps = gt.read_tileset(raw.tobytes(), 16)
    assert fps == 64 and np.array_equal(rows, raw // 4) and rows.max() < 16
    assert np.array_equal(parse_gts(raw.tobytes(), 16)[0], rows)


def test_rescale_is_kept_as_a_byte():
    # (v * palsize) div file_palsize stored back into a byte: 255 * 64 div 16 = 1020 -> 252
    data = bytes([16]) + bytes([255] * 64)
    rows, fps = gt.read_tileset(data, 64)
    assert fps == 16 and (rows == (1020 & 255)).all()


# ---- PalSigni ----
def test_pal_signi_known_tiles():
    flat = np.full(64, 7, np.uint8)
    assert gt.pal_signi(flat)[0] == 0
    t = np.array([2] * 40 + [9] * 14 + [15] * 10, np.uint8)  # zone counts 40 / 14 / 10 -> 64 - 40
    assert gt.pal_signi(t)[0] == 24
    # palette size 64: four indices share a zone
    t64 = np.array([0, 1, 2, 3] * 8 + [60] * 32, np.uint8)
    assert gt.pal_signi(t64, 64)[0] == 32


def test_pal_signi_and_flags_match_the_restatement():
    rng = np.random.default_rng(3)
    for palsize in (16, 64, 13):
        tiles = rng.integers(0, palsize, (50, 64)).astype(np.uint8)
        tiles[:10] = rng.integers(0, 3, (10, 64))  # few colours: large zone counts
        sg = gt.pal_signi(tiles, palsize)
        lines = gt.write_tile_dataset_line(tiles, palsize)
        for i in range(50):
            line, s = dataset_line(tiles[i], palsize)
            assert s == sg[i] and np.array_equal(line, lines[i])


# ---- the step restatement on a case worked out by hand ----
def hand_case():
    half = np.array([0] * 32 + [15] * 32, np.uint8)
    rows = np.stack([np.full(64, 3, np.uint8), np.full(64, 5, np.uint8), half, half, np.full(64, 9, np.uint8)])
    tiles = np.zeros((40, 64), np.uint8)
    tiles[0:10] = 4                                        # PalSigni 0: rows 0, 1, 4
    tiles[10:20] = np.array([2] * 48 + [7] * 16, np.uint8)  # PalSigni 16: no such row -> the whole set
    tiles[20:30] = half                                    # PalSigni 32: rows 2 and 3, both at 0
    tiles[30:35] = 4
    tiles[35:40] = 9
    active = np.ones(40, np.uint8)
    active[30:35] = 0
    return rows, tiles, active


def test_restatement_on_hand_worked_case(oracle):
    rows, tiles, active = hand_case()
    data = gt.write_tileset(rows, np.ones(5, np.uint8), 16)
    pp, idx, dis = restate_match(oracle, tiles, active, parse_gts(data, 16)[0], 16)
    # flat 4 against flat 3 / flat 5: 64 pixels + 2 zone flags differ (66 * 2048), |d| = 1 on bytes 0, 8 (2), on bytes
    # 1, 9 (2 * 256), on bytes 16..63 (48) and on the two flags (2): 135,732 both -> a two-way tie, the last row wins.
    # flat 9 is farther (137,980).
    assert (idx[0:10] == 1).all() and (dis[0:10] == 66 * 2048 + 2 + 512 + 48 + 2).all()
    # 48 x 2 + 16 x 7 has PalSigni 16, an empty bucket -> all rows; flat 3: 64 pixels + flags 2, 7, 3 differ (67),
    # bytes 0, 8: 2, bytes 1, 9: 512, bytes 16..47: 32, bytes 48..63: 16 * 4, flags 3 -> 137,829; flat 5 gives 138,889
    assert (idx[10:20] == 0).all() and (dis[10:20] == 67 * 2048 + 2 + 512 + 32 + 64 + 3).all()
    assert (idx[20:30] == 3).all() and (dis[20:30] == 0).all()  # rows 2 and 3 are equal: the last wins
    assert (idx[30:35] == -1).all() and np.array_equal(pp[30:35], tiles[30:35])  # inactive: skipped
    assert (idx[35:40] == 4).all() and (dis[35:40] == 0).all()
    assert (pp[0:10] == 5).all() and (pp[10:20] == 3).all() and np.array_equal(pp[20:30], tiles[20:30])
    # the tail of the step: MakeTilesUnique over all tiles (its last run keeps its last member, main.pas:2604-2605)
    pp2, act, uc, mi, idx2, _ = restate_reload(oracle, tiles, active, np.ones(40, np.int32), data, 16)
    assert np.array_equal(idx2, idx)
    assert act.sum() < active.sum() and uc[act.astype(bool)].sum() == 35  # merged, every use counted once
    g = gt.make_tiles_unique(pp, active, np.ones(40, np.int64))
    assert np.array_equal(g[0], pp2) and np.array_equal(g[1], act) and np.array_equal(g[2], uc)
