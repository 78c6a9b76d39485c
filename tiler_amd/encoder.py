"""The encoder steps around the hot path, end to end (btnRunAllClick main.pas:1232-1272, steps
MakeUnique -> GlobalTiling -> FrameTiling -> Reindex -> Smooth), as host state + libANN.so calls.

`Encoder` holds what TMainForm keeps in FTiles / FFrames / FKeyFrames for these steps, as flat arrays:
  tiles    palpix [T][64] u8, thm/tvm (TTile.HMirror/VMirror), active, use_count, dith_pal
  tilemaps tile/pal/hm/vm [F][Q] (TFrame.TileMap), sm_* the SmoothedTileMap copies
  keyframes kf_start [KF+1], palettes [KF][P][palsize], centroids [KF][P][192]
Each method is the reference procedure of the same name (file:line in its docstring); the heavy parts
(K-Modes, the k=8 preselection, candidate descriptors, the FrameTiling search, Smooth) run on the GPU
through the C ABI, the rest is the reference's host bookkeeping -- MakeTilesUnique too unless the encoder is made
with gpu_unique=True (tiler_make_tiles_unique; the same result), and Reindex's counts, order and TileMap remaps
unless it is made with gpu_reindex=True (tiler_tile_use_count, tiler_reindex_tiles, tiler_gather_tiles,
tiler_remap_items; the same result), and GlobalTiling's binning, StartingPoints and merges unless it is made with
gpu_global_tiling=True (tiler_global_tiling; the same result).  SURVEY.md 8(f)-1.
"""
from __future__ import annotations

import numpy as np

from . import frame_tiling as ft
from . import global_tiling as gt
from . import gtm
from .smooth import DEFAULT_STRENGTH, smooth_keyframe
from .synth import Video, video_from_frames


def load_and_dither(frames, tm_w: int, tm_h: int, palettes_fn=None, n_palettes: int = 8, gamma: int = -1,
                    use_wavelets: bool = True, use_dl3: bool = True, pal_var: float = 0.95, palsize: int = 16) -> Video:
    """The Load and Dither steps in front of the chain on the GPU (btnLoadClick main.pas:1099-1146, btnDitherClick
    main.pas:858-914): keyframes from the inter-frame correlations, then the keyframe palettes -- PrepareDitherTiles
    (LAB descriptors + k-means -> DitheringPalIndex, PaletteCentroids), QuantizePalette (DLv3), FinishQuantizePalette
    (tiler_amd.palette); use_dl3=False takes QuantizePalette's value-at-risk path with PalVAR = pal_var (chkUseDL3
    unticked, sePalVAR / 100) -- and every tile dithered with its palette (FinishDitherTiles).  palettes_fn(k,
    frames_of_keyframe) -> [P][palsize], when given, replaces the palette generation (with the stand-in palette
    choice of synth.video_from_frames).  palsize: the tile palette size (cbxPalSize: 2, 4, 8, 16, 32 or 64)."""
    from .dither import dither_tiles
    from .keyframes import detect_keyframes
    from .palette import generate_palettes
    from .synth import video_from_dither
    frames = np.ascontiguousarray(frames, np.int32).reshape(-1, tm_w * tm_h, 64)
    kf_of, kf_start, _ = detect_keyframes(frames, tm_w, tm_h)
    if palettes_fn is not None:
        pals = np.stack([np.asarray(palettes_fn(k, frames[kf_start[k]:kf_start[k + 1]]), np.int32)
                         for k in range(kf_start.size - 1)])
        return video_from_frames(frames, kf_of, pals, dither_tiles, palsize)
    pals, cents, dith, _ = generate_palettes(frames, kf_start, n_palettes, palsize, gamma=gamma,
                                             use_wavelets=use_wavelets, use_dl3=use_dl3, pal_var=pal_var)
    return video_from_dither(frames, kf_start, pals, cents, dith, dither_tiles, palsize)


def load_and_dither_raster(images, fmt: str = "rgb24", scale=None, size=None, **kw) -> Video:
    """load_and_dither over pictures as a decoder leaves them: uint8 [F][H][W][3|4] in `fmt` ("rgb24", "bgr24",
    "bgra32", "rgba32"), tiled on the GPU as LoadFrame cuts them (tiler_amd.load.frames_to_tiles); scale= (cbxScaling)
    or size=(out_w, out_h) resizes them there first; **kw goes to load_and_dither."""
    from .load import frames_to_tiles
    frames, tm_w, tm_h = frames_to_tiles(images, fmt, scale=scale, size=size)
    return load_and_dither(frames, tm_w, tm_h, **kw)


class Encoder:
    """frames: the global frame indices this encoder holds the frames and tilemaps of (sorted, whole keyframes;
    None = all).  The tileset (palpix, flags, Active, UseCount) is always the whole clip's.  Tilemap arrays are
    [len(frames)][Q]: row r is frame frames[r]."""

    def __init__(self, v: Video, palsize: int | None = None, frames=None, gpu_unique: bool = False,
                 gpu_reindex: bool = False, gpu_global_tiling: bool = False):
        F, Q = v.frames, v.tiles_per_frame
        vsize = int(np.asarray(v.palettes).shape[-1])  # the palette size is the palettes' last dimension
        if palsize is not None and int(palsize) != vsize:
            raise ValueError(f"palsize {palsize} given, but the video's palettes have {vsize} entries")
        self.palsize = vsize
        self.gpu_unique = bool(gpu_unique)  # MakeTilesUnique on the GPU (tiler_make_tiles_unique)
        # UseCount, ReindexTiles and every TileMap remap on the GPU (tiler_tile_use_count, tiler_reindex_tiles,
        # tiler_gather_tiles, tiler_remap_items); the arrays stay numpy, as with gpu_unique
        self.gpu_reindex = bool(gpu_reindex)
        # DoGlobalTiling's plan, K-Modes, medoids and merges in one library call (tiler_global_tiling)
        self.gpu_global_tiling = bool(gpu_global_tiling)
        self.n_frames = F
        self.kf_start = np.asarray(v.kf_start, np.int64)
        own = np.arange(F) if frames is None else np.asarray(frames, np.int64)
        self.frame_idx = own
        # only the held frames are read (a memory-mapped Video pages in just these)
        self.frame_rgb = v.frame_rgb if frames is None else np.ascontiguousarray(v.frame_rgb[own])
        self.palettes = np.asarray(v.palettes, np.int32)
        self.centroids = np.asarray(v.centroids, np.float64)
        self.n_palettes = self.palettes.shape[1]
        # FTiles after Dither (LoadFrame main.pas:3226-3236 + FinishDitherTiles 2497-2519)
        self.palpix = np.array(v.palpix, np.uint8, copy=True)
        self.thm = np.array(v.thm, np.uint8, copy=True)
        self.tvm = np.array(v.tvm, np.uint8, copy=True)
        self.dith_pal = np.array(v.dith_pal, np.int32, copy=True)
        self.active = np.ones(F * Q, np.uint8)
        self.use_count = np.ones(F * Q, np.int64)
        # TileMap: GlobalTileIndex = own tile, PalIdx = DitheringPalIndex, mirrors false
        self.tile = (own[:, None] * Q + np.arange(Q, dtype=np.int64)[None, :])
        self.pal = self.dith_pal.reshape(F, Q)[own].astype(np.int64)
        self.hm = np.zeros((own.size, Q), np.uint8)
        self.vm = np.zeros((own.size, Q), np.uint8)
        self.sm = None
        # the keyframes held (every frame of each), and their first tilemap row
        self.kfs = [k for k in range(self.kf_start.size - 1)
                    if np.isin(np.arange(self.kf_start[k], self.kf_start[k + 1]), own).all()]
        self._row0 = {k: int(np.searchsorted(own, self.kf_start[k])) for k in self.kfs}
        if sum(int(self.kf_start[k + 1] - self.kf_start[k]) for k in self.kfs) != own.size:
            raise ValueError("an encoder holds whole keyframes only")

    @property
    def frames(self) -> int:
        return self.tile.shape[0]

    @property
    def tiles_per_frame(self) -> int:
        return self.tile.shape[1]

    def rows(self, k: int) -> slice:
        """Tilemap rows of keyframe k."""
        r0 = self._row0[k]
        return slice(r0, r0 + int(self.kf_start[k + 1] - self.kf_start[k]))

    # --- tile-list bookkeeping --------------------------------------------------------------------
    def finish_merge_tiles(self, merge_index):
        """FinishMergeTiles main.pas:3722-3734: TileMap items of merged tiles point at the survivor."""
        if self.gpu_reindex:
            self.tile = gt.remap_items_gpu(self.tile, merge_index, keep_unmapped=True)
            return
        m = np.asarray(merge_index, np.int64)[self.tile]
        self.tile = np.where(m >= 0, m, self.tile)

    def make_tiles_unique(self, first: int = 0, count: int | None = None):
        """MakeTilesUnique main.pas:2555-2612 over tiles [first, first+count): identical PalPixels merge
        into the lowest index (TFPList.Sort is unstable, the canonical order is stable)."""
        count = self.palpix.shape[0] - first if count is None else count
        s = slice(first, first + count)
        unique = gt.make_tiles_unique_gpu if self.gpu_unique else gt.make_tiles_unique
        pp, act, uc, mi = unique(self.palpix[s], self.active[s], self.use_count[s])
        self.palpix[s], self.active[s], self.use_count[s] = pp, act, uc
        full = np.full(self.palpix.shape[0], -1, np.int64)
        full[s] = np.where(mi >= 0, mi + first, -1)
        self.finish_merge_tiles(full)

    def reindex_tiles(self):
        """ReindexTiles main.pas:4483-4527: drop inactive tiles, order by (UseCount desc, old index asc),
        remap every TileMap."""
        if self.gpu_reindex:
            idx_map, order = gt.reindex_tiles_gpu(self.active, self.use_count, return_order=True)
            self.palpix, self.thm, self.tvm, self.dith_pal, self.use_count = gt.gather_tiles_gpu(
                order, self.palpix, self.thm, self.tvm, self.dith_pal, self.use_count)
            self.active = np.ones(order.size, np.uint8)
            self.tile = gt.remap_items_gpu(self.tile, idx_map)
            if self.sm is not None:
                self.sm["tile"] = gt.remap_items_gpu(self.sm["tile"], idx_map)
            return
        idx_map = gt.reindex_tiles(self.active, self.use_count)
        keep = np.nonzero(idx_map >= 0)[0]
        order = np.empty(keep.size, np.int64)
        order[idx_map[keep]] = keep
        self.palpix = np.ascontiguousarray(self.palpix[order])
        self.thm, self.tvm = self.thm[order], self.tvm[order]
        self.dith_pal, self.use_count = self.dith_pal[order], self.use_count[order]
        self.active = np.ones(order.size, np.uint8)
        self.tile = idx_map[self.tile]
        if self.sm is not None:
            self.sm["tile"] = idx_map[self.sm["tile"]]

    # --- steps ------------------------------------------------------------------------------------
    def do_make_unique(self):
        """btnDoMakeUniqueClick main.pas:916-938: MakeTilesUnique per chunk of FTileMapSize * 25 tiles (gpu_unique:
        every chunk a segment of one GPU call, then one combined merge_index applied to the tilemaps -- a chunk's
        merges stay inside it, so this equals the per-chunk loop)."""
        chunk = self.tiles_per_frame * 25
        T = self.palpix.shape[0]
        if self.gpu_unique:
            seg_off = np.append(np.arange(0, T, chunk, dtype=np.int64), T)
            self.palpix, self.active, self.use_count, mi = gt.make_tiles_unique_gpu(self.palpix, self.active,
                                                                                    self.use_count, seg_off)
            self.finish_merge_tiles(mi)
            return
        for first in range(0, T, chunk):
            self.make_tiles_unique(first, min(chunk, T - first))

    def do_global_tiling(self, desired: int, restart: int = gt.CRANDOM_KMODES_COUNT):
        """DoGlobalTiling main.pas:4256-4370: K-Modes merge per palette bin (GPU, all bins batched),
        FinishMergeTiles, MakeTilesUnique over all tiles, ReindexTiles."""
        step = gt.do_global_tiling_gpu if self.gpu_global_tiling else gt.do_global_tiling
        pp, act, uc, mi, kpb = step(self.palpix, self.dith_pal, self.n_palettes, desired, self.palsize, restart,
                                    self.active, self.use_count)
        self.palpix, self.active, self.use_count = pp, act, uc
        self.finish_merge_tiles(mi)
        self.make_tiles_unique()
        self.reindex_tiles()
        return kpb

    def save_tileset(self, path_or_file=None) -> bytes:
        """The .gts file DoGlobalTiling ends with (main.pas:4357-4367): the palette size and every Active tile's
        PalPixels in index order.  Valid after do_global_tiling; also written to a path or a binary file if given."""
        data = gt.write_tileset(self.palpix, self.active, self.palsize)
        if isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__"):
            with open(path_or_file, "wb") as f:
                f.write(data)
        elif path_or_file is not None:
            path_or_file.write(data)
        return data

    def do_reload_tiling(self, tileset):
        """btnDoGlobalTilingClick with chkReload (main.pas:845-850) -> ReloadPreviousTiling main.pas:4372-4470, the
        step that takes the place of do_global_tiling: every Active tile snapped to its closest tile of a saved
        tileset (.gts bytes, a path or a binary file; matched on the GPU), then MakeTilesUnique over all tiles.  No
        K-Modes and no ReindexTiles.  Returns the per-tile (idx, dis) of the match."""
        if isinstance(tileset, str) or hasattr(tileset, "__fspath__"):
            with open(tileset, "rb") as f:
                tileset = f.read()
        elif hasattr(tileset, "read"):
            tileset = tileset.read()
        with gt.Tileset(tileset, self.palsize) as ts:
            self.palpix, idx, dis = ts.match(self.palpix, self.active)
        self.make_tiles_unique()  # (on the GPU with gpu_unique, as in do_global_tiling)
        return idx, dis

    def do_frame_tiling(self, quality: int = ft.FT_MEDIUM, use_wavelets: bool = True, gamma: int = -1):
        """btnDoFrameTilingClick main.pas:945-977: PrepareGlobalFT, then per keyframe PrepareFrameTiling
        (over the keyframe's current TileMap items), DoFrameTiling of all its frames, FinishFrameTiling."""
        gds = ft.prepare_global_ft(self.palpix, self.active)
        errs = np.zeros(self.tile.shape, np.float32)
        Q = self.tiles_per_frame
        try:
            for k in self.kfs:
                r = self.rows(k)
                kt = ft.prepare_frame_tiling(self.palpix, self.thm, self.tvm, self.palettes[k], gds,
                                             self.pal[r].ravel(), self.tile[r].ravel(), quality,
                                             self.centroids[k], use_wavelets, gamma)
                try:
                    t, p, h, v, e = kt.do_frame_tiling(self.frame_rgb[r])
                finally:
                    kt.finish_frame_tiling()
                n = (r.stop - r.start, Q)
                self.tile[r], self.pal[r] = t.reshape(n), p.reshape(n)
                self.hm[r], self.vm[r], errs[r] = h.reshape(n), v.reshape(n), e.reshape(n)
        finally:
            gds.kdt.close()
        return errs

    def _use_count(self, T: int) -> np.ndarray:
        if self.gpu_reindex:
            return gt.use_count_gpu(self.tile, T)[0]
        return np.bincount(self.tile.ravel(), minlength=T).astype(np.int64)

    def do_reindex(self):
        """btnReindexClick main.pas:1199-1230: UseCount / Active from the TileMaps, then ReindexTiles."""
        self.use_count = self._use_count(self.palpix.shape[0])
        self.active = (self.use_count > 0).astype(np.uint8)
        self.reindex_tiles()

    def do_smooth(self, strength: float = DEFAULT_STRENGTH):
        """btnSmoothClick main.pas:1338-1370: SmoothedTileMap := TileMap, then DoTemporalSmoothing along
        every position (frames of one keyframe only, main.pas:4081-4082) -> one GPU call per keyframe."""
        sm = {"tile": self.tile.copy(), "pal": self.pal.copy(), "hm": self.hm.copy(), "vm": self.vm.copy(),
              "smoothed": np.zeros(self.tile.shape, np.uint8)}
        for k in self.kfs:
            r = self.rows(k)
            t, p, h, v, s, _ = smooth_keyframe(sm["tile"][r], sm["pal"][r], sm["hm"][r], sm["vm"][r],
                                               sm["smoothed"][r], self.palpix, self.palettes[k], strength)
            sm["tile"][r], sm["pal"][r], sm["hm"][r], sm["vm"][r] = t, p, h, v
            sm["smoothed"][r] = s
        self.sm = sm
        return sm

    def _keyframe_streams(self, width: int, height: int, fps: float, gpu: bool = False,
                          gpu_matches: bool = False) -> dict:
        """LZCompress'd command stream of every held keyframe (SaveStream main.pas:4724-4734), compressed
        concurrently.  gpu: the command words by libANN.so's kernel, LZMA on its thread pool (tiler_gtm_streams);
        gpu_matches (with gpu): the LZMA match search on the GPU as well."""
        if gpu_matches and not gpu:
            raise ValueError("gpu_matches needs gpu=True (the native writer)")
        sm = self.sm
        if sm is None:
            raise RuntimeError("SaveStream needs the SmoothedTileMaps: run do_smooth first")
        if gpu:
            if not self.kfs:
                return {}
            rows = [self.rows(k) for k in self.kfs]  # the held keyframes' rows follow one another
            kf_start = np.cumsum([0] + [r.stop - r.start for r in rows])
            r = slice(rows[0].start, rows[-1].stop)
            comps = gtm.keyframe_streams_gpu(self.palpix, self.thm, self.tvm, kf_start, self.palettes[self.kfs],
                                             sm["tile"][r], sm["pal"][r], sm["hm"][r], sm["vm"][r], sm["smoothed"][r],
                                             width=width, height=height, fps=fps, palsize=self.palsize,
                                             first_keyframe=self.kfs[0] == 0, gpu_matches=gpu_matches)
            return dict(zip(self.kfs, comps))
        raws = []
        for k in self.kfs:
            r = self.rows(k)
            raws.append(gtm.keyframe_raw(k, self.palpix, self.thm, self.tvm, self.palettes[k], sm["tile"][r],
                                         sm["pal"][r], sm["hm"][r], sm["vm"][r], sm["smoothed"][r], width=width,
                                         height=height, fps=fps, palsize=self.palsize))
        return dict(zip(self.kfs, gtm.compress_streams(raws)))

    def save_stream(self, width: int, height: int, fps: float = 24.0, gpu: bool = False,
                    gpu_matches: bool = False) -> bytes:
        """btnSaveClick -> SaveStream main.pas:4529-4763 (the .gtm bytes; needs do_smooth first).  gpu: the same
        bytes from the native writer; gpu_matches (with gpu): its LZMA match search on the GPU, the same bytes."""
        comps = self._keyframe_streams(width, height, fps, gpu, gpu_matches)
        return gtm.assemble_stream([comps[k] for k in range(self.kf_start.size - 1)], self.kf_start, width, height,
                                   fps)

    def render(self, on_screen: bool = False):
        """The held frames rebuilt from the tilemaps on the GPU (DrawTile main.pas:3308-3343), each frame with its
        keyframe's palettes: from the SmoothedTileMaps if do_smooth has run -- the items SaveStream writes, so the
        picture a GTM player shows -- else from the TileMaps.  on_screen = True gives what Render draws instead
        (main.pas:3416-3418: the SmoothedTileMap item only where Smoothed is set, the TileMap item elsewhere); the
        two differ where DoTemporalSmoothing rewrote a previous frame's item and left its flag clear (main.pas:4110).
        Returns (rgb [frames][Q][64] int32 0x00BBGGRR, invalid [frames])."""
        from .quality import render_frames
        P = self.n_palettes
        row0 = np.zeros(self.frames, np.int32)
        for k in self.kfs:
            row0[self.rows(k)] = k * P
        tail = (self.palpix, self.thm, self.tvm, self.palettes.reshape(-1, self.palettes.shape[-1]), row0, P)
        sm = self.sm
        if sm is None:
            return render_frames(self.tile, self.pal, self.hm, self.vm, *tail)
        if on_screen:
            return render_frames(self.tile, self.pal, self.hm, self.vm, *tail, sm["tile"], sm["pal"], sm["hm"],
                                 sm["vm"], sm["smoothed"])
        return render_frames(sm["tile"], sm["pal"], sm["hm"], sm["vm"], *tail)

    def render_raster(self, fmt: str = "rgb24", *, width: int, height: int, on_screen: bool = False):
        """render() as pictures an image writer or video encoder takes: (uint8 [frames][height][width][3|4] in `fmt`,
        X = 0xFF, invalid [frames]).  width, height: the screen in pixels, as save_stream takes them (the encoder
        holds only their product in tiles)."""
        from .load import tiles_to_frames
        tm_w, tm_h = int(width) // 8, int(height) // 8
        if tm_w < 1 or tm_h < 1 or tm_w * tm_h != self.tiles_per_frame:
            raise ValueError(f"render_raster: {width} x {height} is not the {self.tiles_per_frame} tiles of a frame")
        rgb, invalid = self.render(on_screen)
        return tiles_to_frames(rgb, tm_w, tm_h, fmt), invalid

    def _stream_frames(self, data):
        """The held frames as a GTM player shows them: `data` (.gtm bytes, a path or a binary file holding the whole
        clip), the frames of `frame_idx` alone drawn on the GPU (gtm.Stream.frames: the player's checkpoint index gives
        the pixels a skipped position carries, so the frames this encoder does not hold are neither drawn nor
        copied) -> (rgb [frames][Q][64] int32 0x00BBGGRR, the top byte of the stream's 0xAABBGGRR masked off;
        undrawn [frames])."""
        Q = self.tiles_per_frame
        with gtm.Stream(data) as st:
            if st.positions != Q or st.frames != self.n_frames:
                raise ValueError(f"the stream holds {st.frames} frames of {st.positions} positions, the encoder "
                                 f"{self.n_frames} of {Q}")
            rgb = np.zeros((self.frames, Q, 64), np.int32)
            undrawn = np.zeros(self.frames, np.int32)
            chunk = max(1, (1 << 27) // (Q * 256))
            for r0 in range(0, self.frames, chunk):
                got, und = st.frames(self.frame_idx[r0:r0 + chunk], "tiles", chunk)
                rgb[r0:r0 + chunk] = (got & 0x00FFFFFF).astype(np.int32)
                undrawn[r0:r0 + chunk] = und
        return rgb, undrawn

    def verify_stream(self, data=None, *, width: int, height: int, fps: float = 24.0) -> dict:
        """Closes the loop on SaveStream: plays `data` (default: self.save_stream(width, height, fps)) with the GPU
        player and compares every held frame, top byte masked, with render() -- the frames quality() scores.  They
        are equal exactly when the written bytes (SkipBlock runs, Short/Long indices, the mirror xor, per-keyframe
        palette loads, LZMA) show what the SmoothedTileMaps say.  Returns frames (compared), differing_frames,
        differing (their global frame indices), first = (frame, position) of the first difference or None, and
        undrawn (positions of the held frames nothing had drawn, summed)."""
        if data is None:
            data = self.save_stream(width, height, fps)
        played, undrawn = self._stream_frames(data)
        rgb, _ = self.render()
        bad = np.nonzero((played != rgb).any(axis=(1, 2)))[0]
        first = None
        if bad.size:
            r = int(bad[0])
            first = (int(self.frame_idx[r]), int(np.nonzero((played[r] != rgb[r]).any(axis=1))[0][0]))
        return {"frames": self.frames, "differing_frames": int(bad.size),
                "differing": [int(f) for f in self.frame_idx[bad]], "first": first, "undrawn": int(undrawn.sum())}

    def quality(self, frames=None, *, width: int, height: int, stream=None) -> dict:
        """The figure Render shows (lblCorrel main.pas:3488) for every held frame: the frames of render() (the
        SmoothedTileMaps if Smooth has run, i.e. the encode as it is written, else the TileMaps) scored against
        `frames` ([held frames][Q][64], default: the source frames given to the constructor).  width / height in
        pixels as for save_stream (the Video carries only Q, and the figure's transposed half depends on the
        shape).  stream: .gtm bytes, a path or a binary file of the whole clip -> the file's frames, played on the
        GPU, are scored instead of the in-memory tilemaps (`invalid` is then the never-drawn positions per frame).
        Returns per-frame corr (bit-identical to ComputeCorrelationBGR), psnr, sse [.][3], and the
        rendered frames (rgb, invalid).  A DistributedEncoder returns its own frames' values (rows as `frame_idx`);
        neither this nor verify_stream is a collective."""
        from .quality import frame_quality, psnr
        Q = self.tiles_per_frame
        tm_w, tm_h = int(width) // 8, int(height) // 8
        if tm_w <= 0 or tm_h <= 0 or tm_w * tm_h != Q:
            raise ValueError("quality: width x height does not match the tilemap size")
        src = np.asarray(self.frame_rgb if frames is None else frames)
        if src.size != self.frames * Q * 64:
            raise ValueError("quality: frames must be the held frames, [frames][Q][64]")
        rgb, invalid = self.render() if stream is None else self._stream_frames(stream)
        corr, sse = frame_quality(src, rgb, tm_w, tm_h)
        return {"corr": corr, "psnr": psnr(sse, tm_w, tm_h), "sse": sse, "rgb": rgb, "invalid": invalid}

    def run_all(self, desired: int, quality: int = ft.FT_MEDIUM, strength: float = DEFAULT_STRENGTH, reload=None):
        """btnRunAllClick main.pas:1232-1272 from MakeUnique to Smooth.  reload: a saved tileset (.gts bytes, path
        or file) -> the GlobalTiling step is do_reload_tiling(reload) instead of do_global_tiling(desired)."""
        self.do_make_unique()
        if reload is not None:
            self.do_reload_tiling(reload)
        else:
            self.do_global_tiling(desired)
        self.do_frame_tiling(quality)
        self.do_reindex()
        return self.do_smooth(strength)


class DistributedEncoder(Encoder):
    """The same chain with one process per GPU (tiler_amd.dist).  Call inside an initialised
    torch.distributed process group (backend "nccl" = RCCL over xGMI; "gloo" for CPU-side tests).

    Device: each rank binds its own GPU -- libANN.so through tiler_init(device) and torch through
    torch.cuda.set_device(device) -- with device = LOCAL_RANK (torchrun's one process per GPU) unless given.
    Work: palette bins (K-Modes) and keyframes (FrameTiling, then Smooth, same plan) are assigned longest-first
    across the ranks; a rank computes only its own units.  Memory: a rank holds the tileset (replicated, the north
    star's all-gathered tileset) and ONLY its own keyframes' frames and tilemaps ([own frames][Q]; `frame_idx`
    maps rows to frames).  Exchanges (fixed-layout tensors, tiler_amd.dist): the K-Modes merge map (all-reduce
    MAX) so every rank holds the reduced tileset, the UseCount histogram (all-reduce SUM) for ReindexTiles, and for
    SaveStream each rank's compressed keyframe streams onto rank `save_rank` (gather_units).  save_stream is a
    collective: every rank calls it, save_rank gets the .gtm bytes, the others None.
    do_reload_tiling is inherited: every rank matches the whole, replicated tile list against the saved tileset and
    gets the same answer; sharding the match across ranks is out of scope."""

    def __init__(self, v: Video, palsize: int | None = None, device: int | None = None, save_rank: int = 0,
                 gpu_unique: bool = False, gpu_reindex: bool = False):
        import os

        import torch
        import torch.distributed as dist

        from ._lib import check, load
        from . import dist as tdist
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        kf_start = np.asarray(v.kf_start, np.int64)
        nkf = kf_start.size - 1
        kf_frames = [int(kf_start[k + 1] - kf_start[k]) for k in range(nkf)]
        self.plan = tdist.plan_keyframes(kf_frames, v.tiles_per_frame, self.world)
        self.owner_of = [0] * nkf
        for r, units in enumerate(self.plan):
            for k in units:
                self.owner_of[k] = r
        mine = sorted(self.plan[self.rank])
        own = np.concatenate([np.arange(kf_start[k], kf_start[k + 1]) for k in mine]) if mine \
            else np.zeros(0, np.int64)
        super().__init__(v, palsize, frames=own, gpu_unique=gpu_unique, gpu_reindex=gpu_reindex)
        self.device = int(os.environ.get("LOCAL_RANK", "0")) if device is None else int(device)
        if self.device >= 0:  # device = -1: no GPU binding (host-side steps only, e.g. SaveStream in CPU tests)
            check(load().tiler_init(self.device), "tiler_init")
            if torch.cuda.is_available():
                torch.cuda.set_device(self.device)
        self.save_rank = save_rank

    def do_global_tiling(self, desired: int, restart: int = gt.CRANDOM_KMODES_COUNT):
        from . import dist as tdist
        plan = gt.plan_global_tiling(self.palpix, self.dith_pal, self.n_palettes, desired, self.palsize, restart,
                                     self.active)
        run = plan.run
        costs = [plan.bins[p].size * max(1, int(plan.k_per_bin[p])) for p in run]
        mine = [run[u] for u in tdist.lpt_assign(costs, self.world)[self.rank]]
        local = gt.kmodes_bins(plan, mine, self.palsize)  # this rank's bins in one GPU batch
        merge_to = tdist.allreduce(gt.kmodes_merge_map(plan, local, self.palpix.shape[0]), "max")
        pp, act, uc, mi = gt.apply_merge_map(merge_to, self.palpix, self.active, self.use_count)
        self.palpix, self.active, self.use_count = pp, act, uc
        self.finish_merge_tiles(mi)
        self.make_tiles_unique()
        self.reindex_tiles()
        return plan.k_per_bin

    def _use_count(self, T: int) -> np.ndarray:
        """btnReindexClick main.pas:1208-1221: the UseCount histogram over every rank's keyframes."""
        from . import dist as tdist
        return tdist.allreduce(super()._use_count(T), "sum")

    def verify_stream(self, data=None, *, width: int, height: int, fps: float = 24.0) -> dict:
        """Encoder.verify_stream over this rank's own frames of a complete file.  Not a collective, so the file
        must be given: save_stream, which would write it, is one."""
        if data is None:
            raise ValueError("verify_stream on a DistributedEncoder needs the complete file (save_stream is a "
                             "collective; pass save_rank's bytes)")
        return super().verify_stream(data, width=width, height=height, fps=fps)

    def save_stream(self, width: int, height: int, fps: float = 24.0, gpu: bool = False,
                    gpu_matches: bool = False) -> bytes | None:
        """SaveStream as a collective: every rank writes and compresses its own keyframes' streams (gpu: with the
        native writer; gpu_matches: its LZMA match search on the GPU), rank save_rank receives the others' and
        assembles the file (None on the other ranks)."""
        from . import dist as tdist
        comps = tdist.gather_units(self._keyframe_streams(width, height, fps, gpu, gpu_matches), self.owner_of,
                                   self.save_rank)
        if comps is None:
            return None
        return gtm.assemble_stream(comps, self.kf_start, width, height, fps)
