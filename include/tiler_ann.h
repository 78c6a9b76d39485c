/*
 * tiler_ann.h -- C-ABI of libANN.so, the MI355X-native drop-in for the reference's ANN.dll
 * boundary plus batched/device extensions for the FrameTiling, Smooth and GlobalTiling hot path.
 *
 * Reference interface replaced (b0nefish/tiler, /root/reference):
 *   extern.pas:63  function ann_kdtree_create(pa: PPANNFloat; n, dd, bs: Integer; split: TANNsplitRule): PANNkdtree; cdecl;
 *   extern.pas:64  procedure ann_kdtree_destroy(akd: PANNkdtree); cdecl;
 *   extern.pas:65  function ann_kdtree_search(akd: PANNkdtree; q: PANNFloat; eps: TANNFloat; err: PANNFloat): Integer; cdecl;
 *   extern.pas:66  function ann_kdtree_pri_search(akd: PANNkdtree; q: PANNFloat; eps: TANNFloat; err: PANNFloat): Integer; cdecl;
 *   extern.pas:67  function ann_kdtree_search_multi(akd: PANNkdtree; idxs: PInteger; errs: PANNFloat; cnt: Integer;
 *                                                    q: PANNFloat; eps: TANNFloat): Integer; cdecl;
 * Types: TANNFloat = Single (extern.pas:30), Integer = int32, TANNsplitRule = int32 enum (extern.pas:21-28).
 *
 * Semantics kept from ANN 1.1.2: exact nearest neighbours of the fp32
 * squared distance accumulated in dimension order with every operation rounded (no FMA); err =
 * squared distance (no sqrt); k results ascending; among equal distances the candidate ANN's own
 * kd-tree search finds first (split = ANN_KD_STD, bucket size bs: the tree is built exactly as
 * ANN's kd_tree constructor builds it, and the search result is the one annkSearch returns, its
 * box-distance pruning included).  Differences (superset behaviour):
 *   - split = TILER_SPLIT_INDEX_ORDER (100): no tree, equal distances resolve to the lowest index;
 *     the other ANN split rules (1..5, never used by the reference) are rejected;
 *   - eps > 0 is accepted and ignored: the exact answer satisfies every eps bound;
 *   - ann_kdtree_pri_search returns annkPriSearch's answer (the priority search replayed on the GPU: its leaf
 *     visit order by box distance, hence its own choice among equal distances, and its (1 + eps)^2 termination,
 *     so eps > 0 gives ANN's approximate answer there); the reference declares it (extern.pas:66) and never
 *     calls it;
 *   - the dataset rows are copied to device memory at create (ANN borrows pa until destroy);
 *   - no process abort: errors return -1 (or NULL) and tiler_last_error() explains;
 *   - every entry point is thread-safe.  Concurrent single-query calls on one handle (ann_kdtree_search /
 *     _search_multi from many threads: the reference's ProcThreadPool pattern, main.pas:972, 4027, 3830) are
 *     coalesced: callers that arrive while a batch is in flight are searched together as the next batch,
 *     each woken with its own answer (identical to a lone call's); other calls on one handle are serialised.
 * The search runs on the GPU only.  There is no CPU fallback: if the HIP runtime or a gfx950
 * device is missing every call fails with -1 / NULL.
 */
#ifndef TILER_ANN_H
#define TILER_ANN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ann_kdtree ann_kdtree; /* opaque */

/* ---- the reference ANN.dll surface (extern.pas:63-67), symbol- and ABI-identical ---- */
ann_kdtree *ann_kdtree_create(float **pa, int n, int dd, int bs, int split);
void ann_kdtree_destroy(ann_kdtree *akd);
int ann_kdtree_search(ann_kdtree *akd, float *q, float eps, float *err);
int ann_kdtree_pri_search(ann_kdtree *akd, float *q, float eps, float *err);
int ann_kdtree_search_multi(ann_kdtree *akd, int *idxs, float *errs, int cnt, float *q, float eps);

#define TILER_SPLIT_ANN_KD_STD 0     /* ANN_KD_STD (extern.pas:22): the reference's rule */
#define TILER_SPLIT_INDEX_ORDER 100 /* split value: no kd-tree, ties to the lowest index (faster to create) */

/* Create from fp32 rows already in HBM (d_rows[n][dd], copied); e.g. descriptors made by tiler_psyv_batch_dev.
 * ann_kdtree_create_dev = ann_kdtree_create_dev_ex(..., bs = 1, split = ANN_KD_STD, ...) (main.pas:3961). */
ann_kdtree *ann_kdtree_create_dev(const float *d_rows, int n, int dd, void *stream);
ann_kdtree *ann_kdtree_create_dev_ex(const float *d_rows, int n, int dd, int bs, int split, void *stream);

/* ---- batched extensions; host buffers, row-major q[nq][dd] ---- */
/* k = 1 for every query: idx[nq], err[nq].  Returns 0 or -1. */
int ann_kdtree_search_batch(ann_kdtree *akd, const float *q, int nq, float eps, int *idx, float *err);
/* k results per query, ascending by (err, index): idxs[nq][k], errs[nq][k] (missing: -1 / FLT_MAX). k <= 32. */
int ann_kdtree_search_multi_batch(ann_kdtree *akd, const float *q, int nq, int k, float eps, int *idxs, float *errs);
/* nq ann_kdtree_pri_search calls at once (host arrays; idx / err [nq]) */
int ann_kdtree_pri_search_batch(ann_kdtree *akd, const float *q, int nq, float eps, int *idx, float *err);
/* Same with device-resident buffers (HBM) on a HIP stream (NULL = default stream); asynchronous. */
int ann_kdtree_search_batch_dev(ann_kdtree *akd, const float *d_q, int nq, int k, int *d_idx, float *d_err,
                                void *stream);

/* Search statistics of the last call on this handle (shortlist sizes, exact fallbacks). */
typedef struct {
    int64_t queries;
    int64_t fallback_queries;   /* tier 2: shortlist overflowed -> MFMA collect pass + exact rescoring (any number of
                                   queries; the mirror-orbit tier 2 has no per-query candidate limit) */
    int64_t exhaustive_queries; /* tier 3: exhaustive reference-order scan (k > 8, non-finite / fp16-overflowing data,
                                   and > 1024 candidates for a query of the generic, non-orbit tier 2) */
    int32_t exact_integer;    /* 1 when the dataset is small integers: MFMA keys are exact */
    int32_t splits;           /* candidate splits used by the last launch */
    int64_t orbit_groups;     /* mirror orbits found in the dataset (0: mirror-orbit path unavailable) */
    int32_t orbit_search;     /* 1 when the last search ran the mirror-orbit shortlist */
    int32_t orbit_ksteps;     /* 16-deep MFMA k-steps over 32 groups the orbit shortlist issues per query (12 per
                                 block; fewer on blocks of mirror-symmetric tiles, whose zero blocks are skipped) */
    int64_t orbit_expansions; /* TILER_ORBIT_STATS=1 only: 4-entry re-key passes of the orbit rescore */
    int64_t orbit_rescored;   /* TILER_ORBIT_STATS=1 only: candidates rescored with the reference distance */
    int32_t tie_order;        /* 0: ANN kd-tree first-found (ANN_KD_STD), 1: lowest index */
    int32_t kd_levels;        /* levels of the kd-tree build */
    double kd_build_ms;       /* kd-tree build time at create */
    int64_t kd_replayed;      /* queries of the last search replayed exactly (ANN's pruning not vouched for) */
    int64_t flat_queries;     /* queries of the last FrameTiling call in shortlist workgroups made of flat tiles only
                                 (flat tiles are grouped last; such a workgroup runs isotypic block 0 only: 3 k-steps
                                 per candidate block instead of orbit_ksteps / blocks).  Flat tiles that share a
                                 workgroup with non-flat ones are not counted.  0 for searches without flat grouping.
                                 Always in the units of the call's own tiles: when the call searched its distinct
                                 tiles only (dup_queries > 0) this is queries - ceil(n / W) * W for the call's n
                                 non-flat tiles, duplicates included, and W queries per workgroup -- the layout the
                                 call would have had without dedupe; searched_flat_queries is what ran. */
    int64_t searched_queries; /* queries the last search ran: `queries`, or the distinct tiles of a FrameTiling call of
                                 >= 8,192 tiles in which at least one tile in eight repeats another of the same call
                                 (each distinct tile is searched once and its result copied to its repeats) */
    int64_t searched_flat_queries; /* searched queries in shortlist workgroups made of flat tiles only */
    int64_t dup_queries;      /* queries - searched_queries (0 when the call was searched tile by tile) */
} tiler_search_stats;
int ann_kdtree_get_stats(ann_kdtree *akd, tiler_search_stats *out);
/* Search batches of at most max_k1 queries (k = 1; default 64) or max_k8 (k <= 8; default 16) -- the coalesced
 * per-tile calls -- run an exhaustive exact scan spread over the whole GPU instead of the MFMA shortlist and its
 * tiers (same answers; 0 disables it, e.g. to test those tiers on small batches).  Process-wide.  0 / -1. */
int tiler_set_scan_limits(int max_k1, int max_k8);
/* Test hook (process-wide): on != 0 makes ANN's pruning check vouch for no result, so every query of every kd-order
 * search takes the exact replay of annkSearch (kd_replay_kernel); answers are identical either way.  0. */
int tiler_debug_force_replay(int on);
/* Test hook (read-only): how the handle's last ann_kdtree_pri_search_batch answered its queries at eps = 0 --
 * out[0] decided from the exact tie set, out[1] the priority search replayed in full, out[2] the heap order alone
 * simulated up to the first tied leaf.  All three are 0 after a call with eps != 0 (every query is replayed without
 * the resolve step), on a handle without a tree and before the first call.  0 / -1. */
int tiler_debug_pri_outcomes(ann_kdtree *akd, int64_t out[3]);
/* Test / bench hook (process-wide): on = 0 switches off the k = 1 generic shortlist's exact insertion gate (the query's
 * best key so far bounds what its lists may need), for A/B timing; answers are identical either
 * way.  Default 1.  0. */
int tiler_debug_shortlist_gate(int on);
/* Test / bench hook (process-wide): how a FrameTiling call of >= 8,192 tiles treats tiles that repeat inside the call.
 * 1 (default): every distinct tile is searched once (exact: a hash table groups the tiles, all 64 words are compared
 * before two tiles share a result); 0: every tile is searched, for A/B timing; 2: as 1 with the hash cut to 4 bits, so
 * nearly every lookup meets a different tile and the word comparison carries the load.  Answers are identical in all
 * three.  0, or -1 for another mode. */
int tiler_debug_ft_dedup(int mode);
/* Coalescing counters of the single-query entry points on this handle: calls, batches searched, largest batch. */
int tiler_combine_stats(ann_kdtree *akd, int64_t *calls, int64_t *batches, int32_t *max_batch);
/* Test / bench hook: the reference's per-call pattern timed natively (no interpreter between the calls): the first
 * min(nq, 64) queries as lone calls on one thread (median latency -> *lone_us), then all nq from `threads` native
 * threads calling ann_kdtree_search (k = 1) or ann_kdtree_search_multi (k > 1) once per query on this one handle
 * (query i on thread i % threads) -> *wall_s.  q[nq][dd] host rows; idx / err [nq][k] receive every answer.  0 / -1. */
int tiler_debug_percall_bench(ann_kdtree *akd, const float *q, int nq, int k, int threads, int32_t *idx, float *err,
                              double *wall_s, double *lone_us);
/* Leaf position of every dataset point in ANN's kd-tree (the order of its depth-first scan with every near
 * child LO): pos[n].  -1 when the handle was created with TILER_SPLIT_INDEX_ORDER. */
int tiler_kdtree_positions(ann_kdtree *akd, int32_t *pos);

/* ---- runtime ---- */
/* Binds the library to one HIP device (one process per GPU: device = LOCAL_RANK), or with TILER_ALL_DEVICES to
 * every visible gfx950 device (one process driving the node: the unmodified FreePascal encoder, whose keyframes run
 * concurrently in one process, main.pas:972 / 3961 / 4005-4011).  Optional; the first call of any other entry point
 * binds device 0.  Re-binding differently once bound fails with -1.
 * With all devices bound: ann_kdtree_create puts each new handle on the least loaded device (live dataset bytes,
 * ties to the lowest device), so concurrent keyframes' handles spread over the GPUs with no call-site change;
 * device-buffer entry points (_dev, ann_kdtree_create_dev*) run on the device their buffers live on, and a handle
 * used there from another device (e.g. the global 64-d dataset in tiler_prepare_frame_tiling_dev) is replicated to
 * it on first use (rows peer-copied over xGMI, the identical index built there); every other call of a handle runs
 * on the handle's device.  Host entry points without a handle run on the caller's current device if bound. */
#define TILER_ALL_DEVICES (-1)
int tiler_init(int device);
int tiler_device_count(void);                              /* devices bound (binds device 0 if none yet) */
int tiler_kdtree_device(ann_kdtree *akd);                  /* the device a handle lives on */
/* Copy a handle's index to device (TILER_ALL_DEVICES: to every bound device) now instead of on first use. 0 / -1. */
int tiler_kdtree_replicate(ann_kdtree *akd, int device);
/* The placement rule alone (host only, no device needed): dev_out[i] = the device ann_kdtree_create would give the
 * i-th of n handles of bytes[i] dataset bytes created in order on ndev empty devices (none destroyed).  0 / -1. */
int tiler_placement_plan(int ndev, const int64_t *bytes, int n, int32_t *dev_out);
/* Test hook (process-wide): on != 0 makes the first device-buffer call of a handle (and tiler_kdtree_replicate) build
 * its copy even on the handle's own device, so the replication path (peer copy, index rebuild, maps copy, routing)
 * runs on a one-GPU box; results are identical either way.  Only with TILER_ALL_DEVICES.  0. */
int tiler_debug_force_replicas(int on);
int tiler_shutdown(void);
const char *tiler_last_error(void); /* thread-local message of the last failure */
int tiler_set_gamma(double g0, double g1); /* gGamma main.pas:586 / 1441-1447; rebuilds gGammaCorLut */
/* Kernel timing with HIP events on the launching stream (bench/profiling): enable, then read the
 * summed milliseconds and launch count of one kernel family ("psyv", "nn_prep", "nn_shortlist",
 * "nn_rescore", "nn_exact", "smooth", "kmodes", "render", "quality", "reload_match", "unique_insert", "unique_last",
 * "unique_merge", "unique_zero", "ft_dedup": FrameTiling's duplicate-tile passes and scatter, "reindex_count",
 * "reindex_active", "reindex_order", "reindex_gather", "reindex_remap", "load_frames", "store_frames", "load_frames_scaled").  Reading
 * synchronises the recorded events. */
int tiler_timing_enable(int on);
double tiler_timing_get(const char *kernel, int *launches);
int tiler_timing_reset(void);

/* ---- PsyV descriptor (ComputeTilePsyVisFeatures main.pas:2997-3177) ----
 * flags: 1 FromPal, 2 UseWavelets, 4 UseLAB (RGBToLAB main.pas:2711-2747, the Dither step's descriptors),
 * 8 QWeighting, 16 HMirror, 32 VMirror.
 * RGB mode: rgb[n][64] (0x00BBGGRR).  Pal mode: palpix[*][64] indexed by tile_of[i] (or i when NULL),
 * palettes[*][16] indexed by pal_of[i] (or 0), per-item extra flags flags_per[i] (or NULL).
 * gamma: -1 (r/255) or 0/1 (gGammaCorLut).  Outputs: out64[n][192] and/or out32[n][192]. */
int tiler_psyv_batch(int n, const int32_t *rgb, int n_tiles, const uint8_t *palpix, const int32_t *tile_of, int n_palettes,
                     const int32_t *palettes,
                     const int32_t *pal_of, const uint8_t *flags_per, int flags, int gamma, double *out64, float *out32);
/* device-pointer variant (every pointer in HBM); asynchronous on stream */
int tiler_psyv_batch_dev(int n, const int32_t *rgb, const uint8_t *palpix, const int32_t *tile_of,
                         const int32_t *palettes, const int32_t *pal_of, const uint8_t *flags_per, int flags, int gamma,
                         double *out64, float *out32, void *stream);
/* The same two with an explicit palette size: palettes[*][palsize], palsize 1..256 (the reference offers 2, 4, 8, 16,
 * 32 and 64, cbxPalSize main.lfm:452-470).  tiler_psyv_batch[_dev] above mean palsize = 16 and run the same code; the
 * size is an argument, not a process-wide setting, so encoders of different sizes share a process.  The host-buffer
 * forms reject a tile byte >= palsize (the message names the first such tile); the _dev forms cannot report one and
 * read colour 0 of the item's palette for it, never past the table. */
int tiler_psyv_batch_ps(int n, const int32_t *rgb, int n_tiles, const uint8_t *palpix, const int32_t *tile_of,
                        int n_palettes, int palsize, const int32_t *palettes, const int32_t *pal_of,
                        const uint8_t *flags_per, int flags, int gamma, double *out64, float *out32);
int tiler_psyv_batch_ps_dev(int n, const int32_t *rgb, const uint8_t *palpix, const int32_t *tile_of,
                            const int32_t *palettes, int palsize, const int32_t *pal_of, const uint8_t *flags_per,
                            int flags, int gamma, double *out64, float *out32, void *stream);
/* Test hook (process-wide): palette-mode DCT descriptors (no wavelets, no LAB, per-item flags absent or mirrors
 * only) of min_items items or more are computed one lane per item, fewer one wave per item; 0 restores the default,
 * 32768.  Results are identical for every value.  0 / -1 (min_items < 0). */
int tiler_debug_psyv_lane_items(int64_t min_items);

/* ---- FrameTiling (DoFrameTiling main.pas:3992-4047) ----
 * Attach the keyframe dataset's row -> (tile, palette, attrs) maps (TTilingDataset.TRTo*, main.pas:181-189)
 * to a handle created over the keyframe's candidate descriptors. */
int tiler_ft_set_maps(ann_kdtree *akd, const int32_t *tr_tile, const int32_t *tr_pal, const uint8_t *tr_attr);
/* Read them back (host arrays of the handle's n rows), e.g. the candidate set tiler_prepare_frame_tiling_dev built. */
int tiler_ft_get_maps(ann_kdtree *akd, int32_t *tr_tile, int32_t *tr_pal, uint8_t *tr_attr);
/* For Q frame tiles (RGB): query descriptor (UseWavelets, gamma, no mirror) -> fp32 -> exact NN ->
 * tilemap item {GlobalTileIndex, PalIdx, HMirror = attr&1, VMirror = attr&2} + err. Host buffers. */
int tiler_frame_tiling(ann_kdtree *akd, const int32_t *rgb, int Q, int use_wavelets, int gamma, int32_t *out_tile,
                       int32_t *out_pal, uint8_t *out_hm, uint8_t *out_vm, float *out_err);
/* PrepareFrameTiling (main.pas:3791-3967) for one keyframe, on the device: its tilemap items d_item_tile /
 * d_item_pal [n_items] (TFrame.TileMap GlobalTileIndex / PalIdx of every frame tile; -1 = none) -> the distinct
 * (PalIdx, tile) items -> UseOne's k = 8 preselection in global_ds (the handle over PrepareGlobalFT's 64-d rows, its
 * TRTo maps set with tiler_ft_set_maps; ANN's tie order) -> used[palette][tile][attr] (results of equal err after
 * the first skipped, main.pas:3832-3852; quality 0 Fast: the item's palette, 1 Medium: every palette p' with
 * near[p' * n_palettes + p] != 0 -- the host's corr(p', p) < cFTPaletteTol * HighestCorr, BuildPaletteCorrTriangle
 * main.pas:3855-3867 --, 2 Slow: all) -> DoPsyV's candidates in emission order -> their descriptors -> a new
 * search handle over them with its TRTo maps set, ready for tiler_frame_tiling_dev.  The tileset d_palpix[n_tiles]
 * [64], d_thm / d_tvm[n_tiles] (TTile.HMirror / VMirror) and d_palettes[n_palettes][16] are in HBM; near is a host
 * array (Medium only).  Runs on stream (synchronising it twice: the distinct-item and candidate counts); info
 * (optional) returns those counts.  Calls sharing global_ds are serialised on the host and ordered on the device: a
 * call on another stream waits (hipStreamWaitEvent) until the previous call's work that reads the shared scratch has
 * run, so concurrent prepares on different streams are safe.  NULL on error. */
typedef struct {
    int64_t items;      /* distinct (PalIdx, GlobalTileIndex) items searched */
    int64_t candidates; /* KNNSize: candidate descriptors of the keyframe's dataset */
} tiler_prepare_info;
ann_kdtree *tiler_prepare_frame_tiling_dev(ann_kdtree *global_ds, const int32_t *d_item_tile,
                                           const int32_t *d_item_pal, int64_t n_items, const uint8_t *d_palpix,
                                           const uint8_t *d_thm, const uint8_t *d_tvm, int n_tiles,
                                           const int32_t *d_palettes, int n_palettes, int quality, const uint8_t *near,
                                           int use_wavelets, int gamma, void *stream, tiler_prepare_info *info);
/* The same with d_palettes[n_palettes][palsize] (1..256); tiler_prepare_frame_tiling_dev means palsize = 16.  The
 * 64-d rows of global_ds then hold values up to palsize - 1; the k = 8 preselection stays exact (integer rows). */
ann_kdtree *tiler_prepare_frame_tiling_ps_dev(ann_kdtree *global_ds, const int32_t *d_item_tile,
                                              const int32_t *d_item_pal, int64_t n_items, const uint8_t *d_palpix,
                                              const uint8_t *d_thm, const uint8_t *d_tvm, int n_tiles,
                                              const int32_t *d_palettes, int n_palettes, int palsize, int quality,
                                              const uint8_t *near, int use_wavelets, int gamma, void *stream,
                                              tiler_prepare_info *info);
/* Same, every buffer in HBM, asynchronous on stream (the benchmarked path): no host synchronisation inside, every
 * data-dependent count (flat tiles, tier-2 / tier-3 queries) stays on the device. */
int tiler_frame_tiling_dev(ann_kdtree *akd, const int32_t *d_rgb, int Q, int use_wavelets, int gamma,
                           int32_t *d_tile, int32_t *d_pal, uint8_t *d_hm, uint8_t *d_vm, float *d_err, void *stream);

/* ---- Smooth (DoTemporalSmoothing main.pas:4071-4119 over one keyframe) ----
 * Items are [F][Q] arrays (F frames of one keyframe, Q tilemap positions), updated in place exactly
 * as btnSmoothClick does after SmoothedTileMap := TileMap.  palpix[T][64], palettes[P][16]. */
int tiler_smooth_keyframe(int F, int Q, int32_t *tile, int32_t *tmpidx, int32_t *pal, uint8_t *hm, uint8_t *vm,
                          uint8_t *smoothed, int T, const uint8_t *palpix, int P, const int32_t *palettes,
                          double strength);
/* Same with every array in HBM (tmpidx may be NULL); asynchronous on stream. */
int tiler_smooth_keyframe_dev(int F, int Q, int32_t *d_tile, int32_t *d_tmpidx, int32_t *d_pal, uint8_t *d_hm,
                              uint8_t *d_vm, uint8_t *d_smoothed, const uint8_t *d_palpix, const int32_t *d_palettes,
                              double strength, void *stream);
/* The same two with palettes[P][palsize] (1..256); the forms above mean palsize = 16.  The host form rejects a tile
 * byte >= palsize, naming the first such tile; the _dev form reads colour 0 for it. */
int tiler_smooth_keyframe_ps(int F, int Q, int32_t *tile, int32_t *tmpidx, int32_t *pal, uint8_t *hm, uint8_t *vm,
                             uint8_t *smoothed, int T, const uint8_t *palpix, int P, int palsize,
                             const int32_t *palettes, double strength);
int tiler_smooth_keyframe_ps_dev(int F, int Q, int32_t *d_tile, int32_t *d_tmpidx, int32_t *d_pal, uint8_t *d_hm,
                                 uint8_t *d_vm, uint8_t *d_smoothed, const uint8_t *d_palpix,
                                 const int32_t *d_palettes, int palsize, double strength, void *stream);

/* ---- GlobalTiling K-Modes (TKModes.ComputeKModes kmodes.pas:917-1060) ----
 * X[n][nattr] bytes; k clusters; start_point = -ANumInit (the DoKModes call, main.pas:4218); labels[n]
 * (0-based), centroids[k][nattr].  Returns k or -1.  n_iter / cost optional. */
int tiler_kmodes_compute(const uint8_t *X, int n, int nattr, int k, int start_point, int n_modalities,
                         int32_t *labels, uint8_t *centroids, int *n_iter, uint64_t *cost);
/* DoKModes medoids (main.pas:4231-4253): for every cluster j, the member row minimising the K-Modes
 * dissimilarity to centroid j (ties -> last member, as GetMinMatchingDissim); medoid[j] = -1 and
 * counts[j] = 0 for empty clusters.  X[n][80], labels[n] in 0..k-1, centroids[k][80]. */
int tiler_kmodes_medoids(const uint8_t *X, int n, const int32_t *labels, const uint8_t *centroids, int k,
                         int32_t *medoid, int32_t *counts);
/* All of DoGlobalTiling's palette bins in one call (DoKModes per bin, main.pas:4195-4254, which the
 * reference runs concurrently with ProcThreadPool at main.pas:4339): X[N][80] with bin b = rows
 * [bin_off[b], bin_off[b+1]), k[b] clusters and start[b] (bin-local) per bin; labels[N] bin-local,
 * centroids[sum k][80] bin after bin; n_iter[b] / cost[b] optional.  Each bin's result is exactly
 * tiler_kmodes_compute's on that bin alone.  Returns 0 or -1. */
int tiler_kmodes_batch(const uint8_t *X, const int32_t *bin_off, int nbins, const int32_t *k, const int32_t *start,
                       int n_modalities, int32_t *labels, uint8_t *centroids, int32_t *n_iter, uint64_t *cost);
/* The same with X / labels / centroids in HBM (X 16-byte aligned) on a HIP stream (NULL = default);
 * bin_off / k / start / n_iter / cost are host arrays.  Synchronous. */
int tiler_kmodes_batch_dev(const uint8_t *d_X, const int32_t *bin_off, int nbins, const int32_t *k,
                           const int32_t *start, int n_modalities, int32_t *d_labels, uint8_t *d_centroids,
                           int32_t *n_iter, uint64_t *cost, void *stream);
/* Work counters of the last tiler_kmodes_batch[_dev] call (process-wide): the (point, centroid) dissimilarities its
 * assignment launches evaluated (the initial assignment + every chunk step's), and its dependent chunk steps. */
int tiler_kmodes_last_stats(int64_t *assign_pairs, int64_t *chunk_steps);
/* Test hook (process-wide): on != 0 makes the persistent farthest-first launch give up at its first grid barrier,
 * as a barrier that times out on a contended GPU would, so every batch takes the recovery path (state re-initialised,
 * the rounds re-run one launch each).  Results are identical either way.  0. */
int tiler_debug_kmodes_ff_fallback(int on);
/* Medoids of every bin's clusters (as tiler_kmodes_medoids per bin): medoid[sum k] bin-local rows. */
int tiler_kmodes_medoids_batch(const uint8_t *X, const int32_t *bin_off, int nbins, const int32_t *k,
                               const int32_t *labels, const uint8_t *centroids, int32_t *medoid, int32_t *counts);
/* The same with X / labels / centroids (X and centroids 16-byte aligned) and the outputs medoid[sum k] / counts[sum k]
 * in HBM; bin_off / k are host arrays; labels must lie in [0, k) of their bin (not checked).  Nothing is decoded on
 * the host, so a kernel can consume the result where it lies.  Synchronous on `stream`. */
int tiler_kmodes_medoids_batch_dev(const uint8_t *d_X, const int32_t *bin_off, int nbins, const int32_t *k,
                                   const int32_t *d_labels, const uint8_t *d_centroids, int32_t *d_medoid,
                                   int32_t *d_counts, void *stream);

/* ---- GlobalTiling, reload branch (ReloadPreviousTiling main.pas:4372-4470) ----
 * Batched GetMinMatchingDissim (kmodes.pas:598-604): rows[n][80] dataset lines of arbitrary bytes, group g = rows
 * [grp_off[g], grp_off[g+1]); every item items[i][80] is searched in group item_grp[i], or in all n rows when that is
 * -1, out of range or an empty group.  idx_out[i] = the row of minimal dissimilarity (2048 mismatch + W0 + W4, the
 * asm's int8 wrap and mod-2^16 words included), ties to the LAST row; -1 (and dis ~0) when n = 0, as the asm returns.
 * At most 1023 groups.  0 / -1. */
int tiler_min_matching_dissim_groups(const uint8_t *rows, int64_t n, const int32_t *grp_off, int ngroups,
                                     const uint8_t *items, const int32_t *item_grp, int64_t m, int32_t *idx_out,
                                     uint64_t *dis_out);
/* The same with rows / items (16-byte aligned) / item_grp / idx / dis in HBM; grp_off is a host array.  Synchronous. */
int tiler_min_matching_dissim_groups_dev(const uint8_t *d_rows, int64_t n, const int32_t *grp_off, int ngroups,
                                         const uint8_t *d_items, const int32_t *d_item_grp, int64_t m, int32_t *d_idx,
                                         uint64_t *d_dis, void *stream);
/* A saved tileset (.gts, main.pas:4359-4367) resident in HBM.  raw[n][64]: the file's tiles in file order (host);
 * every byte becomes (v * palsize) div file_palsize kept as a byte (main.pas:4436-4438), every tile its 80-byte
 * dataset line (WriteTileDatasetLine) bucketed by PalSigni (GetTilePalZoneThres' return value, 16 zones of the clip's
 * palsize).  n = 0 is allowed.  NULL on error. */
typedef struct tiler_tileset tiler_tileset;
tiler_tileset *tiler_tileset_load(const uint8_t *raw, int64_t n, int file_palsize, int palsize);
int tiler_tileset_destroy(tiler_tileset *ts);
/* DoFindBest (main.pas:4377-4410) over a tile list: every tile with active[i] != 0 gets the first 64 bytes of its
 * closest line of the tileset -- searched in the bucket of the tile's own PalSigni, in the whole set when that bucket
 * is empty; ties to the last row -- written over palpix[i]; idx_out[i] = that line's file-order row, dis_out[i] its
 * dissimilarity (either may be NULL).  Inactive tiles are untouched, idx -1.  With an empty tileset nothing changes
 * and every idx is -1.  Host buffers.  0 / -1. */
int tiler_tileset_match(tiler_tileset *ts, uint8_t *palpix, const uint8_t *active, int64_t nt, int32_t *idx_out,
                        uint64_t *dis_out);
/* The same with every array in HBM (palpix 16-byte aligned); queries go through in passes of bounded scratch.
 * Synchronous. */
int tiler_tileset_match_dev(tiler_tileset *ts, uint8_t *d_palpix, const uint8_t *d_active, int64_t nt, int32_t *d_idx,
                            uint64_t *d_dis, void *stream);
/* Test / study hook (process-wide): chunk > 0 = queries per pass (0: the default, 2^20); qpt = queries per thread of
 * the argmin kernel, 1 or 2 (0: the default); slices > 0 = row slices per query block (0: chosen from the number of
 * query blocks).  Results are identical either way.  0 / -1. */
int tiler_debug_reload(int64_t chunk, int qpt, int slices);
/* (query, row) dissimilarities the last tiler_tileset_match[_dev] / tiler_min_matching_dissim_groups[_dev] call of
 * the process evaluated. */
int tiler_reload_last_pairs(int64_t *pairs);

/* ---- MakeTilesUnique (main.pas:2555-2612): the exact duplicate-tile merge ----
 * palpix[nt][64], active[nt], use_count[nt] in and out, merge_index[nt] out.  Segment s = tiles [seg_off[s],
 * seg_off[s+1]) (seg_off[nseg+1], a host array, non-decreasing from 0 to nt; nseg >= 1): one MakeTilesUnique per
 * segment, as btnDoMakeUniqueClick runs one per chunk (main.pas:916-938); {0, nt} is the whole list.  Inside a
 * segment the tiles with active != 0 and identical palpix merge into the one of lowest index (MergeTiles
 * main.pas:3688-3712: use_count summed into it, active cleared, merge_index = its index, palpix zeroed) -- except that
 * the segment's last tile in sorted order (the greatest 16 little-endian dwords, dword 0 first; among equals the
 * highest index) never merges, as the reference's final DoOneMerge leaves it out (main.pas:2604-2605).  merge_index
 * is -1 for every tile that was not merged.  The result does not depend on the order threads run in.  nt = 0 is
 * allowed.  Host buffers.  0 / -1. */
int tiler_make_tiles_unique(uint8_t *palpix, uint8_t *active, int64_t *use_count, int64_t *merge_index, int64_t nt,
                            const int64_t *seg_off, int nseg);
/* The same with the four arrays in HBM (palpix 16-byte aligned); seg_off stays a host array.  Synchronous. */
int tiler_make_tiles_unique_dev(uint8_t *d_palpix, uint8_t *d_active, int64_t *d_use_count, int64_t *d_merge_index,
                                int64_t nt, const int64_t *seg_off, int nseg, void *stream);
/* Test hook (process-wide): keep only the low hash_bits bits of a tile's hash (0: every tile probes one chain of the
 * table), -1 = the default (all bits).  Results are identical either way; for collision tests only.  0 / -1. */
int tiler_debug_unique(int hash_bits);

/* ---- Reindex (btnReindexClick main.pas:1199-1230, ReindexTiles main.pas:4483-4527) and the TileMap remap of
 * FinishMergeTiles (main.pas:3722-3734) ----
 * Tilemap items are int32, use_count int64, index maps int64 with -1 = none (a merge_index of
 * tiler_make_tiles_unique is such a map).  Every call: n_items, n, nt in [0, 2^31); 0, or -1 with tiler_last_error();
 * the result does not depend on the order threads run in (integer atomics only).  The host-array forms stage their
 * arrays to HBM and run the _dev forms; the _dev forms take device pointers, run on `stream` and wait once (for the
 * error word, and n_active).
 *
 * Use counts (main.pas:1208-1221): use_count[t] = the number of items equal to t, added to what use_count holds when
 * accumulate != 0 (one call per keyframe's TileMaps, or per rank), after clearing the nt counts when accumulate == 0;
 * active[t] = (use_count[t] > 0) of the accumulated count (active may be NULL).  An item outside [0, nt) is never
 * used as an index: the call returns -1, the message names the lowest such item, and use_count / active hold
 * unspecified values.  n_items = 0 and nt = 0 are allowed. */
int tiler_tile_use_count(const int32_t *tile, int64_t n_items, int64_t nt, int64_t *use_count, uint8_t *active,
                         int accumulate);
int tiler_tile_use_count_dev(const int32_t *d_tile, int64_t n_items, int64_t nt, int64_t *d_use_count,
                             uint8_t *d_active, int accumulate, void *stream);
/* The order of ReindexTiles (CompareTileUseCountRev main.pas:4472-4481) over the tiles with active != 0: use_count
 * descending, old index ascending among equals.  idx_map[nt]: the new index of a tile, -1 for an inactive one;
 * order[nt]: order[i] = the old index of new tile i for i < *n_active, -1 from there on; *n_active (a host word) =
 * the active tiles.  An active tile of count 0 is kept and sorts last; an inactive tile is dropped whatever its
 * count.  Every use_count must lie in [0, 2^31), the reference's Integer: else -1, naming the first such tile. */
int tiler_reindex_tiles(const uint8_t *active, const int64_t *use_count, int64_t nt, int64_t *idx_map, int64_t *order,
                        int64_t *n_active);
int tiler_reindex_tiles_dev(const uint8_t *d_active, const int64_t *d_use_count, int64_t nt, int64_t *d_idx_map,
                            int64_t *d_order, int64_t *n_active, void *stream);
/* The tile list in its new order: out[i] = in[order[i]] for i < n, for each pair given (palpix rows of 64 bytes,
 * thm / tvm bytes, dith_pal, use_count; in arrays [nt], out arrays [n]).  A pair is skipped when both its pointers
 * are NULL; an output equal to its input is refused (the gather is not in place).  order[i] outside [0, nt) gives -1
 * (that row is not written).  _dev: palpix and palpix_out 16-byte aligned. */
int tiler_gather_tiles(const int64_t *order, int64_t n, const uint8_t *palpix, uint8_t *palpix_out, const uint8_t *thm,
                       uint8_t *thm_out, const uint8_t *tvm, uint8_t *tvm_out, const int32_t *dith_pal,
                       int32_t *dith_pal_out, const int64_t *use_count, int64_t *use_count_out, int64_t nt);
int tiler_gather_tiles_dev(const int64_t *d_order, int64_t n, const uint8_t *d_palpix, uint8_t *d_palpix_out,
                           const uint8_t *d_thm, uint8_t *d_thm_out, const uint8_t *d_tvm, uint8_t *d_tvm_out,
                           const int32_t *d_dith_pal, int32_t *d_dith_pal_out, const int64_t *d_use_count,
                           int64_t *d_use_count_out, int64_t nt, void *stream);
/* TileMap items through an index map, in place: keep_unmapped == 0: tile = map[tile] (ReindexTiles main.pas:4523-4526;
 * an item of a dropped tile becomes -1); keep_unmapped != 0: tile = map[tile] where that is >= 0, unchanged elsewhere
 * (FinishMergeTiles).  map[nt], values below 2^31.  An item outside [0, nt) is left as it is and gives -1, naming the
 * lowest such item; in the _dev form the other items may already be remapped by then (the host-array form leaves the
 * host array untouched on a failure). */
int tiler_remap_items(int32_t *tile, int64_t n_items, const int64_t *map, int64_t nt, int keep_unmapped);
int tiler_remap_items_dev(int32_t *d_tile, int64_t n_items, const int64_t *d_map, int64_t nt, int keep_unmapped,
                          void *stream);
/* Test hook (process-wide): the counting strategy of tiler_tile_use_count: 0 = per-workgroup LDS counters in windows
 * of 65,536 tiles, 1 = wave-combined global atomics, -1 = the default (by nt).  Results are identical.  0 / -1. */
int tiler_debug_reindex(int strategy);

/* ---- GlobalTiling, K-Modes branch (DoGlobalTiling main.pas:4256-4343, DoKModes 4195-4254) as one call ----
 * The step between MakeTilesUnique and FinishMergeTiles over a tile list: palpix[nt][64], active[nt], use_count[nt]
 * (int64) in and out, dith_pal[nt] (DitheringPalIndex) in, merge_index[nt] out.
 *   1. the Active tiles are binned by dith_pal, ascending tile index inside a bin (TileIndices[signi]);
 *   2. bin p of size n gets ClusterCount = ceil(EqualQualityTileCount(n) * desired / sum of EqualQualityTileCount)
 *      (tiler_global_tiling_counts) and runs K-Modes iff n > ClusterCount;
 *   3. its rows are the tiles' 80-byte dataset lines (tiler_tile_dataset_lines), its StartingPoint the LAST row of
 *      minimal byte sum;
 *   4. K-Modes of all such bins (tiler_kmodes_batch_dev with n_modalities = palsize) and their medoids;
 *   5. every tile of a cluster with >= 2 members other than the cluster's medoid tile is merged into it (MergeTiles
 *      main.pas:3688-3712, NewTile = nil): use_count summed into the medoid tile, active cleared, merge_index = the
 *      medoid tile, palpix zeroed.  merge_index is -1 for every other tile.
 * The call ends where FinishMergeTiles begins: apply merge_index with tiler_remap_items(..., keep_unmapped = 1).
 * Optional host outputs, each [n_palettes], any may be NULL: bin_size[p] = the Active tiles of bin p; k[p] =
 * round(ClusterCount) of every bin, run or not; start[p] = the bin-local StartingPoint, -restart for an empty bin
 * (restart = cRandomKModesCount, 7, has no other effect).
 * Limits, checked before the device is touched (-1): 0 <= nt < 2^31, 1 <= n_palettes <= 4096, 1 <= palsize <= 256,
 * 1 <= desired <= 2^30.  Every tile with active != 0 must have dith_pal in [0, n_palettes) and all 64 bytes below
 * palsize (the reference would index out of bounds): otherwise the tile is never used as an index, the call returns
 * -1 and tiler_last_error() names the lowest such tile and what is wrong with it; inactive tiles may hold anything.
 * nt = 0, no Active tile or no bin to run: 0, nothing merged, merge_index all -1.  The result does not depend on the
 * order threads run in (integer atomics only).  On failure the host form leaves every caller array untouched; in the
 * _dev form they are unspecified.
 * _dev: the five arrays in HBM (palpix 16-byte aligned), bin_size / k / start host arrays, on `stream`.  It waits
 * three times -- for the histogram and the error word, for the StartingPoints, and for the merges at the end --
 * beside the waits of the K-Modes batch in between; the tile bytes never leave HBM. */
int tiler_global_tiling(uint8_t *palpix, const int32_t *dith_pal, uint8_t *active, int64_t *use_count,
                        int64_t *merge_index, int64_t nt, int n_palettes, int palsize, int desired, int restart,
                        int32_t *bin_size, int32_t *k, int32_t *start);
int tiler_global_tiling_dev(uint8_t *d_palpix, const int32_t *d_dith_pal, uint8_t *d_active, int64_t *d_use_count,
                            int64_t *d_merge_index, int64_t nt, int n_palettes, int palsize, int desired, int restart,
                            int32_t *bin_size, int32_t *k, int32_t *start, void *stream);
/* The cluster counts alone (host code, no device): eq(n) = round(sqrt(n) * (ln(1 + n) * 1.4426950408889634079)), half
 * to even (EqualQualityTileCount main.pas:722-725); share = desired / sum eq; k[p] = ceil(eq(bin_size[p]) * share);
 * run[p] = bin_size[p] > k[p].  k / run may be NULL.  All bins empty: every k and run is 0.  -1 for a NULL or negative
 * bin_size, n_palettes outside [1, 4096], desired outside [1, 2^30]. */
int tiler_global_tiling_counts(const int32_t *bin_size, int n_palettes, int desired, int32_t *k, uint8_t *run);
/* WriteTileDatasetLine (main.pas:4167-4183) of every tile: lines[nt][80] = the 64 indices, then the 16 zone flags
 * count(idx * 16 div palsize == z) > palsize div 16 (the threshold is 0 for palsize < 16; an index whose zone is past
 * the 16th is counted nowhere); pal_signi[nt] = GetTilePalZoneThres' return value, 64 - the largest zone count.
 * Either output may be NULL.  1 <= palsize <= 256.  _dev: palpix and lines 16-byte aligned; synchronous. */
int tiler_tile_dataset_lines(const uint8_t *palpix, int64_t nt, int palsize, uint8_t *lines, int32_t *pal_signi);
int tiler_tile_dataset_lines_dev(const uint8_t *d_palpix, int64_t nt, int palsize, uint8_t *d_lines,
                                 int32_t *d_pal_signi, void *stream);

/* ---- Load-step keyframe detection (btnLoadClick main.pas:1099-1146) ----------------
 * frames[F][tm_h*tm_w][64] int32 0x00BBGGRR (TFrame.Tiles[].RGBPixels, tile-major, as FrameTiling takes
 * them).  corr[F-1] (host): corr[i-1] = ComputeInterFrameCorrelation(frame i-1, frame i) (main.pas:811-828,
 * PearsonCorrelation main.pas:1465-1492 over LoadFrame's FSPixels), bit-identical to the reference's
 * sequential fp64 evaluation.  0 ok, -1 error.  No reference interface exists for this step (it is inline
 * in btnLoadClick); these exports let the Pascal Load step hand its frames over instead. */
int tiler_interframe_correlation(const int32_t *rgb, int F, int tm_w, int tm_h, double *corr);
/* Same with the frames in HBM (16-byte aligned); corr is a host array; synchronous on stream. */
int tiler_interframe_correlation_dev(const int32_t *d_rgb, int F, int tm_w, int tm_h, double *corr, void *stream);
/* The shot-transition split (main.pas:1099-1132): kf_of_frame[F] = keyframe index of each frame.
 * tile_map_size = FTileMapSize.  Returns the keyframe count, or -1. */
int tiler_find_keyframes(const double *corr, int F, int tile_map_size, int32_t *kf_of_frame);

/* ---- Load-step raster ingest (LoadFrame main.pas:3211-3286, ReframeUI main.pas:1931-1938) and its inverse ----
 * Pictures as a decoder leaves them -> the tile-major frames every other entry point takes, and back.  Decoding
 * image files stays with the caller; the pictures arrive in memory.
 * Source: F pictures of src_w x src_h pixels; row j of frame f starts at byte f * frame_stride + j * pitch, with
 * pitch >= src_w * bpp and frame_stride >= src_h * pitch (any alignment: odd pitches and bases take a byte path at
 * the ends of a row only).  Pixel formats (alpha / X is dropped, as SwapRB main.pas:561-564 drops it): */
#define TILER_PIX_RGB24 0  /* bytes R,G,B (ffmpeg -pix_fmt rgb24) */
#define TILER_PIX_BGR24 1  /* bytes B,G,R */
#define TILER_PIX_BGRA32 2 /* bytes B,G,R,X: the integer 0x00RRGGBB of a pf32bit ScanLine, which LoadFrame SwapRBs */
#define TILER_PIX_RGBA32 3 /* bytes R,G,B,X: the integer 0xXXBBGGRR (the GTM player's raster) */
/* ReframeUI: *tm_w = min(src_w div 8, 240), *tm_h = min(src_h div 8, 135); the picture's top-left tm_w*8 x tm_h*8
 * pixels are used, the rest ignored.  -1 when src_w or src_h is below 8. */
int tiler_load_dims(int src_w, int src_h, int *tm_w, int *tm_h);
/* Pictures in HBM -> d_rgb[F][tm_h*tm_w][64] int32 0x00BBGGRR (16-byte aligned): tile tm_w * (j div 8) + (i div 8),
 * element (j and 7) * 8 + (i and 7) (main.pas:3252-3258).  Asynchronous on stream.  Every argument is checked
 * before anything is launched: -1 with tiler_last_error() naming it.  F = 0 does nothing and returns 0. */
int tiler_load_frames_dev(const uint8_t *d_src, int fmt, int F, int src_w, int src_h, int64_t pitch,
                          int64_t frame_stride, int32_t *d_rgb, void *stream);
/* Host arrays.  Staged in chunks of whole frames on a pool stream -- copy in, kernel, copy out -- each chunk at most
 * 256 MiB of picture plus tile bytes (at least one frame), so a clip of any length needs two device blocks of that
 * size together.  Only the used rectangle of every picture is copied: row padding is never read. */
int tiler_load_frames(const uint8_t *src, int fmt, int F, int src_w, int src_h, int64_t pitch, int64_t frame_stride,
                      int32_t *rgb);
/* The inverse: rgb[F][tm_h*tm_w][64] (the top byte of a pixel is ignored) -> pictures of tm_w*8 x tm_h*8 pixels in
 * fmt; X bytes are written 0xFF; the bytes of a row past tm_w * 8 * bpp and between frames are not written. */
int tiler_store_frames_dev(const int32_t *d_rgb, int F, int tm_w, int tm_h, int fmt, uint8_t *d_dst, int64_t pitch,
                           int64_t frame_stride, void *stream);
int tiler_store_frames(const int32_t *rgb, int F, int tm_w, int tm_h, int fmt, uint8_t *dst, int64_t pitch,
                       int64_t frame_stride);
/* The Load step in one call: frames tiled into d_rgb, then corr[F-1] and kf_of_frame[F] (host arrays) from them
 * (tiler_interframe_correlation_dev + tiler_find_keyframes).  Synchronous on stream.  Returns the keyframe count
 * or -1. */
int tiler_load_clip_dev(const uint8_t *d_src, int fmt, int F, int src_w, int src_h, int64_t pitch,
                        int64_t frame_stride, int32_t *d_rgb, double *corr, int32_t *kf_of_frame, void *stream);
/* Test hook (process-wide): frames per staging chunk of tiler_load_frames / tiler_store_frames; 0 restores the
 * default (the 256 MiB rule above).  Results are identical for every value.  0 / -1 (frames < 0). */
int tiler_debug_load_chunk(int64_t frames);

/* ---- Load-step input scaling (cbxScaling main.pas:4780-4782, 1042, main.lfm:524-545) fused with the tile cut ----
 * The reference's Load step has ffmpeg resize every picture (scale=iw*S:ih*S:flags=lanczos, S one of 0.25, 0.375,
 * 0.5, 0.75, 1, 1.5, 2) before ReframeUI crops it.  Here the resize runs on the device in front of the tile cut.
 * Parity with swscale's fixed-point Lanczos is NOT pinned: the arithmetic is Pillow's 8-bit
 * Image.resize(size, Image.LANCZOS), bit for bit -- one pass per axis, the horizontal one first, a pass skipped when
 * its axis keeps its size, an 8-bit clipped picture between the passes; per axis scale = in / out,
 * support = 3 * max(scale, 1), taps L((x + xmin - center + 0.5) / max(scale, 1)) with L(t) = sinc(t) sinc(t / 3),
 * normalised in double on the host, rounded to 22 fractional bits, result clip((2^21 + sum pixel * tap) >> 22).
 * out = floor(src * scale) per axis (exact for the seven factors).  -1 when scale is not finite and positive, or a
 * side comes out below 8 or above 16384. */
int tiler_scale_dims(int src_w, int src_h, double scale, int *out_w, int *out_h);
/* The tap table of one axis (host code; needs no GPU): returns ksize = 2 * ceil(3 * max(in / out, 1)) + 1 and fills
 * bounds[out][2] = (xmin, xmax) and taps[out][ksize] (tap x of output xx weighs source sample xmin + x; 0 past xmax).
 * cap = the int32 that taps holds (at least out * ksize).  bounds and taps both NULL: only ksize.  in and out are
 * 1 .. 2^24.  -1 on error. */
int tiler_scale_coeffs(int n_in, int n_out, int32_t *bounds, int32_t *taps, int64_t cap);
/* tiler_load_frames_dev / tiler_load_frames / tiler_load_clip_dev on the pictures resized to out_w x out_h (the
 * size, not the factor: ffmpeg's rounding of a fractional product is the caller's choice).  The tilemap is
 * tiler_load_dims(out_w, out_h); only the top-left tm_w*8 x tm_h*8 pixels of the resized picture are computed, and
 * source rows and columns beyond the last kept pixel's taps are never read.  out_w, out_h are 8 .. 16384 and at
 * least src / 8 per axis.  With out_w == src_w and out_h == src_h each call is its unscaled form.  Every argument
 * is checked before anything is launched: -1 with tiler_last_error() naming it.  F = 0 returns 0.  The tap tables
 * and the intermediate picture of a (src, out) size live in a small cache inside the library; calls on different
 * streams are ordered on the device where they share it. */
int tiler_load_frames_scaled_dev(const uint8_t *d_src, int fmt, int F, int src_w, int src_h, int64_t pitch,
                                 int64_t frame_stride, int out_w, int out_h, int32_t *d_rgb, void *stream);
int tiler_load_frames_scaled(const uint8_t *src, int fmt, int F, int src_w, int src_h, int64_t pitch,
                             int64_t frame_stride, int out_w, int out_h, int32_t *rgb);
/* Correlations and the keyframe split come from the scaled frames, as the reference takes them from the scaled
 * pictures.  Returns the keyframe count or -1. */
int tiler_load_clip_scaled_dev(const uint8_t *d_src, int fmt, int F, int src_w, int src_h, int64_t pitch,
                               int64_t frame_stride, int out_w, int out_h, int32_t *d_rgb, double *corr,
                               int32_t *kf_of_frame, void *stream);

/* ---- Quality readout (Render main.pas:3305-3493, lblCorrel main.pas:3470-3489) ------------------------
 * Render's destination frame from the tilemaps, as Render draws it with dithered, reduced and mirrored on and
 * palIdx < 0.  Items are [F][Q] arrays (Q = tm_w * tm_h positions): tile/pal/hm/vm the TileMap, sm_* / smoothed the
 * SmoothedTileMap (all five NULL: no Smooth was run); the item of a position is the smoothed one where
 * smoothed != 0 (main.pas:3416-3418).  palpix[T][64], thm/tvm[T] the tileset; pixel (ty, tx) reads
 * palpix[tile][tym*8+txm] with txm = 7-tx iff hm xor thm[tile], tym = 7-ty iff vm xor tvm[tile] (DrawTile
 * main.pas:3318-3324) and takes colour palettes[pal_row0[f] + pal][index] out of palettes[n_rows][palsize]
 * (0x00BBGGRR; pal_row0[F] = the row of palette 0 of the frame's keyframe, n_palettes per keyframe).
 * out_rgb[F][Q][64] int32 0x00BBGGRR, tile-major (the layout FrameTiling and keyframe detection take frames in).
 * Positions whose tile is outside [0, T) or whose pal is outside [0, n_palettes) (the reference skips them,
 * main.pas:3422 / 3432, leaving the hatch brush) render 0 and are counted in invalid[F] (or NULL).  0 / -1. */
int tiler_render_frames(int F, int Q, const int32_t *tile, const int32_t *pal, const uint8_t *hm, const uint8_t *vm,
                        const int32_t *sm_tile, const int32_t *sm_pal, const uint8_t *sm_hm, const uint8_t *sm_vm,
                        const uint8_t *smoothed, int T, const uint8_t *palpix, const uint8_t *thm, const uint8_t *tvm,
                        int n_rows, int palsize, const int32_t *palettes, const int32_t *pal_row0, int n_palettes,
                        int32_t *out_rgb, int32_t *invalid);
/* Same with every array in HBM (out_rgb 16-byte, palpix 4-byte aligned); asynchronous on stream. */
int tiler_render_frames_dev(int F, int Q, const int32_t *d_tile, const int32_t *d_pal, const uint8_t *d_hm,
                            const uint8_t *d_vm, const int32_t *d_sm_tile, const int32_t *d_sm_pal,
                            const uint8_t *d_sm_hm, const uint8_t *d_sm_vm, const uint8_t *d_smoothed, int T,
                            const uint8_t *d_palpix, const uint8_t *d_thm, const uint8_t *d_tvm, int n_rows, int palsize,
                            const int32_t *d_palettes, const int32_t *d_pal_row0, int n_palettes, int32_t *d_out_rgb,
                            int32_t *d_invalid, void *stream);
/* The figure under Render: corr[f] = ComputeCorrelationBGR(oriCorr, chgCorr) (main.pas:769-788) of source frame f
 * against rendered frame f, both [tm_h*tm_w][64] tile-major, over the raster copy followed by the transposed copy
 * (main.pas:3472-3486), bit-identical to the reference's sequential fp64 PearsonCorrelation (main.pas:1465-1492).
 * sse[f][3]: the exact sum of squared byte differences of the R, G, B channels.  corr[F] and sse[F][3] are host
 * arrays (either may be NULL).  0 / -1. */
int tiler_frame_quality(const int32_t *src, const int32_t *dst, int F, int tm_w, int tm_h, double *corr,
                        uint64_t *sse);
/* Same with the frames in HBM (16-byte aligned); synchronous on stream. */
int tiler_frame_quality_dev(const int32_t *d_src, const int32_t *d_dst, int F, int tm_w, int tm_h, double *corr,
                            uint64_t *sse, void *stream);

/* ---- Dither step, per tile (FinishDitherTiles main.pas:2482-2544) -------------------------
 * For n frame tiles rgb[n][64] (0x00BBGGRR) and their keyframe palette pal_of[n] (DitheringPalIndex) out of
 * palettes[n_palettes][palsize] (PaletteRGB, palsize 1, 2, 4, 8, 16, 32 or 64): DitherTile with Thomas Knoll mixing
 * (the default, main.pas:1998-2055 / 1828-1875) then PrepareTileMirrors (main.pas:4049-4069) ->
 * palpix[n][64] palette indices in canonical orientation, hm/vm[n] (TTile.HMirror / VMirror).
 * Palette generation (yakmo k-means) and DitheringPalIndex selection are not part of this call.  0 / -1. */
int tiler_dither_tiles(int n, const int32_t *rgb, const int32_t *pal_of, const int32_t *palettes, int n_palettes,
                       int palsize, uint8_t *palpix, uint8_t *hm, uint8_t *vm);
/* Same with every array in HBM; asynchronous on stream. */
int tiler_dither_tiles_dev(int n, const int32_t *d_rgb, const int32_t *d_pal_of, const int32_t *d_palettes,
                           int n_palettes, int palsize, uint8_t *d_palpix, uint8_t *d_hm, uint8_t *d_vm, void *stream);
/* The same step with Yliluoma mixing instead (chkUseTK unchecked, main.lfm:272-282): DitherTile's other branch
 * (main.pas:2055-2067) with DeviseBestMixingPlanYliluoma (main.pas:1573-1826, the ASM_DBMP form the reference build
 * compiles), mixed_colors = FY2MixedColors (cbxYilMix: 1, 2, 4 (the form's default), 8, 16; here 1..64), palsize
 * 1..16 (any size), 32 or 64.  Then PrepareTileMirrors as above.  0 / -1. */
int tiler_dither_tiles_yliluoma(int n, const int32_t *rgb, const int32_t *pal_of, const int32_t *palettes,
                                int n_palettes, int palsize, int mixed_colors, uint8_t *palpix, uint8_t *hm,
                                uint8_t *vm);
int tiler_dither_tiles_yliluoma_dev(int n, const int32_t *d_rgb, const int32_t *d_pal_of, const int32_t *d_palettes,
                                    int n_palettes, int palsize, int mixed_colors, uint8_t *d_palpix, uint8_t *d_hm,
                                    uint8_t *d_vm, void *stream);

/* ---- Dither step, palette generation (QuantizePalette / FinishQuantizePalette) ------------
 * QuantizePalette with the default Dennis Lee v3 quantizer (chkUseDL3, main.pas:2154-2254 -> dl3quant,
 * dlquant/quantizer.c:437-663) for n_palettes (keyframe, palette) pairs at once: tiles rgb[n_tiles][64] (0x00BBGGRR,
 * each keyframe's frames in order), pal_of[n_tiles] the pair of each tile (DitheringPalIndex, stacked over
 * keyframes as kf * FPaletteCount + palette; out-of-range indices are skipped), active[n_tiles] or NULL (all
 * Active) -> palettes[n_palettes][palsize] (PaletteIndexes: the palsize DLv3 colours sorted by CompareCMULHS,
 * main.pas:2413-2417; 0 beyond a table that has fewer colours), use_count[n_palettes] (PaletteUseCount.UseCount),
 * colors[n_palettes] or NULL (the DLv3 colour-table size of each pair).  lookup_bpc = cbxDLBPC (7 by default,
 * 1..8).  Outputs are host arrays in both forms.  0 / -1. */
int tiler_quantize_palettes(long n_tiles, const int32_t *rgb, const int32_t *pal_of, const uint8_t *active,
                            int n_palettes, int palsize, int lookup_bpc, int32_t *palettes, int32_t *use_count,
                            int32_t *colors);
int tiler_quantize_palettes_dev(long n_tiles, const int32_t *d_rgb, const int32_t *d_pal_of, const uint8_t *d_active,
                                int n_palettes, int palsize, int lookup_bpc, int32_t *palettes, int32_t *use_count,
                                int32_t *colors, void *stream);
/* QuantizePalette with the value-at-risk path (chkUseDL3 unticked: DoValueAtRiskBased, main.pas:2256-2394) for
 * n_pairs (keyframe, palette) pairs at once.  rgb / pal_of / active as above; n_palettes = FPaletteCount (a pair's
 * PalIdx is pair mod n_palettes; it picks the gPalettePattern row and bounds CmlPct from below by
 * min(U, palsize * n_palettes)); acc0[n_pairs] = round(FrameCount * FTileMapSize * 64 * PalVAR) of each pair's
 * keyframe (main.pas:2325-2326: all of the keyframe's tiles, banker's rounding) -> palettes[n_pairs][palsize]
 * (PaletteIndexes: the picked items sorted by CompareCMULHS on their stored Luma / Val / Sat / Hue),
 * use_count[n_pairs], stats[n_pairs][4] = U (distinct colours), CmlPct, merges, stop reason (0: Count <= CmlPct,
 * 1: the round's best difference repeated).  Among colours of equal (Count, Hue, Val, Sat) the list order is colour
 * value ascending (the reference's unstable QuickSort leaves it undefined).  A pair without a colour (no Active tile)
 * fails the call, the message names the pair.  acc0 and the outputs are host arrays in both forms.  0 / -1. */
int tiler_quantize_palettes_var(long n_tiles, const int32_t *rgb, const int32_t *pal_of, const uint8_t *active,
                                int n_pairs, int palsize, int n_palettes, const int32_t *acc0, int32_t *palettes,
                                int32_t *use_count, int32_t *stats);
int tiler_quantize_palettes_var_dev(long n_tiles, const int32_t *d_rgb, const int32_t *d_pal_of,
                                    const uint8_t *d_active, int n_pairs, int palsize, int n_palettes,
                                    const int32_t *acc0, int32_t *palettes, int32_t *use_count, int32_t *stats,
                                    void *stream);
/* Test hook (process-wide) for the DLv3 merges: at most list_cap listed recount_next entries are kept in LDS
 * (list_cap <= 0 or above the built-in 1024 restores 1024); a smaller cap runs the global-memory overflow and the
 * multi-batch path on small tables.  Results are identical for every cap.  0. */
int tiler_debug_dl3(int list_cap);
/* PrepareDitherTiles for one keyframe (main.pas:2097-2152): ComputeTilePsyVisFeatures(UseLAB, use_wavelets,
 * gamma) of its n_tiles RGB tiles (frame order), then the k-means of yakmo_create(n_palettes, 1, MaxInt, k-means++,
 * seed, no normalisation) -> labels[n_tiles] (DitheringPalIndex), centroids[n_palettes][192] (PaletteCentroids),
 * *iterations (Lloyd assignments).  yakmo.dll is binary-only: the k-means is its published algorithm written out
 * exactly (DESIGN.md "Dither: palette generation"), not pinned to the DLL.  max_iter <= 0 means unbounded
 * (MaxInt).  Fewer than 2 tiles or palettes: labels 0, centroids 0.  Host arrays / device pointers.  0 / -1. */
int tiler_prepare_dither_tiles(long n_tiles, const int32_t *rgb, int n_palettes, int gamma, int use_wavelets,
                               int max_iter, uint32_t seed, int32_t *labels, double *centroids, int *iterations);
int tiler_prepare_dither_tiles_dev(long n_tiles, const int32_t *d_rgb, int n_palettes, int gamma, int use_wavelets,
                                   int max_iter, uint32_t seed, int32_t *d_labels, double *d_centroids,
                                   int *iterations, void *stream);
/* The k-means alone over X[n][d] (d <= 192, fp64, host arrays). */
int tiler_kmeans(const double *X, long n, int d, int k, int max_iter, uint32_t seed, int32_t *labels,
                 double *centroids, int *iterations);
/* FinishQuantizePalette's order of one keyframe's palettes (main.pas:2444-2455): the reference QuickSort
 * (kmodes.pas:89-136) by use count, descending -> lut[old palette] = new palette.  0 / -1. */
int tiler_finish_quantize_order(int n_palettes, const int32_t *use_count, int32_t *lut);

/* ---- GTM keyframe stream compression (host code) ---------------------------------------------------
 * Replaces LZCompress (extern.pas:202-240: temp file + external `lzma.exe e src dst -lc8 -eos`, called
 * per keyframe by SaveStream main.pas:4734).  Writes an LZMA-alone stream (13-byte header: properties
 * (pb*5+lp)*9+lc, dictionary size u32, uncompressed size u64 = all ones when eos != 0) into dst.
 * dst == NULL: only *out_len (the exact size) is computed; cap too small: -1 with *out_len = size needed.
 * 0 ok, -1 error (tiler_last_error). */
int tiler_lzma_encode(const uint8_t *src, size_t n, int lc, int lp, int pb, uint32_t dict_size, int eos,
                      uint8_t *dst, size_t cap, size_t *out_len);
/* ---- LZMA match tables: the match search of tiler_lzma_encode ahead of its parse, on the host or on the GPU ----
 * A match table holds, for every position p of a buffer, what the encoder's match finder answers there, as
 * len | dist << 9 in one uint32: len 0 (no match; the whole entry is 0) or 2..273, dist = the back distance - 1.
 * The finder's rule (hash chains of 2^18 buckets, depth 24, nice length 128): the candidates of p are the positions
 * q < p with q + 3 <= n whose three bytes hash to p's bucket (collisions included), nearest first; at most 24 are
 * looked at (one whose bytes differ at once still counts), the walk stops at the first with p - q > dict; with
 * lim = min(273, n - p) a candidate replaces the best only if strictly longer, and the walk ends after one of length
 * >= 128 or == lim; a result below 2, and every p with p + 3 > n, is 0.  That answer depends on the buffer and p
 * alone, so a parse that reads it from a table writes the stream of tiler_lzma_encode, byte for byte.  The packing
 * needs dict <= 2^21 (the GTM writer's dictionary): these entry points refuse a larger one.
 *
 * tiler_lzma_match_table: the table of src[0..n) into table[n] with the encoder's own finder (host code, no GPU). */
int tiler_lzma_match_table(const uint8_t *src, size_t n, uint32_t dict_size, uint32_t *table);
/* tiler_lzma_encode with the finder answered from table[n] (no hash chains are built).  Every entry the parse reads
 * is checked before it is acted on -- len <= min(273, n - p), dist + 1 <= p, dist < dict_size, and the len bytes
 * equal -- else -1, the message names the position: a wrong table never yields a stream that decodes to other bytes,
 * nor a read outside src.  table == NULL: tiler_lzma_encode. */
int tiler_lzma_encode_table(const uint8_t *src, size_t n, int lc, int lp, int pb, uint32_t dict_size, int eos,
                            const uint32_t *table, uint8_t *dst, size_t cap, size_t *out_len);
/* The tables of S streams that lie back to back in HBM (as tiler_gtm_commands_dev leaves them): stream k is
 * d_src[raw_off[k] .. raw_off[k + 1]) (raw_off: HOST, [S + 1], from 0, non-decreasing; d_src at any alignment), its
 * table d_table[raw_off[k] ..] (HBM, 4-byte aligned).  Streams never match across their borders.  One hash pass, one
 * stable radix sort of (stream, hash) with the position as value, and a kernel that compares a position with its up
 * to 24 predecessors in the sorted order.  Scratch is one stream-ordered block of at most 1 GiB (16 bytes per raw
 * byte and the sort's own), so whole streams are taken in batches of at most 2^26 bytes.  A stream longer than that
 * (or than 2^31 - 1 bytes) is left to the host finder: its part of d_table is not written.  Queued on `stream`
 * (asynchronous).  Returns the number of streams left without a table (0: none), or -1. */
int tiler_lzma_match_table_dev(const uint8_t *d_src, const int64_t *raw_off, int S, uint32_t dict_size,
                               uint32_t *d_table, void *stream);
/* One stream from host arrays (staged to HBM and back); a stream above the batch limit is answered by
 * tiler_lzma_match_table instead, so table[n] is always complete.  0 / -1. */
int tiler_lzma_match_table_gpu(const uint8_t *src, size_t n, uint32_t dict_size, uint32_t *table);
/* Test hook (process-wide): the scratch budget of tiler_lzma_match_table_dev in bytes (a batch holds at most
 * budget_bytes / 16 raw bytes; at least 1 KiB), 0 = the default, 1 GiB.  Tables are identical for every budget that
 * holds the longest stream.  Returns the previous budget, or -1. */
int64_t tiler_debug_lzma_match(int64_t budget_bytes);
/* The inverse (host code): one LZMA-alone stream at src[0..n) -> dst[0..cap); any valid lc / lp / pb, the end-marker
 * and the known-size form.  0: done, *out_len = the decoded bytes, *consumed (optional) = the compressed bytes the
 * stream took, header included, so concatenated streams can be walked.  TILER_LZMA_GROW: cap is too small -- *out_len
 * holds the size the header gives (known-size form; nothing was decoded) or the bytes that fitted (end-marker form):
 * grow the buffer and call again.  -1: corrupt or truncated input (tiler_last_error).  Never reads past n or writes
 * past cap. */
#define TILER_LZMA_GROW 1
int tiler_lzma_decode(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *out_len, size_t *consumed);

/* ---- GTM playback (the reference player, decoders/htmljs/gtm.player.js) ----------------------------
 * A .gtm file read back: the optional GTMv header + GTMk records, the LZMA-alone streams, the command tokens
 * (cmd = word & 63, arg = word >> 6), and a player that reproduces the reference player's framebuffer on the GPU.
 * Stricter than the JS player: a FrameEnd at a position != width * height, a skip or item past the end of the
 * tilemap, a tile index >= the tile count, a palette index never loaded, an unknown command, a truncated token and a
 * tile byte >= the palette size are errors naming the frame and the position.  Not supported (errors too): a second
 * SetDimensions that changes the size or tile count, and a TileSet after the first frame. */
#define TILER_GTM_SKIP_BLOCK 0
#define TILER_GTM_SHORT_TILE_IDX 1
#define TILER_GTM_LONG_TILE_IDX 2
#define TILER_GTM_LOAD_PALETTE 3
#define TILER_GTM_FRAME_END 28
#define TILER_GTM_TILE_SET 29
#define TILER_GTM_SET_DIMENSIONS 30
typedef struct tiler_gtm tiler_gtm;
typedef struct {
    int32_t width, height;  /* tilemap size in tiles; a frame is 8 width x 8 height pixels */
    uint32_t frame_ns;      /* SetDimensions' frame length */
    int32_t palsize;        /* TileSet's palette size */
    int64_t frames, keyframes, tiles;
    int64_t pal_rows;       /* R: palette versions, one per LoadPalette */
    int32_t has_header;     /* 1 when the file starts with GTMv */
    uint32_t avg_bytes_per_sec, kf_max_bytes_per_sec; /* the header's byte-rate fields (0 without a header) */
    int32_t streams;        /* LZMA-alone streams decoded */
    int64_t next_frame;     /* the frame the next play call starts at */
} tiler_gtm_info_t;
/* Parse data[0..n) (copied; host code, needs no GPU).  With a header the streams are split by CompressedSize and
 * decoded on up to `threads` threads (0: min(16, usable CPUs)), each checked to consume exactly its CompressedSize,
 * and KFCount / FrameCount / the dimensions are cross-checked against the streams; without one they are decoded one
 * after the other to the end of the data.  max_raw_bytes (0: 1 GiB) caps what one stream, and the tileset, may expand
 * to; the dense items may take 16 times that.  NULL on error. */
tiler_gtm *tiler_gtm_open(const uint8_t *data, size_t n, int threads, size_t max_raw_bytes);
int tiler_gtm_close(tiler_gtm *h);
int tiler_gtm_info(tiler_gtm *h, tiler_gtm_info_t *info);
/* Host getters (host memory only): tiles[T][64]; palettes[R][palsize] RGBA dwords as stored (byte 0 = R); the dense
 * items of frames [f0, f0 + n): tile[n][Q] (-1 = skipped), attrs[n][Q] (pal << 2 | V << 1 | H), palrow[n][Q] (the
 * palette version in effect when the item was drawn; -1 where skipped) -- any of the three may be NULL; per frame
 * kf_end[F] (FrameEnd bit 0), skipped[F], undrawn[F] (positions no frame so far has drawn) -- any may be NULL;
 * kf_start[KF + 1] (each keyframe's first frame, then F); raw[S] / comp[S] bytes of every stream.  0 / -1. */
int tiler_gtm_tiles(tiler_gtm *h, uint8_t *tiles);
int tiler_gtm_palettes(tiler_gtm *h, uint32_t *palettes);
int tiler_gtm_items(tiler_gtm *h, int64_t f0, int64_t n, int32_t *tile, uint16_t *attrs, int32_t *palrow);
int tiler_gtm_frame_flags(tiler_gtm *h, uint8_t *kf_end, int32_t *skipped, int32_t *undrawn);
int tiler_gtm_kf_start(tiler_gtm *h, int32_t *kf_start);
int tiler_gtm_stream_sizes(tiler_gtm *h, uint64_t *raw, uint64_t *comp);
/* Play the next n frames into HBM on stream (asynchronous; the only calls of a handle that need the device).  A drawn
 * item writes its 8x8 tile through the palette contents in effect at that moment (H mirrors x, V mirrors y); a
 * skipped position keeps its pixels, across keyframes and across a later reload of its palette index; a pixel no
 * item has drawn yet is opaque black.  A pixel is the stream's palette dword as stored, 0xAABBGGRR (AA = 0xFF in this
 * writer's streams; never drawn: 0xFF000000) -- mask the top byte to compare with the project's 0x00BBGGRR frames.
 * layout TILER_GTM_TILES: d_rgb[n][Q][64], the project's tile-major frames (tiler_frame_quality_dev takes them);
 * TILER_GTM_RASTER: d_rgb[n][8 height][8 width], what a player shows.  d_rgb is 16-byte aligned.  d_undrawn[n]
 * (optional) = the frame's count of never-drawn positions.  Plays on from the handle's position: the handle keeps each
 * position's last drawn item between calls.  After tiler_gtm_seek the next play call first rebuilds those items for
 * the new position, drawing nothing: it copies the nearest row at or before it of a checkpoint index -- the carried
 * items at the first frame of every s-th keyframe, s the smallest stride whose rows fit 256 MiB of HBM, built on the
 * device by the first call that needs it -- and walks the items between, at most s keyframes' frames however far into
 * the stream.  The picture is exactly what a play from frame 0 shows there, for any well-formed stream (keyframes
 * that begin with skipped items or reload a palette index included).  Returns the frames produced (fewer than n at
 * the end of the stream, then 0), or -1. */
#define TILER_GTM_TILES 0
#define TILER_GTM_RASTER 1
int64_t tiler_gtm_play_dev(tiler_gtm *h, int64_t n, int layout, int32_t *d_rgb, int32_t *d_undrawn, void *stream);
/* The same into host arrays. */
int64_t tiler_gtm_play(tiler_gtm *h, int64_t n, int layout, int32_t *rgb, int32_t *undrawn);
int tiler_gtm_rewind(tiler_gtm *h); /* the next play call starts at frame 0 with nothing drawn */
/* The next play call starts at `frame`, 0 <= frame <= frames (frames: the end, the next play returns 0).  Host code,
 * needs no GPU; clears the state a failed play call leaves.  Another frame: -1, the error names it and the range, and
 * the position stays.  Seeking to the current position changes nothing; tiler_gtm_seek(h, 0) is tiler_gtm_rewind. */
int tiler_gtm_seek(tiler_gtm *h, int64_t frame);
/* Random access: frames[0..n) in any order, repeats allowed -> request i's picture in d_rgb[i] (either layout, as
 * play) and d_undrawn[i] (optional), exactly as a play from frame 0 shows that frame.  The position of sequential
 * play and its carried items are not touched, and a failure does not disturb them.  Distinct frames are resolved
 * once, each checkpoint interval is walked once.  Every index is checked before the device is touched: one outside
 * [0, frames) is -1 naming the entry and its value; n = 0 returns 0 and needs no GPU.  Asynchronous on stream, on the
 * handle's device, ordered behind the handle's earlier calls like play.  Returns n or -1. */
int64_t tiler_gtm_frames_dev(tiler_gtm *h, const int64_t *frames, int64_t n, int layout, int32_t *d_rgb,
                             int32_t *d_undrawn, void *stream);
/* The same into host arrays. */
int64_t tiler_gtm_frames(tiler_gtm *h, const int64_t *frames, int64_t n, int layout, int32_t *rgb, int32_t *undrawn);
/* Tests: the items per pass of the seek and frames walks and the checkpoint index budget in bytes (0: the default, 2^22
 * items and 256 MiB), for handles that build their index afterwards.  Sequential play keeps its own pass size.
 * Negative: -1. */
int tiler_debug_gtm_seek(int64_t pass_items, int64_t index_bytes);

/* ---- GTM writing (SaveStream main.pas:4529-4763) -----------------------------------------------------
 * The SmoothedTileMaps of whole keyframes -> each keyframe's command stream, built on the GPU, LZMA-compressed on
 * the host (tiler_lzma_encode's lc 8, lp 0, pb 2, dictionary 2^21, end marker), and the .gtm container.
 * A keyframe's raw stream: for the first keyframe of the file only WriteTiles (SetDimensions, TileSet, 64 B per
 * tile), then WriteKFAttributes (LoadPalette per palette, colour | 0xFF000000), then per frame, restarted at every
 * frame: each maximal run of smoothed positions as SkipBlock words of at most 1024 positions, every other position
 * as Short/LongTileIdx (tile < 65536: one index word, else low then high word) with arg = pal << 2 | (vm ^
 * tvm[tile]) << 1 | (hm ^ thm[tile]), then FrameEnd (arg 1 on the keyframe's last frame).  Little-endian words.
 * Checked on the device, before a byte of output is written: a non-smoothed item's tile in [0, tiles) and pal in
 * [0, min(n_palettes, 256)); the error names the rule and the first offending (frame, position), lowest frame
 * first.  Smoothed positions are not looked at (the reference never reads their item). */
typedef struct {
    const int32_t *tile, *pal;         /* [frames][positions] */
    const uint8_t *hm, *vm, *smoothed; /* [frames][positions] flags: any non-zero value counts */
    const uint8_t *palpix;             /* [tiles][64]; read only when first_keyframe is set */
    const uint8_t *thm, *tvm;          /* [tiles] flags */
    const int32_t *palettes;           /* [keyframes][n_palettes][palsize] 0x00BBGGRR */
    const int32_t *kf_start;           /* HOST memory in every form: [keyframes + 1] rows, 0 < ... < frames */
    int64_t frames, positions, tiles;  /* positions = (width / 8) * (height / 8), at most 2^24 */
    int32_t keyframes, n_palettes, palsize;
    int32_t first_keyframe;            /* 1: stream 0 is the file's first keyframe and starts with WriteTiles */
    int32_t width, height;             /* pixels */
    double fps;
} tiler_gtm_source_t;
/* The raw command streams, back to back in d_raw (HBM, 2-byte aligned): stream k is [raw_off[k], raw_off[k + 1]);
 * raw_off (host, [keyframes + 1]) is always filled once the input has passed the checks.  d_raw == NULL: only the
 * sizes; cap < raw_off[keyframes]: -1 with raw_off filled.  The arrays of src are HBM pointers; the call waits once,
 * for the offsets, then queues the writing kernels on `stream` and returns.  0 / -1. */
int tiler_gtm_commands_dev(const tiler_gtm_source_t *src, uint8_t *d_raw, size_t cap, int64_t *raw_off, void *stream);
/* The same from host arrays into a host buffer. */
int tiler_gtm_commands(const tiler_gtm_source_t *src, uint8_t *raw, size_t cap, int64_t *raw_off);
/* The compressed streams of the given keyframes, back to back in dst (host), comp_len[keyframes] (host) each one's
 * size, *out_len their sum: what a caller that holds only some keyframes keeps until every stream is there
 * (tiler_gtm_assemble).  A stream is copied to the host and handed to a pool of at most `threads` compressor
 * threads (0: min(16, usable CPUs)) as soon as it is complete.  dst == NULL: only the sizes; cap too small: -1
 * with *out_len = the size needed.  _dev: src's arrays are HBM pointers and the device work runs on `stream`;
 * dst, comp_len and out_len are host memory, complete on return. */
int tiler_gtm_streams_dev(const tiler_gtm_source_t *src, int threads, uint8_t *dst, size_t cap, size_t *comp_len,
                          size_t *out_len, void *stream);
int tiler_gtm_streams(const tiler_gtm_source_t *src, int threads, uint8_t *dst, size_t cap, size_t *comp_len,
                      size_t *out_len);
/* The .gtm file (host code, needs no GPU) from every keyframe's compressed stream, back to back in comps:
 * TGTMHeader, one TGTMKeyFrameInfo per keyframe (RawSize 0 as the reference leaves it, KFMaxBytesPerSec over
 * keyframes k > 0 or the only one, FPC Round = ties to even), the streams.  kf_start[keyframes + 1]: the clip's,
 * 0 < ... < frame count.  dst / cap / out_len as above. */
int tiler_gtm_assemble(const uint8_t *comps, const size_t *comp_len, const int32_t *kf_start, int keyframes, int width,
                       int height, double fps, uint8_t *dst, size_t cap, size_t *out_len);
/* The whole file: tiler_gtm_streams over every keyframe of the clip (first_keyframe must be 1), then
 * tiler_gtm_assemble.  dst / cap / out_len as above; on any error dst is left untouched. */
int tiler_gtm_write_dev(const tiler_gtm_source_t *src, int threads, uint8_t *dst, size_t cap, size_t *out_len,
                        void *stream);
int tiler_gtm_write(const tiler_gtm_source_t *src, int threads, uint8_t *dst, size_t cap, size_t *out_len);
/* Process-wide switch (atomic), default 0.  On: tiler_gtm_streams(_dev) and tiler_gtm_write(_dev) queue
 * tiler_lzma_match_table_dev behind the command kernels, copy each stream's table to the host with its bytes and
 * compress with tiler_lzma_encode_table; a stream the table call leaves out is compressed as with the switch off.
 * The files are the same, byte for byte.  Returns the previous value. */
int tiler_gtm_set_gpu_matches(int on);

#ifdef __cplusplus
}
#endif
#endif
