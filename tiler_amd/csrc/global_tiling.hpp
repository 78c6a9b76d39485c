// global_tiling.hpp -- DoGlobalTiling's K-Modes branch (main.pas:4256-4343, DoKModes 4195-4254, MergeTiles 3688-3712)
// on gfx950 (internal interface; the contracts are in include/tiler_ann.h).
#pragma once
#include "tiler_common.hpp"

namespace tiler {
constexpr int GT_MAX_PALETTES = 4096;  // bins of a call: one LDS counter each in the histogram kernel
constexpr int GT_MAX_DESIRED = 1 << 30;

// EqualQualityTileCount shares (host only, no device): k[p] = round(ClusterCount), run[p] = size > ClusterCount
int global_tiling_counts(const int32_t *bin_size, int n_palettes, int desired, int32_t *k, uint8_t *run);
// the argument checks of the two forms below that need no device
int global_tiling_check_args(long nt, int n_palettes, int palsize, int desired);

int global_tiling_dev(uint8_t *d_palpix, const int32_t *d_dith_pal, uint8_t *d_active, int64_t *d_use_count,
                      int64_t *d_merge_index, long nt, int n_palettes, int palsize, int desired, int restart,
                      int32_t *bin_size, int32_t *k, int32_t *start, hipStream_t st);
int global_tiling_host(uint8_t *palpix, const int32_t *dith_pal, uint8_t *active, int64_t *use_count,
                       int64_t *merge_index, long nt, int n_palettes, int palsize, int desired, int restart,
                       int32_t *bin_size, int32_t *k, int32_t *start);
int tile_dataset_lines_dev(const uint8_t *d_palpix, long nt, int palsize, uint8_t *d_lines, int32_t *d_pal_signi,
                           hipStream_t st);
int tile_dataset_lines_host(const uint8_t *palpix, long nt, int palsize, uint8_t *lines, int32_t *pal_signi);
// medoid[sum k] (bin-local rows, -1 for an empty cluster) and counts[sum k] in HBM; bin_off / k are host arrays
int kmodes_medoids_batch_devout(const uint8_t *d_X, const int32_t *h_boff, int nb, const int32_t *h_k,
                                const int32_t *d_labels, const uint8_t *d_centroids, int32_t *d_medoid,
                                int32_t *d_counts, hipStream_t st);
}  // namespace tiler
