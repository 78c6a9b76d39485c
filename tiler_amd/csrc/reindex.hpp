// reindex.hpp -- Reindex (btnReindexClick main.pas:1199-1230, ReindexTiles 4483-4527) and the FinishMergeTiles
// tilemap remap (3722-3734) on gfx950 (internal interface; the contracts are in include/tiler_ann.h).
#pragma once
#include "tiler_common.hpp"

namespace tiler {
// every _dev form: device pointers, synchronous on st (one wait, for the error word / n_active).  0 / -1
int tile_use_count_dev(const int32_t *d_tile, long n_items, long nt, int64_t *d_use_count, uint8_t *d_active,
                       int accumulate, hipStream_t st);
int reindex_tiles_dev(const uint8_t *d_active, const int64_t *d_use_count, long nt, int64_t *d_idx_map,
                      int64_t *d_order, int64_t *n_active, hipStream_t st);
struct GatherArgs {  // tiler_gather_tiles' pairs (both null: skipped)
    const uint8_t *palpix, *thm, *tvm;
    const int32_t *dith_pal;
    const int64_t *use_count;
    uint8_t *palpix_out, *thm_out, *tvm_out;
    int32_t *dith_pal_out;
    int64_t *use_count_out;
};
int gather_tiles_dev(const int64_t *d_order, long n, const GatherArgs &a, long nt, hipStream_t st);
int remap_items_dev(int32_t *d_tile, long n_items, const int64_t *d_map, long nt, int keep_unmapped, hipStream_t st);

int tile_use_count_host(const int32_t *tile, long n_items, long nt, int64_t *use_count, uint8_t *active,
                        int accumulate);
int reindex_tiles_host(const uint8_t *active, const int64_t *use_count, long nt, int64_t *idx_map, int64_t *order,
                       int64_t *n_active);
int gather_tiles_host(const int64_t *order, long n, const GatherArgs &a, long nt);
int remap_items_host(int32_t *tile, long n_items, const int64_t *map, long nt, int keep_unmapped);
// test hook: the counting strategy, -1 = chosen by nt (0: LDS windows, 1: global atomics)
int reindex_debug(int strategy);
}  // namespace tiler
