// reload.hpp -- ReloadPreviousTiling's tile matcher (main.pas:4372-4470) on gfx950 (internal interface).
#pragma once
#include "tiler_common.hpp"

namespace tiler {
struct Tileset;  // a loaded .gts tileset, resident in HBM: dataset lines, prepared rows, PalSigni buckets

// raw [n][64] file bytes (host), rescaled (v * palsize) div file_palsize; nullptr on error
Tileset *tileset_load(const uint8_t *raw, long n, int file_palsize, int palsize);
void tileset_destroy(Tileset *ts);
int tileset_device(const Tileset *ts);
long tileset_rows(const Tileset *ts);
// DoFindBest over nt tiles: palpix [nt][64] in/out, active [nt], idx [nt] (file-order row, -1 = inactive), dis [nt]
// (idx / dis may be null).  Device pointers (palpix 16-byte aligned); synchronous on st.  0 / -1
int tileset_match_dev(Tileset *ts, uint8_t *d_palpix, const uint8_t *d_active, long nt, int32_t *d_idx,
                      uint64_t *d_dis, hipStream_t st);
int tileset_match_host(Tileset *ts, uint8_t *palpix, const uint8_t *active, long nt, int32_t *idx, uint64_t *dis);
// batched GetMinMatchingDissim: rows [n][80], group g = rows [grp_off[g], grp_off[g+1]) (grp_off on the host), items
// [m][80] each searched in the group item_grp[i] (-1, out of range or an empty group: all rows); idx = row index
// (-1 when n = 0), ties to the last row.  rows / items / item_grp / idx / dis device pointers.  0 / -1
int min_dissim_groups_dev(const uint8_t *d_rows, long n, const int32_t *grp_off, int ngroups, const uint8_t *d_items,
                          const int32_t *d_item_grp, long m, int32_t *d_idx, uint64_t *d_dis, hipStream_t st);
int min_dissim_groups_host(const uint8_t *rows, long n, const int32_t *grp_off, int ngroups, const uint8_t *items,
                           const int32_t *item_grp, long m, int32_t *idx, uint64_t *dis);
// test / study hooks: queries per pass, queries per thread of the argmin kernel (1 or 2), row slices per query block
// (0 = the default of each)
int reload_debug(long chunk, int qpt, int slices);
// (query, row) dissimilarities the last match / min_dissim_groups call of the process evaluated
long long reload_last_pairs();
}  // namespace tiler
