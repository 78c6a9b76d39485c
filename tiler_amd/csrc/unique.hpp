// unique.hpp -- MakeTilesUnique (main.pas:2555-2612), the exact duplicate-tile merge, on gfx950 (internal interface).
#pragma once
#include "tiler_common.hpp"

namespace tiler {
// MakeTilesUnique over nseg consecutive segments [seg_off[s], seg_off[s+1]) of nt tiles (seg_off on the host,
// non-decreasing from 0 to nt): inside a segment the Active tiles with identical PalPixels merge into the lowest index
// (MergeTiles main.pas:3688-3712: UseCount summed, Active cleared, MergeIndex = the survivor, PalPixels zeroed), less
// the reference's last-member quirk (see unique.hip).  palpix [nt][64] / active [nt] / use_count [nt] in and out,
// merge_index [nt] out (-1: not merged).  Device pointers (palpix 16-byte aligned); synchronous on st.  0 / -1
int make_tiles_unique_dev(uint8_t *d_palpix, uint8_t *d_active, int64_t *d_use_count, int64_t *d_merge_index, long nt,
                          const int64_t *seg_off, int nseg, hipStream_t st);
int make_tiles_unique_host(uint8_t *palpix, uint8_t *active, int64_t *use_count, int64_t *merge_index, long nt,
                           const int64_t *seg_off, int nseg);
// test hook: keep only the low hash_bits bits of a tile's hash (0: every tile probes one chain), -1 = the default
int unique_debug(int hash_bits);
}  // namespace tiler
