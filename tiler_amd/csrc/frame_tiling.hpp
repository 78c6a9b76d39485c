// frame_tiling.hpp -- FrameTiling's batch stage (internal): RGB tiles -> descriptors -> search -> tilemap items.
#pragma once
#include "tiler_common.hpp"

namespace tiler {

struct NNIndex;  // nn_search.hpp
struct FtMaps;

// the stage's buffers, owned by the index (freed by nn_index_destroy)
struct FtScratch {
    float *qrows = nullptr;  // [cap_rows][192] fp32 descriptors of the searched tiles
    // a grouped or deduplicated batch [cap_flat]: fperm: searched position -> tile; dpos: tile -> searched position;
    // fflag: 1 = flat tile; fbcnt [3][blocks]: per-block counts (non-flat representatives, flat representatives, the
    // call's non-flat tiles; without dedupe only the first row, the non-flat tiles) and fcnt [4] their totals;
    // fidx .. fvm: the search's outputs in searched order
    int *fperm = nullptr, *dpos = nullptr, *fbcnt = nullptr, *fcnt = nullptr;
    uint8_t *fflag = nullptr;
    int *fidx = nullptr;
    float *ferr = nullptr;
    int32_t *ftile = nullptr, *fpal = nullptr;
    uint8_t *fhm = nullptr, *fvm = nullptr;
    // each distinct tile searched once: dkey / dmin [cap_tab]: the call's hash table (key, smallest tile index of the
    // key); dslot [cap_flat]: a tile's table slot; drep [cap_flat]: the tile whose result a tile takes (itself: a
    // representative)
    unsigned long long *dkey = nullptr;
    unsigned int *dmin = nullptr;
    int *dslot = nullptr, *drep = nullptr;
    size_t cap_rows = 0, cap_flat = 0, cap_tab = 0;
    int *h_cnt = nullptr;  // pinned [4]: the dedupe counts read back inside the call
};
void ft_scratch_free(FtScratch &f);  // (the caller has waited for the device: nn_index_destroy)

// tiler_debug_ft_dedup: 1 (default) distinct tiles of a FrameTiling call searched once, 0 off, 2 on with a 4-bit hash
void nn_set_ft_dedup(int mode);

int nn_frame_tiling_dev(NNIndex *ix, const int32_t *d_rgb, int Q, int use_wavelets, int gamma, int *d_idx,
                        float *d_err, const FtMaps *maps, hipStream_t stream);

}  // namespace tiler
