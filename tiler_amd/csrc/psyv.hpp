// psyv.hpp -- descriptor kernel interface (internal).
#pragma once
#include "tiler_common.hpp"

namespace tiler {

enum { PSYV_FROM_PAL = 1, PSYV_WAVELETS = 2, PSYV_LAB = 4, PSYV_QWEIGHT = 8, PSYV_HMIRROR = 16, PSYV_VMIRROR = 32 };

struct PsyvArgs {
    long n = 0;
    const int32_t *rgb = nullptr;       // [n][64]
    const uint8_t *palpix = nullptr;    // [T][64]
    const int32_t *tile_of = nullptr;   // [n] or null (identity)
    const int32_t *palettes = nullptr;  // [P][palsize]
    int palsize = 16;                   // palette stride (FTilePaletteSize); a tile byte >= palsize reads colour 0
    const int32_t *pal_of = nullptr;    // [n] or null (palette 0)
    const uint8_t *flags_per = nullptr; // [n] or null
    bool flags_per_mirrors_only = false; // flags_per holds only PSYV_HMIRROR / PSYV_VMIRROR bits (caller's promise)
    int flags = 0;
    int gamma = -1;
    double *out64 = nullptr;            // [n][192]
    float *out32 = nullptr;             // [n][192]
    // optional (RGB Haar query path only): annBoxDistance of the fp32 descriptor to box[2][192] (a kd-tree's
    // enclosing box, kdtree.hpp) -> rootbox[n], fused so the FrameTiling search's pruning check needs no re-read
    const float *box = nullptr;
    float *rootbox = nullptr;
    // optional (RGB Haar query path only): descriptor i is made of tile rgb[perm[i]] (FrameTiling's flat grouping)
    const int *perm = nullptr;
    // filled by launch_psyv from the shared LUTs
    const double *gamma_lut = nullptr, *dct_lut = nullptr, *qmul = nullptr, *ratio = nullptr, *lab_lin = nullptr;
    double haar_f = 0, u_mul = 0, v_mul = 0;
};

int launch_psyv(PsyvArgs args, hipStream_t stream);
int psyv_lane_items_debug(long min_items);  // tiler_debug_psyv_lane_items

// host-buffer form (tiler_psyv_batch[_ps]): palpix [n_tiles][64] and palettes [n_palettes][palsize] are read only
// when the descriptors come from palettes (PSYV_FROM_PAL or flags_per); a tile byte >= palsize is an error;
// out64 / out32: either or both
int psyv_batch_host(int n, const int32_t *rgb, int n_tiles, const uint8_t *palpix, const int32_t *tile_of,
                    int n_palettes, int palsize, const int32_t *palettes, const int32_t *pal_of,
                    const uint8_t *flags_per, int flags, int gamma, double *out64, float *out32);

// the palette sizes the descriptor paths take (cbxPalSize offers 2..64; the tile bytes allow 256)
inline bool psyv_palsize_ok(int palsize) { return palsize >= 1 && palsize <= 256; }
// first tile of palpix[n_tiles][64] with a byte >= palsize, or -1
long first_bad_tile(const uint8_t *palpix, long n_tiles, int palsize);

}  // namespace tiler
