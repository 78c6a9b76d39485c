// raster_dev.hpp -- device helpers the raster kernels share (load.hip, scale.hip).
#pragma once
#include "tiler_common.hpp"

namespace tiler {

// dword j of a span row whose first byte is al[s]: whole where it lies inside [s, s + n), else its bytes that do
__device__ __forceinline__ uint32_t fetch_dword(const uint8_t *al, int s, int n, int j, int nd) {
    uint32_t v = 0;
    const int lo = 4 * j;
    if (j < nd) {
        if (lo >= s && lo + 4 <= s + n) {
            v = *(const uint32_t *)(al + lo);
        } else {
            for (int b = 0; b < 4; b++)
                if (lo + b >= s && lo + b < s + n) v |= (uint32_t)al[lo + b] << (8 * b);
        }
    }
    return v;
}

}  // namespace tiler
