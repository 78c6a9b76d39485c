// lzma_match.hpp -- LZMA match tables on gfx950 (lzma_match.hip): what tiler_lzma_encode's match finder answers at
// every position of a set of streams, computed for all positions at once.  See include/tiler_ann.h.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace tiler {

// The tables of S streams back to back in HBM, queued on `stream` (a hipStream_t).  has (optional): has[k] = 1 when
// stream k's table is written, 0 when the stream is left to the host finder (longer than a batch, or than 2^31 - 1).
// Returns the number of streams left out, or -1 with set_error().
int lzma_match_table_dev(const uint8_t *d_src, const int64_t *raw_off, int S, uint32_t dict, uint32_t *d_table,
                         void *stream, std::vector<uint8_t> *has);
int lzma_match_table_host(const uint8_t *src, size_t n, uint32_t dict, uint32_t *table);
int64_t lzma_match_debug(int64_t budget_bytes);

}  // namespace tiler
