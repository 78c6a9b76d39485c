// gtm_read.hpp -- the .gtm container and command stream read back on the host (plain C++, no HIP headers).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace tiler {

constexpr size_t GTM_DEFAULT_MAX_RAW = (size_t)1 << 30;  // per-stream output cap (decompression bombs)
constexpr int GTM_MAX_PALROWS = 1 << 29;                 // palrow << 2 | V << 1 | H fits an int32

// Everything a .gtm file holds, validated: every tile index is < n_tiles, every tile byte < palsize, every palrow a
// row of `palettes`, every frame complete -- the player's kernels trust it.
struct GtmData {
    bool has_header = false;
    uint32_t avg_bytes_per_sec = 0, kf_max_bytes_per_sec = 0;  // the header's two byte-rate fields
    int width = 0, height = 0;                                 // tilemap size in tiles
    uint32_t frame_ns = 0;
    int64_t n_tiles = 0;
    int palsize = 0;
    std::vector<uint8_t> tiles;      // [n_tiles][64]
    std::vector<uint32_t> palettes;  // [R][palsize] RGBA dwords as stored: a new row for every LoadPalette
    // dense per-frame items [F][Q]: tile -1 = skipped; palrow = the row of `palettes` in effect when it was drawn
    std::vector<int32_t> tile, palrow;
    std::vector<uint16_t> attrs;
    std::vector<uint8_t> kf_end;     // [F] FrameEnd bit 0
    std::vector<int32_t> skipped;    // [F] skipped positions
    std::vector<int32_t> undrawn;    // [F] positions no frame up to this one has drawn
    std::vector<int32_t> kf_start;   // [KF + 1] first frame of every keyframe, then F
    std::vector<uint64_t> stream_raw, stream_comp;  // per LZMA stream: decoded / compressed bytes

    int64_t Q() const { return (int64_t)width * height; }
    int64_t frames() const { return (int64_t)kf_end.size(); }
    int64_t pal_rows() const { return palsize ? (int64_t)(palettes.size() / (size_t)palsize) : 0; }
    int64_t keyframes() const { return kf_start.empty() ? 0 : (int64_t)kf_start.size() - 1; }
};

// Parses `data`: the optional GTMv header and GTMk records, the LZMA-alone streams (with a header: split by
// CompressedSize and decoded on up to `threads` threads, 0 = min(16, usable CPUs); without: one after the other to
// the end of the data), then the command tokens.  max_raw = 0: GTM_DEFAULT_MAX_RAW.  false with set_error() on any
// malformed input.
bool gtm_parse(const uint8_t *data, size_t n, int threads, size_t max_raw, GtmData &out);

}  // namespace tiler
