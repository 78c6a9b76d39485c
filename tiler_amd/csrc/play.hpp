// play.hpp -- GTM playback: a parsed .gtm file (gtm_read.hpp) and its frame player on gfx950 (internal).
#pragma once
#include "gtm_read.hpp"
#include "tiler_common.hpp"

namespace tiler {
struct Player;
// host only (no device is touched until the first play call); nullptr with set_error()
Player *player_open(const uint8_t *data, size_t n, int threads, size_t max_raw);
// releases the device buffers on the device they live on (the caller makes it current: player_device)
void player_close(Player *p);
const GtmData &player_data(const Player *p);
int64_t player_next_frame(Player *p);
int player_device(const Player *p);  // -1 until the first play call
// the next n frames into d_rgb (layout 0 tile-major [n][Q][64], 1 raster [n][8 H][8 W]; 16-byte aligned) and
// d_undrawn[n] (or NULL) on `stream`, asynchronous; returns the frames produced or -1
int64_t player_play_dev(Player *p, int64_t n, int layout, int32_t *d_rgb, int32_t *d_undrawn, hipStream_t stream);
int64_t player_play_host(Player *p, int64_t n, int layout, int32_t *rgb, int32_t *undrawn);
int player_rewind(Player *p);
}  // namespace tiler
