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
// host only: the next play call starts at `frame` (0 <= frame <= frames) on the framebuffer a play from frame 0 shows
// there; it rebuilds the carried items from the checkpoint index (play.hip) before its first pass
int player_seek(Player *p, int64_t frame);
// host only: n >= 0, a known layout and every frames[i] inside the stream, else -1 naming the entry
int player_check_frames(Player *p, const int64_t *frames, int64_t n, int layout);
// frames[0..n), any order, repeats allowed: request i into d_rgb[i] and d_undrawn[i] (or NULL), as play shows them;
// neither the next frame nor the carried items of sequential play are touched.  Returns n or -1
int64_t player_frames_dev(Player *p, const int64_t *frames, int64_t n, int layout, int32_t *d_rgb, int32_t *d_undrawn,
                          hipStream_t stream);
int64_t player_frames_host(Player *p, const int64_t *frames, int64_t n, int layout, int32_t *rgb, int32_t *undrawn);
// the pass size (items) of the seek paths and the index budget (bytes), 0 = the default; for handles that build their
// index afterwards
int player_seek_debug(int64_t pass_items, int64_t index_bytes);
}  // namespace tiler
