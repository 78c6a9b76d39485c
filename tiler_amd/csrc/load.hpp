// load.hpp -- the Load step's front door (LoadFrame main.pas:3211-3286, ReframeUI main.pas:1931-1938) on gfx950:
// raster pictures as a decoder leaves them -> the project's tile-major frames, and back (internal).
#pragma once
#include "tiler_common.hpp"

namespace tiler {

// Byte orders of a raster pixel (tiler_ann.h: TILER_PIX_*).  Tiles are int32 0x00BBGGRR = bytes R,G,B,0.
enum PixFmt : int { PIX_RGB24 = 0, PIX_BGR24 = 1, PIX_BGRA32 = 2, PIX_RGBA32 = 3, PIX_COUNT = 4 };
inline int pix_bytes(int fmt) { return fmt == PIX_RGB24 || fmt == PIX_BGR24 ? 3 : 4; }

// ReframeUI: tm_w = min(src_w div 8, 240), tm_h = min(src_h div 8, 135); -1 when a side is below 8
int load_dims(int src_w, int src_h, int *tm_w, int *tm_h);

// Every argument of a load / store call, checked on the host before anything touches the device: 0, or -1 with the
// error naming the argument.  `dev`: the tile array is a device pointer and must be 16-byte aligned.
int load_check(const char *who, const void *src, int fmt, int F, int src_w, int src_h, int64_t pitch,
               int64_t frame_stride, const void *rgb, bool dev);
int store_check(const char *who, const void *rgb, int F, int tm_w, int tm_h, int fmt, const void *dst, int64_t pitch,
                int64_t frame_stride, bool dev);

// Pictures in HBM: row j of frame f at d_src + f * frame_stride + j * pitch (bytes, any alignment) ->
// d_rgb[F][tm_h * tm_w][64].  Asynchronous on `stream`.  The arguments have passed load_check.
int load_frames_dev(const uint8_t *d_src, int fmt, int F, int src_w, int src_h, int64_t pitch, int64_t frame_stride,
                    int32_t *d_rgb, hipStream_t stream);
// The inverse: d_rgb[F][tm_h * tm_w][64] -> tm_w * 8 x tm_h * 8 pictures; a row's bytes past tm_w * 8 * bpp are not
// written; the X byte of the 32-bit formats is 0xFF.  Asynchronous on `stream`.
int store_frames_dev(const int32_t *d_rgb, int F, int tm_w, int tm_h, int fmt, uint8_t *d_dst, int64_t pitch,
                     int64_t frame_stride, hipStream_t stream);
// Host arrays, staged in chunks of whole frames (load_chunk_frames) on a pool stream: only the bytes of the used
// rectangle travel, so padding is neither read (load) nor written (store).
int load_frames_host(const uint8_t *src, int fmt, int F, int src_w, int src_h, int64_t pitch, int64_t frame_stride,
                     int32_t *rgb);
int store_frames_host(const int32_t *rgb, int F, int tm_w, int tm_h, int fmt, uint8_t *dst, int64_t pitch,
                      int64_t frame_stride);
// load_frames_dev, then the correlations and the keyframe split from the tiles; synchronises `stream`.  Returns the
// keyframe count or -1.
int load_clip_dev(const uint8_t *d_src, int fmt, int F, int src_w, int src_h, int64_t pitch, int64_t frame_stride,
                  int32_t *d_rgb, double *corr, int32_t *kf_of_frame, hipStream_t stream);
// Test hook: frames per chunk of the host forms (0: the default, LOAD_CHUNK_BYTES of picture + tile bytes)
int load_chunk_debug(int64_t frames);
// Frames per staging chunk of a host form whose frame takes frame_bytes of device memory (picture + tiles)
int load_chunk_frames(int F, int64_t frame_bytes);

constexpr int64_t LOAD_CHUNK_BYTES = 256ll << 20;
}  // namespace tiler
