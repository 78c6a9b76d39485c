// scale.hpp -- the Load step's input scaling (cbxScaling main.pas:4780-4782, 1042; ffmpeg scale=...:flags=lanczos)
// on gfx950, fused with the tile cut: raster pictures -> Lanczos-resized, tile-major frames (internal).
// The arithmetic is Pillow's 8-bit Image.resize(size, LANCZOS): one pass per axis, horizontal first, integer taps
// with 22 fractional bits built on the host in double, an 8-bit clipped picture between the passes.
#pragma once
#include "tiler_common.hpp"

namespace tiler {

constexpr int SCALE_PRECISION_BITS = 22;
constexpr int SCALE_MAX_OUT = 16384;  // largest side of a scaled picture
constexpr int SCALE_MAX_RATIO = 8;    // largest src / out per axis the kernels take (twice cbxScaling's smallest 0.25)

// out = floor(src * scale) per axis; -1 for a scale that is not finite and positive, an out below 8 or above
// SCALE_MAX_OUT
int scale_dims(int src_w, int src_h, double scale, int *out_w, int *out_h);
// One axis' tap table (host code, no GPU): returns ksize = 2 * ceil(3 * max(in / out, 1)) + 1, or -1.  bounds[out][2]
// = (xmin, xmax), taps[out][ksize] (0 past xmax); cap = the int32 taps holds.  Both null: only ksize.
int scale_coeffs(int n_in, int n_out, int32_t *bounds, int32_t *taps, int64_t cap);

// out_w / out_h against the source and the limits above; 0, or -1 with the error naming the argument
int scale_check(const char *who, int src_w, int src_h, int out_w, int out_h);

// load_frames_dev / load_frames_host / load_clip_dev on the pictures resized to out_w x out_h: d_rgb[F][tm_h * tm_w]
// [64] with (tm_w, tm_h) = load_dims(out_w, out_h).  Only the kept tm_w*8 x tm_h*8 pixels are computed, and no source
// row or column past their taps is read.  out == src is the unscaled call itself.  The arguments have passed
// load_check and scale_check.
int load_frames_scaled_dev(const uint8_t *d_src, int fmt, int F, int src_w, int src_h, int64_t pitch,
                           int64_t frame_stride, int out_w, int out_h, int32_t *d_rgb, hipStream_t stream);
int load_frames_scaled_host(const uint8_t *src, int fmt, int F, int src_w, int src_h, int64_t pitch,
                            int64_t frame_stride, int out_w, int out_h, int32_t *rgb);
int load_clip_scaled_dev(const uint8_t *d_src, int fmt, int F, int src_w, int src_h, int64_t pitch,
                         int64_t frame_stride, int out_w, int out_h, int32_t *d_rgb, double *corr,
                         int32_t *kf_of_frame, hipStream_t stream);

}  // namespace tiler
