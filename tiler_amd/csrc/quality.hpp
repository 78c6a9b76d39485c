// quality.hpp -- quality readout: Render's destination frame (main.pas:3305-3493) and its lblCorrel figure
// (ComputeCorrelationBGR main.pas:769-788 over the raster + transposed copies, main.pas:3470-3489) on gfx950 (internal).
#pragma once
#include "tiler_common.hpp"

namespace tiler {
// Tilemap items [F][Q] (the sm_* / smoothed arrays all NULL: no Smooth was run) -> out_rgb[F][Q][64] int32 0x00BBGGRR,
// tile-major; invalid[F] (or NULL) counts the positions whose tile / palette is out of range (rendered 0).
// Every buffer in HBM; asynchronous on `stream`.
int render_frames_dev(int F, int Q, const int32_t *d_tile, const int32_t *d_pal, const uint8_t *d_hm,
                      const uint8_t *d_vm, const int32_t *d_sm_tile, const int32_t *d_sm_pal, const uint8_t *d_sm_hm,
                      const uint8_t *d_sm_vm, const uint8_t *d_smoothed, int T, const uint8_t *d_palpix,
                      const uint8_t *d_thm, const uint8_t *d_tvm, int n_rows, int palsize, const int32_t *d_palettes,
                      const int32_t *d_pal_row0, int n_palettes, int32_t *d_out_rgb, int32_t *d_invalid,
                      hipStream_t stream);
// the same with host arrays
int render_frames_host(int F, int Q, const int32_t *tile, const int32_t *pal, const uint8_t *hm, const uint8_t *vm,
                       const int32_t *sm_tile, const int32_t *sm_pal, const uint8_t *sm_hm, const uint8_t *sm_vm,
                       const uint8_t *smoothed, int T, const uint8_t *palpix, const uint8_t *thm, const uint8_t *tvm,
                       int n_rows, int palsize, const int32_t *palettes, const int32_t *pal_row0, int n_palettes,
                       int32_t *out_rgb, int32_t *invalid);
// frames [F][tm_h*tm_w][64] in HBM (16-byte aligned); corr[F] and sse[F][3] (R, G, B) are HOST buffers (either may
// be NULL); synchronises `stream`
int frame_quality_dev(const int32_t *d_src, const int32_t *d_dst, int F, int tm_w, int tm_h, double *corr,
                      uint64_t *sse, hipStream_t stream);
int frame_quality_host(const int32_t *src, const int32_t *dst, int F, int tm_w, int tm_h, double *corr, uint64_t *sse);
}  // namespace tiler
