// quality.hip -- the quality readout on gfx950: Render's destination frame (main.pas:3305-3493, dithered, reduced and
// mirrored on, palIdx < 0) from the tilemaps, and the figure Render prints under it, lblCorrel =
// ComputeCorrelationBGR(oriCorr, chgCorr) (main.pas:769-788 over the bitmaps' raster copy followed by their
// transposed copy, main.pas:3470-3489; PearsonCorrelation main.pas:1465-1492), plus the exact per-channel SSE.
//
// Element order of the Pearson pass.  W = 8 tm_w, H = 8 tm_h, L = 2 W H.  Element e = c L + i (channel-major,
// c = 0 red * 2126, 1 green * 7152, 2 blue * 722); pixel i < W H is raster (y = i div W, x = i mod W), pixel
// i >= W H is the transposed copy (j = i - W H: x = j div H, y = j mod H).  Frames are tile-major ([Q][64] int32
// 0x00BBGGRR), so the order is walked in GROUPS of 8 elements that are 8 pixels of one tile:
//   raster half      group (sy, tx):  tile (sy / 8, tx), row sy % 8          -> 8 consecutive words (two 16-byte loads)
//   transposed half  group (x, ty):   tile (ty, x / 8), column x % 8, top down -> 8 words 32 bytes apart
// Every (channel, half) block has 8 Q groups; a frame has 48 Q groups.
//
// Bit-exact plan, as keyframes.hip: the means are exact integer sums (parallel u64 reduction, one correctly rounded
// division each); the three chains num, denx, deny are rounded in the reference's order by one lane per frame.
// Producer waves compute the rounded terms of a stage of groups into LDS, one consumer wave adds them in order.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "quality.hpp"
#include "stage.hpp"

namespace tiler {

// ---- Render ---------------------------------------------------------------------------------------------------
// 16 threads per tilemap position, 4 pixels (one 16-byte store) each; 16 positions per workgroup.  The 4 palette
// indices of a thread are one aligned word of the tile's row (byte-reversed under a horizontal flip); the palette row
// (at most 64 bytes) is read through the cache -- 16 lanes of a position share it.
constexpr int RD_POS = 16;

__global__ __launch_bounds__(256) void render_frames_kernel(
    long n_pos, int Q, const int32_t *__restrict__ tile, const int32_t *__restrict__ pal, const uint8_t *__restrict__ hm,
    const uint8_t *__restrict__ vm, const int32_t *__restrict__ sm_tile, const int32_t *__restrict__ sm_pal,
    const uint8_t *__restrict__ sm_hm, const uint8_t *__restrict__ sm_vm, const uint8_t *__restrict__ smoothed, int T,
    const uint8_t *__restrict__ palpix, const uint8_t *__restrict__ thm, const uint8_t *__restrict__ tvm, int n_rows,
    int palsize, const int32_t *__restrict__ palettes, const int32_t *__restrict__ pal_row0, int n_palettes,
    int4 *__restrict__ out, int32_t *__restrict__ invalid) {
    const long pos = (long)blockIdx.x * RD_POS + (threadIdx.x >> 4);
    if (pos >= n_pos) return;
    const int t16 = threadIdx.x & 15;
    const int f = (int)(pos / Q);
    // TMItem := TileMap; if SmoothedTileMap.Smoothed then TMItem := SmoothedTileMap (main.pas:3416-3418)
    const bool sm = smoothed && smoothed[pos] != 0;
    const int ti = sm ? sm_tile[pos] : tile[pos];
    const int pi = sm ? sm_pal[pos] : pal[pos];
    const bool ih = (sm ? sm_hm[pos] : hm[pos]) != 0, iv = (sm ? sm_vm[pos] : vm[pos]) != 0;
    const long row = (long)pal_row0[f] + pi;
    // InRange(ti, 0, High(FTiles)) and InRange(PalIdx, 0, High(PaletteRGB)) (main.pas:3422, 3432); such items are
    // never used as an index
    const bool ok = ti >= 0 && ti < T && pi >= 0 && pi < n_palettes && row >= 0 && row < n_rows;
    int4 o = make_int4(0, 0, 0, 0);
    if (ok) {
        const bool fh = ih != (thm[ti] != 0), fv = iv != (tvm[ti] != 0);  // DrawTile main.pas:3318-3324
        const int ty = t16 >> 1, tx0 = (t16 & 1) * 4;
        const int tym = fv ? 7 - ty : ty;
        unsigned w = *reinterpret_cast<const unsigned *>(palpix + (long)ti * 64 + tym * 8 + (fh ? 4 - tx0 : tx0));
        if (fh) w = __builtin_bswap32(w);
        const int32_t *prow = palettes + row * palsize;
        int c[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int idx = (int)((w >> (8 * k)) & 0xffu);
            c[k] = idx < palsize ? (prow[idx] & 0x00ffffff) : 0;  // an index past the palette renders 0
        }
        o = make_int4(c[0], c[1], c[2], c[3]);
    } else if (t16 == 0 && invalid) {
        atomicAdd(&invalid[f], 1);
    }
    out[pos * 16 + t16] = o;
}

static bool render_args_ok(int F, int Q, const void *tile, const void *pal, const void *hm, const void *vm,
                           const void *sm_tile, const void *sm_pal, const void *sm_hm, const void *sm_vm,
                           const void *smoothed, int T, const void *palpix, const void *thm, const void *tvm, int n_rows,
                           int palsize, const void *palettes, const void *pal_row0, int n_palettes, const void *out) {
    if (F < 0 || Q <= 0 || T < 0 || n_rows < 0 || palsize <= 0 || palsize > 256 || n_palettes < 0) return false;
    const int n_sm = (sm_tile != nullptr) + (sm_pal != nullptr) + (sm_hm != nullptr) + (sm_vm != nullptr) +
                     (smoothed != nullptr);
    if (n_sm != 0 && n_sm != 5) return false;  // the smoothed items come all together or not at all
    if (F == 0) return true;
    if (!tile || !pal || !hm || !vm || !pal_row0 || !out) return false;
    if ((T > 0 && (!palpix || !thm || !tvm)) || (n_rows > 0 && !palettes)) return false;
    return true;
}

int render_frames_dev(int F, int Q, const int32_t *d_tile, const int32_t *d_pal, const uint8_t *d_hm,
                      const uint8_t *d_vm, const int32_t *d_sm_tile, const int32_t *d_sm_pal, const uint8_t *d_sm_hm,
                      const uint8_t *d_sm_vm, const uint8_t *d_smoothed, int T, const uint8_t *d_palpix,
                      const uint8_t *d_thm, const uint8_t *d_tvm, int n_rows, int palsize, const int32_t *d_palettes,
                      const int32_t *d_pal_row0, int n_palettes, int32_t *d_out_rgb, int32_t *d_invalid,
                      hipStream_t stream) {
    if (!render_args_ok(F, Q, d_tile, d_pal, d_hm, d_vm, d_sm_tile, d_sm_pal, d_sm_hm, d_sm_vm, d_smoothed, T, d_palpix,
                        d_thm, d_tvm, n_rows, palsize, d_palettes, d_pal_row0, n_palettes, d_out_rgb)) {
        set_error("render: invalid arguments");
        return -1;
    }
    if (F == 0) return 0;
    const long n_pos = (long)F * Q;
    const long blocks = (n_pos + RD_POS - 1) / RD_POS;
    if (blocks > 0x7fffffffL || (uintptr_t)d_out_rgb % 16 || (uintptr_t)d_palpix % 4) {
        set_error("render: too many positions, or out_rgb not 16-byte / palpix not 4-byte aligned");
        return -1;
    }
    if (d_invalid) TILER_HIP_CHECK(hipMemsetAsync(d_invalid, 0, (size_t)F * 4, stream));
    {
        KTimer tm("render", stream);
        hipLaunchKernelGGL(render_frames_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, n_pos, Q, d_tile, d_pal,
                           d_hm, d_vm, d_sm_tile, d_sm_pal, d_sm_hm, d_sm_vm, d_smoothed, T, d_palpix, d_thm, d_tvm,
                           n_rows, palsize, d_palettes, d_pal_row0, n_palettes, reinterpret_cast<int4 *>(d_out_rgb),
                           d_invalid);
    }
    TILER_HIP_CHECK(hipGetLastError());
    return 0;
}

int render_frames_host(int F, int Q, const int32_t *tile, const int32_t *pal, const uint8_t *hm, const uint8_t *vm,
                       const int32_t *sm_tile, const int32_t *sm_pal, const uint8_t *sm_hm, const uint8_t *sm_vm,
                       const uint8_t *smoothed, int T, const uint8_t *palpix, const uint8_t *thm, const uint8_t *tvm,
                       int n_rows, int palsize, const int32_t *palettes, const int32_t *pal_row0, int n_palettes,
                       int32_t *out_rgb, int32_t *invalid) {
    if (!render_args_ok(F, Q, tile, pal, hm, vm, sm_tile, sm_pal, sm_hm, sm_vm, smoothed, T, palpix, thm, tvm, n_rows,
                        palsize, palettes, pal_row0, n_palettes, out_rgb)) {
        set_error("render: invalid arguments");
        return -1;
    }
    if (F == 0) return 0;
    const size_t n = (size_t)F * Q;
    HostStage s("render");
    const int32_t *d_tile = s.in(tile, n), *d_pal = s.in(pal, n);
    const uint8_t *d_hm = s.in(hm, n), *d_vm = s.in(vm, n);
    const int32_t *d_sm_tile = s.in(sm_tile, n), *d_sm_pal = s.in(sm_pal, n);
    const uint8_t *d_sm_hm = s.in(sm_hm, n), *d_sm_vm = s.in(sm_vm, n), *d_smoothed = s.in(smoothed, n);
    // empty tile / palette tables keep a valid (never read) address
    const uint8_t *d_palpix = s.in(palpix, (size_t)T * 64), *d_thm = s.in(thm, (size_t)T), *d_tvm = s.in(tvm, (size_t)T);
    const int32_t *d_palettes = s.in(palettes, (size_t)n_rows * palsize), *d_row0 = s.in(pal_row0, (size_t)F);
    int32_t *d_out = s.out(out_rgb, n * 64), *d_invalid = s.out(invalid, (size_t)F);
    if (!s.ok() || render_frames_dev(F, Q, d_tile, d_pal, d_hm, d_vm, d_sm_tile, d_sm_pal, d_sm_hm, d_sm_vm, d_smoothed, T,
                                     d_palpix, d_thm, d_tvm, n_rows, palsize, d_palettes, d_row0, n_palettes, d_out,
                                     d_invalid, s.stream()))
        return -1;
    return s.finish();
}

// ---- Quality --------------------------------------------------------------------------------------------------
// per frame, exact u64: [0..2] Σ r, g, b of the source, [3..5] of the rendered frame, [6..8] Σ (byte difference)^2
constexpr int QL_SUMS = 9;

__global__ __launch_bounds__(256) void quality_sums_kernel(const int4 *__restrict__ src, const int4 *__restrict__ dst,
                                                             long vec_per_frame, unsigned long long *__restrict__ sums) {
    const int f = blockIdx.y;
    const int4 *a = src + (long)f * vec_per_frame, *b = dst + (long)f * vec_per_frame;
    unsigned long long acc[QL_SUMS] = {};
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < vec_per_frame; i += (long)gridDim.x * blockDim.x) {
        const int4 va = a[i], vb = b[i];
        const unsigned wa[4] = {(unsigned)va.x, (unsigned)va.y, (unsigned)va.z, (unsigned)va.w};
        const unsigned wb[4] = {(unsigned)vb.x, (unsigned)vb.y, (unsigned)vb.z, (unsigned)vb.w};
        unsigned s[QL_SUMS] = {};  // 4 pixels: at most 4 * 255^2
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int x = (int)((wa[k] >> (8 * c)) & 0xffu), y = (int)((wb[k] >> (8 * c)) & 0xffu);
                s[c] += (unsigned)x;
                s[3 + c] += (unsigned)y;
                s[6 + c] += (unsigned)((x - y) * (x - y));
            }
#pragma unroll
        for (int j = 0; j < QL_SUMS; j++) acc[j] += s[j];
    }
#pragma unroll
    for (int j = 0; j < QL_SUMS; j++) {
        unsigned long long v = acc[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&sums[(long)f * QL_SUMS + j], v);
    }
}

// Workgroup of 4 waves over QL_FRAMES = 16 frame pairs.  Unlike the inter-frame kernel of keyframes.hip the y term
// is the same lane's other frame (source against rendered), so no DPP row is involved and a 16-lane row is full.
//   waves 1-3 (producers): lane = (frame lane & 15, sub = lane >> 4); producer p handles group 12 s + 4 p + sub of
//     stage s: fetches its 8 words of both frames (register ring QL_PD stages ahead), computes the rounded terms
//     (x - mx)(y - my), (x - mx)^2, (y - my)^2 and stores them lane-contiguously (s_t[.][p][e][term][lane]: 512
//     consecutive bytes per store, no bank conflict);
//   wave 0 (consumer): lane & 15 = frame; reads the 16 doubles of (group, e, term) (rows 1-3 mirror row 0: identical
//     addresses broadcast) and does the three chained adds per element, in order.
constexpr int QL_FRAMES = 16;
constexpr int QL_PRODUCERS = 3;
constexpr int QL_STAGE_GROUPS = QL_PRODUCERS * 4;
constexpr int QL_PD = 2;

__global__ __launch_bounds__(256) void quality_chain_kernel(const int32_t *__restrict__ src,
                                                              const int32_t *__restrict__ dst, int F, int tm_w, int tm_h,
                                                              const unsigned long long *__restrict__ sums,
                                                              double *__restrict__ out) {
    __shared__ double s_t[2][QL_PRODUCERS][8][3][64];
    static_assert(sizeof(s_t) <= 160 * 1024, "stage ring exceeds the LDS");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int fi = lane & 15, sub = lane >> 4;
    const int f = blockIdx.x * QL_FRAMES + fi;
    const int fl = f < F ? f : F - 1;  // lanes past the end replay the last frame
    const int Q = tm_w * tm_h;
    const long fs = (long)Q * 64;
    const int total = 48 * Q;  // groups of a frame in summation order (Q <= 2^24)
    const int nstage = (total + QL_STAGE_GROUPS - 1) / QL_STAGE_GROUPS;
    if (w > 0) {
        const int p = w - 1;
        const unsigned long long *s = sums + (long)fl * QL_SUMS;
        // mean = Σ / (3 L): the transposed half doubles the raster sums; exact integers below 2^53, one division
        const double n3l = 6.0 * (double)fs;
        const double mx = (double)(2ull * (2126ull * s[0] + 7152ull * s[1] + 722ull * s[2])) / n3l;
        const double my = (double)(2ull * (2126ull * s[3] + 7152ull * s[4] + 722ull * s[5])) / n3l;
        const unsigned *a = reinterpret_cast<const unsigned *>(src) + fl * fs;
        const unsigned *b = reinterpret_cast<const unsigned *>(dst) + fl * fs;
        // group cursor: block blk = 2 c + half (6 = past the end), ca = major index (screen row sy / screen column
        // x), cb = minor index (tile column tx / tile row ty) of this lane's group of the next stage to fetch
        int blk = 0, ca = 0, cb = 0;
        int minor = tm_w, major = 8 * tm_h;
        auto advance = [&](int n) {
            cb += n;
            while (blk < 6 && cb >= minor) {
                cb -= minor;
                if (++ca == major) {
                    ca = 0;
                    ++blk;
                    minor = (blk & 1) ? tm_h : tm_w;
                    major = 8 * ((blk & 1) ? tm_w : tm_h);
                }
            }
        };
        advance(p * 4 + sub);
        unsigned ra[QL_PD][8], rb[QL_PD][8];
        int rc[QL_PD];
        auto fetch = [&](unsigned *va, unsigned *vb, int &vc) {
            // groups past the end re-read group 0 (never summed)
            const bool live = blk < 6;
            const int half = live ? (blk & 1) : 0, ga = live ? ca : 0, gb = live ? cb : 0;
            vc = live ? (blk >> 1) : 0;
            if (!half) {  // row ga & 7 of tile (ga >> 3, gb)
                const long o = ((long)(ga >> 3) * tm_w + gb) * 64 + (ga & 7) * 8;
                const uint4 a0 = *reinterpret_cast<const uint4 *>(a + o), a1 = *reinterpret_cast<const uint4 *>(a + o + 4);
                const uint4 b0 = *reinterpret_cast<const uint4 *>(b + o), b1 = *reinterpret_cast<const uint4 *>(b + o + 4);
                va[0] = a0.x, va[1] = a0.y, va[2] = a0.z, va[3] = a0.w;
                va[4] = a1.x, va[5] = a1.y, va[6] = a1.z, va[7] = a1.w;
                vb[0] = b0.x, vb[1] = b0.y, vb[2] = b0.z, vb[3] = b0.w;
                vb[4] = b1.x, vb[5] = b1.y, vb[6] = b1.z, vb[7] = b1.w;
            } else {  // column ga & 7 of tile (gb, ga >> 3), top down
                const long o = ((long)gb * tm_w + (ga >> 3)) * 64 + (ga & 7);
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    va[e] = a[o + 8 * e];
                    vb[e] = b[o + 8 * e];
                }
            }
            advance(QL_STAGE_GROUPS);
        };
#pragma unroll
        for (int q = 0; q < QL_PD; q++) fetch(ra[q], rb[q], rc[q]);
        for (int s0 = 0; s0 < nstage; s0 += QL_PD) {
#pragma unroll
            for (int q = 0; q < QL_PD; q++) {
                const int st = s0 + q;
                if (st < nstage) {
                    unsigned xa[8], xb[8];
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        xa[e] = ra[q][e];
                        xb[e] = rb[q][e];
                    }
                    const int c = rc[q];
                    if (st + QL_PD < nstage) fetch(ra[q], rb[q], rc[q]);
                    const unsigned sh = 8u * (unsigned)c;
                    const unsigned mul = c == 0 ? 2126u : c == 1 ? 7152u : 722u;  // cRedMul, cGreenMul, cBlueMul
                    double *buf = &s_t[st & 1][p][0][0][lane];
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        // (double)(byte * mul) exactly: 2^52 + v built from its bits, minus 2^52
                        const double xd =
                            __hiloint2double(0x43300000, (int)(__builtin_amdgcn_ubfe(xa[e], sh, 8u) * mul)) -
                            4503599627370496.0;
                        const double yd =
                            __hiloint2double(0x43300000, (int)(__builtin_amdgcn_ubfe(xb[e], sh, 8u) * mul)) -
                            4503599627370496.0;
                        const double dx = xd - mx, dy = yd - my;
                        buf[(e * 3 + 0) * 64] = dx * dy;
                        buf[(e * 3 + 1) * 64] = dx * dx;
                        buf[(e * 3 + 2) * 64] = dy * dy;
                    }
                    __syncthreads();
                }
            }
        }
        __syncthreads();
    } else {
        double acc_n = 0.0, acc_x = 0.0, acc_y = 0.0;
        __syncthreads();
        for (int st = 0; st < nstage; st++) {
            const double *buf = &s_t[st & 1][0][0][0][fi];
            const int left = total - st * QL_STAGE_GROUPS;
            if (left >= QL_STAGE_GROUPS) {
#pragma unroll
                for (int g = 0; g < QL_STAGE_GROUPS; g++)
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const double *t = buf + (((g >> 2) * 8 + e) * 3) * 64 + (g & 3) * 16;
                        acc_n = acc_n + t[0];
                        acc_x = acc_x + t[64];
                        acc_y = acc_y + t[128];
                    }
            } else {
                for (int g = 0; g < left; g++)
                    for (int e = 0; e < 8; e++) {
                        const double *t = buf + (((g >> 2) * 8 + e) * 3) * 64 + (g & 3) * 16;
                        acc_n = acc_n + t[0];
                        acc_x = acc_x + t[64];
                        acc_y = acc_y + t[128];
                    }
            }
            __syncthreads();
        }
        if (lane < QL_FRAMES && f < F) {
            out[(long)f * 3 + 0] = acc_n;
            out[(long)f * 3 + 1] = acc_x;
            out[(long)f * 3 + 2] = acc_y;
        }
    }
}

int frame_quality_dev(const int32_t *d_src, const int32_t *d_dst, int F, int tm_w, int tm_h, double *corr,
                      uint64_t *sse, hipStream_t stream) {
    if (F < 0 || tm_w <= 0 || tm_h <= 0 || (F > 0 && (!d_src || !d_dst))) {
        set_error("quality: invalid arguments");
        return -1;
    }
    if (F == 0 || (!corr && !sse)) return 0;
    if ((long)tm_w * tm_h > (1L << 24) || F > 65535 || (uintptr_t)d_src % 16 || (uintptr_t)d_dst % 16) {
        set_error("quality: frame too large, more than 65535 frames, or frames not 16-byte aligned");
        return -1;
    }
    const long fs = (long)tm_w * tm_h * 64;
    const size_t b_sums = (size_t)F * QL_SUMS * 8, b_out = (size_t)F * 3 * 8;
    char *buf = nullptr;
    TILER_HIP_CHECK(hipMallocAsync((void **)&buf, b_sums + b_out, stream));
    unsigned long long *d_sums = (unsigned long long *)buf;
    double *d_out = (double *)(buf + b_sums);
    std::vector<unsigned long long> h_sums((size_t)F * QL_SUMS);
    std::vector<double> h_out((size_t)F * 3);
    int rc = -1;
    do {
        if (hipMemsetAsync(d_sums, 0, b_sums, stream) != hipSuccess) break;
        {
            KTimer tm("quality", stream);
            const int bx = (int)std::min<long>(64, (fs / 4 + 4095) / 4096);
            hipLaunchKernelGGL(quality_sums_kernel, dim3(bx, F), dim3(256), 0, stream, (const int4 *)d_src,
                               (const int4 *)d_dst, fs / 4, d_sums);
            if (hipGetLastError() != hipSuccess) break;
            if (corr) {
                hipLaunchKernelGGL(quality_chain_kernel, dim3((F + QL_FRAMES - 1) / QL_FRAMES), dim3(256), 0, stream,
                                   d_src, d_dst, F, tm_w, tm_h, d_sums, d_out);
                if (hipGetLastError() != hipSuccess) break;
            }
        }
        if (hipMemcpyAsync(h_sums.data(), d_sums, b_sums, hipMemcpyDeviceToHost, stream) != hipSuccess) break;
        if (corr && hipMemcpyAsync(h_out.data(), d_out, b_out, hipMemcpyDeviceToHost, stream) != hipSuccess) break;
        if (hipStreamSynchronize(stream) != hipSuccess) break;
        rc = 0;
    } while (0);
    (void)hipFreeAsync(buf, stream);
    if (rc) {
        set_error(std::string("quality: HIP failure: ") + hipGetErrorString(hipGetLastError()));
        return -1;
    }
    for (int f = 0; f < F; f++) {
        if (sse)
            for (int c = 0; c < 3; c++) sse[(size_t)f * 3 + c] = h_sums[(size_t)f * QL_SUMS + 6 + c];
        if (corr) {  // PearsonCorrelation tail main.pas:1485-1491
            const double denx = sqrt(h_out[(size_t)f * 3 + 1]), deny = sqrt(h_out[(size_t)f * 3 + 2]);
            const double den = denx * deny;
            corr[f] = den != 0.0 ? h_out[(size_t)f * 3] / den : 0.0;
        }
    }
    return 0;
}

int frame_quality_host(const int32_t *src, const int32_t *dst, int F, int tm_w, int tm_h, double *corr,
                       uint64_t *sse) {
    if (F < 0 || tm_w <= 0 || tm_h <= 0 || (F > 0 && (!src || !dst))) {
        set_error("quality: invalid arguments");
        return -1;
    }
    if (F == 0) return 0;
    const size_t n = (size_t)F * tm_w * tm_h * 64;
    HostStage s("quality");
    const int32_t *d_src = s.in(src, n), *d_dst = s.in(dst, n);
    if (!s.ok() || frame_quality_dev(d_src, d_dst, F, tm_w, tm_h, corr, sse, s.stream())) return -1;
    return s.finish();
}

}  // namespace tiler
