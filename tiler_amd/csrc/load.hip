// load.hip -- raster pictures <-> tile-major frames on gfx950 (LoadFrame main.pas:3211-3286, ReframeUI
// main.pas:1931-1938, SwapRB main.pas:561-564).
//
// A workgroup takes a span of one 8-scanline strip of one frame: SPAN_TILES tiles = 256 pixels.  The strip's raw
// bytes and the tiles are two views of one LDS image of 8 rows:
//   * the scanline side moves a row as aligned dwords, one per lane (256 contiguous bytes per wave-instruction).  A row
//     that does not start on a dword (RGB24 with an odd pitch, a cropped base) keeps its byte phase s = address & 3
//     in LDS: the dwords that lie wholly inside the span are still moved whole, the one or two that straddle its ends
//     byte by byte, so nothing outside the span's own bytes is read or written;
//   * the tile side moves 16 bytes per lane: 4 pixels of one tile row = piece q = 2 * tile + half of LDS row r, at
//     byte s + q * 4 * BPP.  It reads (writes) BPP + 1 (BPP) dwords and shifts the phase out with v_alignbyte_b32.
// Banks (ds_read_b32 / ds_write_b32: bank = dword mod 32, the two 32-lane halves of a wave apart): the scanline
// side is lane-linear.  The tile side's dword k of a lane is r * RP + BPP * q + k:
//   BPP 3, RP = 204 = 12 mod 32, lane = tile * 16 + r * 2 + half: a half-wave's 32 dwords are 12 r + 6 tile + 3 half,
//     r = 0..7, which is every residue mod 32 once;
//   BPP 4, RP = 257 = 1 mod 32, lane = (r / 4) * 32 + tile * 8 + half * 4 + r % 4: r % 4 + 4 half + 8 tile,
//     every residue once.
// A wave's 64 lanes cover 4 whole tiles in both mappings, so a tile-side wave-instruction is 1 KiB contiguous in HBM.
// Every source / destination / tile address is formed in 64 bits.
#include "load.hpp"

#include <algorithm>
#include <atomic>
#include <string>

#include "keyframes.hpp"
#include "raster_dev.hpp"
#include "stage.hpp"

namespace tiler {

constexpr int SPAN_TILES = 32;
constexpr int LOAD_THREADS = 256;
constexpr int TM_MAX_W = 1920 / 8, TM_MAX_H = 1080 / 8;  // ReframeUI's cap

template <int BPP>
struct Span {
    static constexpr int RP = BPP == 3 ? 204 : 257;           // LDS row pitch in dwords (the span + 1, and the banks)
    static constexpr int ITERS = (SPAN_TILES * 2 * BPP + 1 + 63) / 64;  // dwords of a row per lane
    static_assert(RP >= SPAN_TILES * 2 * BPP + 1, "a row holds the span and the phase's spill-over");
};

// lane of a tile-side wave -> (tile of the wave's 4, tile row, half row)
template <int BPP>
__device__ __forceinline__ void piece_of_lane(int lane, int &tl, int &r, int &h) {
    if (BPP == 3) {
        h = lane & 1;
        r = (lane >> 1) & 7;
        tl = lane >> 4;
    } else {
        r = ((lane >> 5) << 2) | (lane & 3);
        h = (lane >> 2) & 1;
        tl = (lane >> 3) & 3;
    }
}

__device__ __forceinline__ uint32_t swap_rb(uint32_t c) {  // SwapRB main.pas:561-564 (drops the top byte)
    return ((c & 0xffu) << 16) | ((c >> 16) & 0xffu) | (c & 0xff00u);
}

struct SpanAt {
    int64_t frame;
    int ty, tx0, nt;
};
__device__ __forceinline__ SpanAt span_of_block(int tm_w, int tm_h, int spans) {
    unsigned b = blockIdx.x;
    SpanAt a;
    const int sp = (int)(b % (unsigned)spans);
    b /= (unsigned)spans;
    a.ty = (int)(b % (unsigned)tm_h);
    a.frame = (int64_t)(b / (unsigned)tm_h);
    a.tx0 = sp * SPAN_TILES;
    a.nt = min(SPAN_TILES, tm_w - a.tx0);
    return a;
}

template <int BPP>
__global__ __launch_bounds__(LOAD_THREADS) void load_frames_kernel(const uint8_t *__restrict__ src, int64_t pitch,
                                                                   int64_t frame_stride, int32_t *__restrict__ rgb,
                                                                   int tm_w, int tm_h, int spans, int swap) {
    constexpr int RP = Span<BPP>::RP, ITERS = Span<BPP>::ITERS;
    __shared__ uint32_t img[8 * RP];
    const SpanAt a = span_of_block(tm_w, tm_h, spans);
    const int n = a.nt * 8 * BPP;  // bytes of a span row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *strip = src + a.frame * frame_stride + (int64_t)a.ty * 8 * pitch + (int64_t)a.tx0 * 8 * BPP;

    // scanline side: wave w stages rows w and w + 4; every load is issued before the first LDS write
    uint32_t v[2][ITERS];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const uint8_t *row = strip + (int64_t)(wave + 4 * k) * pitch;
        const int s = (int)((uintptr_t)row & 3);
        const int nd = (s + n + 3) >> 2;
#pragma unroll
        for (int it = 0; it < ITERS; it++) v[k][it] = fetch_dword(row - s, s, n, lane + 64 * it, nd);
    }
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
        for (int it = 0; it < ITERS; it++)
            if (lane + 64 * it < RP) img[(wave + 4 * k) * RP + lane + 64 * it] = v[k][it];
    __syncthreads();

    // tile side
    int4 *out = (int4 *)rgb + (((a.frame * tm_h + a.ty) * (int64_t)tm_w + a.tx0) << 4);
    for (int u = threadIdx.x; u < SPAN_TILES * 16; u += LOAD_THREADS) {
        int tl, r, h;
        piece_of_lane<BPP>(u & 63, tl, r, h);
        const int t = (u >> 6) * 4 + tl;
        if (t >= a.nt) continue;
        const int s = (int)((uintptr_t)(strip + (int64_t)r * pitch) & 3);
        const uint32_t *p = img + r * RP + (2 * t + h) * BPP;
        uint32_t w[BPP];
#pragma unroll
        for (int i = 0; i < BPP; i++) w[i] = __builtin_amdgcn_alignbyte(p[i + 1], p[i], (uint32_t)s);
        uint32_t c[4];
        if (BPP == 3) {
            c[0] = w[0] & 0xffffffu;
            c[1] = ((w[0] >> 24) | (w[1] << 8)) & 0xffffffu;
            c[2] = ((w[1] >> 16) | (w[2] << 16)) & 0xffffffu;
            c[3] = w[2] >> 8;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) c[i] = w[i] & 0xffffffu;  // alpha / X dropped
        }
        if (swap) {
#pragma unroll
            for (int i = 0; i < 4; i++) c[i] = swap_rb(c[i]);
        }
        out[t * 16 + r * 2 + h] = make_int4((int)c[0], (int)c[1], (int)c[2], (int)c[3]);
    }
}

template <int BPP>
__global__ __launch_bounds__(LOAD_THREADS) void store_frames_kernel(const int32_t *__restrict__ rgb,
                                                                    uint8_t *__restrict__ dst, int64_t pitch,
                                                                    int64_t frame_stride, int tm_w, int tm_h, int spans,
                                                                    int swap) {
    constexpr int RP = Span<BPP>::RP;
    __shared__ uint32_t img[8 * RP];
    const SpanAt a = span_of_block(tm_w, tm_h, spans);
    const int n = a.nt * 8 * BPP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t *strip = dst + a.frame * frame_stride + (int64_t)a.ty * 8 * pitch + (int64_t)a.tx0 * 8 * BPP;

    // tile side: the span's raw bytes into LDS, every row from its byte 0
    const int4 *in = (const int4 *)rgb + (((a.frame * tm_h + a.ty) * (int64_t)tm_w + a.tx0) << 4);
    for (int u = threadIdx.x; u < SPAN_TILES * 16; u += LOAD_THREADS) {
        int tl, r, h;
        piece_of_lane<BPP>(u & 63, tl, r, h);
        const int t = (u >> 6) * 4 + tl;
        if (t >= a.nt) continue;
        const int4 px = in[t * 16 + r * 2 + h];
        uint32_t c[4] = {(uint32_t)px.x & 0xffffffu, (uint32_t)px.y & 0xffffffu, (uint32_t)px.z & 0xffffffu,
                         (uint32_t)px.w & 0xffffffu};
        if (swap) {
#pragma unroll
            for (int i = 0; i < 4; i++) c[i] = swap_rb(c[i]);
        }
        uint32_t *p = img + r * RP + (2 * t + h) * BPP;
        if (BPP == 3) {
            p[0] = c[0] | (c[1] << 24);
            p[1] = (c[1] >> 8) | (c[2] << 16);
            p[2] = (c[2] >> 16) | (c[3] << 8);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) p[i] = c[i] | 0xff000000u;
        }
    }
    __syncthreads();

    // scanline side: wave w writes rows w and w + 4; the dword at al + 4 j holds the row's bytes 4 j - s ..
    for (int r = wave; r < 8; r += 4) {
        uint8_t *row = strip + (int64_t)r * pitch;
        const int s = (int)((uintptr_t)row & 3);
        uint8_t *al = row - s;
        const int nd = (s + n + 3) >> 2;
        const uint32_t *line = img + r * RP;
        for (int j = lane; j < nd; j += 64) {
            const int lo = 4 * j;
            if (lo >= s && lo + 4 <= s + n) {
                const int k = lo - s;
                *(uint32_t *)(al + lo) = __builtin_amdgcn_alignbyte(line[(k >> 2) + 1], line[k >> 2], (uint32_t)(k & 3));
            } else {
                for (int b = 0; b < 4; b++)
                    if (lo + b >= s && lo + b < s + n) al[lo + b] = ((const uint8_t *)line)[lo + b - s];
            }
        }
    }
}

int load_dims(int src_w, int src_h, int *tm_w, int *tm_h) {
    if (src_w < 8 || src_h < 8) {
        set_error("tiler_load_dims: src_w and src_h must be at least 8 (one tile)");
        return -1;
    }
    if (tm_w) *tm_w = std::min(src_w / 8, TM_MAX_W);
    if (tm_h) *tm_h = std::min(src_h / 8, TM_MAX_H);
    return 0;
}

static int bad(const char *who, const char *what) {
    set_error(std::string(who) + ": " + what);
    return -1;
}

// pitch and frame_stride against their minima for pictures of w x h pixels
static int strides_check(const char *who, int fmt, int w, int h, int64_t pitch, int64_t frame_stride) {
    if (fmt < 0 || fmt >= PIX_COUNT) return bad(who, "fmt is not one of the four pixel formats");
    if (pitch < (int64_t)w * pix_bytes(fmt)) return bad(who, "pitch is below src_w * bytes per pixel");
    if (pitch > INT64_MAX / h || frame_stride < (int64_t)h * pitch)
        return bad(who, "frame_stride is below src_h * pitch");
    return 0;
}

int load_check(const char *who, const void *src, int fmt, int F, int src_w, int src_h, int64_t pitch,
               int64_t frame_stride, const void *rgb, bool dev) {
    if (F < 0) return bad(who, "F is negative");
    if (src_w < 8 || src_h < 8) return bad(who, "src_w and src_h must be at least 8 (one tile)");
    if (strides_check(who, fmt, src_w, src_h, pitch, frame_stride)) return -1;
    if (F > 0 && frame_stride > INT64_MAX / F) return bad(who, "F * frame_stride overflows");
    if (F > 0 && !src) return bad(who, "src is null");
    if (F > 0 && !rgb) return bad(who, "rgb is null");
    if (dev && (uintptr_t)rgb % 16) return bad(who, "d_rgb is not 16-byte aligned");
    return 0;
}

int store_check(const char *who, const void *rgb, int F, int tm_w, int tm_h, int fmt, const void *dst, int64_t pitch,
                int64_t frame_stride, bool dev) {
    if (F < 0) return bad(who, "F is negative");
    if (tm_w < 1 || tm_h < 1 || tm_w > (1 << 20) || tm_h > (1 << 20)) return bad(who, "tm_w or tm_h out of range");
    if (strides_check(who, fmt, tm_w * 8, tm_h * 8, pitch, frame_stride)) return -1;
    if (F > 0 && frame_stride > INT64_MAX / F) return bad(who, "F * frame_stride overflows");
    if (F > 0 && !rgb) return bad(who, "rgb is null");
    if (F > 0 && !dst) return bad(who, "dst is null");
    if (dev && (uintptr_t)rgb % 16) return bad(who, "d_rgb is not 16-byte aligned");
    return 0;
}

// frames of one launch: at most 2^23 workgroups, so that a grid's threads stay below 2^32
static int frames_per_launch(int tm_h, int spans) {
    return (int)std::max<int64_t>(1, (1ll << 23) / ((int64_t)tm_h * spans));
}

int load_frames_dev(const uint8_t *d_src, int fmt, int F, int src_w, int src_h, int64_t pitch, int64_t frame_stride,
                    int32_t *d_rgb, hipStream_t stream) {
    int tm_w, tm_h;
    if (load_dims(src_w, src_h, &tm_w, &tm_h)) return -1;
    if (F <= 0) return 0;
    const int spans = (tm_w + SPAN_TILES - 1) / SPAN_TILES, per = frames_per_launch(tm_h, spans);
    const int swap = fmt == PIX_BGR24 || fmt == PIX_BGRA32;
    KTimer tm("load_frames", stream);
    for (int f0 = 0; f0 < F; f0 += per) {
        const int nf = std::min(per, F - f0);
        const dim3 grid((unsigned)((int64_t)nf * tm_h * spans));
        const uint8_t *s = d_src + (int64_t)f0 * frame_stride;
        int32_t *o = d_rgb + (int64_t)f0 * tm_w * tm_h * 64;
        if (pix_bytes(fmt) == 3)
            hipLaunchKernelGGL(load_frames_kernel<3>, grid, dim3(LOAD_THREADS), 0, stream, s, pitch, frame_stride, o,
                               tm_w, tm_h, spans, swap);
        else
            hipLaunchKernelGGL(load_frames_kernel<4>, grid, dim3(LOAD_THREADS), 0, stream, s, pitch, frame_stride, o,
                               tm_w, tm_h, spans, swap);
        TILER_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

int store_frames_dev(const int32_t *d_rgb, int F, int tm_w, int tm_h, int fmt, uint8_t *d_dst, int64_t pitch,
                     int64_t frame_stride, hipStream_t stream) {
    if (F <= 0) return 0;
    const int spans = (tm_w + SPAN_TILES - 1) / SPAN_TILES, per = frames_per_launch(tm_h, spans);
    const int swap = fmt == PIX_BGR24 || fmt == PIX_BGRA32;
    KTimer tm("store_frames", stream);
    for (int f0 = 0; f0 < F; f0 += per) {
        const int nf = std::min(per, F - f0);
        const dim3 grid((unsigned)((int64_t)nf * tm_h * spans));
        const int32_t *i = d_rgb + (int64_t)f0 * tm_w * tm_h * 64;
        uint8_t *o = d_dst + (int64_t)f0 * frame_stride;
        if (pix_bytes(fmt) == 3)
            hipLaunchKernelGGL(store_frames_kernel<3>, grid, dim3(LOAD_THREADS), 0, stream, i, o, pitch, frame_stride,
                               tm_w, tm_h, spans, swap);
        else
            hipLaunchKernelGGL(store_frames_kernel<4>, grid, dim3(LOAD_THREADS), 0, stream, i, o, pitch, frame_stride,
                               tm_w, tm_h, spans, swap);
        TILER_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

static std::atomic<int64_t> g_chunk_frames{0};
int load_chunk_debug(int64_t frames) {
    if (frames < 0) {
        set_error("tiler_debug_load_chunk: frames is negative");
        return -1;
    }
    g_chunk_frames.store(frames);
    return 0;
}

// The device image of a chunk's pictures: only the used rectangle, rows 4-byte aligned (the kernels' dword path).
struct Dense {
    int64_t row, pitch, frame;  // used bytes of a row, device row pitch, device bytes per frame
    int rows;
    Dense(int fmt, int tm_w, int tm_h) : row((int64_t)tm_w * 8 * pix_bytes(fmt)), pitch((row + 3) & ~3ll),
                                         frame(pitch * tm_h * 8), rows(tm_h * 8) {}
};
int load_chunk_frames(int F, int64_t frame_bytes) {
    const int64_t forced = g_chunk_frames.load();
    const int64_t n = forced > 0 ? forced : std::max<int64_t>(1, LOAD_CHUNK_BYTES / frame_bytes);
    return (int)std::min<int64_t>(n, F);
}
static int chunk_frames(int F, const Dense &d, int64_t tile_bytes) { return load_chunk_frames(F, d.frame + tile_bytes); }

int load_frames_host(const uint8_t *src, int fmt, int F, int src_w, int src_h, int64_t pitch, int64_t frame_stride,
                     int32_t *rgb) {
    int tm_w, tm_h;
    if (load_dims(src_w, src_h, &tm_w, &tm_h)) return -1;
    if (F <= 0) return 0;
    const Dense d(fmt, tm_w, tm_h);
    const int64_t tile_bytes = (int64_t)tm_w * tm_h * 256;
    const int per = chunk_frames(F, d, tile_bytes);
    PoolStream ps;
    if (!ps.ok) return bad("tiler_load_frames", "no stream");
    Blocks blocks(ps.st);
    uint8_t *d_src = nullptr;
    int32_t *d_rgb = nullptr;
    if (!blocks.get(d_src, (size_t)(per * d.frame)) || !blocks.get(d_rgb, (size_t)(per * tile_bytes)))
        return bad("tiler_load_frames", "out of device memory");
    for (int f0 = 0; f0 < F; f0 += per) {
        const int nf = std::min(per, F - f0);
        for (int f = 0; f < nf; f++)
            TILER_HIP_CHECK(hipMemcpy2DAsync(d_src + f * d.frame, (size_t)d.pitch, src + (int64_t)(f0 + f) * frame_stride,
                                             (size_t)pitch, (size_t)d.row, (size_t)d.rows, hipMemcpyHostToDevice,
                                             ps.st));
        if (load_frames_dev(d_src, fmt, nf, tm_w * 8, tm_h * 8, d.pitch, d.frame, d_rgb, ps.st)) return -1;
        TILER_HIP_CHECK(hipMemcpyAsync(rgb + (int64_t)f0 * tm_w * tm_h * 64, d_rgb, (size_t)(nf * tile_bytes),
                                       hipMemcpyDeviceToHost, ps.st));
    }
    TILER_HIP_CHECK(hipStreamSynchronize(ps.st));
    return 0;
}

int store_frames_host(const int32_t *rgb, int F, int tm_w, int tm_h, int fmt, uint8_t *dst, int64_t pitch,
                      int64_t frame_stride) {
    if (F <= 0) return 0;
    const Dense d(fmt, tm_w, tm_h);
    const int64_t tile_bytes = (int64_t)tm_w * tm_h * 256;
    const int per = chunk_frames(F, d, tile_bytes);
    PoolStream ps;
    if (!ps.ok) return bad("tiler_store_frames", "no stream");
    Blocks blocks(ps.st);
    uint8_t *d_dst = nullptr;
    int32_t *d_rgb = nullptr;
    if (!blocks.get(d_dst, (size_t)(per * d.frame)) || !blocks.get(d_rgb, (size_t)(per * tile_bytes)))
        return bad("tiler_store_frames", "out of device memory");
    for (int f0 = 0; f0 < F; f0 += per) {
        const int nf = std::min(per, F - f0);
        TILER_HIP_CHECK(hipMemcpyAsync(d_rgb, rgb + (int64_t)f0 * tm_w * tm_h * 64, (size_t)(nf * tile_bytes),
                                       hipMemcpyHostToDevice, ps.st));
        if (store_frames_dev(d_rgb, nf, tm_w, tm_h, fmt, d_dst, d.pitch, d.frame, ps.st)) return -1;
        for (int f = 0; f < nf; f++)
            TILER_HIP_CHECK(hipMemcpy2DAsync(dst + (int64_t)(f0 + f) * frame_stride, (size_t)pitch, d_dst + f * d.frame,
                                             (size_t)d.pitch, (size_t)d.row, (size_t)d.rows, hipMemcpyDeviceToHost,
                                             ps.st));
    }
    TILER_HIP_CHECK(hipStreamSynchronize(ps.st));
    return 0;
}

int load_clip_dev(const uint8_t *d_src, int fmt, int F, int src_w, int src_h, int64_t pitch, int64_t frame_stride,
                  int32_t *d_rgb, double *corr, int32_t *kf_of_frame, hipStream_t stream) {
    int tm_w, tm_h;
    if (load_dims(src_w, src_h, &tm_w, &tm_h)) return -1;
    if (F <= 0) return 0;
    if (load_frames_dev(d_src, fmt, F, src_w, src_h, pitch, frame_stride, d_rgb, stream)) return -1;
    if (interframe_corr_dev(d_rgb, F, tm_w, tm_h, corr, stream)) return -1;
    if (F == 1) TILER_HIP_CHECK(hipStreamSynchronize(stream));  // no correlation to wait for
    return find_keyframes(corr, F, tm_w * tm_h, kf_of_frame);
}

}  // namespace tiler
