// scale.hip -- Lanczos input scaling fused with the tile cut (cbxScaling main.pas:4780-4782, 1042; ReframeUI
// main.pas:1931-1938), pinned to Pillow's 8-bit Image.resize(size, LANCZOS).
//
// Two kernels per group of frames, an 8-bit picture [frames][rows][KW][3] (bytes R,G,B) in HBM between them; the
// group is sized so that this picture stays within SCALE_INTER_BYTES, which the L2s and the Infinity Cache hold,
// so what HBM sees is the source read once and the tiles written once.
//   * scale_h_kernel: a workgroup takes H_SPAN output columns of H_ITERS * 8 source rows.  The span's taps go to LDS
//     once, [tap][column], read back 16 bytes per lane (ds_read_b128: 4 columns of one tap).  Eight rows at a time
//     their source bytes go to LDS as load.hip's scanline side moves them: aligned dwords with the row's byte phase
//     kept, bytes only at the two ends.  A lane owns 4 adjacent output pixels of one row; a 32-lane half of a wave is
//     one row, so the two halves of a ds_read_b32 never meet on a bank.  Four taps of a pixel are 4 * BPP contiguous
//     bytes = BPP dwords at a phase that does not change along the taps; v_alignbyte_b32 shifts it out.
//   * scale_v_kernel: lanes are tile pieces in load.hip's RGB24 order (4 whole tiles per wave, 1 KiB contiguous per
//     store instruction); a tap is 12 bytes = 4 pixels of one row of the intermediate picture.
// The kernels see integers only: the taps are built on the host in double (scale_coeffs) and live, per
// (src, out) size and device, in a small cached plan with the intermediate picture.
// Every address is formed in 64 bits.
#include "scale.hpp"

#include <algorithm>
#include <cmath>
#include <list>
#include <mutex>
#include <string>
#include <vector>

#include "keyframes.hpp"
#include "load.hpp"
#include "raster_dev.hpp"
#include "stage.hpp"

namespace tiler {

constexpr int H_THREADS = 256, H_SPAN = 128, H_ITERS = 4;  // 8 rows x 32 lanes x 4 pixels; 32 rows per workgroup
constexpr int V_THREADS = 256, V_TILES = 16;
constexpr int64_t SCALE_INTER_BYTES = 32ll << 20;
constexpr size_t SCALE_LDS_MAX = 64 << 10;
constexpr int SCALE_PLANS = 4;

// 12 bytes in three dwords -> four 24-bit pixels (load.hip's RGB24 tile side); 4-byte pixels: the low 24 bits
template <int BPP>
__device__ __forceinline__ void four_pixels(const uint32_t *q, uint32_t *c) {
    if (BPP == 3) {
        c[0] = q[0] & 0xffffffu;
        c[1] = ((q[0] >> 24) | (q[1] << 8)) & 0xffffffu;
        c[2] = ((q[1] >> 16) | (q[2] << 16)) & 0xffffffu;
        c[3] = q[2] >> 8;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) c[i] = q[i] & 0xffffffu;
    }
}

__device__ __forceinline__ uint32_t clip8(int acc) { return (uint32_t)min(max(acc >> SCALE_PRECISION_BITS, 0), 255); }

template <int BPP>
__global__ __launch_bounds__(H_THREADS) void scale_h_kernel(const uint8_t *__restrict__ src, int64_t pitch,
                                                            int64_t frame_stride, const int2 *__restrict__ bounds,
                                                            const int32_t *__restrict__ hk, int KWp, int ksp, int KW,
                                                            int rows, int RP, int spans, int rgroups, int swap,
                                                            uint8_t *__restrict__ inter) {
    extern __shared__ __align__(16) uint32_t lds[];
    uint32_t *img = lds;                          // [8][RP]: source bytes of 8 rows, each at its own byte phase
    int32_t *wl = (int32_t *)(lds + 8 * RP);      // [ksp][H_SPAN]
    unsigned b = blockIdx.x;
    const int sp = (int)(b % (unsigned)spans);
    b /= (unsigned)spans;
    const int rg = (int)(b % (unsigned)rgroups);
    const int64_t frame = (int64_t)(b / (unsigned)rgroups);
    const int x0 = sp * H_SPAN, xl = min(x0 + H_SPAN, KW) - 1;
    const int2 bl = bounds[xl];
    const int col0 = bounds[x0].x;
    const int n = (bl.x + bl.y - col0) * BPP;  // bytes of a span row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l32 = threadIdx.x & 31, r = threadIdx.x >> 5;
    const int x = x0 + l32 * 4;
    const uint8_t *span = src + frame * frame_stride + (int64_t)col0 * BPP;

    for (int i = threadIdx.x; i < ksp * H_SPAN; i += H_THREADS)
        wl[i] = hk[(int64_t)(i / H_SPAN) * KWp + x0 + (i % H_SPAN)];
    int off[4];
#pragma unroll
    for (int i = 0; i < 4; i++) off[i] = (bounds[x + i].x - col0) * BPP;

    for (int it = 0; it < H_ITERS; it++) {
        const int y0 = (rg * H_ITERS + it) * 8;
        if (y0 >= rows) break;
        if (it) __syncthreads();  // the rows before have been read
        // scanline side: wave w stages rows w and w + 4 (a row past the last is the last again)
        for (int k = 0; k < 2; k++) {
            const int rr = wave + 4 * k;
            const uint8_t *row = span + (int64_t)min(y0 + rr, rows - 1) * pitch;
            const int s = (int)((uintptr_t)row & 3);
            const int nd = (s + n + 3) >> 2;
            for (int j = lane; j < nd; j += 64) img[rr * RP + j] = fetch_dword(row - s, s, n, j, nd);
        }
        __syncthreads();

        const int y = y0 + r;
        const int s = (int)((uintptr_t)(span + (int64_t)min(y, rows - 1) * pitch) & 3);
        int acc[4][3];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int c = 0; c < 3; c++) acc[i][c] = 1 << (SCALE_PRECISION_BITS - 1);
        for (int t = 0; t < ksp; t += 4) {
            int w[4][4];  // [tap][pixel]
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int4 v = *(const int4 *)(wl + (t + j) * H_SPAN + l32 * 4);
                w[j][0] = v.x, w[j][1] = v.y, w[j][2] = v.z, w[j][3] = v.w;
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int bo = s + off[i] + t * BPP;
                const uint32_t *p = img + r * RP + (bo >> 2);
                uint32_t q[BPP], c[4];
#pragma unroll
                for (int k = 0; k < BPP; k++) q[k] = __builtin_amdgcn_alignbyte(p[k + 1], p[k], (uint32_t)(bo & 3));
                four_pixels<BPP>(q, c);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    acc[i][0] += (int)(c[j] & 0xffu) * w[j][i];
                    acc[i][1] += (int)((c[j] >> 8) & 0xffu) * w[j][i];
                    acc[i][2] += (int)(c[j] >> 16) * w[j][i];
                }
            }
        }
        if (x < KW && y < rows) {
            uint32_t v[4][3];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                v[i][0] = clip8(acc[i][swap ? 2 : 0]);
                v[i][1] = clip8(acc[i][1]);
                v[i][2] = clip8(acc[i][swap ? 0 : 2]);
            }
            uint32_t *o = (uint32_t *)(inter + ((frame * rows + y) * (int64_t)KW + x) * 3);
            o[0] = v[0][0] | (v[0][1] << 8) | (v[0][2] << 16) | (v[1][0] << 24);
            o[1] = v[1][1] | (v[1][2] << 8) | (v[2][0] << 16) | (v[2][1] << 24);
            o[2] = v[2][2] | (v[3][0] << 8) | (v[3][1] << 16) | (v[3][2] << 24);
        }
    }
}

__global__ __launch_bounds__(V_THREADS) void scale_v_kernel(const uint8_t *__restrict__ inter, int rows, int KW,
                                                            const int2 *__restrict__ bounds,
                                                            const int32_t *__restrict__ vk, int ksv, int tm_w, int tm_h,
                                                            int tspans, int32_t *__restrict__ rgb) {
    unsigned b = blockIdx.x;
    const int sp = (int)(b % (unsigned)tspans);
    b /= (unsigned)tspans;
    const int ty = (int)(b % (unsigned)tm_h);
    const int64_t frame = (int64_t)(b / (unsigned)tm_h);
    const int lane = threadIdx.x & 63;
    const int h = lane & 1, r = (lane >> 1) & 7;  // load.hip's piece_of_lane<3>
    const int t = sp * V_TILES + (threadIdx.x >> 6) * 4 + (lane >> 4);
    if (t >= tm_w) return;
    const int y = ty * 8 + r, x = t * 8 + h * 4;
    const int ymin = bounds[y].x;
    const int32_t *k = vk + (int64_t)y * ksv;
    const uint8_t *col = inter + (frame * rows * (int64_t)KW + x) * 3;
    int acc[4][3];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int c = 0; c < 3; c++) acc[i][c] = 1 << (SCALE_PRECISION_BITS - 1);
    for (int tt = 0; tt < ksv; tt++) {
        const uint32_t *p = (const uint32_t *)(col + (int64_t)min(ymin + tt, rows - 1) * KW * 3);
        const uint32_t q[3] = {p[0], p[1], p[2]};
        const int w = k[tt];
        uint32_t c[4];
        four_pixels<3>(q, c);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            acc[i][0] += (int)(c[i] & 0xffu) * w;
            acc[i][1] += (int)((c[i] >> 8) & 0xffu) * w;
            acc[i][2] += (int)(c[i] >> 16) * w;
        }
    }
    int px[4];
#pragma unroll
    for (int i = 0; i < 4; i++) px[i] = (int)(clip8(acc[i][0]) | (clip8(acc[i][1]) << 8) | (clip8(acc[i][2]) << 16));
    int4 *out = (int4 *)rgb + (((frame * tm_h + ty) * (int64_t)tm_w + t) << 4);
    out[r * 2 + h] = make_int4(px[0], px[1], px[2], px[3]);
}

// ---- sizes and taps (host) ----

static int bad(const char *who, const char *what) {
    set_error(std::string(who) + ": " + what);
    return -1;
}

int scale_dims(int src_w, int src_h, double scale, int *out_w, int *out_h) {
    const char *who = "tiler_scale_dims";
    if (src_w < 1 || src_h < 1) return bad(who, "src_w and src_h must be positive");
    if (!std::isfinite(scale) || !(scale > 0.0)) return bad(who, "scale must be finite and positive");
    const double w = std::floor(src_w * scale), h = std::floor(src_h * scale);
    if (w < 8 || h < 8) return bad(who, "scale leaves a side below 8 (one tile)");
    if (w > SCALE_MAX_OUT || h > SCALE_MAX_OUT) return bad(who, "scale leaves a side above 16384");
    if (out_w) *out_w = (int)w;
    if (out_h) *out_h = (int)h;
    return 0;
}

static double sinc(double t) {
    if (t == 0.0) return 1.0;
    t = t * M_PI;
    return sin(t) / t;
}
static double lanczos(double t) { return -3.0 <= t && t < 3.0 ? sinc(t) * sinc(t / 3.0) : 0.0; }

static int64_t ksize_of(int n_in, int n_out) {
    const double fs = std::max((double)n_in / n_out, 1.0);
    return (int64_t)std::ceil(3.0 * fs) * 2 + 1;
}

// the first n of an axis' n_out outputs: bounds[n][2], taps[n][ksize]
static void axis_taps(int n_in, int n_out, int n, int ksize, int32_t *bounds, int32_t *taps) {
    const double scale = (double)n_in / n_out, fs = std::max(scale, 1.0), support = 3.0 * fs;
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < n; xx++) {
        const double center = (xx + 0.5) * scale;
        const int xmin = std::max((int)(center - support + 0.5), 0);
        const int xmax = std::min((int)(center + support + 0.5), n_in) - xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; x++) ww += w[x] = lanczos((x + xmin - center + 0.5) / fs);
        int32_t *k = taps + (int64_t)xx * ksize;
        std::fill(k, k + ksize, 0);
        for (int x = 0; x < xmax; x++) {
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int)(v * (1 << SCALE_PRECISION_BITS) - 0.5) : (int)(v * (1 << SCALE_PRECISION_BITS) + 0.5);
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

int scale_coeffs(int n_in, int n_out, int32_t *bounds, int32_t *taps, int64_t cap) {
    const char *who = "tiler_scale_coeffs";
    if (n_in < 1 || n_in > (1 << 24)) return bad(who, "in is out of range (1 .. 2^24)");
    if (n_out < 1 || n_out > (1 << 24)) return bad(who, "out is out of range (1 .. 2^24)");
    const int64_t ksize = ksize_of(n_in, n_out);
    if (!bounds && !taps) return (int)ksize;
    if (!bounds || !taps) return bad(who, "bounds and taps are given together");
    if (cap < ksize * n_out) return bad(who, "cap is below out * ksize");
    axis_taps(n_in, n_out, n_out, (int)ksize, bounds, taps);
    return (int)ksize;
}

int scale_check(const char *who, int src_w, int src_h, int out_w, int out_h) {
    if (out_w < 8 || out_w > SCALE_MAX_OUT) return bad(who, "out_w is out of range (8 .. 16384)");
    if (out_h < 8 || out_h > SCALE_MAX_OUT) return bad(who, "out_h is out of range (8 .. 16384)");
    if ((int64_t)src_w > (int64_t)SCALE_MAX_RATIO * out_w) return bad(who, "out_w is below src_w / 8");
    if ((int64_t)src_h > (int64_t)SCALE_MAX_RATIO * out_h) return bad(who, "out_h is below src_h / 8");
    return 0;
}

// ---- the plan: the kept pixels' taps on the device, and the intermediate picture ----

struct ScalePlan {
    int dev = -1, src_w = 0, src_h = 0, out_w = 0, out_h = 0;
    int tm_w = 0, tm_h = 0, KW = 0, KH = 0;
    int cols = 0, rows = 0;  // source columns / rows that the kept pixels' taps reach
    int ksp = 0, ksv = 0;    // taps per output: horizontal (a multiple of 4), vertical
    int spans = 0, KWp = 0, span_px = 0;
    int2 *d_hb = nullptr, *d_vb = nullptr;
    int32_t *d_hk = nullptr, *d_vk = nullptr;
    uint8_t *d_inter = nullptr;
    int group = 0;  // frames the intermediate picture holds
    hipEvent_t done = nullptr;  // the last call's kernels: the next call's stream waits for it
    ~ScalePlan() {
        if (done) {
            (void)hipEventSynchronize(done);
            (void)hipEventDestroy(done);
        }
        for (void *p : {(void *)d_hb, (void *)d_vb, (void *)d_hk, (void *)d_vk, (void *)d_inter})
            if (p) dfree(p);
    }
};

// One axis: bounds[np][2] and taps for the first n outputs, the rest of np padded with (last xmin, 0) and zero taps.
// A pass that is skipped (in == out) is the identity: one tap of 1.0 on the pixel itself.
struct AxisTaps {
    int ks = 0, reach = 0;
    std::vector<int32_t> bounds, taps;  // taps [np][ks]
    AxisTaps(int n_in, int n_out, int n, int np, int ks_mult) {
        const int k0 = n_in == n_out ? 1 : (int)ksize_of(n_in, n_out);
        ks = (k0 + ks_mult - 1) / ks_mult * ks_mult;
        bounds.assign((size_t)np * 2, 0);
        taps.assign((size_t)np * ks, 0);
        if (n_in == n_out) {
            for (int i = 0; i < n; i++) {
                bounds[2 * i] = i, bounds[2 * i + 1] = 1;
                taps[(size_t)i * ks] = 1 << SCALE_PRECISION_BITS;
            }
        } else {
            std::vector<int32_t> t((size_t)n * k0);
            axis_taps(n_in, n_out, n, k0, bounds.data(), t.data());
            for (int i = 0; i < n; i++) std::copy(t.begin() + (size_t)i * k0, t.begin() + (size_t)(i + 1) * k0,
                                                  taps.begin() + (size_t)i * ks);
        }
        reach = bounds[2 * (n - 1)] + bounds[2 * (n - 1) + 1];
        for (int i = n; i < np; i++) bounds[2 * i] = bounds[2 * (n - 1)];
    }
};

static std::mutex g_plan_mu;
static std::list<ScalePlan> &g_plans = *new std::list<ScalePlan>;  // most recent first; never destroyed at exit

template <class T>
static bool upload(T *&d, const void *h, size_t bytes) {
    void *p = nullptr;
    if (dmalloc(&p, std::max<size_t>(bytes, 256)) != hipSuccess) return false;
    d = (T *)p;
    return hipMemcpy(p, h, bytes, hipMemcpyHostToDevice) == hipSuccess;
}

// g_plan_mu is held
static ScalePlan *plan_for(int src_w, int src_h, int out_w, int out_h) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    for (auto it = g_plans.begin(); it != g_plans.end(); ++it)
        if (it->dev == dev && it->src_w == src_w && it->src_h == src_h && it->out_w == out_w && it->out_h == out_h) {
            g_plans.splice(g_plans.begin(), g_plans, it);
            return &g_plans.front();
        }
    while ((int)g_plans.size() >= SCALE_PLANS) g_plans.pop_back();
    g_plans.emplace_front();
    ScalePlan &p = g_plans.front();
    p.dev = dev, p.src_w = src_w, p.src_h = src_h, p.out_w = out_w, p.out_h = out_h;
    load_dims(out_w, out_h, &p.tm_w, &p.tm_h);
    p.KW = p.tm_w * 8, p.KH = p.tm_h * 8;
    p.spans = (p.KW + H_SPAN - 1) / H_SPAN;
    p.KWp = p.spans * H_SPAN;
    const AxisTaps h(src_w, out_w, p.KW, p.KWp, 4), v(src_h, out_h, p.KH, p.KH, 1);
    p.ksp = h.ks, p.ksv = v.ks, p.cols = h.reach, p.rows = v.reach;
    for (int s = 0; s < p.spans; s++) {
        const int xl = std::min((s + 1) * H_SPAN, p.KW) - 1;
        p.span_px = std::max(p.span_px, h.bounds[2 * xl] + h.bounds[2 * xl + 1] - h.bounds[2 * s * H_SPAN]);
    }
    std::vector<int32_t> hk((size_t)p.ksp * p.KWp);  // [tap][column]
    for (int x = 0; x < p.KWp; x++)
        for (int t = 0; t < p.ksp; t++) hk[(size_t)t * p.KWp + x] = h.taps[(size_t)x * p.ksp + t];
    const int64_t frame_bytes = (int64_t)p.rows * p.KW * 3;
    p.group = (int)std::max<int64_t>(1, SCALE_INTER_BYTES / frame_bytes);
    bool ok = upload(p.d_hb, h.bounds.data(), h.bounds.size() * 4) && upload(p.d_hk, hk.data(), hk.size() * 4) &&
              upload(p.d_vb, v.bounds.data(), v.bounds.size() * 4) && upload(p.d_vk, v.taps.data(), v.taps.size() * 4);
    void *inter = nullptr;
    ok = ok && dmalloc(&inter, (size_t)(p.group * frame_bytes)) == hipSuccess;
    p.d_inter = (uint8_t *)inter;
    ok = ok && hipEventCreateWithFlags(&p.done, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        g_plans.pop_front();
        set_error("tiler_load_frames_scaled: out of device memory for the scaling plan");
        return nullptr;
    }
    return &p;
}

template <int BPP>
static int launch_h(const ScalePlan &p, const uint8_t *s, int64_t pitch, int64_t frame_stride, int nf, int swap,
                    hipStream_t stream) {
    // a row holds the span, the phase, and the zero-weight taps read past the last pixel's
    const int RP = (3 + (p.span_px + p.ksp) * BPP + 8) / 4 + 1;
    const size_t lds = ((size_t)8 * RP + (size_t)p.ksp * H_SPAN) * 4;
    if (lds > SCALE_LDS_MAX) return bad("tiler_load_frames_scaled", "out_w is below src_w / 8");
    const int rgroups = (p.rows + 8 * H_ITERS - 1) / (8 * H_ITERS);
    const dim3 grid((unsigned)((int64_t)nf * rgroups * p.spans));
    hipLaunchKernelGGL(scale_h_kernel<BPP>, grid, dim3(H_THREADS), lds, stream, s, pitch, frame_stride, p.d_hb, p.d_hk,
                       p.KWp, p.ksp, p.KW, p.rows, RP, p.spans, rgroups, swap, p.d_inter);
    TILER_HIP_CHECK(hipGetLastError());
    return 0;
}

int load_frames_scaled_dev(const uint8_t *d_src, int fmt, int F, int src_w, int src_h, int64_t pitch,
                           int64_t frame_stride, int out_w, int out_h, int32_t *d_rgb, hipStream_t stream) {
    if (out_w == src_w && out_h == src_h)
        return load_frames_dev(d_src, fmt, F, src_w, src_h, pitch, frame_stride, d_rgb, stream);
    if (F <= 0) return 0;
    std::lock_guard<std::mutex> lk(g_plan_mu);
    ScalePlan *pp = plan_for(src_w, src_h, out_w, out_h);
    if (!pp) return -1;
    const ScalePlan &p = *pp;
    const int swap = fmt == PIX_BGR24 || fmt == PIX_BGRA32;
    const int tspans = (p.tm_w + V_TILES - 1) / V_TILES;
    const int rgroups = (p.rows + 8 * H_ITERS - 1) / (8 * H_ITERS);
    const int64_t per_frame = std::max((int64_t)rgroups * p.spans, (int64_t)p.tm_h * tspans);
    const int per = (int)std::min<int64_t>(p.group, std::max<int64_t>(1, (1ll << 23) / per_frame));
    TILER_HIP_CHECK(hipStreamWaitEvent(stream, p.done, 0));  // the intermediate picture is one per plan
    KTimer tm("load_frames_scaled", stream);
    for (int f0 = 0; f0 < F; f0 += per) {
        const int nf = std::min(per, F - f0);
        const uint8_t *s = d_src + (int64_t)f0 * frame_stride;
        if (pix_bytes(fmt) == 3 ? launch_h<3>(p, s, pitch, frame_stride, nf, swap, stream)
                                : launch_h<4>(p, s, pitch, frame_stride, nf, swap, stream))
            return -1;
        hipLaunchKernelGGL(scale_v_kernel, dim3((unsigned)((int64_t)nf * p.tm_h * tspans)), dim3(V_THREADS), 0, stream,
                           p.d_inter, p.rows, p.KW, p.d_vb, p.d_vk, p.ksv, p.tm_w, p.tm_h, tspans,
                           d_rgb + (int64_t)f0 * p.tm_w * p.tm_h * 64);
        TILER_HIP_CHECK(hipGetLastError());
    }
    TILER_HIP_CHECK(hipEventRecord(p.done, stream));
    return 0;
}

int load_frames_scaled_host(const uint8_t *src, int fmt, int F, int src_w, int src_h, int64_t pitch,
                            int64_t frame_stride, int out_w, int out_h, int32_t *rgb) {
    if (out_w == src_w && out_h == src_h) return load_frames_host(src, fmt, F, src_w, src_h, pitch, frame_stride, rgb);
    if (F <= 0) return 0;
    int tm_w, tm_h, cols, rows;
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        const ScalePlan *p = plan_for(src_w, src_h, out_w, out_h);
        if (!p) return -1;
        tm_w = p->tm_w, tm_h = p->tm_h, cols = p->cols, rows = p->rows;
    }
    // the device image of a chunk: only the source rectangle that the kept pixels' taps reach, rows 4-byte aligned
    const int64_t row = (int64_t)cols * pix_bytes(fmt), dpitch = (row + 3) & ~3ll, dframe = dpitch * rows;
    const int64_t tile_bytes = (int64_t)tm_w * tm_h * 256;
    const int per = load_chunk_frames(F, dframe + tile_bytes);
    PoolStream ps;
    if (!ps.ok) return bad("tiler_load_frames_scaled", "no stream");
    Blocks blocks(ps.st);
    uint8_t *d_src = nullptr;
    int32_t *d_rgb = nullptr;
    if (!blocks.get(d_src, (size_t)(per * dframe)) || !blocks.get(d_rgb, (size_t)(per * tile_bytes)))
        return bad("tiler_load_frames_scaled", "out of device memory");
    for (int f0 = 0; f0 < F; f0 += per) {
        const int nf = std::min(per, F - f0);
        for (int f = 0; f < nf; f++)
            TILER_HIP_CHECK(hipMemcpy2DAsync(d_src + f * dframe, (size_t)dpitch, src + (int64_t)(f0 + f) * frame_stride,
                                             (size_t)pitch, (size_t)row, (size_t)rows, hipMemcpyHostToDevice, ps.st));
        if (load_frames_scaled_dev(d_src, fmt, nf, src_w, src_h, dpitch, dframe, out_w, out_h, d_rgb, ps.st)) return -1;
        TILER_HIP_CHECK(hipMemcpyAsync(rgb + (int64_t)f0 * tm_w * tm_h * 64, d_rgb, (size_t)(nf * tile_bytes),
                                       hipMemcpyDeviceToHost, ps.st));
    }
    TILER_HIP_CHECK(hipStreamSynchronize(ps.st));
    return 0;
}

int load_clip_scaled_dev(const uint8_t *d_src, int fmt, int F, int src_w, int src_h, int64_t pitch,
                         int64_t frame_stride, int out_w, int out_h, int32_t *d_rgb, double *corr,
                         int32_t *kf_of_frame, hipStream_t stream) {
    int tm_w, tm_h;
    if (load_dims(out_w, out_h, &tm_w, &tm_h)) return -1;
    if (F <= 0) return 0;
    if (load_frames_scaled_dev(d_src, fmt, F, src_w, src_h, pitch, frame_stride, out_w, out_h, d_rgb, stream)) return -1;
    if (interframe_corr_dev(d_rgb, F, tm_w, tm_h, corr, stream)) return -1;
    if (F == 1) TILER_HIP_CHECK(hipStreamSynchronize(stream));  // no correlation to wait for
    return find_keyframes(corr, F, tm_w * tm_h, kf_of_frame);
}

}  // namespace tiler
