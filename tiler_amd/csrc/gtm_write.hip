// gtm_write.hip -- SaveStream's command words (main.pas:4675-4725) on gfx950, from the SmoothedTileMap arrays in HBM,
// for every frame of any number of keyframes in four launches, whatever the frame count:
//   count   a workgroup per frame: the words of each of its 16 wave segments, the frame's bytes, and the checks
//           (tile in [0, T), pal in [0, min(P, 256)) at every non-smoothed position; atomicMin of
//           (frame * Q + position) * 2 + rule keeps the first offender);
//   scan    one workgroup: exclusive sum of the frames' bytes, each keyframe's fixed prefix (WriteTiles for the
//           file's first keyframe, WriteKFAttributes) added in front of its first frame -> raw_off[KF + 1],
//           frame_off[F], and which frames end a keyframe;
//   fixed   a workgroup per keyframe: the LoadPalette block (and SetDimensions / TileSet's 24 bytes; the tiles
//           themselves are one device-to-device copy);
//   emit    a workgroup per frame: the words, at frame_off[f].
// The host waits once, between scan and fixed, for raw_off[KF + 1] and the error word: a call that fails the checks
// has written nothing, and the output can be sized exactly.
//
// A frame (count and emit are the two instances of gtm_frame_kernel).  The 1,024 threads are 16 waves; wave w owns the positions
// [w seg, (w + 1) seg), seg = ceil(Q / 1024) * 64, and walks them 64 at a time with no workgroup barrier inside
// the walk.  What a position needs from outside its 64:
//   the last non-smoothed position before it (the run it is in started right after): inside the 64 from the
//   64-bit __ballot of the non-smoothed lanes, before them from a carry the wave keeps; the carry into a segment is the
//   last non-smoothed position of the nearest earlier segment that has one -- each wave finds its own from its end
//   backwards (it stops at the first 64 that hold one) and leaves it in LDS, one barrier;
//   whether the next position is smoothed: one more byte read, past the segment's end too, never past the frame's;
//   its word offset: the lanes' word counts are 0..3, so two ballots and two popcounts give the prefix within the
//   64; across segments the count pass's per-segment totals are summed.
// SkipBlock words.  The reference emits a run's word when the run ends or reaches 1024; the word for the chunk of
// a run that covers places r0 .. r0 + len - 1 (r0 a multiple of 1024) is written here by the chunk's LAST position,
// which knows len = (r mod 1024) + 1 without looking further ahead than one position.  A chunk holds no other token,
// so the order and the count of the words are those of the reference.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): count 20 VGPRs, emit 31, scan 30 (8 KiB LDS),
// fixed 9; no spills, no scratch, 128 / 64 B LDS in count / emit, occupancy 8 waves per SIMD for all four.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "gtm_write.hpp"
#include "lzma_match.hpp"
#include "stage.hpp"

namespace tiler {

namespace {

constexpr int GW_THREADS = 1024, GW_WAVES = GW_THREADS / 64;
constexpr int GW_MAX_Q = 1 << 24;
constexpr unsigned long long GW_NO_ERROR = ~0ull;

struct GwMaps {
    const int32_t *tile, *pal;
    const uint8_t *hm, *vm, *sm, *thm, *tvm;
    int Q;
    long T;
    int pal_limit;
};

struct GwHeader {
    uint16_t w[12];  // SetDimensions + its 5 words, TileSet + its 4 words
};

// One frame's walk.  EMIT = false: counts, checks.  EMIT = true: writes the words; the input has passed the checks
// (a tile index is clamped all the same, so the flag reads stay in bounds whatever the arrays hold by then).
template <bool EMIT>
__global__ __launch_bounds__(GW_THREADS) void gtm_frame_kernel(GwMaps a, int32_t *__restrict__ seg_words,
                                                              int32_t *__restrict__ frame_bytes,
                                                              unsigned long long *__restrict__ err,
                                                              const int64_t *__restrict__ frame_off,
                                                              const uint8_t *__restrict__ frame_last,
                                                              uint8_t *__restrict__ out) {
    __shared__ int s_last[GW_WAVES];
    const int f = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int Q = a.Q;
    const int seg = (Q + GW_THREADS - 1) / GW_THREADS * 64;
    const int q0 = min(Q, wave * seg), q1 = min(Q, q0 + seg);
    const long row = (long)f * Q;
    const uint8_t *__restrict__ sm = a.sm + row;
    const unsigned long long below = (1ull << lane) - 1;

    int last = -1;  // the segment's last non-smoothed position
    for (int b = q0 + ((q1 - q0 + 63) / 64 - 1) * 64; b >= q0 && last < 0; b -= 64) {
        const int q = b + lane;
        const unsigned long long bal = __ballot(q < q1 && sm[q] == 0);
        if (bal) last = b + 63 - __clzll((long long)bal);
    }
    if (lane == 0) s_last[wave] = last;
    __syncthreads();
    int carry = -1;
    for (int w = 0; w < wave; w++)
        if (s_last[w] >= 0) carry = s_last[w];

    long woff = 0;  // words before the current 64 positions (EMIT: from the frame's start; else: from the segment's)
    uint16_t *o = nullptr;
    if (EMIT) {
        for (int w = 0; w < wave; w++) woff += seg_words[f * GW_WAVES + w];
        o = reinterpret_cast<uint16_t *>(out + frame_off[f]);
    }
    for (int b = q0; b < q1; b += 64) {
        const int q = b + lane;
        const bool in = q < q1;
        const bool s = in && sm[q] != 0, ns = in && !s;
        const unsigned long long bal = __ballot(ns), m = bal & below;
        int w = 0;
        unsigned w0 = 0, w1 = 0, w2 = 0;
        if (ns) {
            int t = a.tile[row + q];
            const int p = a.pal[row + q];
            const bool bad_t = t < 0 || t >= a.T, bad_p = p < 0 || p >= a.pal_limit;
            w = t >= 65536 ? 3 : 2;
            if (EMIT) {
                if (bad_t) t = 0;
                const unsigned h = (a.hm[row + q] != 0) ^ (a.thm[t] != 0), v = (a.vm[row + q] != 0) ^ (a.tvm[t] != 0);
                const unsigned attrs = ((unsigned)p << 2 | v << 1 | h) & 1023u;
                w0 = attrs << 6 | (w == 3 ? TILER_GTM_LONG_TILE_IDX : TILER_GTM_SHORT_TILE_IDX);
                w1 = (unsigned)t & 0xFFFFu;
                w2 = (unsigned)t >> 16;
            } else if (bad_t || bad_p) {
                atomicMin(err, (unsigned long long)(row + q) * 2 + (bad_t ? 0 : 1));
            }
        } else if (s) {
            const int prev = m ? b + 63 - __clzll((long long)m) : carry;
            const int r = (q - prev - 1) & 1023;  // the place within the run's current chunk
            const bool next_s = q + 1 < Q && sm[q + 1] != 0;
            if (r == 1023 || !next_s) {
                w = 1;
                w0 = (unsigned)r << 6 | TILER_GTM_SKIP_BLOCK;
            }
        }
        const unsigned long long b0 = __ballot(w & 1), b1 = __ballot(w & 2);
        if (EMIT) {
            uint16_t *dst = o + woff + __popcll(b0 & below) + 2 * __popcll(b1 & below);
            if (w >= 1) dst[0] = (uint16_t)w0;
            if (w >= 2) dst[1] = (uint16_t)w1;
            if (w == 3) dst[2] = (uint16_t)w2;
        }
        woff += __popcll(b0) + 2 * __popcll(b1);
        if (bal) carry = b + 63 - __clzll((long long)bal);
    }
    if (EMIT) {
        if (threadIdx.x == 0) {
            long total = 0;
            for (int w = 0; w < GW_WAVES; w++) total += seg_words[f * GW_WAVES + w];
            o[total] = (uint16_t)((unsigned)frame_last[f] << 6 | TILER_GTM_FRAME_END);
        }
    } else {
        __shared__ int s_words[GW_WAVES];
        if (lane == 0) {
            s_words[wave] = (int)woff;
            seg_words[f * GW_WAVES + wave] = (int)woff;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int total = 1;  // FrameEnd
            for (int w = 0; w < GW_WAVES; w++) total += s_words[w];
            frame_bytes[f] = 2 * total;
        }
    }
}

// raw_off[k] = the bytes of the keyframes before k; frame_off[f] = where frame f's words start
__global__ __launch_bounds__(GW_THREADS) void gtm_scan_kernel(const int32_t *__restrict__ frame_bytes, int F,
                                                             const int32_t *__restrict__ kf_start, int KF,
                                                             long tiles_bytes, long attr_bytes,
                                                             int64_t *__restrict__ frame_off,
                                                             uint8_t *__restrict__ frame_last,
                                                             int64_t *__restrict__ raw_off) {
    __shared__ long s[GW_THREADS];
    const int tid = threadIdx.x;
    long carry = 0;
    for (int base = 0; base < F; base += GW_THREADS) {
        const int f = base + tid;
        long v = 0, fixed = 0;
        int k = 0;
        bool first = false;
        if (f < F) {
            int lo = 0, hi = KF;  // the largest k with kf_start[k] <= f
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (kf_start[mid] <= f) lo = mid; else hi = mid;
            }
            k = lo;
            first = kf_start[k] == f;
            if (first) fixed = attr_bytes + (k == 0 ? tiles_bytes : 0);
            v = frame_bytes[f] + fixed;
        }
        s[tid] = v;
        __syncthreads();
        for (int d = 1; d < GW_THREADS; d <<= 1) {
            const long add = tid >= d ? s[tid - d] : 0;
            __syncthreads();
            s[tid] += add;
            __syncthreads();
        }
        const long before = carry + s[tid] - v;
        if (f < F) {
            if (first) raw_off[k] = before;
            frame_off[f] = before + fixed;
            frame_last[f] = kf_start[k + 1] == f + 1;
        }
        carry += s[GW_THREADS - 1];
        __syncthreads();
    }
    if (tid == 0) raw_off[KF] = carry;
}

// WriteKFAttributes (main.pas:4589-4601) of keyframe blockIdx.x; block 0 also WriteTiles' 12 words when tiles_bytes
__global__ __launch_bounds__(256) void gtm_fixed_kernel(const int32_t *__restrict__ palettes, int P, int palsize,
                                                        const int64_t *__restrict__ raw_off, long tiles_bytes,
                                                        GwHeader hdr, uint8_t *__restrict__ out) {
    const int k = blockIdx.x;
    uint16_t *o = reinterpret_cast<uint16_t *>(out + raw_off[k]);
    if (k == 0 && tiles_bytes) {
        if (threadIdx.x < 12) o[threadIdx.x] = hdr.w[threadIdx.x];
        o += tiles_bytes / 2;
    }
    const int per = 2 + 2 * palsize;  // LoadPalette, (index, format 0), palsize dwords
    for (int i = threadIdx.x; i < P * per; i += 256) {
        const int j = i / per, c = i - j * per;
        unsigned w;
        if (c == 0) {
            w = TILER_GTM_LOAD_PALETTE;
        } else if (c == 1) {
            w = (unsigned)j & 0xFFu;
        } else {
            const unsigned v = (unsigned)palettes[((long)k * P + j) * palsize + (c - 2) / 2] | 0xFF000000u;
            w = (c & 1) ? v >> 16 : v & 0xFFFFu;
        }
        o[i] = (uint16_t)w;
    }
}

// the per-call scratch: one stream-ordered block
struct GwScratch {
    hipStream_t st;
    char *base = nullptr;
    unsigned long long *err = nullptr;
    int64_t *raw_off = nullptr, *frame_off = nullptr;
    int32_t *kf_start = nullptr, *seg_words = nullptr, *frame_bytes = nullptr;
    uint8_t *frame_last = nullptr;
    explicit GwScratch(hipStream_t s) : st(s) {}
    ~GwScratch() {
        if (base) (void)hipFreeAsync(base, st);
    }
    int alloc(int64_t F, int KF) {
        auto up = [](size_t n) { return (n + 15) & ~(size_t)15; };
        const size_t o_off = 16, o_foff = o_off + up((size_t)(KF + 1) * 8), o_kf = o_foff + up((size_t)F * 8),
                     o_seg = o_kf + up((size_t)(KF + 1) * 4), o_fb = o_seg + up((size_t)F * GW_WAVES * 4),
                     o_fl = o_fb + up((size_t)F * 4), total = o_fl + up((size_t)F);
        TILER_HIP_CHECK(hipMallocAsync((void **)&base, total, st));
        err = (unsigned long long *)base;
        raw_off = (int64_t *)(base + 8);
        frame_off = (int64_t *)(base + o_foff);
        kf_start = (int32_t *)(base + o_kf);
        seg_words = (int32_t *)(base + o_seg);
        frame_bytes = (int32_t *)(base + o_fb);
        frame_last = (uint8_t *)(base + o_fl);
        return 0;
    }
};

int gw_fail(const std::string &what) {
    set_error("gtm_write: " + what);
    return -1;
}

int gw_check_source(const tiler_gtm_source_t *s) {
    if (!s) return gw_fail("null source");
    if (s->keyframes <= 0 || s->frames <= 0 || s->positions <= 0 || s->tiles <= 0 || !s->kf_start)
        return gw_fail("keyframes, frames, positions and tiles must be positive, kf_start given");
    if (!s->tile || !s->pal || !s->hm || !s->vm || !s->smoothed || !s->thm || !s->tvm || !s->palettes)
        return gw_fail("a null array");
    if (s->positions > GW_MAX_Q || s->frames > INT32_MAX / GW_WAVES || s->tiles > (int64_t)UINT32_MAX)
        return gw_fail("more than 2^24 positions, 2^27 frames or 2^32 tiles");
    if (s->n_palettes <= 0 || s->palsize <= 0 || s->palsize >= 1024)
        return gw_fail("n_palettes must be positive, palsize in [1, 1024)");
    if ((int64_t)s->n_palettes * (2 + 2 * s->palsize) > INT32_MAX) return gw_fail("too many palettes");
    if (s->kf_start[0] != 0 || s->kf_start[s->keyframes] != s->frames)
        return gw_fail("kf_start must run from 0 to frames");
    for (int k = 0; k < s->keyframes; k++)
        if (s->kf_start[k + 1] <= s->kf_start[k]) return gw_fail("kf_start must increase: a keyframe holds a frame");
    if (s->first_keyframe) {
        if (!s->palpix) return gw_fail("the first keyframe needs the tiles (palpix)");
        if (!(s->fps > 0.0) || s->width < 0 || s->height < 0 || s->width / 8 > 65535 || s->height / 8 > 65535)
            return gw_fail("fps must be positive, width / 8 and height / 8 fit 16 bits");
    }
    return 0;
}

long gw_tiles_bytes(const tiler_gtm_source_t *s) { return s->first_keyframe ? 24 + 64 * (long)s->tiles : 0; }

GwMaps gw_maps(const tiler_gtm_source_t *s) {
    return GwMaps{s->tile, s->pal, s->hm, s->vm, s->smoothed, s->thm, s->tvm, (int)s->positions, (long)s->tiles,
                  std::min(s->n_palettes, 256)};
}

// count + scan, then the one wait: raw_off on the host, or the first offending item as the error
int gw_count(const tiler_gtm_source_t *s, GwScratch &sc, int64_t *raw_off, hipStream_t st) {
    const int F = (int)s->frames, KF = s->keyframes;
    if (sc.alloc(F, KF)) return -1;
    TILER_HIP_CHECK(hipMemsetAsync(sc.err, 0xFF, 8, st));
    TILER_HIP_CHECK(hipMemcpyAsync(sc.kf_start, s->kf_start, (size_t)(KF + 1) * 4, hipMemcpyHostToDevice, st));
    {
        KTimer tm("gtm_count", st);
        hipLaunchKernelGGL(gtm_frame_kernel<false>, dim3((unsigned)F), dim3(GW_THREADS), 0, st, gw_maps(s),
                           sc.seg_words, sc.frame_bytes, sc.err, (const int64_t *)nullptr, (const uint8_t *)nullptr,
                           (uint8_t *)nullptr);
    }
    TILER_HIP_CHECK(hipGetLastError());
    {
        KTimer tm("gtm_scan", st);
        hipLaunchKernelGGL(gtm_scan_kernel, dim3(1), dim3(GW_THREADS), 0, st, sc.frame_bytes, F, sc.kf_start, KF,
                           gw_tiles_bytes(s), (long)s->n_palettes * (4 + 4 * s->palsize), sc.frame_off, sc.frame_last,
                           sc.raw_off);
    }
    TILER_HIP_CHECK(hipGetLastError());
    std::vector<int64_t> h((size_t)KF + 2);  // the error word, then raw_off
    TILER_HIP_CHECK(hipMemcpyAsync(h.data(), sc.err, h.size() * 8, hipMemcpyDeviceToHost, st));
    TILER_HIP_CHECK(hipStreamSynchronize(st));
    const unsigned long long e = (unsigned long long)h[0];
    if (e != GW_NO_ERROR) {
        const int64_t at = (int64_t)(e >> 1), f = at / s->positions, q = at % s->positions;
        int32_t v = 0;
        TILER_HIP_CHECK(hipMemcpy(&v, ((e & 1) ? s->pal : s->tile) + at, 4, hipMemcpyDeviceToHost));
        const std::string where = " (frame " + std::to_string(f) + ", position " + std::to_string(q) + ")";
        if (e & 1)
            return gw_fail("palette index " + std::to_string(v) + " outside [0, " +
                           std::to_string(std::min(s->n_palettes, 256)) +
                           "): the palette count, and 256, the 10 attribute bits" + where);
        return gw_fail("tile index " + std::to_string(v) + " outside [0, " + std::to_string(s->tiles) +
                       "), the tile count" + where);
    }
    std::copy(h.begin() + 1, h.end(), raw_off);
    return 0;
}

// the fixed parts and the frames' words into d_raw (raw_off[KF] bytes), queued on st
int gw_emit(const tiler_gtm_source_t *s, GwScratch &sc, uint8_t *d_raw, hipStream_t st) {
    GwHeader hdr{};
    const long tiles_bytes = gw_tiles_bytes(s);
    if (tiles_bytes) {
        const uint32_t ns = (uint32_t)(uint64_t)(int64_t)fpc_round(1000 * 1000 * 1000 / s->fps);
        const uint32_t T = (uint32_t)s->tiles;
        const uint16_t w[12] = {(uint16_t)TILER_GTM_SET_DIMENSIONS,
                                (uint16_t)(s->width / 8),
                                (uint16_t)(s->height / 8),
                                (uint16_t)ns,
                                (uint16_t)(ns >> 16),
                                (uint16_t)T,
                                (uint16_t)(T >> 16),
                                (uint16_t)(s->palsize << 6 | TILER_GTM_TILE_SET),
                                0,
                                0,
                                (uint16_t)(T - 1),
                                (uint16_t)((T - 1) >> 16)};
        std::copy(w, w + 12, hdr.w);
    }
    {
        KTimer tm("gtm_fixed", st);
        if (tiles_bytes)
            TILER_HIP_CHECK(hipMemcpyAsync(d_raw + 24, s->palpix, (size_t)s->tiles * 64, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(gtm_fixed_kernel, dim3((unsigned)s->keyframes), dim3(256), 0, st, s->palettes,
                           s->n_palettes, s->palsize, (const int64_t *)sc.raw_off, tiles_bytes, hdr, d_raw);
    }
    TILER_HIP_CHECK(hipGetLastError());
    {
        KTimer tm("gtm_emit", st);
        hipLaunchKernelGGL(gtm_frame_kernel<true>, dim3((unsigned)s->frames), dim3(GW_THREADS), 0, st, gw_maps(s),
                           sc.seg_words, (int32_t *)nullptr, (unsigned long long *)nullptr,
                           (const int64_t *)sc.frame_off, (const uint8_t *)sc.frame_last, d_raw);
    }
    TILER_HIP_CHECK(hipGetLastError());
    return 0;
}

// a result of `need` bytes into dst[cap] by tiler_lzma_encode's rules; *out_len = need either way
int gw_deliver(const uint8_t *data, size_t need, uint8_t *dst, size_t cap, size_t *out_len) {
    if (out_len) *out_len = need;
    if (!dst) return 0;
    if (cap < need)
        return gw_fail("the output buffer holds " + std::to_string(cap) + " bytes, " + std::to_string(need) +
                       " are needed");
    if (need) memcpy(dst, data, need);
    return 0;
}

// the source with its arrays staged to HBM (kf_start stays on the host)
tiler_gtm_source_t gw_stage(const tiler_gtm_source_t *s, HostStage &hs) {
    tiler_gtm_source_t d = *s;
    const size_t n = (size_t)s->frames * (size_t)s->positions, T = (size_t)s->tiles;
    d.tile = hs.in(s->tile, n);
    d.pal = hs.in(s->pal, n);
    d.hm = hs.in(s->hm, n);
    d.vm = hs.in(s->vm, n);
    d.smoothed = hs.in(s->smoothed, n);
    d.palpix = s->first_keyframe ? hs.in(s->palpix, T * 64) : nullptr;
    d.thm = hs.in(s->thm, T);
    d.tvm = hs.in(s->tvm, T);
    d.palettes = hs.in(s->palettes, (size_t)s->keyframes * (size_t)s->n_palettes * (size_t)s->palsize);
    return d;
}

}  // namespace

int gtm_commands_dev(const tiler_gtm_source_t *src, uint8_t *d_raw, size_t cap, int64_t *raw_off, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (gw_check_source(src)) return -1;
    if (!raw_off) return gw_fail("raw_off is null");
    if ((uintptr_t)d_raw % 2) return gw_fail("the output is not 2-byte aligned");
    GwScratch sc(st);
    if (gw_count(src, sc, raw_off, st)) return -1;
    if (!d_raw) return 0;
    const size_t need = (size_t)raw_off[src->keyframes];
    if (cap < need)
        return gw_fail("the output buffer holds " + std::to_string(cap) + " bytes, " + std::to_string(need) +
                       " are needed");
    return gw_emit(src, sc, d_raw, st);
}

int gtm_commands_host(const tiler_gtm_source_t *src, uint8_t *raw, size_t cap, int64_t *raw_off) {
    if (gw_check_source(src)) return -1;
    if (!raw_off) return gw_fail("raw_off is null");
    HostStage hs("gtm_write");
    const tiler_gtm_source_t d = gw_stage(src, hs);
    if (!hs.ok()) return -1;
    hipStream_t st = hs.stream();
    GwScratch sc(st);
    if (gw_count(&d, sc, raw_off, st)) return -1;
    if (!raw) return 0;
    const size_t need = (size_t)raw_off[src->keyframes];
    if (cap < need)
        return gw_fail("the output buffer holds " + std::to_string(cap) + " bytes, " + std::to_string(need) +
                       " are needed");
    uint8_t *d_raw = hs.out(raw, need);
    if (!hs.ok() || gw_emit(&d, sc, d_raw, st)) return -1;
    return hs.finish();
}

int gtm_pack_dev(const tiler_gtm_source_t *src, int threads, bool whole_file, uint8_t *dst, size_t cap,
                 size_t *comp_len, size_t *out_len, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (gw_check_source(src)) return -1;
    if (threads < 0) return gw_fail("threads < 0");
    if (whole_file && !src->first_keyframe) return gw_fail("a whole file starts with the first keyframe");
    const int KF = src->keyframes;
    std::vector<int64_t> raw_off((size_t)KF + 1);
    GtmPacker pk(KF, threads);
    {
        GwScratch sc(st);
        if (gw_count(src, sc, raw_off.data(), st)) return -1;
        uint8_t *d_raw = nullptr;
        TILER_HIP_CHECK(hipMallocAsync((void **)&d_raw, std::max<size_t>((size_t)raw_off[(size_t)KF], 256), st));
        int rc = gw_emit(src, sc, d_raw, st);
        // tiler_gtm_set_gpu_matches: every stream's match table behind the command kernels (lzma_match.hip)
        uint32_t *d_table = nullptr;
        std::vector<uint8_t> has_table;
        if (rc == 0 && gtm_gpu_matches() && raw_off[(size_t)KF] > 0) {
            hipError_t e = hipMallocAsync((void **)&d_table, (size_t)raw_off[(size_t)KF] * 4, st);
            if (e != hipSuccess) rc = gw_fail(std::string("the match tables: ") + hipGetErrorString(e));
            if (rc == 0 && lzma_match_table_dev(d_raw, raw_off.data(), KF, 1u << 21, d_table, st, &has_table) < 0) rc = -1;
        }
        // a keyframe's stream (and its table) to the host, then to the compressors while the next one is copied
        for (int k = 0; k < KF && rc == 0; k++) {
            std::vector<uint8_t> &r = pk.raw(k);
            r.resize((size_t)(raw_off[(size_t)k + 1] - raw_off[(size_t)k]));
            hipError_t e = hipMemcpyAsync(r.data(), d_raw + raw_off[(size_t)k], r.size(), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess && d_table && has_table[(size_t)k] && !r.empty()) {
                KTimer tm("gtm_table_copy", st);
                std::vector<uint32_t> &t = pk.table(k);
                t.resize(r.size());
                e = hipMemcpyAsync(t.data(), d_table + raw_off[(size_t)k], t.size() * 4, hipMemcpyDeviceToHost, st);
            }
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) {
                rc = gw_fail(std::string("copying a stream to the host: ") + hipGetErrorString(e));
                break;
            }
            pk.ready(k);
        }
        if (d_table) (void)hipFreeAsync(d_table, st);
        (void)hipFreeAsync(d_raw, st);
        if (rc) return -1;
    }
    if (!pk.finish()) return -1;
    std::vector<uint8_t> all, file;
    std::vector<size_t> len((size_t)KF);
    for (int k = 0; k < KF; k++) {
        len[(size_t)k] = pk.comp(k).size();
        all.insert(all.end(), pk.comp(k).begin(), pk.comp(k).end());
    }
    if (whole_file) {
        if (!gtm_assemble(all.data(), len.data(), src->kf_start, KF, src->width, src->height, src->fps, file))
            return -1;
        return gw_deliver(file.data(), file.size(), dst, cap, out_len);
    }
    if (gw_deliver(all.data(), all.size(), dst, cap, out_len)) return -1;
    if (comp_len) std::copy(len.begin(), len.end(), comp_len);
    return 0;
}

int gtm_pack_host(const tiler_gtm_source_t *src, int threads, bool whole_file, uint8_t *dst, size_t cap,
                  size_t *comp_len, size_t *out_len) {
    if (gw_check_source(src)) return -1;
    HostStage hs("gtm_write");
    const tiler_gtm_source_t d = gw_stage(src, hs);
    if (!hs.ok()) return -1;
    return gtm_pack_dev(&d, threads, whole_file, dst, cap, comp_len, out_len, hs.stream());
}

}  // namespace tiler
