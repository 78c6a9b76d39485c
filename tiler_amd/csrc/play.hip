// play.hip -- the GTM frame player on gfx950: the reference player's framebuffer (drawTilemapItem / decodeFrame,
// decoders/htmljs/gtm.player.js:182-353) reproduced from a parsed .gtm file (gtm_read.cpp).
//
// Semantics.  A drawn item writes its 8x8 tile through the palette contents in effect at that moment; H mirrors x,
// V mirrors y.  A skipped position keeps its pixels -- across keyframe boundaries, and when its palette index is
// reloaded later: the reader gives every LoadPalette a row of its own in the palette version table and every item the
// row it was drawn with.  Before the first draw a pixel is opaque black.  A pixel is the stream's palette dword as
// stored, 0xAABBGGRR (AA = 0xFF in this writer's streams), never-drawn pixels 0xFF000000; comparing with the project's
// 0x00BBGGRR frames (render_frames_kernel) masks the top byte.
// Not supported (the reader rejects them): a second SetDimensions that changes the size or the tile count, and a
// TileSet after the first frame.  The reader sees every item and validates it (tile < T, tile bytes < palsize, palrow
// < R), so the kernels trust their input.
//
// The handle plays sequentially in chunks of frames; between calls it keeps, per position, the last drawn item
// (tile, palrow << 2 | V << 1 | H), tile -1 = never drawn.  A call is cut into passes of at most PL_PASS_ITEMS items,
// so the staged items and the resolved items take bounded HBM whatever n is.  Per pass:
//   stage    the frames' dense items (tile int32, attrs uint16, palrow int32: 10 B per item) to HBM;
//   resolve  one lane per position walks the pass's frames in order carrying the last drawn item and writes the
//            resolved item of every (frame, position): 10 B read + 8 B written per item, coalesced across positions,
//            no atomics;
//   draw     one resolved item -> 64 pixels: a lane owns 4 adjacent output pixels -- one 32-bit word of the tile row
//            selected by V, byte-reversed under H, four palette dwords (the version table is small and L2-resident),
//            one 16-byte store.  256 B written per item: the draw is bound by the HBM write rate.
// Two output layouts, two instances of the draw: tile-major [n][Q][64] (the project's frame layout: 16 lanes write a
// tile's 256 contiguous bytes) and raster [n][8 H][8 W] (lane order follows the pixel row across adjacent tiles of a
// tilemap row, so consecutive lanes still store consecutive 16-byte pieces; each lane pair reads its own item).
// The per-frame count of never-drawn positions is a property of the stream alone: the reader counts it during its
// token walk and the call copies those counts out, so nothing on the result path is reduced on the device.
#include "play.hpp"

#include <algorithm>
#include <mutex>
#include <string>

#include "stage.hpp"

namespace tiler {

constexpr int64_t PL_PASS_ITEMS = (int64_t)1 << 22;  // 40 MiB staged + 32 MiB resolved per pass
constexpr int64_t PL_PASS_FRAMES = 32768;            // gridDim.y of the draw

struct Player {
    GtmData g;
    std::mutex mu;
    int dev = -1;
    int64_t next = 0;
    bool fresh = true;    // the carried items must be reset before the next pass (new or rewound)
    bool broken = false;  // a play call failed half way: rewind first
    uint8_t *d_tiles = nullptr;
    uint32_t *d_pal = nullptr;
    int2 *d_carry = nullptr, *d_res = nullptr;
    int32_t *d_tile = nullptr, *d_palrow = nullptr;
    uint16_t *d_attrs = nullptr;
    int64_t cap_items = 0;
    hipEvent_t done = nullptr;  // after the last call's work: the next call, on any stream, is ordered behind it
};

__global__ __launch_bounds__(256) void play_resolve_kernel(int n, int Q, const int32_t *__restrict__ tile,
                                                            const uint16_t *__restrict__ attrs,
                                                            const int32_t *__restrict__ palrow,
                                                            int2 *__restrict__ carry, int2 *__restrict__ res) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    int2 cur = carry[q];
#pragma unroll 4
    for (int f = 0; f < n; f++) {
        const long i = (long)f * Q + q;
        const int t = tile[i], a = attrs[i], r = palrow[i];
        if (t >= 0) cur = make_int2(t, (r << 2) | (a & 3));
        res[i] = cur;
    }
    carry[q] = cur;
}

// grid (ceil(16 Q / 256), frames of the pass); lane g of a frame stores the frame's g-th 16-byte piece in both layouts
template <bool RASTER>
__global__ __launch_bounds__(256) void play_draw_kernel(int Q, int W, const int2 *__restrict__ res,
                                                         const uint8_t *__restrict__ tiles,
                                                         const uint32_t *__restrict__ pal, int palsize,
                                                         int4 *__restrict__ out) {
    const int g = blockIdx.x * 256 + threadIdx.x;  // 16 Q <= 2^28
    if (g >= Q * 16) return;
    const long f = blockIdx.y;
    int q, ty, half;
    if (RASTER) {  // piece x4 of pixel row y: tile (y / 8, x4 / 2), its row y % 8, half x4 % 2
        const int row4 = W * 2;
        const int y = g / row4, x4 = g - y * row4;
        q = (y >> 3) * W + (x4 >> 1);
        ty = y & 7;
        half = x4 & 1;
    } else {
        q = g >> 4;
        ty = (g >> 1) & 7;
        half = g & 1;
    }
    const int2 it = res[f * Q + q];
    const int black = (int)0xFF000000u;
    int4 o = make_int4(black, black, black, black);
    if (it.x >= 0) {
        const bool fh = it.y & 1, fv = it.y & 2;
        const int tym = fv ? 7 - ty : ty, tx0 = half * 4;
        unsigned w = *reinterpret_cast<const unsigned *>(tiles + (long)it.x * 64 + tym * 8 + (fh ? 4 - tx0 : tx0));
        if (fh) w = __builtin_bswap32(w);
        const uint32_t *prow = pal + (long)(it.y >> 2) * palsize;
        o = make_int4((int)prow[w & 0xffu], (int)prow[(w >> 8) & 0xffu], (int)prow[(w >> 16) & 0xffu],
                      (int)prow[w >> 24]);
    }
    out[f * Q * 16 + g] = o;
}

Player *player_open(const uint8_t *data, size_t n, int threads, size_t max_raw) {
    Player *p = new Player();
    if (!gtm_parse(data, n, threads, max_raw, p->g)) {
        delete p;
        return nullptr;
    }
    return p;
}

// back to the state before the first play call (on the handle's device, which the caller has made current)
static void player_release(Player *p) {
    if (p->dev < 0) return;
    (void)hipDeviceSynchronize();
    for (void **b : {(void **)&p->d_tiles, (void **)&p->d_pal, (void **)&p->d_carry, (void **)&p->d_res,
                     (void **)&p->d_tile, (void **)&p->d_palrow, (void **)&p->d_attrs}) {
        if (*b) dfree(*b);
        *b = nullptr;
    }
    if (p->done) (void)hipEventDestroy(p->done);
    p->done = nullptr;
    p->cap_items = 0;
    p->dev = -1;
}

void player_close(Player *p) {
    if (!p) return;
    player_release(p);
    delete p;
}

const GtmData &player_data(const Player *p) { return p->g; }
int player_device(const Player *p) { return p->dev; }

int64_t player_next_frame(Player *p) {
    std::lock_guard<std::mutex> lk(p->mu);
    return p->next;
}

int player_rewind(Player *p) {
    std::lock_guard<std::mutex> lk(p->mu);
    p->next = 0;
    p->fresh = true;
    p->broken = false;
    return 0;
}

// the tileset, the palette versions and the carried items, once, on the current device
static int player_upload_locked(Player *p, hipStream_t stream) {
    const GtmData &g = p->g;
    TILER_HIP_CHECK(hipEventCreateWithFlags(&p->done, hipEventDisableTiming));
    TILER_HIP_CHECK(dmalloc((void **)&p->d_tiles, std::max<size_t>(g.tiles.size(), 256)));
    TILER_HIP_CHECK(dmalloc((void **)&p->d_pal, std::max<size_t>(g.palettes.size() * 4, 256)));
    TILER_HIP_CHECK(dmalloc((void **)&p->d_carry, std::max<size_t>((size_t)g.Q() * sizeof(int2), 256)));
    if (!g.tiles.empty())
        TILER_HIP_CHECK(hipMemcpyAsync(p->d_tiles, g.tiles.data(), g.tiles.size(), hipMemcpyHostToDevice, stream));
    if (!g.palettes.empty())
        TILER_HIP_CHECK(
            hipMemcpyAsync(p->d_pal, g.palettes.data(), g.palettes.size() * 4, hipMemcpyHostToDevice, stream));
    return 0;
}
static int player_upload(Player *p, hipStream_t stream) {
    int cur = 0;
    TILER_HIP_CHECK(hipGetDevice(&cur));
    p->dev = cur;
    p->fresh = true;
    if (player_upload_locked(p, stream) == 0) return 0;
    player_release(p);  // nothing half-made stays behind: the next call starts over
    return -1;
}

// room for a pass of `items`; the outgrown blocks are idle once the last call's work is done
static int player_reserve(Player *p, int64_t items) {
    if (items <= p->cap_items) return 0;
    if (p->cap_items) TILER_HIP_CHECK(hipEventSynchronize(p->done));
    for (void **b : {(void **)&p->d_res, (void **)&p->d_tile, (void **)&p->d_palrow, (void **)&p->d_attrs}) {
        if (*b) dfree(*b);
        *b = nullptr;
    }
    p->cap_items = 0;
    TILER_HIP_CHECK(dmalloc((void **)&p->d_res, (size_t)items * sizeof(int2)));
    TILER_HIP_CHECK(dmalloc((void **)&p->d_tile, (size_t)items * 4));
    TILER_HIP_CHECK(dmalloc((void **)&p->d_palrow, (size_t)items * 4));
    TILER_HIP_CHECK(dmalloc((void **)&p->d_attrs, (size_t)items * 2));
    p->cap_items = items;
    return 0;
}

static int play_passes(Player *p, int64_t n, int layout, int32_t *d_rgb, int32_t *d_undrawn, hipStream_t stream) {
    const GtmData &g = p->g;
    const int64_t Q = g.Q();
    if (p->dev < 0) {
        if (player_upload(p, stream)) return -1;
    } else {
        int cur = -1;
        TILER_HIP_CHECK(hipGetDevice(&cur));
        if (cur != p->dev) {
            set_error("gtm_play: the handle plays on device " + std::to_string(p->dev) + ", the output is on " +
                      std::to_string(cur));
            return -1;
        }
        TILER_HIP_CHECK(hipStreamWaitEvent(stream, p->done, 0));  // the staged items and the carry are reused
    }
    const int64_t pass = std::max<int64_t>(1, std::min({n, PL_PASS_ITEMS / Q, PL_PASS_FRAMES}));
    if (player_reserve(p, pass * Q)) return -1;
    if (p->fresh) {  // tile -1: never drawn
        TILER_HIP_CHECK(hipMemsetAsync(p->d_carry, 0xFF, (size_t)Q * sizeof(int2), stream));
        p->fresh = false;
    }
    for (int64_t done = 0; done < n; done += pass) {
        const int64_t m = std::min(pass, n - done);
        const size_t at = (size_t)((p->next + done) * Q), items = (size_t)(m * Q);
        {
            KTimer tm("play_stage", stream);
            TILER_HIP_CHECK(hipMemcpyAsync(p->d_tile, g.tile.data() + at, items * 4, hipMemcpyHostToDevice, stream));
            TILER_HIP_CHECK(hipMemcpyAsync(p->d_palrow, g.palrow.data() + at, items * 4, hipMemcpyHostToDevice, stream));
            TILER_HIP_CHECK(hipMemcpyAsync(p->d_attrs, g.attrs.data() + at, items * 2, hipMemcpyHostToDevice, stream));
        }
        {
            KTimer tm("play_resolve", stream);
            hipLaunchKernelGGL(play_resolve_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, stream, (int)m,
                               (int)Q, p->d_tile, p->d_attrs, p->d_palrow, p->d_carry, p->d_res);
        }
        TILER_HIP_CHECK(hipGetLastError());
        {
            KTimer tm("play_draw", stream);
            const dim3 grid((unsigned)((Q * 16 + 255) / 256), (unsigned)m);
            int4 *out = reinterpret_cast<int4 *>(d_rgb) + (size_t)done * (size_t)Q * 16;
            if (layout == 1)
                hipLaunchKernelGGL(play_draw_kernel<true>, grid, dim3(256), 0, stream, (int)Q, g.width, p->d_res,
                                   p->d_tiles, p->d_pal, g.palsize, out);
            else
                hipLaunchKernelGGL(play_draw_kernel<false>, grid, dim3(256), 0, stream, (int)Q, g.width, p->d_res,
                                   p->d_tiles, p->d_pal, g.palsize, out);
        }
        TILER_HIP_CHECK(hipGetLastError());
    }
    if (d_undrawn)
        TILER_HIP_CHECK(hipMemcpyAsync(d_undrawn, g.undrawn.data() + p->next, (size_t)n * 4, hipMemcpyHostToDevice,
                                       stream));
    TILER_HIP_CHECK(hipEventRecord(p->done, stream));
    return 0;
}

static int64_t play_locked(Player *p, int64_t n, int layout, int32_t *d_rgb, int32_t *d_undrawn, hipStream_t stream) {
    if (n < 0 || (layout != 0 && layout != 1)) {
        set_error("gtm_play: n < 0, or a layout other than 0 (tile-major) / 1 (raster)");
        return -1;
    }
    if (p->broken) {
        set_error("gtm_play: an earlier play call failed half way; rewind the handle first");
        return -1;
    }
    n = std::min(n, p->g.frames() - p->next);
    if (n <= 0) return 0;
    if (!d_rgb || (uintptr_t)d_rgb % 16) {
        set_error("gtm_play: the output is null or not 16-byte aligned");
        return -1;
    }
    if (play_passes(p, n, layout, d_rgb, d_undrawn, stream)) {
        p->broken = p->dev >= 0;
        return -1;
    }
    p->next += n;
    return n;
}

int64_t player_play_dev(Player *p, int64_t n, int layout, int32_t *d_rgb, int32_t *d_undrawn, hipStream_t stream) {
    std::lock_guard<std::mutex> lk(p->mu);
    return play_locked(p, n, layout, d_rgb, d_undrawn, stream);
}

int64_t player_play_host(Player *p, int64_t n, int layout, int32_t *rgb, int32_t *undrawn) {
    std::lock_guard<std::mutex> lk(p->mu);
    if (n < 0 || (n > 0 && !rgb)) {
        set_error("gtm_play: n < 0 or a null output");
        return -1;
    }
    const int64_t m = std::min(n, p->g.frames() - p->next);
    if (m <= 0 || p->broken) return play_locked(p, n, layout, nullptr, nullptr, nullptr);  // 0, or the error
    HostStage s("gtm_play");
    int32_t *d_rgb = s.out(rgb, (size_t)m * (size_t)p->g.Q() * 64), *d_undrawn = s.out(undrawn, (size_t)m);
    if (!s.ok() || play_locked(p, m, layout, d_rgb, d_undrawn, s.stream()) < 0) return -1;
    return s.finish() ? -1 : m;
}

}  // namespace tiler
