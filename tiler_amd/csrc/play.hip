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
//
// Random access.  The framebuffer before frame f is fully described by, per position, the last item drawn in frames
// [0, f) -- the carried items above -- so seeking is computing that carry without drawing.  A checkpoint index
// ckpt[C][Q] keeps the carry at the first frame of every s-th keyframe (keyframe 0 needs no row), s the smallest
// stride whose rows fit the index budget; it is built once per handle, by the first call that needs it, in one sweep
// of the walk kernel over the items up to the last checkpointed frame.  The walk kernel is the resolve kernel without the
// per-frame store: it carries the last drawn item through a pass and writes it only where a per-pass slot_of_frame[]
// names a checkpoint row (the carry *before* that frame) or a slot of the resolved items (the carry *after* it).
// seek(f) copies the checkpoint row at or before f and walks the frames between: at most s keyframes' frames, never
// f.  frames(list) dedupes and sorts the request, walks each checkpoint interval once with a scratch carry, resolves
// every requested frame into a slot, and the mapped draw writes request i's picture from its slot into output i.
#include "play.hpp"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "stage.hpp"

namespace tiler {

constexpr int64_t PL_PASS_ITEMS = (int64_t)1 << 22;  // 40 MiB staged + 32 MiB resolved per pass
constexpr int64_t PL_PASS_FRAMES = 32768;            // gridDim.y of the draw
constexpr int64_t PL_INDEX_BYTES = (int64_t)256 << 20;  // the checkpoint rows of a handle

// tiler_debug_gtm_seek: the pass size of the seek paths and the index budget, read when a handle builds its index
static std::atomic<int64_t> g_seek_pass_items{0}, g_seek_index_bytes{0};

struct Player {
    GtmData g;
    std::mutex mu;
    int dev = -1;
    int64_t next = 0;
    bool stale = true;    // the carried items do not describe `next`: rebuilt before the next pass (new, rewound, sought)
    bool broken = false;  // a play call failed half way: rewind or seek first
    uint8_t *d_tiles = nullptr;
    uint32_t *d_pal = nullptr;
    int2 *d_carry = nullptr, *d_res = nullptr;
    int32_t *d_tile = nullptr, *d_palrow = nullptr;
    uint16_t *d_attrs = nullptr;
    int64_t cap_items = 0;
    hipEvent_t done = nullptr;  // after the last call's work: the next call, on any stream, is ordered behind it
    // random access: the checkpoint index (built once), a carry of its own, the per-pass slot arrays, the draw's map
    bool indexed = false;
    int64_t seek_pass = 0;           // frames per pass of the walks
    int64_t ck_stride = 0;           // s: a row every s keyframes
    std::vector<int64_t> ck_frame;   // [C] the frame each row stands before, ascending
    int2 *d_ckpt = nullptr, *d_scratch = nullptr, *d_map = nullptr;
    int32_t *d_slot_ck = nullptr, *d_slot_res = nullptr;  // [PL_PASS_FRAMES] each
    int64_t cap_map = 0;
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

// The resolve kernel's walk without its per-frame store: one lane per position carries the last drawn item through
// the pass's n frames.  CK: slot_ck[f] >= 0 names the checkpoint row that takes the carry as it stands before frame f;
// RES: slot_res[f] >= 0 names the slot of `res` that takes it after frame f.  The slot arrays are wave-uniform reads;
// 10 B read per item, and the only stores are those rows and the final carry.
template <bool CK, bool RES>
__global__ __launch_bounds__(256) void play_walk_kernel(int n, int Q, const int32_t *__restrict__ tile,
                                                         const uint16_t *__restrict__ attrs,
                                                         const int32_t *__restrict__ palrow,
                                                         int2 *__restrict__ carry,
                                                         const int32_t *__restrict__ slot_ck,
                                                         int2 *__restrict__ ckpt,
                                                         const int32_t *__restrict__ slot_res,
                                                         int2 *__restrict__ res) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    int2 cur = carry[q];
#pragma unroll 4
    for (int f = 0; f < n; f++) {
        if (CK) {
            const int s = slot_ck[f];
            if (s >= 0) ckpt[(long)s * Q + q] = cur;
        }
        const long i = (long)f * Q + q;
        const int t = tile[i], a = attrs[i], r = palrow[i];
        if (t >= 0) cur = make_int2(t, (r << 2) | (a & 3));
        if (RES) {
            const int s = slot_res[f];
            if (s >= 0) res[(long)s * Q + q] = cur;
        }
    }
    carry[q] = cur;
}

// grid (ceil(16 Q / 256), frames of the pass); lane g of a frame stores the frame's g-th 16-byte piece in both layouts.
// MAPPED (the frames calls): row y of the grid draws the resolved items of slot map[y].x into output frame map[y].y.
template <bool RASTER, bool MAPPED = false>
__global__ __launch_bounds__(256) void play_draw_kernel(int Q, int W, const int2 *__restrict__ res,
                                                         const uint8_t *__restrict__ tiles,
                                                         const uint32_t *__restrict__ pal, int palsize,
                                                         int4 *__restrict__ out, const int2 *__restrict__ map) {
    const int g = blockIdx.x * 256 + threadIdx.x;  // 16 Q <= 2^28
    if (g >= Q * 16) return;
    long f = blockIdx.y, fo = blockIdx.y;
    if (MAPPED) {
        const int2 m = map[blockIdx.y];
        f = m.x;
        fo = m.y;
    }
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
    out[fo * Q * 16 + g] = o;
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
                     (void **)&p->d_tile, (void **)&p->d_palrow, (void **)&p->d_attrs, (void **)&p->d_ckpt,
                     (void **)&p->d_scratch, (void **)&p->d_map, (void **)&p->d_slot_ck, (void **)&p->d_slot_res}) {
        if (*b) dfree(*b);
        *b = nullptr;
    }
    if (p->done) (void)hipEventDestroy(p->done);
    p->done = nullptr;
    p->cap_items = p->cap_map = 0;
    p->indexed = false;
    p->ck_frame.clear();
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
    p->stale = true;
    p->broken = false;
    return 0;
}

int player_seek(Player *p, int64_t frame) {
    std::lock_guard<std::mutex> lk(p->mu);
    if (frame < 0 || frame > p->g.frames()) {
        set_error("gtm_seek: frame " + std::to_string(frame) + " is outside [0, " + std::to_string(p->g.frames()) +
                  "]");
        return -1;
    }
    if (frame != p->next || p->broken) p->stale = true;  // else the carry already stands before `frame`
    p->next = frame;
    p->broken = false;
    return 0;
}

int player_seek_debug(int64_t pass_items, int64_t index_bytes) {
    if (pass_items < 0 || index_bytes < 0) {
        set_error("debug_gtm_seek: a negative pass size or index budget");
        return -1;
    }
    g_seek_pass_items = pass_items;
    g_seek_index_bytes = index_bytes;
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
    p->stale = true;
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

// the first call uploads on the current device; later calls must be on it and are ordered behind the last one
static int player_attach(Player *p, hipStream_t stream) {
    if (p->dev < 0) return player_upload(p, stream);
    int cur = -1;
    TILER_HIP_CHECK(hipGetDevice(&cur));
    if (cur != p->dev) {
        set_error("gtm_play: the handle plays on device " + std::to_string(p->dev) + ", the output is on " +
                  std::to_string(cur));
        return -1;
    }
    TILER_HIP_CHECK(hipStreamWaitEvent(stream, p->done, 0));  // the staged items and the carries are reused
    return 0;
}

static int stage_items(Player *p, int64_t f0, int64_t m, hipStream_t stream) {
    const GtmData &g = p->g;
    const size_t at = (size_t)(f0 * g.Q()), items = (size_t)(m * g.Q());
    KTimer tm("play_stage", stream);
    TILER_HIP_CHECK(hipMemcpyAsync(p->d_tile, g.tile.data() + at, items * 4, hipMemcpyHostToDevice, stream));
    TILER_HIP_CHECK(hipMemcpyAsync(p->d_palrow, g.palrow.data() + at, items * 4, hipMemcpyHostToDevice, stream));
    TILER_HIP_CHECK(hipMemcpyAsync(p->d_attrs, g.attrs.data() + at, items * 2, hipMemcpyHostToDevice, stream));
    return 0;
}

// ---- random access: the walk, the checkpoint index, the carry before any frame -----------------------------------
// One pass of the walk over frames [f0, f0 + m), m <= seek_pass: staged, then carried through `carry`.  slot_ck /
// slot_res (host, [m], -1 = none, or null): the frames whose carry goes to a checkpoint row / a slot of d_res.
static int walk_pass(Player *p, int64_t f0, int64_t m, int2 *carry, const int32_t *slot_ck, const int32_t *slot_res,
                     hipStream_t stream) {
    const int64_t Q = p->g.Q();
    if (stage_items(p, f0, m, stream)) return -1;
    if (slot_ck)
        TILER_HIP_CHECK(hipMemcpyAsync(p->d_slot_ck, slot_ck, (size_t)m * 4, hipMemcpyHostToDevice, stream));
    if (slot_res)
        TILER_HIP_CHECK(hipMemcpyAsync(p->d_slot_res, slot_res, (size_t)m * 4, hipMemcpyHostToDevice, stream));
    {
        KTimer tm(slot_ck ? "play_index" : "play_walk", stream);
        const dim3 grid((unsigned)((Q + 255) / 256));
        if (slot_ck)
            hipLaunchKernelGGL((play_walk_kernel<true, false>), grid, dim3(256), 0, stream, (int)m, (int)Q, p->d_tile,
                               p->d_attrs, p->d_palrow, carry, p->d_slot_ck, p->d_ckpt, nullptr, nullptr);
        else if (slot_res)
            hipLaunchKernelGGL((play_walk_kernel<false, true>), grid, dim3(256), 0, stream, (int)m, (int)Q, p->d_tile,
                               p->d_attrs, p->d_palrow, carry, nullptr, nullptr, p->d_slot_res, p->d_res);
        else
            hipLaunchKernelGGL((play_walk_kernel<false, false>), grid, dim3(256), 0, stream, (int)m, (int)Q, p->d_tile,
                               p->d_attrs, p->d_palrow, carry, nullptr, nullptr, nullptr, nullptr);
    }
    TILER_HIP_CHECK(hipGetLastError());
    return 0;
}

// The checkpoint index, once per handle (after a release: again).  A failure leaves the handle without one, and the
// next call that needs it starts over.
static int player_index(Player *p, hipStream_t stream) {
    if (p->indexed) return 0;
    const GtmData &g = p->g;
    const int64_t Q = g.Q(), KF = g.keyframes(), row = Q * (int64_t)sizeof(int2);
    const int64_t pass_items = g_seek_pass_items.load(), budget = g_seek_index_bytes.load();
    p->seek_pass = std::max<int64_t>(1, std::min((pass_items ? pass_items : PL_PASS_ITEMS) / Q, PL_PASS_FRAMES));
    // rows at keyframes s, 2 s, ...: (KF - 1) / s of them; the smallest s that keeps them within the budget
    const int64_t max_rows = (budget ? budget : PL_INDEX_BYTES) / row;
    p->ck_stride = std::max<int64_t>(KF - 1, 0) / (max_rows + 1) + 1;
    p->ck_frame.clear();
    for (int64_t k = p->ck_stride; k < KF; k += p->ck_stride)
        if (g.kf_start[k] > (p->ck_frame.empty() ? 0 : p->ck_frame.back())) p->ck_frame.push_back(g.kf_start[k]);
    const int64_t C = (int64_t)p->ck_frame.size();
    if (p->d_ckpt || p->d_scratch || p->d_slot_ck || p->d_slot_res) {  // an earlier attempt failed half way
        TILER_HIP_CHECK(hipDeviceSynchronize());                        // dfree's rule
        for (void **b :
             {(void **)&p->d_ckpt, (void **)&p->d_scratch, (void **)&p->d_slot_ck, (void **)&p->d_slot_res}) {
            if (*b) dfree(*b);
            *b = nullptr;
        }
    }
    TILER_HIP_CHECK(dmalloc((void **)&p->d_ckpt, std::max<size_t>((size_t)(C * row), 256)));
    TILER_HIP_CHECK(dmalloc((void **)&p->d_scratch, std::max<size_t>((size_t)row, 256)));
    TILER_HIP_CHECK(dmalloc((void **)&p->d_slot_ck, (size_t)PL_PASS_FRAMES * 4));
    TILER_HIP_CHECK(dmalloc((void **)&p->d_slot_res, (size_t)PL_PASS_FRAMES * 4));
    if (player_reserve(p, p->seek_pass * Q)) return -1;
    if (C) {  // one sweep over [0, the last checkpointed frame]: that frame's row is written before its item is read
        TILER_HIP_CHECK(hipMemsetAsync(p->d_scratch, 0xFF, (size_t)row, stream));
        const int64_t end = p->ck_frame.back() + 1;
        std::vector<int32_t> slot;
        size_t c = 0;
        for (int64_t f0 = 0; f0 < end; f0 += p->seek_pass) {
            const int64_t m = std::min(p->seek_pass, end - f0);
            slot.assign((size_t)m, -1);
            for (; c < (size_t)C && p->ck_frame[c] < f0 + m; c++) slot[(size_t)(p->ck_frame[c] - f0)] = (int32_t)c;
            if (walk_pass(p, f0, m, p->d_scratch, slot.data(), nullptr, stream)) return -1;
        }
    }
    p->indexed = true;
    return 0;
}

// `carry` := the items on screen before frame `from` of the nearest checkpoint at or before `target`; returns that
// frame through *from (0: nothing drawn)
static int load_checkpoint(Player *p, int64_t target, int2 *carry, int64_t *from, hipStream_t stream) {
    const size_t row = (size_t)p->g.Q() * sizeof(int2);
    const auto it = std::upper_bound(p->ck_frame.begin(), p->ck_frame.end(), target);
    if (it == p->ck_frame.begin()) {
        TILER_HIP_CHECK(hipMemsetAsync(carry, 0xFF, row, stream));  // tile -1: never drawn
        *from = 0;
        return 0;
    }
    const size_t c = (size_t)(it - p->ck_frame.begin()) - 1;
    TILER_HIP_CHECK(hipMemcpyAsync(carry, p->d_ckpt + c * (size_t)p->g.Q(), row, hipMemcpyDeviceToDevice, stream));
    *from = p->ck_frame[c];
    return 0;
}

// the sequential carry for frame `target`: at most ck_stride keyframes' frames walked, nothing drawn
static int player_rebuild_carry(Player *p, int64_t target, hipStream_t stream) {
    if (target == 0) {  // tile -1: never drawn
        TILER_HIP_CHECK(hipMemsetAsync(p->d_carry, 0xFF, (size_t)p->g.Q() * sizeof(int2), stream));
        return 0;
    }
    if (player_index(p, stream)) return -1;
    int64_t f0 = 0;
    if (load_checkpoint(p, target, p->d_carry, &f0, stream)) return -1;
    for (; f0 < target; f0 += p->seek_pass)
        if (walk_pass(p, f0, std::min(p->seek_pass, target - f0), p->d_carry, nullptr, nullptr, stream)) return -1;
    return 0;
}

static int play_passes(Player *p, int64_t n, int layout, int32_t *d_rgb, int32_t *d_undrawn, hipStream_t stream) {
    const GtmData &g = p->g;
    const int64_t Q = g.Q();
    if (player_attach(p, stream)) return -1;
    if (p->stale) {
        if (player_rebuild_carry(p, p->next, stream)) return -1;
        p->stale = false;
    }
    const int64_t pass = std::max<int64_t>(1, std::min({n, PL_PASS_ITEMS / Q, PL_PASS_FRAMES}));
    if (player_reserve(p, pass * Q)) return -1;
    for (int64_t done = 0; done < n; done += pass) {
        const int64_t m = std::min(pass, n - done);
        if (stage_items(p, p->next + done, m, stream)) return -1;
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
                                   p->d_tiles, p->d_pal, g.palsize, out, nullptr);
            else
                hipLaunchKernelGGL(play_draw_kernel<false>, grid, dim3(256), 0, stream, (int)Q, g.width, p->d_res,
                                   p->d_tiles, p->d_pal, g.palsize, out, nullptr);
        }
        TILER_HIP_CHECK(hipGetLastError());
    }
    if (d_undrawn)
        TILER_HIP_CHECK(hipMemcpyAsync(d_undrawn, g.undrawn.data() + p->next, (size_t)n * 4, hipMemcpyHostToDevice,
                                       stream));
    TILER_HIP_CHECK(hipEventRecord(p->done, stream));
    return 0;
}

// frames[0..n) (validated, any order, repeats allowed) into d_rgb[i] / d_undrawn[i]: the sequential state is not
// touched.  The distinct frames, ascending, are resolved seek_pass at a time into the slots of d_res -- each
// checkpoint interval walked once, the walk going on from one requested frame to the next while no checkpoint lies
// between -- and each batch is drawn through the map (slot, output frame), the requests sorted by frame.
static int frames_passes(Player *p, const int64_t *frames, int64_t n, int layout, int32_t *d_rgb, int32_t *d_undrawn,
                         hipStream_t stream) {
    const GtmData &g = p->g;
    const int64_t Q = g.Q();
    if (player_attach(p, stream) || player_index(p, stream)) return -1;
    const int64_t pass = p->seek_pass;
    std::vector<int64_t> order((size_t)n), uniq;
    for (int64_t i = 0; i < n; i++) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return frames[a] < frames[b]; });
    std::vector<int2> map((size_t)n);
    std::vector<int64_t> batch_at{0};  // the first request (in sorted order) of every batch of `pass` distinct frames
    for (int64_t j = 0; j < n; j++) {
        const int64_t f = frames[order[(size_t)j]];
        if (uniq.empty() || uniq.back() != f) {
            if (!uniq.empty() && (int64_t)uniq.size() % pass == 0) batch_at.push_back(j);
            uniq.push_back(f);
        }
        map[(size_t)j] = make_int2((int)(((int64_t)uniq.size() - 1) % pass), (int)order[(size_t)j]);
    }
    batch_at.push_back(n);
    if (n > p->cap_map) {
        if (p->cap_map) TILER_HIP_CHECK(hipEventSynchronize(p->done));
        if (p->d_map) dfree(p->d_map);
        p->d_map = nullptr;
        p->cap_map = 0;
        TILER_HIP_CHECK(dmalloc((void **)&p->d_map, std::max<size_t>((size_t)n * sizeof(int2), 256)));
        p->cap_map = n;
    }
    TILER_HIP_CHECK(hipMemcpyAsync(p->d_map, map.data(), (size_t)n * sizeof(int2), hipMemcpyHostToDevice, stream));

    int64_t pos = -1;           // the scratch carry stands before frame pos + slot.size(); -1: it holds nothing yet
    std::vector<int32_t> slot;  // the pending pass: frames [pos, pos + slot.size()), the last one requested
    const auto flush = [&]() -> int {
        if (slot.empty()) return 0;
        if (walk_pass(p, pos, (int64_t)slot.size(), p->d_scratch, nullptr, slot.data(), stream)) return -1;
        pos += (int64_t)slot.size();
        slot.clear();
        return 0;
    };
    for (size_t b = 0; b + 1 < batch_at.size(); b++) {
        const size_t u0 = b * (size_t)pass, u1 = std::min(uniq.size(), u0 + (size_t)pass);
        for (size_t u = u0; u < u1; u++) {
            const int64_t f = uniq[u];
            const auto ck = std::upper_bound(p->ck_frame.begin(), p->ck_frame.end(), f);
            const int64_t ckf = ck == p->ck_frame.begin() ? 0 : *(ck - 1);
            if (pos < 0 || ckf > pos + (int64_t)slot.size()) {  // a checkpoint nearer than the walk's own position
                if (flush() || load_checkpoint(p, f, p->d_scratch, &pos, stream)) return -1;
            }
            while (pos + (int64_t)slot.size() <= f) {
                slot.push_back(pos + (int64_t)slot.size() == f ? (int32_t)(u - u0) : -1);
                if ((int64_t)slot.size() == pass && flush()) return -1;
            }
        }
        if (flush()) return -1;
        KTimer tm("play_draw", stream);
        for (int64_t j = batch_at[b]; j < batch_at[b + 1]; j += PL_PASS_FRAMES) {
            const dim3 grid((unsigned)((Q * 16 + 255) / 256), (unsigned)std::min(PL_PASS_FRAMES, batch_at[b + 1] - j));
            int4 *out = reinterpret_cast<int4 *>(d_rgb);
            if (layout == 1)
                hipLaunchKernelGGL((play_draw_kernel<true, true>), grid, dim3(256), 0, stream, (int)Q, g.width, p->d_res,
                                   p->d_tiles, p->d_pal, g.palsize, out, p->d_map + j);
            else
                hipLaunchKernelGGL((play_draw_kernel<false, true>), grid, dim3(256), 0, stream, (int)Q, g.width,
                                   p->d_res, p->d_tiles, p->d_pal, g.palsize, out, p->d_map + j);
            TILER_HIP_CHECK(hipGetLastError());
        }
    }
    if (d_undrawn) {
        std::vector<int32_t> und((size_t)n);
        for (int64_t i = 0; i < n; i++) und[(size_t)i] = g.undrawn[(size_t)frames[i]];
        TILER_HIP_CHECK(hipMemcpyAsync(d_undrawn, und.data(), (size_t)n * 4, hipMemcpyHostToDevice, stream));
    }
    TILER_HIP_CHECK(hipEventRecord(p->done, stream));
    return 0;
}

static int64_t play_locked(Player *p, int64_t n, int layout, int32_t *d_rgb, int32_t *d_undrawn, hipStream_t stream) {
    if (n < 0 || (layout != 0 && layout != 1)) {
        set_error("gtm_play: n < 0, or a layout other than 0 (tile-major) / 1 (raster)");
        return -1;
    }
    if (p->broken) {
        set_error("gtm_play: an earlier play call failed half way; rewind or seek first");
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

int player_check_frames(Player *p, const int64_t *frames, int64_t n, int layout) {
    if (n < 0 || (layout != 0 && layout != 1)) {
        set_error("gtm_frames: n < 0, or a layout other than 0 (tile-major) / 1 (raster)");
        return -1;
    }
    if (n > 0 && !frames) {
        set_error("gtm_frames: a null frame list");
        return -1;
    }
    const int64_t F = p->g.frames();  // fixed at open: no lock
    for (int64_t i = 0; i < n; i++)
        if (frames[i] < 0 || frames[i] >= F) {
            set_error("gtm_frames: frames[" + std::to_string(i) + "] = " + std::to_string(frames[i]) +
                      " is outside [0, " + std::to_string(F) + ")");
            return -1;
        }
    return 0;
}

// a failure leaves the sequential state as it was: only the scratch carry and the staged items were written
static int64_t frames_locked(Player *p, const int64_t *frames, int64_t n, int layout, int32_t *d_rgb,
                             int32_t *d_undrawn, hipStream_t stream) {
    if (player_check_frames(p, frames, n, layout)) return -1;
    if (n == 0) return 0;
    if (!d_rgb || (uintptr_t)d_rgb % 16) {
        set_error("gtm_frames: the output is null or not 16-byte aligned");
        return -1;
    }
    return frames_passes(p, frames, n, layout, d_rgb, d_undrawn, stream) ? -1 : n;
}

int64_t player_frames_dev(Player *p, const int64_t *frames, int64_t n, int layout, int32_t *d_rgb, int32_t *d_undrawn,
                          hipStream_t stream) {
    std::lock_guard<std::mutex> lk(p->mu);
    return frames_locked(p, frames, n, layout, d_rgb, d_undrawn, stream);
}

int64_t player_frames_host(Player *p, const int64_t *frames, int64_t n, int layout, int32_t *rgb, int32_t *undrawn) {
    std::lock_guard<std::mutex> lk(p->mu);
    if (n > 0 && !rgb) {
        set_error("gtm_frames: a null output");
        return -1;
    }
    HostStage s("gtm_frames");
    int32_t *d_rgb = s.out(rgb, (size_t)n * (size_t)p->g.Q() * 64), *d_undrawn = s.out(undrawn, (size_t)n);
    if (!s.ok() || frames_locked(p, frames, n, layout, d_rgb, d_undrawn, s.stream()) < 0) return -1;
    return s.finish() ? -1 : n;
}

}  // namespace tiler
