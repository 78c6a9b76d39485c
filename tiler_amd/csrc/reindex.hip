// reindex.hip -- Reindex on gfx950: UseCount / Active from the TileMaps (btnReindexClick main.pas:1208-1221), the
// order of ReindexTiles (main.pas:4483-4527, CompareTileUseCountRev 4472-4481), the gather of the tile list into that
// order and the TileMap remap (main.pas:4523-4526; FinishMergeTiles 3722-3734 is the same gather with "keep").
//
// Counting.  After FrameTiling a few tiles take a large share of all items, so one global atomic per item would queue
// on a few words.  Two strategies, chosen by the number of tiles (tiler_debug_reindex forces either):
//   rx_count_lds     a workgroup counts RX_CHUNK consecutive items into its own LDS: 65,536 bins as 32,768 dwords of
//                    two 16-bit fields (128 KiB), ds_add of 1 or 1 << 16.  RX_CHUNK < 65,536, so no field can pass
//                    65,535 and nothing ever carries from the low field into the high one, whatever the items are.
//                    More tiles than one window: blockIdx.y is the window, a workgroup reads its chunk and counts the
//                    items of its window alone (the items are read once per window).  The non-zero fields then go to
//                    use_count with one 64-bit atomic each: a hot tile costs one global atomic per chunk, not per item.
//   rx_count_global  above RX_MAX_WINDOWS windows the re-reading costs more than it saves: every item adds to use_count
//                    directly, after the lanes of a wave that hold the same tile as the wave's first pending lane are
//                    combined into one add (one round; the hot tile, if there is one, is most likely that lane's).
// Both validate every item against [0, nt) and keep the lowest offending index in an error word (atomicMin), as
// gtm_write.hip does; an offending item is never used as an index.  Only integer atomics touch a result.
//
// Order.  key = 0x7FFFFFFF - UseCount for an Active tile (UseCount in [0, 2^31), the reference's Integer), 0xFFFFFFFF
// for an inactive one; one stable radix sort (hipcub) of (key, index) over all nt tiles with the indices ascending on
// entry gives UseCount descending, index ascending among equals, the inactive tiles last: no separate compaction.
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <string>

#include "reindex.hpp"
#include "stage.hpp"

namespace tiler {

static constexpr int RX_NT = 1024;             // threads of a counting workgroup (one per CU: it owns 128 KiB of LDS)
static constexpr int RX_WIN = 65536;           // bins of a window
static constexpr long RX_CHUNK = 61440;        // items of a workgroup: < 65,536 (no 16-bit field wraps), 60 per thread
static constexpr long RX_MAX_WINDOWS = 16;     // more: rx_count_global
static constexpr int RX_T = 256;               // threads of every other kernel
static constexpr unsigned long long RX_NO_ERROR = ~0ull;
static_assert(RX_CHUNK < 65536 && RX_CHUNK % 4 == 0, "a chunk must not be able to wrap a 16-bit field");

static std::atomic<int> g_rx_strategy{-1};  // tiler_debug_reindex

// ---- use counts ----
__device__ __forceinline__ void rx_lds_item(int t, long i, unsigned nt, unsigned win, unsigned *cnt,
                                            unsigned long long *err) {
    const unsigned u = (unsigned)t;
    if (u >= nt) {
        if (win == 0) atomicMin(err, (unsigned long long)i);
    } else if ((u >> 16) == win) {
        atomicAdd(&cnt[(u & 0xFFFFu) >> 1], 1u << ((u & 1u) * 16));
    }
}

__global__ __launch_bounds__(RX_NT) void rx_count_lds(const int *__restrict__ tile, long n, unsigned nt, int vec,
                                                       unsigned long long *use_count, unsigned long long *err) {
    __shared__ unsigned cnt[RX_WIN / 2];
    const unsigned win = blockIdx.y;
    for (int w = threadIdx.x; w < RX_WIN / 8; w += RX_NT) reinterpret_cast<uint4 *>(cnt)[w] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const long i0 = (long)blockIdx.x * RX_CHUNK, i1 = min(n, i0 + RX_CHUNK);
    for (long i = i0 + (long)threadIdx.x * 4; i < i1; i += (long)RX_NT * 4) {
        if (vec && i + 4 <= i1) {  // the chunks start at multiples of 4 items: as aligned as the array
            const int4 v = *reinterpret_cast<const int4 *>(tile + i);
            rx_lds_item(v.x, i, nt, win, cnt, err);
            rx_lds_item(v.y, i + 1, nt, win, cnt, err);
            rx_lds_item(v.z, i + 2, nt, win, cnt, err);
            rx_lds_item(v.w, i + 3, nt, win, cnt, err);
        } else {
            for (long j = i; j < min(i + 4, i1); j++) rx_lds_item(tile[j], j, nt, win, cnt, err);
        }
    }
    __syncthreads();
    // a non-zero field was counted from a validated item of this window: its bin is below nt
    for (int w = threadIdx.x; w < RX_WIN / 2; w += RX_NT) {
        const unsigned v = cnt[w];
        if (!v) continue;
        const long bin = (long)win * RX_WIN + 2 * w;
        if (v & 0xFFFFu) atomicAdd(&use_count[bin], (unsigned long long)(v & 0xFFFFu));
        if (v >> 16) atomicAdd(&use_count[bin + 1], (unsigned long long)(v >> 16));
    }
}

__global__ __launch_bounds__(RX_T) void rx_count_global(const int *__restrict__ tile, long n, unsigned nt, int vec,
                                                         unsigned long long *use_count, unsigned long long *err) {
    const int lane = threadIdx.x & 63;
    // base is the same for a whole workgroup, so every lane of a wave takes every trip and the votes are complete
    for (long base = (long)blockIdx.x * RX_T * 4; base < n; base += (long)gridDim.x * RX_T * 4) {
        const long i = base + (long)threadIdx.x * 4;
        const int have = (int)max(0L, min(4L, n - i));
        int v[4] = {0, 0, 0, 0};
        if (vec && have == 4) {
            const int4 q = *reinterpret_cast<const int4 *>(tile + i);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
            for (int k = 0; k < have; k++) v[k] = tile[i + k];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int t = v[k];
            bool pend = k < have;
            if (pend && (unsigned)t >= nt) {
                atomicMin(err, (unsigned long long)(i + k));
                pend = false;
            }
            const unsigned long long any = __ballot(pend);
            if (any) {
                const int key = __shfl(t, __ffsll(any) - 1);
                const unsigned long long same = __ballot(pend && t == key);
                if (pend && t == key) {
                    if (lane == __ffsll(same) - 1) atomicAdd(&use_count[key], (unsigned long long)__popcll(same));
                    pend = false;
                }
            }
            if (pend) atomicAdd(&use_count[t], 1ull);
        }
    }
}

__global__ __launch_bounds__(RX_T) void rx_active(const long long *__restrict__ use_count, long nt,
                                                   uint8_t *__restrict__ active) {
    for (long t = (long)blockIdx.x * RX_T + threadIdx.x; t < nt; t += (long)gridDim.x * RX_T)
        active[t] = use_count[t] > 0;
}

// ---- the order ----
// w[0] = the first tile whose UseCount is outside [0, 2^31), w[1] = the Active tiles
__global__ __launch_bounds__(RX_T) void rx_keys(const uint8_t *__restrict__ active,
                                                 const long long *__restrict__ use_count, long nt,
                                                 unsigned *__restrict__ key, unsigned *__restrict__ val,
                                                 unsigned long long *w) {
    for (long base = (long)blockIdx.x * RX_T; base < nt; base += (long)gridDim.x * RX_T) {
        const long t = base + threadIdx.x;
        bool on = false;
        if (t < nt) {
            const long long c = use_count[t];
            const bool bad = c < 0 || c > 0x7FFFFFFFll;
            if (bad) atomicMin(&w[0], (unsigned long long)t);
            on = active[t] != 0;
            key[t] = on && !bad ? 0x7FFFFFFFu - (unsigned)c : 0xFFFFFFFFu;
            val[t] = (unsigned)t;
        }
        const unsigned long long m = __ballot(on);
        if (m && (threadIdx.x & 63) == 0) atomicAdd(&w[1], (unsigned long long)__popcll(m));
    }
}

__global__ __launch_bounds__(RX_T) void rx_finish(const unsigned *__restrict__ key, const unsigned *__restrict__ val,
                                                   long nt, long long *__restrict__ idx_map,
                                                   long long *__restrict__ order) {
    for (long i = (long)blockIdx.x * RX_T + threadIdx.x; i < nt; i += (long)gridDim.x * RX_T) {
        const unsigned v = val[i];  // a permutation of [0, nt): the sort only moves what rx_keys wrote
        const bool on = key[i] != 0xFFFFFFFFu;
        order[i] = on ? (long long)v : -1;
        idx_map[v] = on ? (long long)i : -1;
    }
}

// ---- gather: 4 lanes per tile, 16 bytes of PalPixels each; lane 0 of the four moves the tile's other fields ----
__global__ __launch_bounds__(RX_T) void rx_gather(const long long *__restrict__ order, long n, GatherArgs a, long nt,
                                                   unsigned long long *err) {
    for (long e = (long)blockIdx.x * RX_T + threadIdx.x; e < n * 4; e += (long)gridDim.x * RX_T) {
        const long i = e >> 2;
        const int q = (int)(e & 3);
        const long long o = order[i];
        if (o < 0 || o >= nt) {
            atomicMin(err, (unsigned long long)i);
            continue;
        }
        if (a.palpix)
            reinterpret_cast<uint4 *>(a.palpix_out)[e] = reinterpret_cast<const uint4 *>(a.palpix)[o * 4 + q];
        if (q) continue;
        if (a.thm) a.thm_out[i] = a.thm[o];
        if (a.tvm) a.tvm_out[i] = a.tvm[o];
        if (a.dith_pal) a.dith_pal_out[i] = a.dith_pal[o];
        if (a.use_count) a.use_count_out[i] = a.use_count[o];
    }
}

// ---- remap ----
__device__ __forceinline__ int rx_map_item(int t, long i, const long long *map, unsigned nt, int keep,
                                           unsigned long long *err) {
    if ((unsigned)t >= nt) {
        atomicMin(err, (unsigned long long)i);
        return t;
    }
    const long long m = map[t];
    return m < 0 ? (keep ? t : -1) : (int)m;
}

__global__ __launch_bounds__(RX_T) void rx_remap(int *tile, long n, const long long *__restrict__ map, unsigned nt,
                                                  int keep, int vec, unsigned long long *err) {
    for (long i = ((long)blockIdx.x * RX_T + threadIdx.x) * 4; i < n; i += (long)gridDim.x * RX_T * 4) {
        if (vec && i + 4 <= n) {
            int4 v = *reinterpret_cast<int4 *>(tile + i);
            v.x = rx_map_item(v.x, i, map, nt, keep, err);
            v.y = rx_map_item(v.y, i + 1, map, nt, keep, err);
            v.z = rx_map_item(v.z, i + 2, map, nt, keep, err);
            v.w = rx_map_item(v.w, i + 3, map, nt, keep, err);
            *reinterpret_cast<int4 *>(tile + i) = v;
        } else {
            for (long j = i; j < min(i + 4, n); j++) tile[j] = rx_map_item(tile[j], j, map, nt, keep, err);
        }
    }
}

// ---- host side ----
namespace {

constexpr long RX_LIMIT = 1L << 31;

unsigned rx_grid(long n, long per_block, long cap = 4096) {
    return (unsigned)std::max<long>(1, std::min<long>(cap, (n + per_block - 1) / per_block));
}

int rx_fail(const char *who, const std::string &what) {
    set_error(std::string(who) + ": " + what);
    return -1;
}

bool misaligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// the error word of a call: -1 on a failure of the copy, else 0 with *e set (one wait)
int rx_wait_word(const unsigned long long *d_w, int words, unsigned long long *h, hipStream_t st) {
    TILER_HIP_CHECK(hipGetLastError());
    TILER_HIP_CHECK(hipMemcpyAsync(h, d_w, (size_t)words * 8, hipMemcpyDeviceToHost, st));
    TILER_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

int rx_bad_item(const char *who, const int32_t *d_tile, unsigned long long at, long nt) {
    int32_t v = 0;
    TILER_HIP_CHECK(hipMemcpy(&v, d_tile + at, 4, hipMemcpyDeviceToHost));
    return rx_fail(who, "item " + std::to_string(at) + " is tile " + std::to_string(v) + ", outside [0, " +
                            std::to_string(nt) + ")");
}

}  // namespace

int tile_use_count_dev(const int32_t *d_tile, long n_items, long nt, int64_t *d_use_count, uint8_t *d_active,
                       int accumulate, hipStream_t st) {
    const char *who = "tile_use_count";
    if (n_items < 0 || nt < 0 || n_items >= RX_LIMIT || nt >= RX_LIMIT)
        return rx_fail(who, "need 0 <= n_items < 2^31 and 0 <= nt < 2^31");
    if ((n_items > 0 && !d_tile) || (nt > 0 && !d_use_count)) return rx_fail(who, "null array");
    if (misaligned(d_tile, 4) || misaligned(d_use_count, 8))
        return rx_fail(who, "tile must be 4-byte aligned, use_count 8-byte aligned");
    if (n_items == 0 && nt == 0) return 0;
    Blocks blk(st);
    unsigned long long *err = nullptr;
    if (!blk.get(err, 8)) return rx_fail(who, "out of device memory");
    unsigned long long *uc = reinterpret_cast<unsigned long long *>(d_use_count);
    TILER_HIP_CHECK(hipMemsetAsync(err, 0xFF, 8, st));
    if (!accumulate && nt > 0) TILER_HIP_CHECK(hipMemsetAsync(uc, 0, (size_t)nt * 8, st));
    if (n_items > 0) {
        const long windows = std::max<long>(1, (nt + RX_WIN - 1) / RX_WIN);
        const int forced = g_rx_strategy.load();
        const bool lds = forced < 0 ? windows <= RX_MAX_WINDOWS : forced == 0;
        const int vec = !misaligned(d_tile, 16);
        KTimer tm("reindex_count", st);
        if (lds)
            hipLaunchKernelGGL(rx_count_lds, dim3((unsigned)((n_items + RX_CHUNK - 1) / RX_CHUNK), (unsigned)windows),
                               dim3(RX_NT), 0, st, (const int *)d_tile, n_items, (unsigned)nt, vec, uc, err);
        else
            hipLaunchKernelGGL(rx_count_global, dim3(rx_grid(n_items, RX_T * 4, 2048)), dim3(RX_T), 0, st,
                               (const int *)d_tile, n_items, (unsigned)nt, vec, uc, err);
    }
    if (d_active && nt > 0) {
        KTimer tm("reindex_active", st);
        hipLaunchKernelGGL(rx_active, dim3(rx_grid(nt, RX_T)), dim3(RX_T), 0, st, (const long long *)d_use_count, nt,
                           d_active);
    }
    unsigned long long e = RX_NO_ERROR;
    if (rx_wait_word(err, 1, &e, st)) return -1;
    return e == RX_NO_ERROR ? 0 : rx_bad_item(who, d_tile, e, nt);
}

int reindex_tiles_dev(const uint8_t *d_active, const int64_t *d_use_count, long nt, int64_t *d_idx_map,
                      int64_t *d_order, int64_t *n_active, hipStream_t st) {
    const char *who = "reindex_tiles";
    if (nt < 0 || nt >= RX_LIMIT || !n_active) return rx_fail(who, "need 0 <= nt < 2^31 and n_active");
    if (nt > 0 && (!d_active || !d_use_count || !d_idx_map || !d_order)) return rx_fail(who, "null array");
    if (misaligned(d_use_count, 8) || misaligned(d_idx_map, 8) || misaligned(d_order, 8))
        return rx_fail(who, "use_count, idx_map and order must be 8-byte aligned");
    *n_active = 0;
    if (nt == 0) return 0;
    size_t tmp_bytes = 0;
    {
        hipcub::DoubleBuffer<unsigned> k(nullptr, nullptr), v(nullptr, nullptr);
        TILER_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, k, v, (int)nt, 0, 32, st));
    }
    Blocks blk(st);
    unsigned long long *w = nullptr;
    unsigned *k0 = nullptr, *k1 = nullptr, *v0 = nullptr, *v1 = nullptr;
    void *tmp = nullptr;
    const size_t b = (size_t)nt * 4;
    if (!blk.get(w, 16) || !blk.get(k0, b) || !blk.get(k1, b) || !blk.get(v0, b) || !blk.get(v1, b) ||
        !blk.get(tmp, tmp_bytes))
        return rx_fail(who, "out of device memory");
    TILER_HIP_CHECK(hipMemsetAsync(w, 0xFF, 8, st));
    TILER_HIP_CHECK(hipMemsetAsync(w + 1, 0, 8, st));
    {
        KTimer tm("reindex_order", st);
        hipLaunchKernelGGL(rx_keys, dim3(rx_grid(nt, RX_T)), dim3(RX_T), 0, st, d_active,
                           (const long long *)d_use_count, nt, k0, v0, w);
        TILER_HIP_CHECK(hipGetLastError());
        hipcub::DoubleBuffer<unsigned> k(k0, k1), v(v0, v1);
        TILER_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, k, v, (int)nt, 0, 32, st));
        hipLaunchKernelGGL(rx_finish, dim3(rx_grid(nt, RX_T)), dim3(RX_T), 0, st, (const unsigned *)k.Current(),
                           (const unsigned *)v.Current(), nt, (long long *)d_idx_map, (long long *)d_order);
    }
    unsigned long long h[2] = {RX_NO_ERROR, 0};
    if (rx_wait_word(w, 2, h, st)) return -1;
    if (h[0] != RX_NO_ERROR) {
        int64_t c = 0;
        TILER_HIP_CHECK(hipMemcpy(&c, d_use_count + h[0], 8, hipMemcpyDeviceToHost));
        return rx_fail(who, "use_count[" + std::to_string(h[0]) + "] is " + std::to_string(c) +
                                ", outside [0, 2^31)");
    }
    *n_active = (int64_t)h[1];
    return 0;
}

int gather_tiles_dev(const int64_t *d_order, long n, const GatherArgs &a, long nt, hipStream_t st) {
    const char *who = "gather_tiles";
    if (n < 0 || nt < 0 || n >= RX_LIMIT || nt >= RX_LIMIT) return rx_fail(who, "need 0 <= n < 2^31 and 0 <= nt < 2^31");
    const void *in[5] = {a.palpix, a.thm, a.tvm, a.dith_pal, a.use_count};
    const void *out[5] = {a.palpix_out, a.thm_out, a.tvm_out, a.dith_pal_out, a.use_count_out};
    static const char *const names[5] = {"palpix", "thm", "tvm", "dith_pal", "use_count"};
    static const uintptr_t align[5] = {16, 1, 1, 4, 8};
    for (int p = 0; p < 5; p++) {
        if (!in[p] != !out[p]) return rx_fail(who, std::string(names[p]) + ": give both arrays of a pair or neither");
        if (in[p] && in[p] == out[p]) return rx_fail(who, std::string(names[p]) + ": the output must not be the input");
        if (misaligned(in[p], align[p]) || misaligned(out[p], align[p]))
            return rx_fail(who, std::string(names[p]) + " must be " + std::to_string(align[p]) + "-byte aligned");
    }
    if (n == 0) return 0;
    if (!d_order || misaligned(d_order, 8)) return rx_fail(who, "order must be an 8-byte aligned array");
    Blocks blk(st);
    unsigned long long *err = nullptr;
    if (!blk.get(err, 8)) return rx_fail(who, "out of device memory");
    TILER_HIP_CHECK(hipMemsetAsync(err, 0xFF, 8, st));
    {
        KTimer tm("reindex_gather", st);
        hipLaunchKernelGGL(rx_gather, dim3(rx_grid(n * 4, RX_T, 8192)), dim3(RX_T), 0, st,
                           (const long long *)d_order, n, a, nt, err);
    }
    unsigned long long e = RX_NO_ERROR;
    if (rx_wait_word(err, 1, &e, st)) return -1;
    if (e != RX_NO_ERROR) {
        int64_t o = 0;
        TILER_HIP_CHECK(hipMemcpy(&o, d_order + e, 8, hipMemcpyDeviceToHost));
        return rx_fail(who, "order[" + std::to_string(e) + "] is " + std::to_string(o) + ", outside [0, " +
                                std::to_string(nt) + ")");
    }
    return 0;
}

int remap_items_dev(int32_t *d_tile, long n_items, const int64_t *d_map, long nt, int keep_unmapped, hipStream_t st) {
    const char *who = "remap_items";
    if (n_items < 0 || nt < 0 || n_items >= RX_LIMIT || nt >= RX_LIMIT)
        return rx_fail(who, "need 0 <= n_items < 2^31 and 0 <= nt < 2^31");
    if (n_items == 0) return 0;
    if (!d_tile || (nt > 0 && !d_map)) return rx_fail(who, "null array");
    if (misaligned(d_tile, 4) || misaligned(d_map, 8)) return rx_fail(who, "tile must be 4-byte aligned, map 8-byte aligned");
    Blocks blk(st);
    unsigned long long *err = nullptr;
    if (!blk.get(err, 8)) return rx_fail(who, "out of device memory");
    TILER_HIP_CHECK(hipMemsetAsync(err, 0xFF, 8, st));
    {
        KTimer tm("reindex_remap", st);
        hipLaunchKernelGGL(rx_remap, dim3(rx_grid(n_items, RX_T * 4, 8192)), dim3(RX_T), 0, st, d_tile, n_items,
                           (const long long *)d_map, (unsigned)nt, keep_unmapped != 0, (int)!misaligned(d_tile, 16),
                           err);
    }
    unsigned long long e = RX_NO_ERROR;
    if (rx_wait_word(err, 1, &e, st)) return -1;
    return e == RX_NO_ERROR ? 0 : rx_bad_item(who, d_tile, e, nt);
}

// ---- host arrays ----
int tile_use_count_host(const int32_t *tile, long n_items, long nt, int64_t *use_count, uint8_t *active,
                        int accumulate) {
    if (n_items < 0 || nt < 0 || (n_items > 0 && !tile) || (nt > 0 && !use_count))
        return rx_fail("tile_use_count", "invalid arguments");
    HostStage s("tile_use_count");
    const int32_t *d_tile = s.in(tile, (size_t)n_items);
    int64_t *d_uc = accumulate ? s.inout(use_count, (size_t)nt) : s.out(use_count, (size_t)nt);
    uint8_t *d_act = s.out(active, (size_t)nt);
    if (!s.ok() || tile_use_count_dev(d_tile, n_items, nt, d_uc, d_act, accumulate, s.stream())) return -1;
    return s.finish();
}

int reindex_tiles_host(const uint8_t *active, const int64_t *use_count, long nt, int64_t *idx_map, int64_t *order,
                       int64_t *n_active) {
    if (nt < 0 || !n_active || (nt > 0 && (!active || !use_count || !idx_map || !order)))
        return rx_fail("reindex_tiles", "invalid arguments");
    HostStage s("reindex_tiles");
    const uint8_t *d_act = s.in(active, (size_t)nt);
    const int64_t *d_uc = s.in(use_count, (size_t)nt);
    int64_t *d_map = s.out(idx_map, (size_t)nt), *d_ord = s.out(order, (size_t)nt);
    if (!s.ok() || reindex_tiles_dev(d_act, d_uc, nt, d_map, d_ord, n_active, s.stream())) return -1;
    return s.finish();
}

int gather_tiles_host(const int64_t *order, long n, const GatherArgs &a, long nt) {
    if (n < 0 || nt < 0 || (n > 0 && !order)) return rx_fail("gather_tiles", "invalid arguments");
    HostStage s("gather_tiles");
    const size_t t = (size_t)nt, m = (size_t)n;
    GatherArgs d{};
    const int64_t *d_order = s.in(order, m);
    d.palpix = s.in(a.palpix, t * 64);
    d.thm = s.in(a.thm, t);
    d.tvm = s.in(a.tvm, t);
    d.dith_pal = s.in(a.dith_pal, t);
    d.use_count = s.in(a.use_count, t);
    d.palpix_out = s.out(a.palpix_out, m * 64);
    d.thm_out = s.out(a.thm_out, m);
    d.tvm_out = s.out(a.tvm_out, m);
    d.dith_pal_out = s.out(a.dith_pal_out, m);
    d.use_count_out = s.out(a.use_count_out, m);
    const void *in[5] = {a.palpix, a.thm, a.tvm, a.dith_pal, a.use_count};
    const void *out[5] = {a.palpix_out, a.thm_out, a.tvm_out, a.dith_pal_out, a.use_count_out};
    for (int p = 0; p < 5; p++)  // the staged copies are always distinct blocks
        if (in[p] && in[p] == out[p]) return rx_fail("gather_tiles", "the output must not be the input");
    if (!s.ok() || gather_tiles_dev(d_order, n, d, nt, s.stream())) return -1;
    return s.finish();
}

int remap_items_host(int32_t *tile, long n_items, const int64_t *map, long nt, int keep_unmapped) {
    if (n_items < 0 || nt < 0 || (n_items > 0 && !tile) || (n_items > 0 && nt > 0 && !map))
        return rx_fail("remap_items", "invalid arguments");
    HostStage s("remap_items");
    int32_t *d_tile = s.inout(tile, (size_t)n_items);
    const int64_t *d_map = s.in(map, (size_t)nt);
    if (!s.ok() || remap_items_dev(d_tile, n_items, d_map, nt, keep_unmapped, s.stream())) return -1;
    return s.finish();
}

int reindex_debug(int strategy) {
    if (strategy < -1 || strategy > 1) return rx_fail("tiler_debug_reindex", "strategy in -1..1");
    g_rx_strategy = strategy;
    return 0;
}

}  // namespace tiler
