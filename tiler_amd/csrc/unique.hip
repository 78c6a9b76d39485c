// unique.hip -- MakeTilesUnique (main.pas:2555-2612), the exact duplicate-tile merge of the chain, on gfx950.
//
// The reference sorts the Active tiles by CompareTilePalPixels (16 little-endian dwords, dword 0 first; equal keys by
// index, the project's canonical order) and merges every run of identical tiles into the run's first member
// (MergeTiles main.pas:3688-3712).  Its final DoOneMerge runs with i = Count - 1 (main.pas:2604-2605), so the last
// run of the sorted list never includes its last member.  No sort is needed for that result; it has a closed form:
//   x   = the Active tile with the greatest (key, index), i.e. the last entry of the sorted list;
//   G   = a group of Active tiles with identical PalPixels, G' = G \ {x};
//   |G'| >= 2: every member of G' but min(G') merges into min(G').  Nothing else changes.
// x is the greatest index of its group, so min(G') = min(G) whenever something merges: "tile i merges into min(G)
// unless i = min(G) or i = x" is the whole rule.  Segments (btnDoMakeUniqueClick's chunks main.pas:916-938, each a
// MakeTilesUnique of its own) only add the segment to the group's identity and one x per segment.
//   unique_insert  group-by through an open-addressing table of int32 slots (-1 = empty): tile i probes linearly from
//                  its hash, claims an empty slot (atomicCAS) or, where the occupant is a tile of its segment with the
//                  same 64 bytes, lowers the slot to min(occupant, i) (atomicMin).  A slot never changes group and is
//                  never emptied, so a group owns exactly one slot, the first free one of its probe path, whatever the
//                  order of arrival; after the launch it holds min(G).  Only atomics' return values are trusted here.
//   unique_last    x of every segment: workgroups reduce spans of tiles to their greatest (key, index), one workgroup
//                  per segment reduces the spans' winners.
//   unique_merge   every Active tile finds its group's slot again (plain loads: another launch wrote them) and merges
//                  by the rule above.  Sources and survivors are disjoint, the UseCount sums are 64-bit integer atomics:
//                  the result does not depend on the order in which threads run.
//   unique_zero    PalPixels of the merged tiles zeroed, after every compare of unique_merge.
// PalPixels are read-only in the first three launches.  Scratch (table, segment tables, span winners) is owned per
// device and reused across calls.
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "stage.hpp"
#include "unique.hpp"

namespace tiler {

static constexpr int UQ_NT = 256;
static constexpr long UQ_SPAN = 2048;  // tiles per workgroup of the first unique_last launch
static constexpr int UQ_MAX_DEV = 64;

static std::atomic<int> g_uq_bits{-1};  // tiler_debug_unique

__device__ __forceinline__ void uq_load(const uint8_t *pix, long i, uint32_t (&w)[16]) {
    const uint4 *s = reinterpret_cast<const uint4 *>(pix + i * 64);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint4 v = s[q];
        w[4 * q] = v.x;
        w[4 * q + 1] = v.y;
        w[4 * q + 2] = v.z;
        w[4 * q + 3] = v.w;
    }
}

// -1 / 0 / 1: CompareTilePalPixels (the first differing dword decides)
__device__ __forceinline__ int uq_cmp(const uint32_t (&a)[16], const uint32_t (&b)[16]) {
    int c = 0;
#pragma unroll
    for (int d = 15; d >= 0; d--)
        if (a[d] != b[d]) c = a[d] > b[d] ? 1 : -1;
    return c;
}

__device__ __forceinline__ bool uq_same(const uint8_t *pix, long j, const uint32_t (&w)[16]) {
    uint32_t o[16];
    uq_load(pix, j, o);
    uint32_t d = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) d |= o[k] ^ w[k];
    return d == 0;
}

__device__ __forceinline__ unsigned long long uq_mix(unsigned long long x) {  // splitmix64's finaliser
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// all 16 dwords and the segment
__device__ __forceinline__ unsigned uq_hash(const uint32_t (&w)[16], int seg) {
    unsigned long long h = uq_mix((unsigned long long)(unsigned)seg + 0x9E3779B97F4A7C15ull);
#pragma unroll
    for (int d = 0; d < 16; d += 2) h = uq_mix(h ^ (((unsigned long long)w[d + 1] << 32) | w[d]));
    return (unsigned)(h ^ (h >> 32));
}

// the s of [0, n) with off[s] <= i < off[s + 1]; off ascends from off[0] <= i to off[n] > i (empty ranges own nothing)
template <class T>
__device__ __forceinline__ int uq_range_of(const T *off, int n, long i) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long)off[mid] <= i)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(UQ_NT) void uq_insert(const uint8_t *__restrict__ pix, const uint8_t *__restrict__ active,
                                                    long nt, const long long *__restrict__ off, int nseg,
                                                    unsigned hmask, int *tab, unsigned tmask,
                                                    long long *__restrict__ merge_index) {
    for (long i = (long)blockIdx.x * UQ_NT + threadIdx.x; i < nt; i += (long)gridDim.x * UQ_NT) {
        merge_index[i] = -1;
        if (!active[i]) continue;
        uint32_t w[16];
        uq_load(pix, i, w);
        const int s = uq_range_of(off, nseg, i);
        const long lo = off[s], hi = off[s + 1];
        unsigned p = uq_hash(w, s) & hmask & tmask;
        // at most nt tiles in >= 2 nt slots: an empty slot or the group's own is always met
        for (unsigned n = 0; n <= tmask; n++) {
            const int j = atomicCAS(&tab[p], -1, (int)i);
            if (j == -1) break;
            if (j >= lo && j < hi && uq_same(pix, j, w)) {
                atomicMin(&tab[p], (int)i);
                break;
            }
            p = (p + 1) & tmask;
        }
    }
}

// the later of two tiles in (key, index) order; -1 = none
__device__ __forceinline__ int uq_later(const uint8_t *pix, int a, int b) {
    if (a < 0) return b;
    if (b < 0 || a == b) return a;
    uint32_t wa[16], wb[16];
    uq_load(pix, a, wa);
    uq_load(pix, b, wb);
    const int c = uq_cmp(wa, wb);
    return c > 0 || (c == 0 && a > b) ? a : b;
}

__device__ __forceinline__ int uq_block_later(const uint8_t *pix, int best, int *cand) {
    cand[threadIdx.x] = best;
    __syncthreads();
    for (int o = UQ_NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) cand[threadIdx.x] = uq_later(pix, cand[threadIdx.x], cand[threadIdx.x + o]);
        __syncthreads();
    }
    return cand[0];
}

// workgroup b = span (b - poff[s]) of segment s: part[b] = its Active tile with the greatest (key, index), -1 = none
__global__ __launch_bounds__(UQ_NT) void uq_last_spans(const uint8_t *__restrict__ pix,
                                                        const uint8_t *__restrict__ active,
                                                        const long long *__restrict__ off,
                                                        const int *__restrict__ poff, int nseg, int *__restrict__ part) {
    __shared__ int cand[UQ_NT];
    const int b = blockIdx.x;
    const int s = uq_range_of(poff, nseg, b);
    const long i0 = off[s] + (long)(b - poff[s]) * UQ_SPAN, i1 = min((long)off[s + 1], i0 + UQ_SPAN);
    uint32_t bw[16] = {};
    int best = -1;
    for (long i = i0 + threadIdx.x; i < i1; i += UQ_NT) {  // ascending: an equal key at a higher index wins
        if (!active[i]) continue;
        uint32_t w[16];
        uq_load(pix, i, w);
        if (best < 0 || uq_cmp(w, bw) >= 0) {
            best = (int)i;
#pragma unroll
            for (int d = 0; d < 16; d++) bw[d] = w[d];
        }
    }
    best = uq_block_later(pix, best, cand);
    if (threadIdx.x == 0) part[b] = best;
}

// workgroup s: last[s] = x of segment s over its spans' winners, -1 = no Active tile
__global__ __launch_bounds__(UQ_NT) void uq_last_final(const uint8_t *__restrict__ pix, const int *__restrict__ part,
                                                        const int *__restrict__ poff, int *__restrict__ last) {
    __shared__ int cand[UQ_NT];
    const int s = blockIdx.x;
    int best = -1;
    for (int k = poff[s] + threadIdx.x; k < poff[s + 1]; k += UQ_NT) best = uq_later(pix, best, part[k]);
    best = uq_block_later(pix, best, cand);
    if (threadIdx.x == 0) last[s] = best;
}

__global__ __launch_bounds__(UQ_NT) void uq_merge(const uint8_t *__restrict__ pix, uint8_t *active, long nt,
                                                   const long long *__restrict__ off, int nseg, unsigned hmask,
                                                   const int *__restrict__ tab, unsigned tmask,
                                                   const int *__restrict__ last, long long *use_count,
                                                   long long *merge_index) {
    for (long i = (long)blockIdx.x * UQ_NT + threadIdx.x; i < nt; i += (long)gridDim.x * UQ_NT) {
        if (!active[i]) continue;
        uint32_t w[16];
        uq_load(pix, i, w);
        const int s = uq_range_of(off, nseg, i);
        const long lo = off[s], hi = off[s + 1];
        unsigned p = uq_hash(w, s) & hmask & tmask;
        int rep = -1;
        for (unsigned n = 0; n <= tmask; n++) {
            const int j = tab[p];
            if (j < 0) break;  // (not met: uq_insert gave this tile's group a slot on this path)
            if (j == i || (j >= lo && j < hi && uq_same(pix, j, w))) {
                rep = j;
                break;
            }
            p = (p + 1) & tmask;
        }
        if (rep < 0 || rep == i || i == last[s]) continue;
        // rep = min(G) is no source and tile i no survivor: use_count[i] is not written in this launch
        merge_index[i] = rep;
        atomicAdd(reinterpret_cast<unsigned long long *>(use_count + rep), (unsigned long long)use_count[i]);
        active[i] = 0;
    }
}

// 4 lanes per tile, 16 bytes each
__global__ __launch_bounds__(UQ_NT) void uq_zero(uint8_t *pix, const long long *__restrict__ merge_index, long nt) {
    for (long e = (long)blockIdx.x * UQ_NT + threadIdx.x; e < nt * 4; e += (long)gridDim.x * UQ_NT)
        if (merge_index[e >> 2] >= 0) reinterpret_cast<uint4 *>(pix)[e] = make_uint4(0, 0, 0, 0);
}

// ---- host side ----
namespace {

unsigned grid_for(long n, long cap = 8192) { return (unsigned)std::max<long>(1, std::min<long>(cap, (n + UQ_NT - 1) / UQ_NT)); }

struct UqScratch {  // of one device; a call holds mu from its first launch to its last wait
    std::mutex mu;
    int *tab = nullptr;  // [cap_tab] slots
    size_t cap_tab = 0;
    long long *off = nullptr;  // [cap_seg + 1] first tile of a segment
    int *poff = nullptr;       // [cap_seg + 1] first span of a segment
    int *last = nullptr;       // [cap_seg] x of a segment
    size_t cap_seg = 0;
    int *part = nullptr;  // [cap_part] winner of a span
    size_t cap_part = 0;
};
UqScratch g_uq[UQ_MAX_DEV];

struct Drain {  // the stream is idle before host buffers and the scratch lock go
    hipStream_t st;
    ~Drain() { (void)hipStreamSynchronize(st); }
};

}  // namespace

int make_tiles_unique_dev(uint8_t *d_palpix, uint8_t *d_active, int64_t *d_use_count, int64_t *d_merge_index, long nt,
                          const int64_t *seg_off, int nseg, hipStream_t st) {
    if (nt < 0 || nt >= (1L << 30) || nseg < 1 || !seg_off ||
        (nt > 0 && (!d_palpix || !d_active || !d_use_count || !d_merge_index))) {
        set_error("make_tiles_unique: invalid arguments (need 0 <= nt < 2^30, nseg >= 1, seg_off [nseg + 1])");
        return -1;
    }
    if (seg_off[0] != 0 || seg_off[nseg] != nt) {
        set_error("make_tiles_unique: seg_off must run from 0 to nt");
        return -1;
    }
    for (int s = 0; s < nseg; s++)
        if (seg_off[s + 1] < seg_off[s]) {
            set_error("make_tiles_unique: seg_off must not decrease");
            return -1;
        }
    if (((uintptr_t)d_palpix & 15) != 0 || (((uintptr_t)d_use_count | (uintptr_t)d_merge_index) & 7) != 0) {
        set_error("make_tiles_unique: palpix must be 16-byte aligned, use_count and merge_index 8-byte aligned");
        return -1;
    }
    if (nt == 0) return 0;
    int dev = 0;
    TILER_HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= UQ_MAX_DEV) {
        set_error("make_tiles_unique: device out of range");
        return -1;
    }
    // spans of the last-member reduction: segment s owns spans [poff[s], poff[s + 1])
    std::vector<long long> h_off(seg_off, seg_off + nseg + 1);
    std::vector<int> h_poff(nseg + 1);
    long spans = 0;
    for (int s = 0; s < nseg; s++) {
        h_poff[s] = (int)spans;
        spans += (seg_off[s + 1] - seg_off[s] + UQ_SPAN - 1) / UQ_SPAN;
    }
    h_poff[nseg] = (int)spans;  // <= nt / UQ_SPAN + nseg
    size_t slots = 2;
    while (slots < 2 * (size_t)nt) slots <<= 1;  // a power of two >= 2 nt >= twice the Active tiles
    const unsigned tmask = (unsigned)(slots - 1);
    const int bits = g_uq_bits.load();
    const unsigned hmask = bits < 0 || bits >= 32 ? ~0u : (1u << bits) - 1u;

    UqScratch &S = g_uq[dev];
    std::lock_guard<std::mutex> lk(S.mu);
    Drain drain{st};
    if (slots > S.cap_tab) {
        S.cap_tab = 0;
        TILER_HIP_CHECK(dregrow({{S.tab, slots * sizeof(int)}}));
        S.cap_tab = slots;
    }
    if ((size_t)nseg > S.cap_seg) {
        S.cap_seg = 0;
        TILER_HIP_CHECK(dregrow({{S.off, ((size_t)nseg + 1) * sizeof(long long)},
                                 {S.poff, ((size_t)nseg + 1) * sizeof(int)},
                                 {S.last, (size_t)nseg * sizeof(int)}}));
        S.cap_seg = (size_t)nseg;
    }
    if ((size_t)spans > S.cap_part) {
        S.cap_part = 0;
        TILER_HIP_CHECK(dregrow({{S.part, (size_t)spans * sizeof(int)}}));
        S.cap_part = (size_t)spans;
    }
    TILER_HIP_CHECK(hipMemcpyAsync(S.off, h_off.data(), ((size_t)nseg + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    TILER_HIP_CHECK(hipMemcpyAsync(S.poff, h_poff.data(), ((size_t)nseg + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    long long *use_count = reinterpret_cast<long long *>(d_use_count);
    long long *merge_index = reinterpret_cast<long long *>(d_merge_index);
    {
        KTimer tm("unique_insert", st);
        TILER_HIP_CHECK(hipMemsetAsync(S.tab, 0xFF, slots * sizeof(int), st));
        hipLaunchKernelGGL(uq_insert, dim3(grid_for(nt)), dim3(UQ_NT), 0, st, (const uint8_t *)d_palpix,
                           (const uint8_t *)d_active, nt, (const long long *)S.off, nseg, hmask, S.tab, tmask,
                           merge_index);
    }
    {
        KTimer tm("unique_last", st);
        hipLaunchKernelGGL(uq_last_spans, dim3((unsigned)spans), dim3(UQ_NT), 0, st, (const uint8_t *)d_palpix,
                           (const uint8_t *)d_active, (const long long *)S.off, (const int *)S.poff, nseg, S.part);
        hipLaunchKernelGGL(uq_last_final, dim3((unsigned)nseg), dim3(UQ_NT), 0, st, (const uint8_t *)d_palpix,
                           (const int *)S.part, (const int *)S.poff, S.last);
    }
    {
        KTimer tm("unique_merge", st);
        hipLaunchKernelGGL(uq_merge, dim3(grid_for(nt)), dim3(UQ_NT), 0, st, (const uint8_t *)d_palpix, d_active, nt,
                           (const long long *)S.off, nseg, hmask, (const int *)S.tab, tmask, (const int *)S.last,
                           use_count, merge_index);
    }
    {
        KTimer tm("unique_zero", st);
        hipLaunchKernelGGL(uq_zero, dim3(grid_for(nt * 4)), dim3(UQ_NT), 0, st, d_palpix,
                           (const long long *)merge_index, nt);
    }
    TILER_HIP_CHECK(hipGetLastError());
    TILER_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

int make_tiles_unique_host(uint8_t *palpix, uint8_t *active, int64_t *use_count, int64_t *merge_index, long nt,
                           const int64_t *seg_off, int nseg) {
    if (nt < 0 || (nt > 0 && (!palpix || !active || !use_count || !merge_index))) {
        set_error("make_tiles_unique: invalid arguments");
        return -1;
    }
    HostStage s("make_tiles_unique");
    const size_t t = (size_t)nt;
    uint8_t *d_pix = s.inout(palpix, t * 64), *d_act = s.inout(active, t);
    int64_t *d_uc = s.inout(use_count, t), *d_mi = s.out(merge_index, t);
    if (!s.ok() || make_tiles_unique_dev(d_pix, d_act, d_uc, d_mi, nt, seg_off, nseg, s.stream())) return -1;
    return s.finish();
}

int unique_debug(int hash_bits) {
    if (hash_bits < -1 || hash_bits > 32) {
        set_error("tiler_debug_unique: hash_bits in -1..32");
        return -1;
    }
    g_uq_bits = hash_bits;
    return 0;
}

}  // namespace tiler
