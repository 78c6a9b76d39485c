// palette_var.hip -- QuantizePalette's value-at-risk path on the GPU: DoValueAtRiskBased
// (main.pas:2256-2394, taken when chkUseDL3 is unticked, main.pas:888, 2406-2409) for every (keyframe, palette) pair
// in one pass, then the CompareCMULHS order of the picked items (main.pas:2413-2417) on the host.
//
// GPU layout, all pairs at once:
//   1. every pixel of every tile -> one 64-bit key (pair << 24 | 24-bit colour; tiles that are skipped go to the
//      sentinel pair P); a radix sort + run-length encode gives (pair, colour, Count) in colour order per pair
//      (TrueColorUsage, main.pas:2270-2299, without the 2^24 - U zero entries the reference sorts to the end and
//      drops).  The keys are 64 bits wide at any P: (P + 1) << 24 passes 2^32 from 255 pairs on.
//   2. the items (TCountIndexArray: Count, Index, Luma and the RGBToHSV bytes) and their order, CompareCMUCntHLS
//      (main.pas:2070-2079) within each pair: two stable radix sorts, by (Hue, Val, Sat), then by (pair, Count
//      descending).  The comparator is no total order and the reference's QuickSort is unstable, so its order among
//      equal (Count, Hue, Val, Sat) is implementation-defined; here it is colour ascending (the sorts are stable and
//      step 1 leaves a pair's colours ascending), the policy of SURVEY.md 8(f)-1.
//   3. one 1024-thread workgroup per pair: the cut-off CmlPct from a prefix sum of the counts against the caller's
//      acc0, then the prune loop (main.pas:2348-2388).  The list stays in place in HBM: a deleted item is unlinked
//      (previous / next live links) and marked, never moved.  ColorCompare of every item with its live predecessor is
//      cached, and a 64-ary tree of minima of (difference << 32 | list index) over it gives the reference's first
//      minimum (strict `<`, ascending scan) at its root.  A merge rewrites three leaves (the deleted item's, the
//      merged item's and its successor's) and the at most three nodes above them per level, so a round costs
//      O(log64 U) whatever U is; the rounds run on the workgroup's first wave.
//   4. the pick (main.pas:2391-2393): round(gPalettePattern[PalIdx, i] * (Count - 1)) in fp64 on the device (the
//      table itself is built on the host), and a ranked walk over the live items by the whole workgroup.
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "palette.hpp"
#include "palette_cm.hpp"
#include "stage.hpp"

namespace tiler {

namespace {

constexpr int VAR_T = 1024;        // prune workgroup
constexpr int VAR_W = VAR_T / 64;  // its waves
constexpr int VAR_MAXPAL = 256;    // palsize the pick holds in LDS
constexpr int VAR_LEVELS = 8;      // 64^6 > 2^31: at most 6 tree levels
constexpr uint32_t VAR_NONE = 0xffffffffu;         // no difference (the first item, a deleted one); High(Int64)
constexpr unsigned long long VAR_NOKEY = ~0ull;    // a node over no difference
constexpr int VAR_DEAD = -2;                       // prev[] of a deleted item

struct VarItem {  // TCountIndexArray (main.pas:193-196)
    int32_t count, index, luma;
    uint32_t hsv;  // hue | sat << 8 | val << 16
};

// ---------------------------------------------------------------------------------------------------------------
// 1. usage: one key per pixel; tiles per pair (PaletteUseCount)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void var_keys_kernel(const int32_t *__restrict__ rgb, const int32_t *__restrict__ pal_of,
                                                       const uint8_t *__restrict__ active, long n_tiles, int P,
                                                       uint64_t *__restrict__ keys, int *__restrict__ use_count) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_tiles * 64) return;
    const long tile = i >> 6;
    const int p = pal_of[tile];
    const bool ok = (!active || active[tile]) && p >= 0 && p < P;
    keys[i] = ok ? ((uint64_t)p << 24) | ((uint32_t)rgb[i] & 0xffffffu) : (uint64_t)P << 24;
    if (ok && (i & 63) == 0) atomicAdd(use_count + p, 1);
}

// seg[p] = first entry of pair p (lower bound of p << 24 in the sorted unique keys), seg[P] = used entries
__global__ void var_seg_kernel(const uint64_t *__restrict__ ukeys, const int *__restrict__ nruns, int P,
                               int *__restrict__ seg) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > P) return;
    const uint64_t key = (uint64_t)p << 24;
    int lo = 0, hi = *nruns;
    while (lo < hi) {
        const int mid = (int)(((long)lo + hi) >> 1);
        if (ukeys[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    seg[p] = lo;
}

// ---------------------------------------------------------------------------------------------------------------
// 2. items and their order
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void var_items_kernel(const uint64_t *__restrict__ ukeys, const int *__restrict__ cnt,
                                                        int total, VarItem *__restrict__ items,
                                                        uint32_t *__restrict__ key_hvs, uint32_t *__restrict__ val) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const CmItem c = cm_item((int32_t)(ukeys[e] & 0xffffffu));
    items[e] = VarItem{cnt[e], c.index, c.luma, (uint32_t)c.hue | ((uint32_t)c.sat << 8) | ((uint32_t)c.val << 16)};
    key_hvs[e] = ((uint32_t)c.hue << 16) | ((uint32_t)c.val << 8) | c.sat;  // Hue, Val, Sat ascending
    val[e] = (uint32_t)e;
}

// the second sort's key of the entries in (Hue, Val, Sat) order: pair, then Count descending
__global__ __launch_bounds__(256) void var_key2_kernel(const uint64_t *__restrict__ ukeys, const int *__restrict__ cnt,
                                                       const uint32_t *__restrict__ val, int total,
                                                       uint64_t *__restrict__ key2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const uint32_t e = val[i];
    key2[i] = ((ukeys[e] >> 24) << 31) | (uint64_t)(0x7fffffff - cnt[e]);
}

// the sorted list: items, counts (for the cut-off's prefix sum), links and the cached ColorCompare of every item
// with its predecessor (links are indices inside the pair)
__global__ __launch_bounds__(256) void var_order_kernel(const VarItem *__restrict__ items, const uint64_t *__restrict__ key2,
                                                        const uint32_t *__restrict__ val, const int *__restrict__ seg,
                                                        int total, VarItem *__restrict__ sorted,
                                                        uint32_t *__restrict__ counts, int *__restrict__ prev,
                                                        int *__restrict__ next, uint32_t *__restrict__ diff) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const VarItem it = items[val[i]];
    const int p = (int)(key2[i] >> 31);
    const int s = seg[p], n = seg[p + 1] - s, k = i - s;
    sorted[i] = it;
    counts[i] = (uint32_t)it.count;
    prev[i] = k - 1;
    next[i] = k + 1 < n ? k + 1 : -1;
    diff[i] = k == 0 ? VAR_NONE : cm_color_compare(it.index, items[val[i - 1]].index);
}

// ---------------------------------------------------------------------------------------------------------------
// 3. + 4. cut-off, prune, pick: one workgroup per pair
// ---------------------------------------------------------------------------------------------------------------
struct VarArgs {
    const int *seg;
    VarItem *it;             // [total] the sorted lists
    uint32_t *diff;          // [total]
    int *prev, *next;        // [total]
    const uint32_t *prefix;  // [total] inclusive sums of the counts
    unsigned long long *tree;  // pair p's levels from (seg[p] >> 5) + 8 p on
    const int32_t *acc0;     // [P]
    const double *pattern;   // [n_palettes][palsize] gPalettePattern
    int palsize, n_palettes;
    VarItem *picked;         // [P][palsize]
    int32_t *stats;          // [P][4]
};

struct VarTree {
    int n[VAR_LEVELS];    // n[0] = U, n[l] = nodes of level l
    int off[VAR_LEVELS];  // level l's first node in the pair's region
    int L;                // the root's level
};

__device__ __forceinline__ unsigned long long var_wave_min(unsigned long long k) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long k2 = __shfl_xor(k, o);
        k = k2 < k ? k2 : k;
    }
    return k;
}

// this lane's child of node k of level l: a leaf's (difference, index) or a node of the level below
__device__ __forceinline__ unsigned long long var_child(const uint32_t *diff, const unsigned long long *tr,
                                                        const VarTree &t, int l, int k, int lane) {
    const int c = (k << 6) + lane;
    if (c >= t.n[l - 1]) return VAR_NOKEY;
    if (l == 1) {
        const uint32_t d = diff[c];
        return d == VAR_NONE ? VAR_NOKEY : ((unsigned long long)d << 32) | (uint32_t)c;
    }
    return tr[t.off[l - 1] + c];
}

__device__ __forceinline__ void var_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

__global__ __launch_bounds__(VAR_T) void var_prune_kernel(VarArgs a) {
    __shared__ VarTree t;
    __shared__ int sh_cml, sh_count, sh_bad;
    __shared__ int sh_t[VAR_MAXPAL];
    __shared__ int sh_w[VAR_W];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int s = a.seg[p], U = a.seg[p + 1] - s;
    if (U <= 0) return;  // the host has refused the call
    VarItem *it = a.it + s;
    uint32_t *diff = a.diff + s;
    int *prev = a.prev + s, *next = a.next + s;
    const long tb = ((long)s >> 5) + 8L * p;
    unsigned long long *tr = a.tree + tb;
    if (tid == 0) {
        // CmlPct (main.pas:2324-2340): the first i at which acc0 minus the counts so far is <= 0, else 0
        const uint32_t base = s > 0 ? a.prefix[s - 1] : 0u;
        const long a0 = a.acc0[p];
        int cml = 0;
        if ((long)(a.prefix[s + U - 1] - base) >= a0) {
            int lo = 0, hi = U - 1;
            while (lo < hi) {
                const int mid = (int)(((long)lo + hi) >> 1);
                if ((long)(a.prefix[s + mid] - base) >= a0)
                    hi = mid;
                else
                    lo = mid + 1;
            }
            cml = lo;
        }
        const long enough = std::min<long>(U, (long)a.palsize * a.n_palettes);  // "ensure enough colors"
        sh_cml = (int)std::max<long>(cml, enough);
        // the tree's levels
        t.n[0] = U;
        int l = 0, off = 0;
        do {
            l++;
            t.n[l] = (t.n[l - 1] + 63) >> 6;
            t.off[l] = off;
            off += t.n[l];
        } while (t.n[l] > 1);
        t.L = l;
        t.off[0] = 0;
        const long avail = (((long)s + U) >> 5) + 8L * (p + 1) - tb;
        sh_bad = off > avail;
        if (sh_bad) a.stats[p * 4 + 3] = -1;
    }
    __syncthreads();
    if (sh_bad) return;
    const int L = t.L;
    for (int l = 1; l <= L; l++) {
        for (int k = w; k < t.n[l]; k += VAR_W) {
            const unsigned long long key = var_wave_min(var_child(diff, tr, t, l, k, lane));
            if (lane == 0) tr[t.off[l] + k] = key;
        }
        __syncthreads();
    }
    if (w == 0) {  // the rounds, in order (main.pas:2348-2388)
        const int cml = sh_cml;
        int count = U, merges = 0, reason;
        uint32_t prev_best = VAR_NONE;
        for (;;) {
            const unsigned long long root = tr[t.off[L]];
            const uint32_t best = (uint32_t)(root >> 32);
            if (root != VAR_NOKEY) {
                const int i = (int)(uint32_t)root;  // bestI: absorbs its predecessor j
                int j = 0, nx = -1;
                if (lane == 0) {
                    j = prev[i];
                    VarItem x = it[i];
                    const VarItem y = it[j];
                    const int pj = prev[j];
                    nx = next[i];
                    const long cx = x.count, cy = y.count, acc = cx + cy;  // 64-bit products (a Win64 reference)
                    const long hue = ((long)(x.hsv & 255u) * cx + (long)(y.hsv & 255u) * cy) / acc;
                    const long sat = ((long)((x.hsv >> 8) & 255u) * cx + (long)((y.hsv >> 8) & 255u) * cy) / acc;
                    const long val = ((long)((x.hsv >> 16) & 255u) * cx + (long)((y.hsv >> 16) & 255u) * cy) / acc;
                    x.luma = (int32_t)(((long)x.luma * cx + (long)y.luma * cy) / acc);
                    x.count = (int32_t)acc;
                    x.hsv = (uint32_t)hue | ((uint32_t)sat << 8) | ((uint32_t)val << 16);
                    x.index = cm_hsv_to_rgb((int)hue, (int)sat, (int)val);
                    it[i] = x;
                    prev[j] = VAR_DEAD;
                    prev[i] = pj;
                    if (pj >= 0) next[pj] = i;
                    diff[j] = VAR_NONE;
                    diff[i] = pj >= 0 ? cm_color_compare(x.index, it[pj].index) : VAR_NONE;
                    if (nx >= 0) diff[nx] = cm_color_compare(it[nx].index, x.index);
                }
                j = __shfl(j, 0);
                nx = __shfl(nx, 0);
                if (nx < 0) nx = i;
                var_fence();
                for (int l = 1; l <= L; l++) {  // the nodes over the three leaves, level by level
                    const int sh = 6 * l;
                    const int k0 = j >> sh, k1 = i >> sh, k2 = nx >> sh;
                    const unsigned long long c0 = var_child(diff, tr, t, l, k0, lane);
                    const unsigned long long c1 = var_child(diff, tr, t, l, k1, lane);
                    const unsigned long long c2 = var_child(diff, tr, t, l, k2, lane);
                    const unsigned long long m0 = var_wave_min(c0), m1 = var_wave_min(c1), m2 = var_wave_min(c2);
                    if (lane == 0) {
                        tr[t.off[l] + k0] = m0;
                        tr[t.off[l] + k1] = m1;
                        tr[t.off[l] + k2] = m2;
                    }
                    var_fence();
                }
                count--;
                merges++;
            }
            if (count <= cml) {
                reason = 0;
                break;
            }
            if (best == prev_best) {
                reason = 1;
                break;
            }
            prev_best = best;
        }
        if (lane == 0) {
            sh_count = count;
            a.stats[p * 4 + 0] = U;
            a.stats[p * 4 + 1] = cml;
            a.stats[p * 4 + 2] = merges;
            a.stats[p * 4 + 3] = reason;
        }
    }
    __syncthreads();
    // the pick: item round(pattern * (Count - 1)) of the live list for each of the palsize entries
    const int count = sh_count;
    if (tid < a.palsize) {
        const double x = a.pattern[(long)(p % a.n_palettes) * a.palsize + tid] * (double)(count - 1);
        const int r = (int)__builtin_rint(x);  // to nearest even, as FPC's Round
        sh_t[tid] = std::min(std::max(r, 0), count - 1);
    }
    const long chunk = ((long)U + VAR_T - 1) / VAR_T;
    const int lo = (int)std::min<long>(U, tid * chunk), hi = (int)std::min<long>(U, (tid + 1) * chunk);
    int live = 0;
    for (int i = lo; i < hi; i++) live += prev[i] != VAR_DEAD;
    int incl = live;  // block-wide exclusive scan of the live counts
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(incl, o);
        if (lane >= o) incl += x;
    }
    if (lane == 63) sh_w[w] = incl;
    __syncthreads();
    int rank = incl - live;
    for (int k = 0; k < w; k++) rank += sh_w[k];
    bool has = false;
    for (int q = 0; q < a.palsize; q++) has |= sh_t[q] >= rank && sh_t[q] < rank + live;
    if (!has) return;
    for (int i = lo; i < hi; i++) {
        if (prev[i] == VAR_DEAD) continue;
        for (int q = 0; q < a.palsize; q++)
            if (sh_t[q] == rank) a.picked[(long)p * a.palsize + q] = it[i];
        rank++;
    }
}

// gPalettePattern (InitLuts, main.pas:627-641) in fp64; power(i + 2, 2.0) is the exact square
std::vector<double> var_pattern(int n_palettes, int palsize) {
    std::vector<double> pat((size_t)n_palettes * palsize);
    double f = 0.0;
    for (int i = 0; i < palsize; i++) {
        const double fp = f;
        f = (double)(i + 2) * (double)(i + 2);
        for (int j = 0; j < n_palettes; j++)
            pat[(size_t)j * palsize + i] = ((j + 1) / (double)n_palettes) * std::max((double)n_palettes, f - fp) + fp;
    }
    for (int j = 0; j < n_palettes; j++)
        for (int i = 0; i < palsize; i++) pat[(size_t)j * palsize + i] /= pat[(size_t)n_palettes * palsize - 1];
    return pat;
}

struct Carve {  // a workspace as the sum of its pieces, each rounded up to 256 bytes
    std::vector<size_t> sizes;
    char *base = nullptr, *cur = nullptr;
    size_t add(size_t b) {
        sizes.push_back(b);
        return sizes.size() - 1;
    }
    size_t bytes() const {
        size_t n = 0;
        for (size_t b : sizes) n += (b + 255) & ~(size_t)255;
        return std::max<size_t>(n, 256);
    }
    template <class T>
    T *take(size_t k) {
        char *r = cur;
        cur += (sizes[k] + 255) & ~(size_t)255;
        return (T *)r;
    }
};

}  // namespace

int quantize_palettes_var_dev(long n_tiles, const int32_t *d_rgb, const int32_t *d_pal_of, const uint8_t *d_active,
                              int P, int palsize, int n_palettes, const int32_t *acc0, int32_t *pal_out,
                              int32_t *use_count, int32_t *stats, hipStream_t stream) {
    if (n_tiles < 0 || P <= 0 || palsize <= 0 || palsize > VAR_MAXPAL || n_palettes <= 0 ||
        (n_tiles > 0 && (!d_rgb || !d_pal_of)) || !acc0 || !pal_out || !use_count || !stats) {
        set_error("quantize_palettes_var: invalid arguments (palsize in 1..256)");
        return -1;
    }
    if (n_tiles * 64 > 0x7fffffffL || P > (1 << 30)) {
        set_error("quantize_palettes_var: more than 2^31 pixels or 2^30 pairs");
        return -1;
    }
    const int npix = (int)(n_tiles * 64);
    int pair_bits = 1;
    while ((1ull << pair_bits) <= (uint64_t)P) pair_bits++;  // the sentinel pair P included
    std::vector<int> seg(P + 1, 0);
    if (npix == 0) {
        set_error("quantize_palettes_var: pair 0 has no Active tile (its colour list is empty)");
        return -1;
    }
    // ---- workspace 1: the pixel keys, their runs, the per-pair arrays
    size_t tmp_sort = 0, tmp_rle = 0;
    {
        hipcub::DoubleBuffer<uint64_t> dk(nullptr, nullptr);
        TILER_HIP_CHECK(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_sort, dk, npix, 0, 24 + pair_bits, stream));
        TILER_HIP_CHECK(hipcub::DeviceRunLengthEncode::Encode(nullptr, tmp_rle, (const uint64_t *)nullptr,
                                                              (uint64_t *)nullptr, (int *)nullptr, (int *)nullptr, npix,
                                                              stream));
    }
    Carve c1;
    const size_t np = (size_t)npix, b_pairs = 4 * ((size_t)P + 2);
    const size_t i_k0 = c1.add(8 * np), i_k1 = c1.add(8 * np), i_uk = c1.add(8 * np), i_cnt = c1.add(4 * np);
    const size_t i_tmp = c1.add(std::max(tmp_sort, tmp_rle) + 256), i_nr = c1.add(256), i_seg = c1.add(b_pairs);
    const size_t i_uc = c1.add(b_pairs);
    char *ws1 = nullptr, *ws2 = nullptr;
    TILER_HIP_CHECK(hipMalloc((void **)&ws1, c1.bytes()));
    c1.base = c1.cur = ws1;
    uint64_t *k0 = c1.take<uint64_t>(i_k0), *k1 = c1.take<uint64_t>(i_k1), *ukeys = c1.take<uint64_t>(i_uk);
    int *d_cnt = c1.take<int>(i_cnt);
    void *tmp1 = c1.take<void>(i_tmp);
    int *d_nruns = c1.take<int>(i_nr), *d_seg = c1.take<int>(i_seg), *d_uc = c1.take<int>(i_uc);
    int rc = -1, step = 0;  // step: the failing call (error message)
    bool said = false;      // the error is already set
    do {
        if (hipMemsetAsync(d_uc, 0, b_pairs, stream) != hipSuccess) { step = 1; break; }
        if (hipMemsetAsync(d_nruns, 0, 4, stream) != hipSuccess) { step = 2; break; }
        {
            KTimer tk("var_usage", stream);
            hipLaunchKernelGGL(var_keys_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, d_rgb, d_pal_of,
                               d_active, n_tiles, P, k0, d_uc);
            if (hipGetLastError() != hipSuccess) { step = 3; break; }
            hipcub::DoubleBuffer<uint64_t> kb(k0, k1);
            size_t ts = tmp_sort;
            if (hipcub::DeviceRadixSort::SortKeys(tmp1, ts, kb, npix, 0, 24 + pair_bits, stream) != hipSuccess) { step = 4; break; }
            size_t tr = tmp_rle;
            if (hipcub::DeviceRunLengthEncode::Encode(tmp1, tr, (const uint64_t *)kb.Current(), ukeys, d_cnt, d_nruns, npix,
                                                      stream) != hipSuccess) {
                step = 5;
                break;
            }
            hipLaunchKernelGGL(var_seg_kernel, dim3((P + 256) / 256), dim3(256), 0, stream, ukeys, d_nruns, P, d_seg);
            if (hipGetLastError() != hipSuccess) { step = 6; break; }
        }
        if (hipMemcpyAsync(seg.data(), d_seg, 4 * ((size_t)P + 1), hipMemcpyDeviceToHost, stream) != hipSuccess) { step = 7; break; }
        if (hipMemcpyAsync(use_count, d_uc, 4 * (size_t)P, hipMemcpyDeviceToHost, stream) != hipSuccess) { step = 8; break; }
        if (hipStreamSynchronize(stream) != hipSuccess) { step = 9; break; }
        for (int p = 0; p < P; p++)
            if (seg[p + 1] == seg[p]) {  // the reference reads CMUsage[0] of an empty list here and raises
                set_error("quantize_palettes_var: pair " + std::to_string(p) +
                          " has no Active tile (its colour list is empty)");
                said = true;
                break;
            }
        if (said) break;
        const int total = seg[P];
        // ---- workspace 2: the lists, sized by the distinct colours
        size_t tmp_a = 0, tmp_b = 0, tmp_scan = 0;
        {
            hipcub::DoubleBuffer<uint32_t> ka(nullptr, nullptr), va(nullptr, nullptr);
            hipcub::DoubleBuffer<uint64_t> kb(nullptr, nullptr);
            if (hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_a, ka, va, total, 0, 24, stream) != hipSuccess ||
                hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_b, kb, va, total, 0, 31 + pair_bits, stream) != hipSuccess ||
                hipcub::DeviceScan::InclusiveSum(nullptr, tmp_scan, (const uint32_t *)nullptr, (uint32_t *)nullptr, total,
                                                 stream) != hipSuccess) {
                step = 10;
                break;
            }
        }
        Carve c2;
        const size_t nt = (size_t)total, n_tree = (nt >> 5) + 8 * (size_t)P + 8;
        const size_t j_it = c2.add(16 * nt), j_so = c2.add(16 * nt), j_ka0 = c2.add(4 * nt), j_ka1 = c2.add(4 * nt);
        const size_t j_v0 = c2.add(4 * nt), j_v1 = c2.add(4 * nt), j_kb0 = c2.add(8 * nt), j_kb1 = c2.add(8 * nt);
        const size_t j_cn = c2.add(4 * nt), j_pf = c2.add(4 * nt), j_df = c2.add(4 * nt), j_pv = c2.add(4 * nt);
        const size_t j_nx = c2.add(4 * nt), j_tr = c2.add(8 * n_tree), j_tmp = c2.add(std::max({tmp_a, tmp_b, tmp_scan}) + 256);
        const size_t j_acc = c2.add(4 * (size_t)P), j_pat = c2.add(8 * (size_t)n_palettes * palsize);
        const size_t j_pick = c2.add(16 * (size_t)P * palsize), j_st = c2.add(16 * (size_t)P);
        if (hipMalloc((void **)&ws2, c2.bytes()) != hipSuccess) { step = 11; break; }
        c2.base = c2.cur = ws2;
        VarItem *items = c2.take<VarItem>(j_it), *sorted = c2.take<VarItem>(j_so);
        uint32_t *ka0 = c2.take<uint32_t>(j_ka0), *ka1 = c2.take<uint32_t>(j_ka1);
        uint32_t *v0 = c2.take<uint32_t>(j_v0), *v1 = c2.take<uint32_t>(j_v1);
        uint64_t *kb0 = c2.take<uint64_t>(j_kb0), *kb1 = c2.take<uint64_t>(j_kb1);
        uint32_t *d_counts = c2.take<uint32_t>(j_cn), *d_prefix = c2.take<uint32_t>(j_pf), *d_diff = c2.take<uint32_t>(j_df);
        int *d_prev = c2.take<int>(j_pv), *d_next = c2.take<int>(j_nx);
        unsigned long long *d_tree = c2.take<unsigned long long>(j_tr);
        void *tmp2 = c2.take<void>(j_tmp);
        int32_t *d_acc = c2.take<int32_t>(j_acc);
        double *d_pat = c2.take<double>(j_pat);
        VarItem *d_pick = c2.take<VarItem>(j_pick);
        int32_t *d_stats = c2.take<int32_t>(j_st);
        const std::vector<double> pat = var_pattern(n_palettes, palsize);
        std::vector<VarItem> pick((size_t)P * palsize);
        if (hipMemcpyAsync(d_acc, acc0, 4 * (size_t)P, hipMemcpyHostToDevice, stream) != hipSuccess) { step = 12; break; }
        if (hipMemcpyAsync(d_pat, pat.data(), 8 * pat.size(), hipMemcpyHostToDevice, stream) != hipSuccess) { step = 13; break; }
        if (hipMemsetAsync(d_stats, 0, 16 * (size_t)P, stream) != hipSuccess) { step = 14; break; }
        if (hipMemsetAsync(d_pick, 0, 16 * (size_t)P * palsize, stream) != hipSuccess) { step = 15; break; }
        const unsigned gt = (unsigned)((total + 255) / 256);
        {
            KTimer ti("var_items", stream);
            hipLaunchKernelGGL(var_items_kernel, dim3(gt), dim3(256), 0, stream, ukeys, d_cnt, total, items, ka0, v0);
            if (hipGetLastError() != hipSuccess) { step = 16; break; }
            hipcub::DoubleBuffer<uint32_t> ka(ka0, ka1), va(v0, v1);
            size_t ta = tmp_a;
            if (hipcub::DeviceRadixSort::SortPairs(tmp2, ta, ka, va, total, 0, 24, stream) != hipSuccess) { step = 17; break; }
            hipLaunchKernelGGL(var_key2_kernel, dim3(gt), dim3(256), 0, stream, ukeys, d_cnt, va.Current(), total, kb0);
            if (hipGetLastError() != hipSuccess) { step = 18; break; }
            hipcub::DoubleBuffer<uint64_t> kb(kb0, kb1);
            size_t tb = tmp_b;
            if (hipcub::DeviceRadixSort::SortPairs(tmp2, tb, kb, va, total, 0, 31 + pair_bits, stream) != hipSuccess) { step = 19; break; }
            hipLaunchKernelGGL(var_order_kernel, dim3(gt), dim3(256), 0, stream, items, kb.Current(), va.Current(), d_seg,
                               total, sorted, d_counts, d_prev, d_next, d_diff);
            if (hipGetLastError() != hipSuccess) { step = 20; break; }
            size_t tsc = tmp_scan;
            if (hipcub::DeviceScan::InclusiveSum(tmp2, tsc, (const uint32_t *)d_counts, d_prefix, total, stream) != hipSuccess) { step = 21; break; }
        }
        {
            KTimer tp("var_prune", stream);
            VarArgs a;
            a.seg = d_seg;
            a.it = sorted;
            a.diff = d_diff;
            a.prev = d_prev;
            a.next = d_next;
            a.prefix = d_prefix;
            a.tree = d_tree;
            a.acc0 = d_acc;
            a.pattern = d_pat;
            a.palsize = palsize;
            a.n_palettes = n_palettes;
            a.picked = d_pick;
            a.stats = d_stats;
            hipLaunchKernelGGL(var_prune_kernel, dim3(P), dim3(VAR_T), 0, stream, a);
            if (hipGetLastError() != hipSuccess) { step = 22; break; }
        }
        if (hipMemcpyAsync(pick.data(), d_pick, 16 * pick.size(), hipMemcpyDeviceToHost, stream) != hipSuccess) { step = 23; break; }
        if (hipMemcpyAsync(stats, d_stats, 16 * (size_t)P, hipMemcpyDeviceToHost, stream) != hipSuccess) { step = 24; break; }
        if (hipStreamSynchronize(stream) != hipSuccess) { step = 25; break; }
        std::vector<CmItem> cm(palsize);
        for (int p = 0; p < P && !said; p++) {
            if (stats[p * 4 + 3] < 0) {
                set_error("quantize_palettes_var: pair " + std::to_string(p) + " outgrew its tree region");
                said = true;
                break;
            }
            for (int i = 0; i < palsize; i++) {  // the stored keys: a merged item's are not those of its colour
                const VarItem &v = pick[(size_t)p * palsize + i];
                cm[i].index = v.index;
                cm[i].luma = v.luma;
                cm[i].hue = (uint8_t)(v.hsv & 255u);
                cm[i].sat = (uint8_t)((v.hsv >> 8) & 255u);
                cm[i].val = (uint8_t)((v.hsv >> 16) & 255u);
            }
            sort_cm_items(cm.data(), palsize);  // CMPal.Sort (main.pas:2413)
            for (int i = 0; i < palsize; i++) pal_out[(size_t)p * palsize + i] = cm[i].index;
        }
        if (said) break;
        rc = 0;
    } while (0);
    if (rc && !said) {
        const hipError_t e = hipGetLastError();
        set_error("quantize_palettes_var: HIP failure at step " + std::to_string(step) + " (" + hipGetErrorString(e) +
                  "), " + std::to_string(npix) + " pixels, " + std::to_string(P) + " pairs");
    }
    if (ws2) (void)hipFree(ws2);
    (void)hipFree(ws1);
    return rc;
}

int quantize_palettes_var_host(long n_tiles, const int32_t *rgb, const int32_t *pal_of, const uint8_t *active, int P,
                               int palsize, int n_palettes, const int32_t *acc0, int32_t *pal_out, int32_t *use_count,
                               int32_t *stats) {
    if (n_tiles < 0 || (n_tiles > 0 && (!rgb || !pal_of))) {
        set_error("quantize_palettes_var: invalid arguments");
        return -1;
    }
    HostStage s("quantize_palettes_var");
    const int32_t *d_rgb = s.in(rgb, (size_t)n_tiles * 64), *d_po = s.in(pal_of, (size_t)n_tiles);
    const uint8_t *d_act = s.in(active, (size_t)n_tiles);
    if (!s.ok() || quantize_palettes_var_dev(n_tiles, d_rgb, d_po, d_act, P, palsize, n_palettes, acc0, pal_out,
                                             use_count, stats, s.stream()))
        return -1;
    return s.finish();
}

}  // namespace tiler
