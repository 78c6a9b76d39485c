// global_tiling.hip -- DoGlobalTiling's K-Modes branch on gfx950 with the tile list in HBM: the plan (main.pas:4272-4331:
// dataset lines, bins by DitheringPalIndex, StartingPoint, ClusterCount), the K-Modes batch and its medoids
// (kmodes.hip, unchanged) and the merges (DoKModes 4246-4251 + MergeTiles 3688-3712, NewTile = nil).
//
//   gt_validate  4 lanes per tile, 16 bytes of PalPixels each: every Active tile's DitheringPalIndex in [0, n_palettes)
//                and bytes < palsize, the lowest offender kept in an error word (atomicMin) and never used as an index;
//                the histogram of the Active tiles by bin in per-workgroup LDS counters, flushed with one atomic each.
//   partition    the host picks the bins that get rows (those that run K-Modes, back to back from row 0: the bin_off
//                layout of kmodes_batch_dev; behind them the other non-empty bins when their StartingPoint is asked
//                for) and numbers them; gt_keys writes (bin number | "no row", tile) and ONE stable radix sort
//                (hipcub, over just the bits the bin numbers need: one 8-bit pass for 128 bins) leaves the tiles of
//                every bin back to back, ascending inside a bin as TileIndices[signi] fills them.  A dedicated
//                count / scan / scatter would need per-workgroup offsets of n_palettes counters each and three
//                launches; the sort moves 8 bytes per tile beside the 144 the lines kernel moves, see DESIGN §4.
//   gt_lines     a thread per row: 4 x 16-byte loads of the tile, the 16 zone counters in two 64-bit words of 8-bit
//                fields, 5 x 16-byte stores of the line; the row's byte sum goes into its bin's packed
//                (sum << 32 | 0xFFFFFFFF - row) word by a 64-bit atomicMin -- once per wave when the wave's rows are of
//                one bin -- which is the bin's last row of minimal sum (acc <= best).
//   gt_merge     4 lanes per row of a K-Modes bin: a row whose cluster has >= 2 members and whose tile is not the
//                cluster's medoid tile adds its UseCount to the medoid's (integer atomic; a merged tile is no medoid,
//                so the count it reads is never written), clears Active, sets MergeIndex and zeroes its PalPixels.
// Only integer atomics touch a result: it does not depend on the order threads run in.
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "global_tiling.hpp"
#include "kmodes.hpp"
#include "stage.hpp"

namespace tiler {

static constexpr int GT_T = 256;
static constexpr int GT_A = 80;  // cKModesFeatureCount
static constexpr unsigned long long GT_NO_ERROR = ~0ull;

__global__ __launch_bounds__(GT_T) void gt_validate(const uint8_t *__restrict__ palpix,
                                                     const int32_t *__restrict__ dith_pal,
                                                     const uint8_t *__restrict__ active, long nt, unsigned n_pal,
                                                     unsigned palsize, unsigned *__restrict__ hist,
                                                     unsigned long long *err) {
    __shared__ unsigned s_hist[GT_MAX_PALETTES];
    for (unsigned p = threadIdx.x; p < n_pal; p += GT_T) s_hist[p] = 0;
    __syncthreads();
    for (long e = (long)blockIdx.x * GT_T + threadIdx.x; e < nt * 4; e += (long)gridDim.x * GT_T) {
        const long t = e >> 2;
        if (!active[t]) continue;
        const unsigned p = (unsigned)dith_pal[t];
        bool bad = p >= n_pal;
        const uint4 v = reinterpret_cast<const uint4 *>(palpix)[e];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int b = 0; b < 4; b++) bad = bad || ((w[k] >> (8 * b)) & 255u) >= palsize;
        if (bad) atomicMin(err, (unsigned long long)t);
        if ((e & 3) == 0 && p < n_pal) atomicAdd(&s_hist[p], 1u);
    }
    __syncthreads();
    for (unsigned p = threadIdx.x; p < n_pal; p += GT_T)
        if (s_hist[p]) atomicAdd(&hist[p], s_hist[p]);
}

// rank[p]: the number of bin p in the row layout, norow for a bin without rows
__global__ __launch_bounds__(GT_T) void gt_keys(const int32_t *__restrict__ dith_pal,
                                                 const uint8_t *__restrict__ active, long nt, unsigned n_pal,
                                                 const unsigned *__restrict__ rank, unsigned norow,
                                                 unsigned *__restrict__ key, unsigned *__restrict__ val) {
    for (long t = (long)blockIdx.x * GT_T + threadIdx.x; t < nt; t += (long)gridDim.x * GT_T) {
        const unsigned p = (unsigned)dith_pal[t];
        key[t] = active[t] && p < n_pal ? rank[p] : norow;
        val[t] = (unsigned)t;
    }
}

// WriteTileDatasetLine of tile rows[r] (rows null: tile r) for r < n: line[r] (may be null), signi[r] (may be null);
// best given: bin[r] = the row's bin number, boff its first row; best[bin] = min (sum << 32 | 0xFFFFFFFF - local row)
__global__ __launch_bounds__(GT_T) void gt_lines(const uint8_t *__restrict__ palpix, const unsigned *__restrict__ rows,
                                                  long n, int palsize, uint8_t *__restrict__ line,
                                                  int32_t *__restrict__ signi, const unsigned *__restrict__ bin,
                                                  const int32_t *__restrict__ boff, unsigned long long *best) {
    __shared__ uint8_t s_zone[256];
    {
        const int z = (threadIdx.x * 16) / palsize;  // GetTilePalZoneThres: zones past the 16th are never read
        s_zone[threadIdx.x] = (uint8_t)(z < 16 ? z : 16);
    }
    __syncthreads();
    const int thr = palsize / 16;
    // base is the same for a whole workgroup, so every lane of a wave takes every trip and the votes are complete
    for (long base = (long)blockIdx.x * GT_T; base < n; base += (long)gridDim.x * GT_T) {
        const long r = base + threadIdx.x;
        const bool on = r < n;
        unsigned sum = 0;
        if (on) {
            const long t = rows ? (long)rows[r] : r;
            const uint4 *src = reinterpret_cast<const uint4 *>(palpix + t * 64);
            uint32_t row[20];
            unsigned long long acc_lo = 0, acc_hi = 0;  // 8 zone counters of 8 bits each (a count is at most 64)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint4 v = src[q];
                row[4 * q] = v.x, row[4 * q + 1] = v.y, row[4 * q + 2] = v.z, row[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int d = 0; d < 16; d++) {
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const unsigned c = (row[d] >> (8 * b)) & 255u;
                    sum += c;
                    const unsigned z = s_zone[c];
                    if (z < 8)
                        acc_lo += 1ull << (8 * z);
                    else if (z < 16)
                        acc_hi += 1ull << (8 * (z - 8));
                }
            }
            int most = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                uint32_t f = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int z = 4 * w + b;
                    const int c = (int)(((z < 8 ? acc_lo : acc_hi) >> (8 * (z & 7))) & 255u);
                    most = max(most, c);
                    if (c > thr) {
                        f |= 1u << (8 * b);
                        sum++;
                    }
                }
                row[16 + w] = f;
            }
            if (signi) signi[r] = 64 - most;
            if (line) {
                uint4 *dl = reinterpret_cast<uint4 *>(line + r * GT_A);
#pragma unroll
                for (int q = 0; q < 5; q++)
                    dl[q] = make_uint4(row[4 * q], row[4 * q + 1], row[4 * q + 2], row[4 * q + 3]);
            }
        }
        if (!best) continue;  // uniform
        const unsigned b = on ? bin[r] : 0u;
        unsigned long long pk = GT_NO_ERROR;
        if (on) pk = ((unsigned long long)sum << 32) | (0xFFFFFFFFu - (unsigned)(r - boff[b]));
        const unsigned long long m = __ballot(on);
        if (!m) continue;
        const unsigned b0 = __shfl(b, __ffsll(m) - 1);
        if (__ballot(on && b != b0) == 0) {
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const unsigned long long o = __shfl_xor(pk, s);
                pk = o < pk ? o : pk;
            }
            if ((threadIdx.x & 63) == 0) atomicMin(&best[b0], pk);
        } else if (on) {
            atomicMin(&best[b], pk);
        }
    }
}

// rows [0, n): the rows of the K-Modes bins.  medw / counts [sum k]: kmb_medoid's packed words and member counts
__global__ __launch_bounds__(GT_T) void gt_merge(const unsigned *__restrict__ rows, const unsigned *__restrict__ bin,
                                                  long n, const int32_t *__restrict__ boff,
                                                  const int32_t *__restrict__ koff, const int32_t *__restrict__ labels,
                                                  const unsigned long long *__restrict__ medw,
                                                  const int32_t *__restrict__ counts, uint8_t *palpix, uint8_t *active,
                                                  unsigned long long *use_count, long long *merge_index) {
    for (long e = (long)blockIdx.x * GT_T + threadIdx.x; e < n * 4; e += (long)gridDim.x * GT_T) {
        const long r = e >> 2;
        const unsigned b = bin[r];
        const long j = (long)koff[b] + labels[r];
        if (counts[j] < 2) continue;
        const long mrow = (long)boff[b] + (long)(0xFFFFFFFFu - (unsigned)(medw[j] & 0xFFFFFFFFull));
        const unsigned med = rows[mrow], tile = rows[r];
        if (tile == med) continue;
        reinterpret_cast<uint4 *>(palpix)[(long)tile * 4 + (e & 3)] = make_uint4(0, 0, 0, 0);
        if (e & 3) continue;
        atomicAdd(&use_count[med], use_count[tile]);
        active[tile] = 0;
        merge_index[tile] = (long long)med;
    }
}

__global__ __launch_bounds__(GT_T) void gt_medoid_rows(const unsigned long long *__restrict__ medw,
                                                        const int32_t *__restrict__ counts, long K,
                                                        int32_t *__restrict__ medoid) {
    for (long j = (long)blockIdx.x * GT_T + threadIdx.x; j < K; j += (long)gridDim.x * GT_T)
        medoid[j] = counts[j] > 0 ? (int32_t)(0xFFFFFFFFu - (unsigned)(medw[j] & 0xFFFFFFFFull)) : -1;
}

// ---- host side ----
namespace {

constexpr long GT_LIMIT = 1L << 31;

unsigned gt_grid(long n, long cap = 8192) {
    return (unsigned)std::max<long>(1, std::min<long>(cap, (n + GT_T - 1) / GT_T));
}

int gt_fail(const char *who, const std::string &what) {
    set_error(std::string(who) + ": " + what);
    return -1;
}

bool misaligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// EqualQualityTileCount main.pas:722-725: round(sqrt(n) * log2(1 + n)), FPC's log2 = ln(x) * (1 / ln 2), half to even
long equal_quality_tile_count(double n) {
    return (long)nearbyint(sqrt(n) * (log(1.0 + n) * 1.4426950408889634079));
}

// what is wrong with tile t (the lowest offender of gt_validate)
int gt_bad_tile(const char *who, const uint8_t *d_palpix, const int32_t *d_dith_pal, unsigned long long t, int n_pal,
                int palsize) {
    int32_t p = 0;
    uint8_t pix[64];
    TILER_HIP_CHECK(hipMemcpy(&p, d_dith_pal + t, 4, hipMemcpyDeviceToHost));
    TILER_HIP_CHECK(hipMemcpy(pix, d_palpix + t * 64, 64, hipMemcpyDeviceToHost));
    if (p < 0 || p >= n_pal)
        return gt_fail(who, "tile " + std::to_string(t) + " has dith_pal " + std::to_string(p) + ", outside [0, " +
                                std::to_string(n_pal) + ")");
    for (int i = 0; i < 64; i++)
        if (pix[i] >= palsize)
            return gt_fail(who, "tile " + std::to_string(t) + " has palette index " + std::to_string(pix[i]) +
                                    " at pixel " + std::to_string(i) + ", not below palsize " + std::to_string(palsize));
    return gt_fail(who, "tile " + std::to_string(t) + " is invalid");
}

}  // namespace

int global_tiling_counts(const int32_t *bin_size, int n_palettes, int desired, int32_t *k, uint8_t *run) {
    const char *who = "global_tiling_counts";
    if (!bin_size) return gt_fail(who, "null bin_size");
    if (n_palettes < 1 || n_palettes > GT_MAX_PALETTES)
        return gt_fail(who, "need 1 <= n_palettes <= " + std::to_string(GT_MAX_PALETTES));
    if (desired < 1 || desired > GT_MAX_DESIRED) return gt_fail(who, "need 1 <= desired <= 2^30");
    long total = 0;
    for (int p = 0; p < n_palettes; p++) {
        if (bin_size[p] < 0) return gt_fail(who, "bin_size[" + std::to_string(p) + "] is negative");
        total += equal_quality_tile_count((double)bin_size[p]);
    }
    for (int p = 0; p < n_palettes; p++) {
        long kc = 0;
        if (total > 0) {
            const double share = (double)desired / (double)total;
            kc = (long)ceil((double)equal_quality_tile_count((double)bin_size[p]) * share);
        }
        if (k) k[p] = (int32_t)kc;
        if (run) run[p] = total > 0 && (long)bin_size[p] > kc;
    }
    return 0;
}

int global_tiling_check_args(long nt, int n_palettes, int palsize, int desired) {
    const char *who = "global_tiling";
    if (nt < 0 || nt >= GT_LIMIT) return gt_fail(who, "need 0 <= nt < 2^31");
    if (n_palettes < 1 || n_palettes > GT_MAX_PALETTES)
        return gt_fail(who, "need 1 <= n_palettes <= " + std::to_string(GT_MAX_PALETTES));
    if (desired < 1 || desired > GT_MAX_DESIRED) return gt_fail(who, "need 1 <= desired <= 2^30");
    if (palsize < 1 || palsize > 256) return gt_fail(who, "need 1 <= palsize <= 256");
    return 0;
}

int global_tiling_dev(uint8_t *d_palpix, const int32_t *d_dith_pal, uint8_t *d_active, int64_t *d_use_count,
                      int64_t *d_merge_index, long nt, int n_palettes, int palsize, int desired, int restart,
                      int32_t *bin_size, int32_t *k, int32_t *start, hipStream_t st) {
    const char *who = "global_tiling";
    if (global_tiling_check_args(nt, n_palettes, palsize, desired)) return -1;
    if (nt > 0 && (!d_palpix || !d_dith_pal || !d_active || !d_use_count || !d_merge_index))
        return gt_fail(who, "null array");
    if (misaligned(d_palpix, 16) || misaligned(d_dith_pal, 4) || misaligned(d_use_count, 8) ||
        misaligned(d_merge_index, 8))
        return gt_fail(who, "palpix must be 16-byte aligned, dith_pal 4-byte, use_count and merge_index 8-byte");
    const int P = n_palettes;
    std::vector<int32_t> size(P, 0), kk(P, 0), first(P, -restart);
    std::vector<uint8_t> run(P, 0);
    auto publish = [&]() {
        for (int p = 0; p < P; p++) {
            if (bin_size) bin_size[p] = size[p];
            if (k) k[p] = kk[p];
            if (start) start[p] = first[p];
        }
        return 0;
    };
    if (nt == 0) return publish();

    Blocks blk(st);
    unsigned *hist = nullptr;  // [P] counters, then the error word (8-byte aligned)
    const size_t hist_bytes = ((size_t)P * 4 + 7) & ~(size_t)7;
    if (!blk.get(hist, hist_bytes + 8)) return gt_fail(who, "out of device memory");
    unsigned long long *err = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(hist) + hist_bytes);
    TILER_HIP_CHECK(hipMemsetAsync(hist, 0, hist_bytes, st));
    TILER_HIP_CHECK(hipMemsetAsync(err, 0xFF, 8, st));
    TILER_HIP_CHECK(hipMemsetAsync(d_merge_index, 0xFF, (size_t)nt * 8, st));
    {
        KTimer tm("gt_validate", st);
        hipLaunchKernelGGL(gt_validate, dim3(gt_grid(nt * 4, 2048)), dim3(GT_T), 0, st, (const uint8_t *)d_palpix,
                           d_dith_pal, (const uint8_t *)d_active, nt, (unsigned)P, (unsigned)palsize, hist, err);
    }
    TILER_HIP_CHECK(hipGetLastError());
    std::vector<unsigned> h_hist(hist_bytes / 4 + 2);
    TILER_HIP_CHECK(hipMemcpyAsync(h_hist.data(), hist, hist_bytes + 8, hipMemcpyDeviceToHost, st));
    TILER_HIP_CHECK(hipStreamSynchronize(st));  // wait 1: the histogram and the error word
    unsigned long long e = 0;
    memcpy(&e, reinterpret_cast<char *>(h_hist.data()) + hist_bytes, 8);
    if (e != GT_NO_ERROR) return gt_bad_tile(who, d_palpix, d_dith_pal, e, P, palsize);
    for (int p = 0; p < P; p++) size[p] = (int32_t)h_hist[p];
    if (global_tiling_counts(size.data(), P, desired, kk.data(), run.data())) return -1;

    // the row layout: the K-Modes bins back to back, then (start asked for) the other non-empty bins
    std::vector<unsigned> rank(P, 0);
    std::vector<int> bins;
    for (int p = 0; p < P; p++)
        if (run[p]) bins.push_back(p);
    const int nrun = (int)bins.size();
    if (start)
        for (int p = 0; p < P; p++)
            if (!run[p] && size[p] > 0) bins.push_back(p);
    const int nlay = (int)bins.size();
    if (nlay == 0) return publish();
    std::vector<int32_t> boff(nlay + 1, 0), koff(nrun + 1, 0), ks(std::max(nrun, 1)), sp(std::max(nrun, 1));
    for (int p = 0; p < P; p++) rank[p] = (unsigned)nlay;
    for (int i = 0; i < nlay; i++) {
        rank[bins[i]] = (unsigned)i;
        boff[i + 1] = boff[i] + size[bins[i]];
    }
    for (int i = 0; i < nrun; i++) {
        ks[i] = kk[bins[i]];
        koff[i + 1] = koff[i] + ks[i];
    }
    const long N = boff[nlay], Nrun = boff[nrun], K = koff[nrun];
    int bits = 1;
    while ((1 << bits) <= nlay) bits++;

    size_t tmp_bytes = 0;
    {
        hipcub::DoubleBuffer<unsigned> kb(nullptr, nullptr), vb(nullptr, nullptr);
        TILER_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, kb, vb, (int)nt, 0, bits, st));
    }
    unsigned *d_rank = nullptr, *k0 = nullptr, *k1 = nullptr, *v0 = nullptr, *v1 = nullptr;
    int32_t *d_boff = nullptr, *d_koff = nullptr, *d_labels = nullptr, *d_counts = nullptr;
    unsigned long long *best = nullptr, *medw = nullptr;
    uint8_t *X = nullptr, *cent = nullptr;
    void *tmp = nullptr;
    const size_t b4 = (size_t)nt * 4;
    if (!blk.get(d_rank, (size_t)P * 4) || !blk.get(k0, b4) || !blk.get(k1, b4) || !blk.get(v0, b4) ||
        !blk.get(v1, b4) || !blk.get(tmp, tmp_bytes) || !blk.get(d_boff, (size_t)(nlay + 1) * 4) ||
        !blk.get(d_koff, (size_t)(nrun + 1) * 4) || !blk.get(best, (size_t)nlay * 8) ||
        !blk.get(X, (size_t)N * GT_A) || !blk.get(d_labels, (size_t)Nrun * 4) || !blk.get(cent, (size_t)K * GT_A) ||
        !blk.get(medw, (size_t)K * 8) || !blk.get(d_counts, (size_t)K * 4))
        return gt_fail(who, "out of device memory");
    TILER_HIP_CHECK(hipMemcpyAsync(d_rank, rank.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
    TILER_HIP_CHECK(hipMemcpyAsync(d_boff, boff.data(), (size_t)(nlay + 1) * 4, hipMemcpyHostToDevice, st));
    TILER_HIP_CHECK(hipMemcpyAsync(d_koff, koff.data(), (size_t)(nrun + 1) * 4, hipMemcpyHostToDevice, st));
    TILER_HIP_CHECK(hipMemsetAsync(best, 0xFF, (size_t)nlay * 8, st));
    const unsigned *rows = nullptr, *rbin = nullptr;
    {
        KTimer tm("gt_partition", st);
        hipLaunchKernelGGL(gt_keys, dim3(gt_grid(nt)), dim3(GT_T), 0, st, d_dith_pal, (const uint8_t *)d_active, nt,
                           (unsigned)P, (const unsigned *)d_rank, (unsigned)nlay, k0, v0);
        TILER_HIP_CHECK(hipGetLastError());
        hipcub::DoubleBuffer<unsigned> kb(k0, k1), vb(v0, v1);
        TILER_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, kb, vb, (int)nt, 0, bits, st));
        rows = vb.Current();
        rbin = kb.Current();
    }
    {
        KTimer tm("gt_lines", st);
        hipLaunchKernelGGL(gt_lines, dim3(gt_grid(N)), dim3(GT_T), 0, st, (const uint8_t *)d_palpix, rows, N, palsize,
                           X, (int32_t *)nullptr, rbin, (const int32_t *)d_boff, best);
    }
    TILER_HIP_CHECK(hipGetLastError());
    std::vector<unsigned long long> h_best(nlay);
    TILER_HIP_CHECK(hipMemcpyAsync(h_best.data(), best, (size_t)nlay * 8, hipMemcpyDeviceToHost, st));
    TILER_HIP_CHECK(hipStreamSynchronize(st));  // wait 2: the StartingPoints
    for (int i = 0; i < nlay; i++) {
        const long s = (long)(0xFFFFFFFFu - (unsigned)(h_best[i] & 0xFFFFFFFFull));
        if (s < 0 || s >= size[bins[i]]) return gt_fail(who, "internal: a StartingPoint outside its bin");
        first[bins[i]] = (int32_t)s;
        if (i < nrun) sp[i] = (int32_t)s;
    }
    if (nrun == 0) return publish();
    // K-Modes (it waits on st itself) and the medoid words, on X where it lies
    if (kmodes_batch_dev(X, boff.data(), nrun, ks.data(), sp.data(), palsize, d_labels, cent, nullptr, nullptr, st))
        return -1;
    {
        KTimer tm("gt_medoids", st);
        if (kmodes_medoids_words_dev(X, d_boff, d_koff, nrun, Nrun, K, d_labels, cent, medw, d_counts, st)) return -1;
    }
    {
        KTimer tm("gt_merge", st);
        hipLaunchKernelGGL(gt_merge, dim3(gt_grid(Nrun * 4)), dim3(GT_T), 0, st, rows, rbin, Nrun,
                           (const int32_t *)d_boff, (const int32_t *)d_koff, (const int32_t *)d_labels,
                           (const unsigned long long *)medw, (const int32_t *)d_counts, d_palpix, d_active,
                           reinterpret_cast<unsigned long long *>(d_use_count), (long long *)d_merge_index);
    }
    TILER_HIP_CHECK(hipGetLastError());
    TILER_HIP_CHECK(hipStreamSynchronize(st));  // wait 3: the results are complete on return
    return publish();
}

int global_tiling_host(uint8_t *palpix, const int32_t *dith_pal, uint8_t *active, int64_t *use_count,
                       int64_t *merge_index, long nt, int n_palettes, int palsize, int desired, int restart,
                       int32_t *bin_size, int32_t *k, int32_t *start) {
    if (global_tiling_check_args(nt, n_palettes, palsize, desired)) return -1;
    if (nt > 0 && (!palpix || !dith_pal || !active || !use_count || !merge_index))
        return gt_fail("global_tiling", "null array");
    // the optional outputs go to the caller only when the whole call succeeds
    std::vector<int32_t> o(3 * (size_t)n_palettes);
    HostStage s("global_tiling");
    const size_t t = (size_t)nt;
    uint8_t *d_pp = s.inout(palpix, t * 64), *d_act = s.inout(active, t);
    const int32_t *d_dp = s.in(dith_pal, t);
    int64_t *d_uc = s.inout(use_count, t), *d_mi = s.out(merge_index, t);
    if (!s.ok() || global_tiling_dev(d_pp, d_dp, d_act, d_uc, d_mi, nt, n_palettes, palsize, desired, restart, o.data(),
                                     o.data() + n_palettes, start ? o.data() + 2 * n_palettes : nullptr, s.stream()))
        return -1;
    if (s.finish()) return -1;
    for (int p = 0; p < n_palettes; p++) {
        if (bin_size) bin_size[p] = o[p];
        if (k) k[p] = o[n_palettes + p];
        if (start) start[p] = o[2 * (size_t)n_palettes + p];
    }
    return 0;
}

int tile_dataset_lines_dev(const uint8_t *d_palpix, long nt, int palsize, uint8_t *d_lines, int32_t *d_pal_signi,
                           hipStream_t st) {
    const char *who = "tile_dataset_lines";
    if (nt < 0 || nt >= GT_LIMIT) return gt_fail(who, "need 0 <= nt < 2^31");
    if (palsize < 1 || palsize > 256) return gt_fail(who, "need 1 <= palsize <= 256");
    if (nt == 0 || (!d_lines && !d_pal_signi)) return 0;
    if (!d_palpix) return gt_fail(who, "null palpix");
    if (misaligned(d_palpix, 16) || misaligned(d_lines, 16) || misaligned(d_pal_signi, 4))
        return gt_fail(who, "palpix and lines must be 16-byte aligned, pal_signi 4-byte aligned");
    {
        KTimer tm("gt_lines", st);
        hipLaunchKernelGGL(gt_lines, dim3(gt_grid(nt)), dim3(GT_T), 0, st, d_palpix, (const unsigned *)nullptr, nt,
                           palsize, d_lines, d_pal_signi, (const unsigned *)nullptr, (const int32_t *)nullptr,
                           (unsigned long long *)nullptr);
    }
    TILER_HIP_CHECK(hipGetLastError());
    TILER_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

int tile_dataset_lines_host(const uint8_t *palpix, long nt, int palsize, uint8_t *lines, int32_t *pal_signi) {
    if (nt < 0 || nt >= GT_LIMIT) return gt_fail("tile_dataset_lines", "need 0 <= nt < 2^31");
    if (palsize < 1 || palsize > 256) return gt_fail("tile_dataset_lines", "need 1 <= palsize <= 256");
    if (nt > 0 && !palpix) return gt_fail("tile_dataset_lines", "null palpix");
    HostStage s("tile_dataset_lines");
    const uint8_t *d_pp = s.in(palpix, (size_t)nt * 64);
    uint8_t *d_l = s.out(lines, (size_t)nt * GT_A);
    int32_t *d_s = s.out(pal_signi, (size_t)nt);
    if (!s.ok() || tile_dataset_lines_dev(d_pp, nt, palsize, d_l, d_s, s.stream())) return -1;
    return s.finish();
}

int kmodes_medoids_batch_devout(const uint8_t *d_X, const int32_t *h_boff, int nb, const int32_t *h_k,
                                const int32_t *d_labels, const uint8_t *d_centroids, int32_t *d_medoid,
                                int32_t *d_counts, hipStream_t st) {
    const char *who = "kmodes_medoids";
    if (!d_X || !h_boff || nb <= 0 || !h_k || !d_labels || !d_centroids || !d_medoid || !d_counts)
        return gt_fail(who, "invalid arguments");
    if (misaligned(d_X, 16) || misaligned(d_centroids, 16))
        return gt_fail(who, "X and centroids must be 16-byte aligned");
    std::vector<int32_t> koff(nb + 1, 0);
    for (int b = 0; b < nb; b++) {
        if (h_k[b] < 0 || h_boff[b + 1] < h_boff[b] || h_boff[0] != 0) return gt_fail(who, "invalid bin");
        koff[b + 1] = koff[b] + h_k[b];
    }
    const long N = h_boff[nb], K = koff[nb];
    if (K == 0) return 0;
    Blocks blk(st);
    int32_t *d_boff = nullptr, *d_koff = nullptr;
    unsigned long long *medw = nullptr;
    if (!blk.get(d_boff, (size_t)(nb + 1) * 4) || !blk.get(d_koff, (size_t)(nb + 1) * 4) ||
        !blk.get(medw, (size_t)K * 8))
        return gt_fail(who, "out of device memory");
    TILER_HIP_CHECK(hipMemcpyAsync(d_boff, h_boff, (size_t)(nb + 1) * 4, hipMemcpyHostToDevice, st));
    TILER_HIP_CHECK(hipMemcpyAsync(d_koff, koff.data(), (size_t)(nb + 1) * 4, hipMemcpyHostToDevice, st));
    if (kmodes_medoids_words_dev(d_X, d_boff, d_koff, nb, N, K, d_labels, d_centroids, medw, d_counts, st)) return -1;
    hipLaunchKernelGGL(gt_medoid_rows, dim3(gt_grid(K)), dim3(GT_T), 0, st, (const unsigned long long *)medw,
                       (const int32_t *)d_counts, K, d_medoid);
    TILER_HIP_CHECK(hipGetLastError());
    TILER_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

}  // namespace tiler
