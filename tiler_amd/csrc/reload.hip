// reload.hip -- the GlobalTiling step's reload branch (ReloadPreviousTiling main.pas:4372-4470) on gfx950.
//
// Every active tile of the clip is snapped to its closest tile of a saved tileset (.gts): the tile's K-Modes dataset
// line (WriteTileDatasetLine main.pas:4167-4183) against the saved tiles that share its PalSigni (GetTilePalZoneThres'
// return value, 0..64), or against all of them when that bucket is empty, by GetMinMatchingDissim (kmodes.pas:598-604:
// the asm dissimilarity, ties to the last row).  The saved rows never change, so they are prepared once at load time
// and stay in HBM; one pass is a single throughput-bound launch:
//   rl_rows     tiles -> optional rescale, 80-byte dataset line, PalSigni, prepared row (km_prep_word), "byte >= 16"
//   rl_keys / rl_scan / rl_scatter   counting sort of the queries by key (bucket, or the whole-set key)
//   rl_match    one workgroup = a run of queries of one key x a slice of that key's rows, rows staged through LDS
//               as they lie in HBM (already prepared); per-thread packed (dis, inverted position) keys, slices
//               combined by atomicMin on (dis << 32) | ~position
//   rl_finish   position -> file-order row index, dis, and the tile's new PalPixels
// Row storage of a loaded tileset: 2n rows, [0, n) in file order (the whole-set key's range) and [n, 2n) ordered by
// PalSigni, file order inside a bucket; perm maps a position to its file-order row.  Inside any range positions
// follow file order, so "last position" is "last row" as the reference's <= loop has it.
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "kmodes_dev.hpp"
#include "reload.hpp"
#include "stage.hpp"

namespace tiler {

static constexpr int RL_NT = 256;
static constexpr int RL_STAGE = 64;    // rows per LDS stage
static constexpr int RL_MAXK = 1024;   // keys at most: the groups and the whole-set key
static constexpr int RL_SIGNI = 65;    // PalSigni values 0..64
static constexpr int RL_SORT_PER = 4;  // queries per thread of the scatter pass
static constexpr long RL_CHUNK = 1L << 20;  // queries per pass

struct RlHead {  // read back by the host before the argmin launch
    unsigned bad;    // some query byte >= 16
    int nblk;        // query blocks of the pass
    unsigned long long pairs;
};
struct RlCtl {
    RlHead h;
    int cnt[RL_MAXK];       // queries per key
    int qoff[RL_MAXK + 1];  // first sorted position of a key
    int boff[RL_MAXK + 1];  // first query block of a key
    int cur[RL_MAXK];       // scatter cursors
};

static std::atomic<long> g_rl_chunk{0};
static std::atomic<int> g_rl_qpt{0}, g_rl_slices{0};
static std::atomic<long long> g_rl_pairs{0};

// tiles [n][64] -> dataset line [n][80], PalSigni [n], prepared row [n][KM_PW]; den > 0: every byte first becomes
// (v * num) div den, kept as a byte (main.pas:4436-4438)
__global__ __launch_bounds__(RL_NT) void rl_rows(const uint8_t *__restrict__ pix, long n, int num, int den, int palsize,
                                                  uint8_t *__restrict__ line, uint4 *__restrict__ prep,
                                                  int32_t *__restrict__ signi, unsigned *bad) {
    __shared__ uint8_t s_resc[256], s_zone[256];
    {
        const int t = threadIdx.x;
        s_resc[t] = den > 0 ? (uint8_t)((t * num) / den) : (uint8_t)t;
        const int z = (t * 16) / palsize;  // GetTilePalZoneThres: zones past the 16th are counted and never read
        s_zone[t] = (uint8_t)(z < 16 ? z : 16);
    }
    __syncthreads();
    const int thr = palsize / 16;
    for (long i = (long)blockIdx.x * RL_NT + threadIdx.x; i < n; i += (long)gridDim.x * RL_NT) {
        uint32_t row[20];
        unsigned long long acc_lo = 0, acc_hi = 0;  // 8 zone counters of 8 bits each (a count is at most 64)
        const uint4 *src = reinterpret_cast<const uint4 *>(pix + i * 64);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint4 v = src[q];
            const uint32_t in[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t o = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const unsigned c = s_resc[(in[k] >> (8 * b)) & 255u];
                    o |= c << (8 * b);
                    const unsigned z = s_zone[c];
                    if (z < 8)
                        acc_lo += 1ull << (8 * z);
                    else if (z < 16)
                        acc_hi += 1ull << (8 * (z - 8));
                }
                row[4 * q + k] = o;
            }
        }
        int sg = 64;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            uint32_t f = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int z = 4 * w + b;
                const int c = (int)(((z < 8 ? acc_lo : acc_hi) >> (8 * (z & 7))) & 255u);
                sg = min(sg, 64 - c);
                f |= (c > thr ? 1u : 0u) << (8 * b);
            }
            row[16 + w] = f;
        }
        uint32_t big = 0;
#pragma unroll
        for (int d = 0; d < 20; d++) big |= row[d] & 0xF0F0F0F0u;
        if (big) atomicOr(bad, 1u);
        signi[i] = sg;
        uint4 *dl = reinterpret_cast<uint4 *>(line + i * KM_A);
#pragma unroll
        for (int q = 0; q < 5; q++) dl[q] = make_uint4(row[4 * q], row[4 * q + 1], row[4 * q + 2], row[4 * q + 3]);
        uint32_t o[KM_PW];
#pragma unroll
        for (int w = 0; w < KM_PW; w++) o[w] = km_prep_word(row, w);
#pragma unroll
        for (int q = 0; q < KM_PW / 4; q++)
            prep[i * (KM_PW / 4) + q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    }
}

// prepared rows of given dataset lines (the bare primitive's rows and items)
__global__ __launch_bounds__(RL_NT) void rl_prep80(const uint8_t *__restrict__ X, long n, uint4 *__restrict__ prep,
                                                    unsigned *bad) {
    for (long i = (long)blockIdx.x * RL_NT + threadIdx.x; i < n; i += (long)gridDim.x * RL_NT) {
        uint32_t row[20];
        load_row(X + i * KM_A, row);
        uint32_t big = 0;
#pragma unroll
        for (int d = 0; d < 20; d++) big |= row[d] & 0xF0F0F0F0u;
        if (big) atomicOr(bad, 1u);
        uint32_t o[KM_PW];
#pragma unroll
        for (int w = 0; w < KM_PW; w++) o[w] = km_prep_word(row, w);
#pragma unroll
        for (int q = 0; q < KM_PW / 4; q++)
            prep[i * (KM_PW / 4) + q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    }
}

// rows [n, 2n) of a loaded tileset: the file-order rows in bucket order
__global__ __launch_bounds__(RL_NT) void rl_bucket_rows(uint8_t *rows, uint4 *prep, const int32_t *perm, long n) {
    for (long j = (long)blockIdx.x * RL_NT + threadIdx.x; j < n; j += (long)gridDim.x * RL_NT) {
        const long s = perm[n + j];
        const uint4 *a = reinterpret_cast<const uint4 *>(rows + s * KM_A);
        uint4 *b = reinterpret_cast<uint4 *>(rows + (n + j) * KM_A);
#pragma unroll
        for (int q = 0; q < 5; q++) b[q] = a[q];
#pragma unroll
        for (int q = 0; q < KM_PW / 4; q++) prep[(n + j) * (KM_PW / 4) + q] = prep[s * (KM_PW / 4) + q];
    }
}

// key of every query: its group, the whole-set key nk - 1 when that group is none or empty, -1 = not searched
__global__ __launch_bounds__(RL_NT) void rl_keys(const int32_t *__restrict__ grp, const uint8_t *__restrict__ active,
                                                  long m, const int2 *__restrict__ range, int nk,
                                                  int32_t *__restrict__ key, unsigned long long *__restrict__ akey,
                                                  RlCtl *ctl) {
    __shared__ int h[RL_MAXK];
    for (int k = threadIdx.x; k < nk; k += RL_NT) h[k] = 0;
    __syncthreads();
    for (long i = (long)blockIdx.x * RL_NT + threadIdx.x; i < m; i += (long)gridDim.x * RL_NT) {
        int k = grp[i];
        if (k < 0 || k >= nk - 1 || range[k].y <= 0) k = nk - 1;
        if (active && !active[i]) k = -1;
        key[i] = k;
        akey[i] = ~0ull;
        if (k >= 0) atomicAdd(&h[k], 1);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nk; k += RL_NT)
        if (h[k]) atomicAdd(&ctl->cnt[k], h[k]);
}

// offsets of the sorted order and of the query blocks (qb queries each); at most RL_MAXK keys: one thread
__global__ void rl_scan(RlCtl *ctl, const int2 *__restrict__ range, int nk, int qb) {
    if (threadIdx.x || blockIdx.x) return;
    int q = 0, b = 0;
    unsigned long long pairs = 0;
    for (int k = 0; k < nk; k++) {
        const int c = ctl->cnt[k];
        ctl->qoff[k] = q;
        ctl->cur[k] = q;
        ctl->boff[k] = b;
        q += c;
        b += (c + qb - 1) / qb;
        pairs += (unsigned long long)c * (unsigned long long)max(range[k].y, 0);
    }
    ctl->qoff[nk] = q;
    ctl->boff[nk] = b;
    ctl->h.nblk = b;
    ctl->h.pairs = pairs;
}

// order[sorted position] = query; a workgroup reserves its share of every key with one atomic per key (the order
// inside a key is arbitrary: queries are independent)
__global__ __launch_bounds__(RL_NT) void rl_scatter(const int32_t *__restrict__ key, long m, int nk, RlCtl *ctl,
                                                     int32_t *__restrict__ order) {
    __shared__ int h[RL_MAXK];
    for (int k = threadIdx.x; k < nk; k += RL_NT) h[k] = 0;
    __syncthreads();
    const long i0 = (long)blockIdx.x * (RL_NT * RL_SORT_PER) + threadIdx.x;
    int kk[RL_SORT_PER], rank[RL_SORT_PER];
#pragma unroll
    for (int j = 0; j < RL_SORT_PER; j++) {
        const long i = i0 + (long)j * RL_NT;
        kk[j] = i < m ? key[i] : -1;
        rank[j] = kk[j] >= 0 ? atomicAdd(&h[kk[j]], 1) : 0;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nk; k += RL_NT)
        if (h[k]) h[k] = atomicAdd(&ctl->cur[k], h[k]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RL_SORT_PER; j++)
        if (kk[j] >= 0) order[h[kk[j]] + rank[j]] = (int32_t)(i0 + (long)j * RL_NT);
}

// The grouped argmin.  blockIdx.x = a run of 256 * QPT sorted queries of one key, blockIdx.y = a slice of that key's
// rows.  FAST: km_dissim16 on prepared rows (every byte of both sides < 16), else km_dissim on the dataset lines.
// Inside a stage the running minimum is a 32-bit key (dis << 6 | 63 - row of the stage; dis < 2^19), folded into the
// 64-bit (dis << 32 | ~position) key once per stage, so neither the slice length nor the position is bounded by it.
template <bool FAST, int QPT>
__global__ __launch_bounds__(RL_NT) void rl_match(const uint8_t *__restrict__ rows, const uint4 *__restrict__ prep,
                                                   const int2 *__restrict__ range, int nk,
                                                   const uint8_t *__restrict__ q80, const uint4 *__restrict__ qprep,
                                                   const int32_t *__restrict__ order, const RlCtl *__restrict__ ctl,
                                                   unsigned long long *__restrict__ akey) {
    constexpr int RW = FAST ? KM_PW / 4 : 5;  // uint4 per row
    constexpr int NW = FAST ? KM_PW : 20;
    __shared__ uint4 st[RL_STAGE * RW];
    __shared__ int s_k;
    const int tid = threadIdx.x, blk = blockIdx.x;
    if (blk >= ctl->boff[nk]) return;
    if (tid == 0) {
        int k = 0;
        while (k + 1 < nk && ctl->boff[k + 1] <= blk) k++;
        s_k = k;
    }
    __syncthreads();
    const int k = s_k;
    const int2 rg = range[k];
    const int per = (rg.y + (int)gridDim.y - 1) / (int)gridDim.y;
    const int r0 = rg.x + (int)blockIdx.y * per, r1 = min(rg.x + rg.y, r0 + per);
    if (per <= 0 || r0 >= r1) return;
    const int q0 = ctl->qoff[k] + (blk - ctl->boff[k]) * (RL_NT * QPT), q1 = min(ctl->qoff[k] + ctl->cnt[k], q0 + RL_NT * QPT);
    int qi[QPT];
    uint32_t x[QPT][NW];
    unsigned long long best[QPT];
#pragma unroll
    for (int j = 0; j < QPT; j++) {
        const int p = q0 + tid + RL_NT * j;
        qi[j] = p < q1 ? order[p] : -1;
        best[j] = ~0ull;
        const uint4 *src = FAST ? qprep + (long)max(qi[j], 0) * RW
                                : reinterpret_cast<const uint4 *>(q80 + (long)max(qi[j], 0) * KM_A);
#pragma unroll
        for (int q = 0; q < RW; q++) {
            const uint4 v = qi[j] >= 0 ? src[q] : make_uint4(0, 0, 0, 0);
            x[j][4 * q] = v.x;
            x[j][4 * q + 1] = v.y;
            x[j][4 * q + 2] = v.z;
            x[j][4 * q + 3] = v.w;
        }
    }
    const uint4 *base = FAST ? prep : reinterpret_cast<const uint4 *>(rows);
    for (int t0 = r0; t0 < r1; t0 += RL_STAGE) {
        const int cnt = min(RL_STAGE, r1 - t0);
        __syncthreads();
        for (int e = tid; e < cnt * RW; e += RL_NT) st[e] = base[(long)t0 * RW + e];
        __syncthreads();
        unsigned b32[QPT];
#pragma unroll
        for (int j = 0; j < QPT; j++) b32[j] = ~0u;
        for (int c = 0; c < cnt; c++) {
            uint32_t r[NW];
#pragma unroll
            for (int q = 0; q < RW; q++) {
                const uint4 v = st[c * RW + q];
                r[4 * q] = v.x;
                r[4 * q + 1] = v.y;
                r[4 * q + 2] = v.z;
                r[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int j = 0; j < QPT; j++) {
                const unsigned d = FAST ? km_dissim16(r, x[j]) : (unsigned)km_dissim(r, x[j]);
                b32[j] = min(b32[j], (d << 6) | (63u - (unsigned)c));
            }
        }
#pragma unroll
        for (int j = 0; j < QPT; j++) {
            const unsigned pos = (unsigned)t0 + 63u - (b32[j] & 63u);
            const unsigned long long key = ((unsigned long long)(b32[j] >> 6) << 32) | (0xFFFFFFFFu - pos);
            best[j] = key < best[j] ? key : best[j];
        }
    }
#pragma unroll
    for (int j = 0; j < QPT; j++)
        if (qi[j] >= 0) atomicMin(&akey[qi[j]], best[j]);
}

// position -> file-order row, dis, and (pix) the tile's new PalPixels = the first 64 bytes of the winning line
__global__ __launch_bounds__(RL_NT) void rl_finish(const unsigned long long *__restrict__ akey,
                                                    const int32_t *__restrict__ key, long m,
                                                    const uint8_t *__restrict__ rows, const int32_t *__restrict__ perm,
                                                    int32_t *__restrict__ idx, unsigned long long *__restrict__ dis,
                                                    uint8_t *__restrict__ pix) {
    for (long i = (long)blockIdx.x * RL_NT + threadIdx.x; i < m; i += (long)gridDim.x * RL_NT) {
        const unsigned long long a = akey[i];
        const bool hit = key[i] >= 0 && a != ~0ull;
        const unsigned pos = 0xFFFFFFFFu - (unsigned)(a & 0xFFFFFFFFull);
        if (idx) idx[i] = hit ? (perm ? perm[pos] : (int32_t)pos) : -1;
        if (dis) dis[i] = hit ? a >> 32 : ~0ull;
        if (pix && hit) {
            const uint4 *s = reinterpret_cast<const uint4 *>(rows + (long)pos * KM_A);
            uint4 *d = reinterpret_cast<uint4 *>(pix + i * 64);
#pragma unroll
            for (int q = 0; q < 4; q++) d[q] = s[q];
        }
    }
}

__global__ __launch_bounds__(RL_NT) void rl_fill_none(long m, int32_t *idx, unsigned long long *dis) {
    for (long i = (long)blockIdx.x * RL_NT + threadIdx.x; i < m; i += (long)gridDim.x * RL_NT) {
        if (idx) idx[i] = -1;
        if (dis) dis[i] = ~0ull;
    }
}

// ---- host side ----
namespace {

unsigned grid_for(long n, long cap = 8192) { return (unsigned)std::max<long>(1, std::min<long>(cap, (n + RL_NT - 1) / RL_NT)); }

struct RowSet {
    const uint8_t *rows;  // [R][80]
    const uint4 *prep;    // [R][KM_PW / 4]
    const int32_t *perm;  // position -> reported row (null: the position)
    const int2 *range;    // device [nk]: (first position, rows) of every key; key nk - 1 = all rows
    int nk;
    bool bad;  // some byte >= 16
};

struct Pass {  // scratch of one pass of at most cap queries
    long cap = 0;
    int32_t *key = nullptr, *order = nullptr;
    unsigned long long *akey = nullptr;
    RlCtl *ctl = nullptr;
    bool alloc(Blocks &B, long c) {
        cap = c;
        return B.get(key, (size_t)c * 4) && B.get(order, (size_t)c * 4) && B.get(akey, (size_t)c * 8) &&
               B.get(ctl, sizeof(RlCtl));
    }
};

template <bool FAST, int QPT>
void launch_match(dim3 grid, hipStream_t st, const RowSet &R, const uint8_t *q80, const uint4 *qprep, const Pass &P) {
    hipLaunchKernelGGL((rl_match<FAST, QPT>), grid, dim3(RL_NT), 0, st, R.rows, R.prep, R.range, R.nk, q80, qprep,
                       (const int32_t *)P.order, (const RlCtl *)P.ctl, P.akey);
}

// One pass: m queries (lines q80, prepared qprep, group grp; P.ctl zeroed and its bad flag set by the caller's row
// kernel on this stream) against R.  Synchronises the stream once (the "bad" flag and the block count).
int match_pass(const RowSet &R, const uint8_t *q80, const uint4 *qprep, const int32_t *grp, const uint8_t *active,
               long m, const Pass &P, int32_t *idx, unsigned long long *dis, uint8_t *pix, hipStream_t st,
               long long *pairs) {
    const int qpt = g_rl_qpt.load() == 2 ? 2 : 1;
    {
        KTimer tm("reload_sort", st);
        hipLaunchKernelGGL(rl_keys, dim3(grid_for(m, 1024)), dim3(RL_NT), 0, st, grp, active, m, R.range, R.nk, P.key,
                           P.akey, P.ctl);
        hipLaunchKernelGGL(rl_scan, dim3(1), dim3(64), 0, st, P.ctl, R.range, R.nk, RL_NT * qpt);
        hipLaunchKernelGGL(rl_scatter, dim3((unsigned)((m + RL_NT * RL_SORT_PER - 1) / (RL_NT * RL_SORT_PER))),
                           dim3(RL_NT), 0, st, (const int32_t *)P.key, m, R.nk, P.ctl, P.order);
    }
    TILER_HIP_CHECK(hipGetLastError());
    RlHead h;
    TILER_HIP_CHECK(hipMemcpyAsync(&h, P.ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    TILER_HIP_CHECK(hipStreamSynchronize(st));
    if (pairs) *pairs += (long long)h.pairs;
    if (h.nblk > 0) {
        // few query blocks: slice the rows so that the launch still fills the device
        const int forced = g_rl_slices.load();
        const int slices = forced > 0 ? forced : h.nblk >= 2048 ? 1 : std::min(16, (2048 + h.nblk - 1) / h.nblk);
        const dim3 grid((unsigned)h.nblk, (unsigned)slices);
        const bool fast = !R.bad && !h.bad;
        KTimer tm("reload_match", st);
        if (fast && qpt == 2)
            launch_match<true, 2>(grid, st, R, q80, qprep, P);
        else if (fast)
            launch_match<true, 1>(grid, st, R, q80, qprep, P);
        else if (qpt == 2)
            launch_match<false, 2>(grid, st, R, q80, qprep, P);
        else
            launch_match<false, 1>(grid, st, R, q80, qprep, P);
    }
    {
        KTimer tm("reload_gather", st);
        hipLaunchKernelGGL(rl_finish, dim3(grid_for(m)), dim3(RL_NT), 0, st, (const unsigned long long *)P.akey,
                           (const int32_t *)P.key, m, R.rows, R.perm, idx, dis, pix);
    }
    TILER_HIP_CHECK(hipGetLastError());
    return 0;
}

long pass_size(long m) {
    const long c = g_rl_chunk.load();
    return std::max<long>(1, std::min<long>(m, c > 0 ? c : RL_CHUNK));
}

}  // namespace

struct Tileset {
    int dev = 0;
    long n = 0;
    int palsize = 16;
    uint8_t *rows = nullptr;  // [2n][80]
    uint4 *prep = nullptr;    // [2n][KM_PW / 4]
    int32_t *perm = nullptr;  // [2n]
    int2 *range = nullptr;    // [RL_SIGNI + 1]
    bool bad = false;
};

int tileset_device(const Tileset *ts) { return ts->dev; }
long tileset_rows(const Tileset *ts) { return ts->n; }

void tileset_destroy(Tileset *ts) {
    if (!ts) return;
    (void)hipDeviceSynchronize();
    dfree(ts->rows);
    dfree(ts->prep);
    dfree(ts->perm);
    dfree(ts->range);
    delete ts;
}

Tileset *tileset_load(const uint8_t *raw, long n, int file_palsize, int palsize) {
    if (n < 0 || (n > 0 && !raw) || n >= (1L << 30) || palsize <= 0 || palsize > 256 || file_palsize <= 0 ||
        file_palsize > 256) {
        set_error("tileset_load: invalid arguments (need 0 <= n < 2^30, palette sizes in 1..256)");
        return nullptr;
    }
    Tileset *ts = new Tileset;
    ts->n = n;
    ts->palsize = palsize;
    (void)hipGetDevice(&ts->dev);
    if (n == 0) return ts;
    hipStream_t st = nullptr;
    if (stream_get(&st) != hipSuccess) {
        set_error("tileset_load: no stream");
        delete ts;
        return nullptr;
    }
    bool ok = false;
    do {
        Blocks tmp(st);
        uint8_t *d_raw = nullptr;
        int32_t *d_signi = nullptr;
        unsigned *d_bad = nullptr;
        if (dmalloc((void **)&ts->rows, (size_t)2 * n * KM_A) != hipSuccess ||
            dmalloc((void **)&ts->prep, (size_t)2 * n * KM_PW * 4) != hipSuccess ||
            dmalloc((void **)&ts->perm, (size_t)2 * n * 4) != hipSuccess ||
            dmalloc((void **)&ts->range, (RL_SIGNI + 1) * sizeof(int2)) != hipSuccess ||
            !tmp.get(d_raw, (size_t)n * 64) || !tmp.get(d_signi, (size_t)n * 4) || !tmp.get(d_bad, 4))
            break;
        if (hipMemcpyAsync(d_raw, raw, (size_t)n * 64, hipMemcpyHostToDevice, st) != hipSuccess) break;
        if (hipMemsetAsync(d_bad, 0, 4, st) != hipSuccess) break;
        {
            KTimer tm("reload_rows", st);
            // a file of the clip's own palette size needs no rescale: (v * p) div p = v
            hipLaunchKernelGGL(rl_rows, dim3(grid_for(n)), dim3(RL_NT), 0, st, (const uint8_t *)d_raw, n, palsize,
                               file_palsize == palsize ? 0 : file_palsize, palsize, ts->rows, ts->prep, d_signi, d_bad);
        }
        if (hipGetLastError() != hipSuccess) break;
        std::vector<int32_t> sg(n), perm(2 * n);
        unsigned bad = 0;
        if (hipMemcpyAsync(sg.data(), d_signi, (size_t)n * 4, hipMemcpyDeviceToHost, st) != hipSuccess) break;
        if (hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st) != hipSuccess) break;
        if (hipStreamSynchronize(st) != hipSuccess) break;
        ts->bad = bad != 0;
        // buckets in file order (SigniIndices main.pas:4442-4443): a stable counting sort over 65 values
        int2 range[RL_SIGNI + 1];
        int cnt[RL_SIGNI] = {};
        bool in_range = true;
        for (long i = 0; i < n; i++) {
            if (sg[i] < 0 || sg[i] >= RL_SIGNI) {
                in_range = false;
                break;
            }
            cnt[sg[i]]++;
        }
        if (!in_range) break;
        int off = (int)n;
        int cur[RL_SIGNI];
        for (int k = 0; k < RL_SIGNI; k++) {
            range[k] = make_int2(off, cnt[k]);
            cur[k] = off;
            off += cnt[k];
        }
        range[RL_SIGNI] = make_int2(0, (int)n);
        for (long i = 0; i < n; i++) {
            perm[i] = (int32_t)i;
            perm[cur[sg[i]]++] = (int32_t)i;
        }
        if (hipMemcpyAsync(ts->perm, perm.data(), (size_t)2 * n * 4, hipMemcpyHostToDevice, st) != hipSuccess) break;
        if (hipMemcpyAsync(ts->range, range, sizeof(range), hipMemcpyHostToDevice, st) != hipSuccess) break;
        hipLaunchKernelGGL(rl_bucket_rows, dim3(grid_for(n)), dim3(RL_NT), 0, st, ts->rows, ts->prep,
                           (const int32_t *)ts->perm, n);
        if (hipGetLastError() != hipSuccess) break;
        if (hipStreamSynchronize(st) != hipSuccess) break;  // perm / range are host stack and vectors
        ok = true;
    } while (0);
    stream_put(st);
    if (!ok) {
        set_error("tileset_load: HIP failure");
        tileset_destroy(ts);
        return nullptr;
    }
    return ts;
}

int tileset_match_dev(Tileset *ts, uint8_t *d_palpix, const uint8_t *d_active, long nt, int32_t *d_idx,
                      uint64_t *d_dis, hipStream_t st) {
    if (!ts || nt < 0 || (nt > 0 && (!d_palpix || !d_active)) || nt >= (1L << 31)) {
        set_error("tileset_match: invalid arguments");
        return -1;
    }
    if (((uintptr_t)d_palpix & 15) != 0) {
        set_error("tileset_match: palpix must be 16-byte aligned");
        return -1;
    }
    g_rl_pairs = 0;
    if (nt == 0) return 0;
    if (ts->n == 0) {  // GetMinMatchingDissim over no rows: -1, the tiles stay as they are
        hipLaunchKernelGGL(rl_fill_none, dim3(grid_for(nt)), dim3(RL_NT), 0, st, nt, d_idx,
                           (unsigned long long *)d_dis);
        TILER_HIP_CHECK(hipGetLastError());
        TILER_HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }
    const long cap = pass_size(nt);
    Blocks B(st);
    Pass P;
    uint8_t *q80 = nullptr;
    uint4 *qprep = nullptr;
    int32_t *signi = nullptr;
    if (!P.alloc(B, cap) || !B.get(q80, (size_t)cap * KM_A) || !B.get(qprep, (size_t)cap * KM_PW * 4) ||
        !B.get(signi, (size_t)cap * 4)) {
        set_error("tileset_match: out of device memory");
        return -1;
    }
    const RowSet R{ts->rows, ts->prep, ts->perm, ts->range, RL_SIGNI + 1, ts->bad};
    long long pairs = 0;
    for (long c0 = 0; c0 < nt; c0 += cap) {
        const long m = std::min(cap, nt - c0);
        TILER_HIP_CHECK(hipMemsetAsync(P.ctl, 0, sizeof(RlCtl), st));
        {
            KTimer tm("reload_rows", st);
            hipLaunchKernelGGL(rl_rows, dim3(grid_for(m)), dim3(RL_NT), 0, st, (const uint8_t *)d_palpix + c0 * 64, m, 0,
                               0, ts->palsize, q80, qprep, signi, &P.ctl->h.bad);
        }
        if (match_pass(R, q80, qprep, signi, d_active + c0, m, P, d_idx ? d_idx + c0 : nullptr,
                       d_dis ? (unsigned long long *)d_dis + c0 : nullptr, d_palpix + c0 * 64, st, &pairs))
            return -1;
    }
    TILER_HIP_CHECK(hipStreamSynchronize(st));
    g_rl_pairs = pairs;
    return 0;
}

int min_dissim_groups_dev(const uint8_t *d_rows, long n, const int32_t *grp_off, int ngroups, const uint8_t *d_items,
                          const int32_t *d_item_grp, long m, int32_t *d_idx, uint64_t *d_dis, hipStream_t st) {
    if (n < 0 || m < 0 || ngroups < 0 || ngroups >= RL_MAXK || (ngroups > 0 && !grp_off) || (n > 0 && !d_rows) ||
        (m > 0 && (!d_items || !d_item_grp)) || n >= (1L << 31) || m >= (1L << 31)) {
        set_error("min_matching_dissim_groups: invalid arguments (at most 1023 groups)");
        return -1;
    }
    if ((((uintptr_t)d_rows | (uintptr_t)d_items) & 15) != 0) {
        set_error("min_matching_dissim_groups: rows and items must be 16-byte aligned");
        return -1;
    }
    for (int g = 0; g < ngroups; g++)
        if (grp_off[g] < 0 || grp_off[g + 1] < grp_off[g] || grp_off[g + 1] > n) {
            set_error("min_matching_dissim_groups: grp_off must ascend within [0, n]");
            return -1;
        }
    g_rl_pairs = 0;
    if (m == 0) return 0;
    if (n == 0) {
        hipLaunchKernelGGL(rl_fill_none, dim3(grid_for(m)), dim3(RL_NT), 0, st, m, d_idx, (unsigned long long *)d_dis);
        TILER_HIP_CHECK(hipGetLastError());
        TILER_HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }
    const long cap = pass_size(m);
    const int nk = ngroups + 1;
    Blocks B(st);
    Pass P;
    uint4 *prep = nullptr, *qprep = nullptr;
    int2 *range = nullptr;
    unsigned *d_bad = nullptr;
    if (!P.alloc(B, cap) || !B.get(prep, (size_t)n * KM_PW * 4) || !B.get(qprep, (size_t)cap * KM_PW * 4) ||
        !B.get(range, (size_t)nk * sizeof(int2)) || !B.get(d_bad, 4)) {
        set_error("min_matching_dissim_groups: out of device memory");
        return -1;
    }
    std::vector<int2> h_range(nk);
    for (int g = 0; g < ngroups; g++) h_range[g] = make_int2(grp_off[g], grp_off[g + 1] - grp_off[g]);
    h_range[ngroups] = make_int2(0, (int)n);
    unsigned bad = 0;
    TILER_HIP_CHECK(hipMemcpyAsync(range, h_range.data(), (size_t)nk * sizeof(int2), hipMemcpyHostToDevice, st));
    TILER_HIP_CHECK(hipMemsetAsync(d_bad, 0, 4, st));
    {
        KTimer tm("reload_rows", st);
        hipLaunchKernelGGL(rl_prep80, dim3(grid_for(n)), dim3(RL_NT), 0, st, d_rows, n, prep, d_bad);
    }
    TILER_HIP_CHECK(hipGetLastError());
    TILER_HIP_CHECK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    TILER_HIP_CHECK(hipStreamSynchronize(st));
    const RowSet R{d_rows, prep, nullptr, range, nk, bad != 0};
    long long pairs = 0;
    for (long c0 = 0; c0 < m; c0 += cap) {
        const long mc = std::min(cap, m - c0);
        TILER_HIP_CHECK(hipMemsetAsync(P.ctl, 0, sizeof(RlCtl), st));
        {
            KTimer tm("reload_rows", st);
            hipLaunchKernelGGL(rl_prep80, dim3(grid_for(mc)), dim3(RL_NT), 0, st, d_items + c0 * KM_A, mc, qprep,
                               &P.ctl->h.bad);
        }
        if (match_pass(R, d_items + c0 * KM_A, qprep, d_item_grp + c0, nullptr, mc, P, d_idx ? d_idx + c0 : nullptr,
                       d_dis ? (unsigned long long *)d_dis + c0 : nullptr, nullptr, st, &pairs))
            return -1;
    }
    TILER_HIP_CHECK(hipStreamSynchronize(st));
    g_rl_pairs = pairs;
    return 0;
}

// ---- host-buffer forms ----
int tileset_match_host(Tileset *ts, uint8_t *palpix, const uint8_t *active, long nt, int32_t *idx, uint64_t *dis) {
    if (!ts || nt < 0 || (nt > 0 && (!palpix || !active))) {
        set_error("tileset_match: invalid arguments");
        return -1;
    }
    if (nt == 0) return 0;
    HostStage s("tileset_match");
    uint8_t *d_pix = s.inout(palpix, (size_t)nt * 64);
    const uint8_t *d_act = s.in(active, (size_t)nt);
    int32_t *d_idx = s.out(idx, (size_t)nt);
    uint64_t *d_dis = s.out(dis, (size_t)nt);
    if (!s.ok() || tileset_match_dev(ts, d_pix, d_act, nt, d_idx, d_dis, s.stream())) return -1;
    return s.finish();
}

int min_dissim_groups_host(const uint8_t *rows, long n, const int32_t *grp_off, int ngroups, const uint8_t *items,
                           const int32_t *item_grp, long m, int32_t *idx, uint64_t *dis) {
    if (n < 0 || m < 0 || (n > 0 && !rows) || (m > 0 && (!items || !item_grp))) {
        set_error("min_matching_dissim_groups: invalid arguments");
        return -1;
    }
    if (m == 0) return 0;
    HostStage s("min_matching_dissim_groups");
    const uint8_t *d_rows = s.in(rows, (size_t)n * KM_A), *d_items = s.in(items, (size_t)m * KM_A);
    const int32_t *d_grp = s.in(item_grp, (size_t)m);
    int32_t *d_idx = s.out(idx, (size_t)m);
    uint64_t *d_dis = s.out(dis, (size_t)m);
    if (!s.ok() || min_dissim_groups_dev(d_rows, n, grp_off, ngroups, d_items, d_grp, m, d_idx, d_dis, s.stream()))
        return -1;
    return s.finish();
}

int reload_debug(long chunk, int qpt, int slices) {
    if (chunk < 0 || qpt < 0 || qpt > 2 || slices < 0 || slices > 64) {
        set_error("tiler_debug_reload: chunk >= 0, qpt in 0..2, slices in 0..64");
        return -1;
    }
    g_rl_chunk = chunk;
    g_rl_qpt = qpt;
    g_rl_slices = slices;
    return 0;
}

long long reload_last_pairs() { return g_rl_pairs.load(); }

}  // namespace tiler
