// lzma_match.hip -- the match search of the LZMA encoder (lzma_alone.cpp, MatchFinder::best) for every position of a
// set of streams at once, on gfx950.  best(p) depends on the buffer and p alone (every position below p is in the
// chains by the time the parse asks for p), so the chains can be replaced by a sort:
//   hash   a lane per position: key = stream << 18 | the 18-bit hash of its three bytes, value = the position; a
//          position with fewer than three bytes left in its stream gets the key past every stream's (it is no
//          candidate and its entry is 0);
//   sort   one stable hipcub::DeviceRadixSort::SortPairs over the key's used bits: positions of one bucket of one
//          stream end up side by side, ascending;
//   find   the candidates of the position at sorted rank r are ranks r - 1 .. r - 24 while the key stays the same:
//          the chain walk's order, nearest first.  32 lanes per position (24 at work, 2 positions per wave): lane j
//          takes candidate j, measures its match length 16 bytes per step, and the group reduces in the walk's order:
//          the first lane whose length is >= 128 or == lim ends the walk, the result is the first maximum up to it.
//          (The host's first-byte test only skips candidates that cannot be strictly longer, and a candidate past
//          the dictionary ends the walk: both distances and keys are monotone along the lanes, so each lane decides
//          for itself whether the walk reaches it.)
// Byte strings start at any alignment: they are read as 16-byte aligned chunks, two per side kept in registers, and a
// 16-byte window is cut out of each pair with dword selects and v_alignbyte_b32.  A chunk is loaded only if it holds
// a byte that the comparison needs, so no load touches a page that the caller's buffer does not.
// Scratch: one stream-ordered block per call: keys and values double-buffered (16 bytes per raw byte of the largest
// batch), the sort's own storage and the batches' stream offsets.  Whole streams are taken in batches that fit
// budget / 16 bytes (LM_BUDGET, 1 GiB -> 2^26 raw bytes; tiler_debug_lzma_match); a stream that alone exceeds that is
// left to the host finder.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): hash 8 VGPRs, find 45; no LDS, no spills, no
// scratch, occupancy 8 waves per SIMD for both.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/tiler_ann.h"
#include "lzma_match.hpp"
#include "stage.hpp"

namespace tiler {

namespace {

constexpr int LM_HASH_BITS = 18, LM_DEPTH = 24, LM_NICE = 128, LM_MAX_LEN = 273, LM_LEN_BITS = 9;
constexpr uint32_t LM_MAX_DICT = 1u << 21;
constexpr int64_t LM_BUDGET = 1ll << 30;  // bytes of scratch a call may hold: 16 per raw byte of a batch
constexpr int LM_MAX_STREAMS = 8191;      // per batch: the stream number sits above the hash, in a 32-bit key
constexpr int LM_THREADS = 256, LM_GROUP = 32, LM_PER_BLOCK = LM_THREADS / LM_GROUP;

std::atomic<int64_t> g_lm_budget{LM_BUDGET};

// off[0 .. nb]: the batch's stream borders from 0 to N; the stream of position g: the last one that starts at or
// before g (an empty stream shares its start with the next one and is never the answer)
__device__ __forceinline__ int lm_stream_of(const uint32_t *__restrict__ off, int nb, uint32_t g) {
    int lo = 0, hi = nb;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(LM_THREADS) void lzma_hash_kernel(const uint8_t *__restrict__ src,
                                                               const uint32_t *__restrict__ off, int nb, uint32_t N,
                                                               uint32_t *__restrict__ keys,
                                                               uint32_t *__restrict__ vals) {
    const uint32_t g = blockIdx.x * LM_THREADS + threadIdx.x;
    if (g >= N) return;
    const int s = lm_stream_of(off, nb, g);
    uint32_t key = (uint32_t)nb << LM_HASH_BITS;
    if (g + 3 <= off[s + 1]) {
        const uint32_t h = ((uint32_t)src[g] * 0x9E3779B1u ^ (uint32_t)src[g + 1] * 0x85EBCA77u ^
                            (uint32_t)src[g + 2] * 0xC2B2AE3Du) >> (32 - LM_HASH_BITS);
        key = (uint32_t)s << LM_HASH_BITS | h;
    }
    keys[g] = key;
    vals[g] = g;
}

// the aligned 16 bytes at c, if they hold a byte below `end` (the last byte the comparison may need)
__device__ __forceinline__ uint4 lm_chunk(const uint8_t *c, const uint8_t *end) {
    return c < end ? *reinterpret_cast<const uint4 *>(c) : make_uint4(0, 0, 0, 0);
}

// the 16 bytes that start sh (0..15) bytes into the 32 of lo, hi
__device__ __forceinline__ void lm_window(const uint4 &lo, const uint4 &hi, uint32_t sh, uint32_t out[4]) {
    const bool s2 = sh & 8, s1 = sh & 4;
    const uint32_t u0 = s2 ? lo.z : lo.x, u1 = s2 ? lo.w : lo.y, u2 = s2 ? hi.x : lo.z, u3 = s2 ? hi.y : lo.w,
                   u4 = s2 ? hi.z : hi.x, u5 = s2 ? hi.w : hi.y;
    const uint32_t t0 = s1 ? u1 : u0, t1 = s1 ? u2 : u1, t2 = s1 ? u3 : u2, t3 = s1 ? u4 : u3, t4 = s1 ? u5 : u4;
    const uint32_t bs = sh & 3;
    out[0] = __builtin_amdgcn_alignbyte(t1, t0, bs);
    out[1] = __builtin_amdgcn_alignbyte(t2, t1, bs);
    out[2] = __builtin_amdgcn_alignbyte(t3, t2, bs);
    out[3] = __builtin_amdgcn_alignbyte(t4, t3, bs);
}

// the number of equal bytes of src[q ..] and src[p ..], at most lim (q < p; p + lim is inside the stream)
__device__ __forceinline__ uint32_t lm_match_len(const uint8_t *__restrict__ src, uint32_t q, uint32_t p,
                                                 uint32_t lim) {
    const uint8_t *pa = src + q, *pb = src + p;
    const uint8_t *ea = pa + lim, *eb = pb + lim;
    const uint32_t sa = (uint32_t)((uintptr_t)pa & 15), sb = (uint32_t)((uintptr_t)pb & 15);
    const uint8_t *ca = pa - sa, *cb = pb - sb;
    uint4 alo = lm_chunk(ca, ea), blo = lm_chunk(cb, eb);
    uint32_t l = 0;
    for (;;) {
        ca += 16;
        cb += 16;
        const uint4 ahi = lm_chunk(ca, ea), bhi = lm_chunk(cb, eb);
        uint32_t a[4], b[4];
        lm_window(alo, ahi, sa, a);
        lm_window(blo, bhi, sb, b);
        const uint32_t x0 = a[0] ^ b[0], x1 = a[1] ^ b[1], x2 = a[2] ^ b[2], x3 = a[3] ^ b[3];
        if (x0 | x1 | x2 | x3) {
            const uint32_t x = x0 ? x0 : x1 ? x1 : x2 ? x2 : x3;
            l += (x0 ? 0u : x1 ? 4u : x2 ? 8u : 12u) + ((uint32_t)(__ffs((int)x) - 1) >> 3);
            break;
        }
        l += 16;
        if (l >= lim) break;
        alo = ahi;
        blo = bhi;
    }
    return min(l, lim);
}

__global__ __launch_bounds__(LM_THREADS) void lzma_find_kernel(const uint8_t *__restrict__ src,
                                                               const uint32_t *__restrict__ keys,
                                                               const uint32_t *__restrict__ vals,
                                                               const uint32_t *__restrict__ off, int nb, uint32_t N,
                                                               uint32_t dict, uint32_t *__restrict__ table) {
    const uint32_t r = blockIdx.x * LM_PER_BLOCK + (threadIdx.x >> 5);
    const int j = threadIdx.x & (LM_GROUP - 1);
    const bool active = r < N;
    uint32_t p = 0, q = 0, lim = 0, l = 0;
    bool valid = false;
    if (active) {
        const uint32_t key = keys[r];
        p = vals[r];
        if (key != (uint32_t)nb << LM_HASH_BITS && j < LM_DEPTH && r > (uint32_t)j) {
            const uint32_t rc = r - 1 - (uint32_t)j;
            if (keys[rc] == key) {
                q = vals[rc];
                valid = p - q <= dict;
            }
            lim = min((uint32_t)LM_MAX_LEN, off[(key >> LM_HASH_BITS) + 1] - p);
        }
    }
    if (valid) l = lm_match_len(src, q, p, lim);
    // the walk's order: the first lane that ends it, then the first maximum up to that lane
    const unsigned long long bal = __ballot(valid && (l >= (uint32_t)LM_NICE || l == lim));
    const uint32_t mine = (uint32_t)(bal >> (threadIdx.x & 32));
    const int last = mine ? __ffs((int)mine) - 1 : LM_GROUP - 1;
    uint32_t score = valid && j <= last ? l << 5 | (uint32_t)(LM_GROUP - 1 - j) : 0;
    for (int d = LM_GROUP / 2; d; d >>= 1) score = max(score, (uint32_t)__shfl_xor((int)score, d, LM_GROUP));
    const uint32_t bl = score >> 5;
    const uint32_t qb = (uint32_t)__shfl((int)q, LM_GROUP - 1 - (int)(score & 31), LM_GROUP);
    if (active && j == 0) table[p] = bl >= 2 ? bl | (p - qb - 1) << LM_LEN_BITS : 0;
}

int lm_fail(const std::string &what) {
    set_error("lzma_match: " + what);
    return -1;
}

struct Batch {
    int s0, s1;       // streams [s0, s1)
    size_t off_at;    // where its nb + 1 borders start in the offsets block
};

size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

int64_t lzma_match_debug(int64_t budget_bytes) {
    if (budget_bytes < 0 || (budget_bytes > 0 && budget_bytes < 1024)) {
        set_error("tiler_debug_lzma_match: budget_bytes is 0 (the default) or at least 1024");
        return -1;
    }
    return g_lm_budget.exchange(budget_bytes ? budget_bytes : LM_BUDGET);
}

int lzma_match_table_dev(const uint8_t *d_src, const int64_t *raw_off, int S, uint32_t dict, uint32_t *d_table,
                         void *stream, std::vector<uint8_t> *has) {
    hipStream_t st = (hipStream_t)stream;
    if (S < 0 || (S && !raw_off)) return lm_fail("S < 0 or raw_off is null");
    if (dict < 4096 || dict > LM_MAX_DICT)
        return lm_fail("dictionary " + std::to_string(dict) + " outside [4096, 2^21]: a table holds distances below 2^21");
    if (has) has->assign((size_t)S, 1);
    if (S == 0) return 0;
    if (raw_off[0] != 0) return lm_fail("raw_off[0] must be 0");
    for (int k = 0; k < S; k++)
        if (raw_off[k + 1] < raw_off[k]) return lm_fail("raw_off must not decrease (stream " + std::to_string(k) + ")");
    if (raw_off[S] && (!d_src || !d_table)) return lm_fail("a null array");
    if ((uintptr_t)d_table % 4) return lm_fail("the table is not 4-byte aligned");

    // whole streams in batches of at most cap bytes and LM_MAX_STREAMS streams; a longer stream closes the batch
    const int64_t cap = std::min<int64_t>(g_lm_budget.load() / 16, INT32_MAX);
    std::vector<Batch> batches;
    std::vector<uint32_t> offs;
    int left_out = 0;
    size_t max_n = 0;
    for (int k = 0; k < S;) {
        if (raw_off[k + 1] - raw_off[k] > cap) {
            if (has) (*has)[(size_t)k] = 0;
            left_out++;
            k++;
            continue;
        }
        int e = k;
        while (e < S && e - k < LM_MAX_STREAMS && raw_off[e + 1] - raw_off[k] <= cap) e++;
        if (raw_off[e] > raw_off[k]) {
            batches.push_back({k, e, offs.size()});
            for (int i = k; i <= e; i++) offs.push_back((uint32_t)(raw_off[i] - raw_off[k]));
            max_n = std::max(max_n, (size_t)(raw_off[e] - raw_off[k]));
        }
        k = e;
    }
    if (batches.empty()) return left_out;

    auto key_bits = [](int nb) {  // the bits of the last key, nb << 18
        int end_bit = LM_HASH_BITS;
        while ((nb >> (end_bit - LM_HASH_BITS)) != 0) end_bit++;
        return end_bit;
    };
    size_t tmp_bytes = 0;  // the sort's own storage: the most any batch asks for
    for (const Batch &b : batches) {
        hipcub::DoubleBuffer<uint32_t> dk(nullptr, nullptr), dv(nullptr, nullptr);
        size_t t = 0;
        TILER_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, t, dk, dv, (int)(raw_off[b.s1] - raw_off[b.s0]), 0,
                                                           key_bits(b.s1 - b.s0), st));
        tmp_bytes = std::max(tmp_bytes, t);
    }
    const size_t arr = up256(max_n * 4), o_off = 4 * arr, o_tmp = o_off + up256(offs.size() * 4),
                 total = o_tmp + up256(tmp_bytes);
    char *base = nullptr;
    TILER_HIP_CHECK(hipMallocAsync((void **)&base, total, st));
    struct Free {
        char *b;
        hipStream_t s;
        ~Free() { (void)hipFreeAsync(b, s); }
    } free_it{base, st};
    uint32_t *k0 = (uint32_t *)base, *k1 = (uint32_t *)(base + arr), *v0 = (uint32_t *)(base + 2 * arr),
             *v1 = (uint32_t *)(base + 3 * arr), *d_off = (uint32_t *)(base + o_off);
    // the borders are host memory of this call: on the device before the call goes on
    TILER_HIP_CHECK(hipMemcpyAsync(d_off, offs.data(), offs.size() * 4, hipMemcpyHostToDevice, st));
    TILER_HIP_CHECK(hipStreamSynchronize(st));

    for (const Batch &b : batches) {
        const int nb = b.s1 - b.s0;
        const uint32_t N = (uint32_t)(raw_off[b.s1] - raw_off[b.s0]);
        const uint8_t *src = d_src + raw_off[b.s0];
        uint32_t *table = d_table + raw_off[b.s0];
        const uint32_t *off = d_off + b.off_at;
        {
            KTimer tm("lzma_match_hash", st);
            hipLaunchKernelGGL(lzma_hash_kernel, dim3((N + LM_THREADS - 1) / LM_THREADS), dim3(LM_THREADS), 0, st, src,
                               off, nb, N, k0, v0);
        }
        TILER_HIP_CHECK(hipGetLastError());
        hipcub::DoubleBuffer<uint32_t> kb(k0, k1), vb(v0, v1);
        const int end_bit = key_bits(nb);
        {
            KTimer tm("lzma_match_sort", st);
            size_t ts = tmp_bytes;
            TILER_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(base + o_tmp, ts, kb, vb, (int)N, 0, end_bit, st));
        }
        {
            KTimer tm("lzma_match_find", st);
            hipLaunchKernelGGL(lzma_find_kernel, dim3((N + LM_PER_BLOCK - 1) / LM_PER_BLOCK), dim3(LM_THREADS), 0, st,
                               src, (const uint32_t *)kb.Current(), (const uint32_t *)vb.Current(), off, nb, N, dict,
                               table);
        }
        TILER_HIP_CHECK(hipGetLastError());
    }
    return left_out;
}

int lzma_match_table_host(const uint8_t *src, size_t n, uint32_t dict, uint32_t *table) {
    if ((!src || !table) && n) return lm_fail("a null array");
    if (dict < 4096 || dict > LM_MAX_DICT)
        return lm_fail("dictionary " + std::to_string(dict) + " outside [4096, 2^21]: a table holds distances below 2^21");
    if (n == 0) return 0;
    if ((int64_t)n > std::min<int64_t>(g_lm_budget.load() / 16, INT32_MAX))  // the fallback: the host finder
        return tiler_lzma_match_table(src, n, dict, table);
    HostStage hs("lzma_match");
    const uint8_t *d_src = hs.in(src, n);
    uint32_t *d_table = hs.out(table, n);
    if (!hs.ok()) return -1;
    const int64_t off[2] = {0, (int64_t)n};
    if (lzma_match_table_dev(d_src, off, 1, dict, d_table, hs.stream(), nullptr) != 0) return -1;
    return hs.finish();
}

}  // namespace tiler
