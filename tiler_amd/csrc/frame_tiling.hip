// frame_tiling.hip -- FrameTiling's batch stage: RGB tiles -> descriptors -> nearest-neighbour search -> tilemap items.
#include "frame_tiling.hpp"

#include <atomic>

#include "nn_search.hpp"
#include "orbit.hpp"
#include "psyv.hpp"

namespace tiler {

// Flat tiles (one colour: every Haar coefficient but the DC is 0, so only isotypic block 0 of q' is nonzero) are
// moved to the end of the batch, where whole shortlist workgroups of them run 3 of the 12 k-steps (orbit_search).
// A: per tile flag + per-block count of the others (this kernel, or fused with the dedupe's hash below); B: one
// workgroup scans the block counts; C: stable positions, which the query kernel reads through; D: the outputs back.
__global__ __launch_bounds__(256) void ft_flat_flag_kernel(const int32_t *__restrict__ rgb, int Q, uint8_t *flag,
                                                           int *bcnt) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    int other = 0;
    if (i < Q) {
        const int4 *t = reinterpret_cast<const int4 *>(rgb + i * 64);
        const int c0 = rgb[i * 64];
        bool flat = true;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int4 v = t[k];
            flat = flat && v.x == c0 && v.y == c0 && v.z == c0 && v.w == c0;
        }
        flag[i] = flat ? 1 : 0;
        other = flat ? 0 : 1;
    }
    const int c = __syncthreads_count(other);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = c;
}

// (one workgroup per row of counts: bcnt [gridDim.x][nb], total [gridDim.x])
__global__ __launch_bounds__(1024) void ft_flat_scan_kernel(int *bcnt, int nb, int *total) {
    __shared__ int sc[1024];
    __shared__ int carry;
    bcnt += (size_t)blockIdx.x * nb;
    total += blockIdx.x;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int b = b0 + threadIdx.x;
        const int v = b < nb ? bcnt[b] : 0;
        sc[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int u = threadIdx.x >= o ? sc[threadIdx.x - o] : 0;
            __syncthreads();
            sc[threadIdx.x] += u;
            __syncthreads();
        }
        if (b < nb) bcnt[b] = carry + sc[threadIdx.x] - v;  // exclusive prefix
        __syncthreads();
        if (threadIdx.x == 1023) carry += sc[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// C: the selected tiles -- the representatives (rep_of[i] == i), or every tile (rep_of null) -- take stable positions,
// non-flat first, flat after, each in tile order (a block scan over the scanned block counts: no atomics, so the
// layout is deterministic).  boff_nf / boff_fl: the selected non-flat / flat tiles before each block; boff_fl null:
// every tile is selected, so the flat ones before a block are the rest of its 256 * block tiles.  total_nf: the
// selected non-flat tiles.  perm[pos] = tile (the query kernel reads tile perm[pos], no copy of the RGB), pos[tile].
__global__ __launch_bounds__(256) void ft_place_kernel(int Q, const uint8_t *__restrict__ flag,
                                                       const int *__restrict__ rep_of, const int *__restrict__ boff_nf,
                                                       const int *__restrict__ boff_fl,
                                                       const int *__restrict__ total_nf, int *perm, int *pos) {
    __shared__ int sc[256];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const bool sel = i < Q && (!rep_of || rep_of[i] == (int)i);
    const int f = sel ? flag[i] : 0;
    const int mine = sel ? (f ? 1 << 16 : 1) : 0;  // low half: selected non-flat tiles, high half: flat ones
    sc[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int u = threadIdx.x >= o ? sc[threadIdx.x - o] : 0;
        __syncthreads();
        sc[threadIdx.x] += u;
        __syncthreads();
    }
    if (!sel) return;
    const int before = sc[threadIdx.x] - mine;
    const int b_nf = boff_nf[blockIdx.x], b_fl = boff_fl ? boff_fl[blockIdx.x] : (int)(blockIdx.x * 256) - b_nf;
    const long p = f ? (long)*total_nf + b_fl + (before >> 16) : (long)b_nf + (before & 0xffff);
    perm[p] = (int)i;
    pos[i] = (int)p;
}

// D: tile o takes the outputs at the position of the tile that was searched for it (rep_of null: itself)
__global__ __launch_bounds__(256) void ft_output_kernel(int Q, const int *__restrict__ rep_of,
                                                        const int *__restrict__ pos, const int *fidx,
                                                        const float *ferr, const int32_t *ftile, const int32_t *fpal,
                                                        const uint8_t *fhm, const uint8_t *fvm, int *idx, float *err,
                                                        FtMaps maps) {
    const long o = (long)blockIdx.x * 256 + threadIdx.x;
    if (o >= Q) return;
    const long p = pos[rep_of ? rep_of[o] : o];
    if (idx) idx[o] = fidx[p];
    if (err) err[o] = ferr[p];
    if (maps.tile) maps.tile[o] = ftile[p];
    if (maps.pal) maps.pal[o] = fpal[p];
    if (maps.hm) maps.hm[o] = fhm[p];
    if (maps.vm) maps.vm[o] = fvm[p];
}

// Each distinct tile of a call is searched once.  A tile's answer is a function of its 64 RGB words and the handle, and
// a keyframe batch is consecutive frames of one shot, so most tiles repeat the tile at their position one frame
// earlier.  Nothing outlives the call: the table is cleared, filled, verified and scattered from in every call.
//   A (ft_dedup_hash_kernel): per tile the flat flag and a 64-bit hash of its words; the key claims a slot of the
//      open-addressing table (64-bit CAS) and the slot keeps the smallest tile index of its key (atomicMin).  Which
//      slot a key gets depends on the race, what a lookup returns does not.
//   B (ft_dedup_rep_kernel): tile i reads its key's first index r; r == i: a representative; else all 64 words are
//      compared with tile r's: equal -> rep_of[i] = r (r is a representative: no chains), different (a hash collision)
//      -> i represents itself, so the method is exact whatever the hash does.  Per-block counts of the non-flat and
//      the flat representatives and of the call's non-flat tiles.
//   ft_flat_scan_kernel over the three rows of counts, then C (ft_place_kernel) places the representatives and
//   D (ft_output_kernel) gives every tile the outputs at its representative's position.
// 16 lanes per tile (one int4 each: a wave reads 1 KiB contiguous), 16 tiles per group, 256 tiles per workgroup.
static constexpr unsigned long long FT_DD_EMPTY = ~0ull;

__device__ __forceinline__ unsigned long long ft_dd_mix(unsigned long long x) {  // splitmix64's finaliser
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// the 16 ballot bits of this lane's group of 16
__device__ __forceinline__ unsigned ft_dd_group_bits(unsigned long long b) {
    return (unsigned)(b >> (threadIdx.x & 48)) & 0xffffu;
}

__global__ __launch_bounds__(256) void ft_dedup_hash_kernel(const int32_t *__restrict__ rgb, int Q,
                                                            unsigned long long kmask, unsigned long long *tkey,
                                                            unsigned int *tmin, unsigned int tmask, uint8_t *flag,
                                                            int *slot) {
    const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
    const long base = (long)blockIdx.x * 256;
    for (int it = 0; it < 16; it++) {
        const long i = base + it * 16 + g;  // uniform over the group of 16
        const bool in = i < Q;
        int4 v = make_int4(0, 0, 0, 0);
        if (in) v = reinterpret_cast<const int4 *>(rgb)[i * 16 + l];
        const int c0 = __shfl(v.x, 0, 16);
        const bool flat = ft_dd_group_bits(__ballot(v.x == c0 && v.y == c0 && v.z == c0 && v.w == c0)) == 0xffffu;
        const unsigned long long a = ((unsigned long long)(unsigned)v.x << 32) | (unsigned)v.y;
        const unsigned long long b = ((unsigned long long)(unsigned)v.z << 32) | (unsigned)v.w;
        // position-salted terms, summed over the 16 lanes
        unsigned long long h = ft_dd_mix(a + 0x9E3779B97F4A7C15ull * (unsigned)(2 * l + 1)) +
                               ft_dd_mix(b + 0x9E3779B97F4A7C15ull * (unsigned)(2 * l + 2));
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) h += __shfl_xor(h, o, 16);
        if (l != 0 || !in) continue;
        unsigned long long key = ft_dd_mix(h) & kmask;
        if (key == FT_DD_EMPTY) key = 0;
        unsigned int s = (unsigned int)(key ^ (key >> 32)) & tmask;
        for (;;) {  // at most Q keys in >= 2 Q slots: an empty slot or the key's own is always met
            unsigned long long cur = __atomic_load_n(&tkey[s], __ATOMIC_RELAXED);  // (a stale EMPTY is settled by the CAS; a key never changes once set)
            if (cur == FT_DD_EMPTY) {
                cur = atomicCAS(&tkey[s], FT_DD_EMPTY, key);
                if (cur == FT_DD_EMPTY) cur = key;
            }
            if (cur == key) break;
            s = (s + 1) & tmask;
        }
        atomicMin(&tmin[s], (unsigned int)i);
        slot[i] = (int)s;
        flag[i] = flat ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void ft_dedup_rep_kernel(const int32_t *__restrict__ rgb, int Q,
                                                           const unsigned int *__restrict__ tmin,
                                                           const int *__restrict__ slot,
                                                           const uint8_t *__restrict__ flag, int *rep_of, int *bcnt,
                                                           int nb) {
    __shared__ int cnt[3];
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
    const long base = (long)blockIdx.x * 256;
    int c_nf = 0, c_fl = 0, c_all = 0;
    for (int it = 0; it < 16; it++) {
        const long i = base + it * 16 + g;
        const bool in = i < Q;
        const long r = in ? (long)tmin[slot[i]] : 0;  // <= i: tile i itself took part in the minimum
        const bool cmp = in && r != i;
        bool eq = true;
        if (cmp) {
            const int4 a = reinterpret_cast<const int4 *>(rgb)[i * 16 + l];
            const int4 b = reinterpret_cast<const int4 *>(rgb)[r * 16 + l];
            eq = a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
        }
        const bool same = ft_dd_group_bits(__ballot(eq)) == 0xffffu;
        if (l != 0 || !in) continue;
        const bool dup = cmp && same;
        rep_of[i] = dup ? (int)r : (int)i;
        const int f = flag[i];
        c_all += f ? 0 : 1;
        if (!dup) {
            c_nf += f ? 0 : 1;
            c_fl += f ? 1 : 0;
        }
    }
    if (l == 0) {
        atomicAdd(&cnt[0], c_nf);
        atomicAdd(&cnt[1], c_fl);
        atomicAdd(&cnt[2], c_all);
    }
    __syncthreads();
    if (threadIdx.x < 3) bcnt[(size_t)threadIdx.x * nb + blockIdx.x] = cnt[threadIdx.x];
}

static std::atomic<int> g_ft_dedup{1};  // tiler_debug_ft_dedup
void nn_set_ft_dedup(int mode) { g_ft_dedup.store(mode); }

// The stage's three buffer groups, each sized in one place (0: released).
static hipError_t ft_size_rows(FtScratch &f, size_t Q, bool idle = false) {
    f.cap_rows = 0;
    const hipError_t e = dregrow({{f.qrows, Q * 192 * sizeof(float)}}, Q > 0, idle);
    if (e == hipSuccess) f.cap_rows = Q;
    return e;
}
static hipError_t ft_size_batch(FtScratch &f, size_t Q, bool idle = false) {
    const size_t nb = (Q + 255) / 256;
    f.cap_flat = 0;
    hipError_t e = dregrow({{f.fperm, Q * sizeof(int)},
                            {f.dpos, Q * sizeof(int)},
                            {f.fbcnt, 3 * nb * sizeof(int)},
                            {f.fflag, Q},
                            {f.fidx, Q * sizeof(int)},
                            {f.ferr, Q * sizeof(float)},
                            {f.ftile, Q * sizeof(int32_t)},
                            {f.fpal, Q * sizeof(int32_t)},
                            {f.fhm, Q},
                            {f.fvm, Q},
                            {f.dslot, Q * sizeof(int)},
                            {f.drep, Q * sizeof(int)}},
                           Q > 0, idle);
    // (the totals keep their block for the index's lifetime: the last search's statistics read it later)
    if (e == hipSuccess && Q > 0 && !f.fcnt) e = dmalloc((void **)&f.fcnt, 4 * sizeof(int));
    if (e == hipSuccess) f.cap_flat = Q;
    return e;
}
static hipError_t ft_size_table(FtScratch &f, size_t slots, bool idle = false) {
    f.cap_tab = 0;
    const hipError_t e = dregrow({{f.dkey, slots * sizeof(unsigned long long)}, {f.dmin, slots * sizeof(unsigned int)}},
                                 slots > 0, idle);
    if (e == hipSuccess) f.cap_tab = slots;
    return e;
}

void ft_scratch_free(FtScratch &f) {
    (void)ft_size_rows(f, 0, true);
    (void)ft_size_batch(f, 0, true);
    (void)ft_size_table(f, 0, true);
    dfree(f.fcnt);
    pinned_slot_free(f.h_cnt);
    f = FtScratch();
}

// The call decides whether it groups its flat tiles last (group) and whether it looks for repeated tiles (dedup), and
// from that makes a plan: nq tiles to search, perm (searched position -> tile, or null: the batch as it stands),
// flat_cnt (device count of the searched non-flat tiles, or null) and, with a perm, rep_of (the tile searched for each
// tile, or null: itself).  Descriptors and search then run once over the plan, and a plan with a perm ends in
// ft_output_kernel.
int nn_frame_tiling_dev(NNIndex *ix, const int32_t *d_rgb, int Q, int use_wavelets, int gamma, int *d_idx,
                        float *d_err, const FtMaps *maps, hipStream_t stream) {
    if (Q <= 0) return 0;
    if (ix->d != 192) {
        set_error("frame tiling: dataset dimension must be 192 (cTileDCTSize)");
        return -1;
    }
    FtScratch &f = ix->ft;
    if ((size_t)Q > f.cap_rows) TILER_HIP_CHECK(ft_size_rows(f, Q));
    const bool fuse_rb = ix->kd && use_wavelets && ix->kd->dd == 192;
    if (fuse_rb && nn_ensure_rootbox(ix, Q)) return -1;
    const bool orbit = ix->orbit && use_wavelets;
    // flat grouping on the generic path (datasets without mirror orbits: real PrepareFrameTiling candidate sets):
    // the 16x16x32 shortlist's flat workgroups contract k-step 0 only (dc_first_dim)
    const bool flat_generic = !ix->orbit && use_wavelets && nn_generic_takes_flat(ix);
    // flat tiles last (see ft_flat_flag_kernel) when the shortlist is long enough to repay the ~0.1 ms of grouping: C3
    // (2,048 group blocks) -0.6..-1.1 ms per step; C2 (512 blocks, whose ragged last round the mixed split already
    // fills) +0.08 ms (profiles/flat_c2_ab.sh), so not there
    const bool group = Q >= 8192 && (flat_generic || (orbit && ((const OrbitIndex *)ix->orbit)->gblk >= 1024));
    // each distinct tile searched once (see ft_dedup_hash_kernel); the query kernels read through a permutation on
    // the Haar path only
    const int dd_mode = g_ft_dedup.load(std::memory_order_relaxed);
    const bool dedup = dd_mode != 0 && use_wavelets && Q >= 8192;

    int nq = Q;
    const int *perm = nullptr, *flat_cnt = nullptr, *rep_of = nullptr;
    const int nb = (Q + 255) / 256;
    if (group || dedup) {
        if ((size_t)Q > f.cap_flat) TILER_HIP_CHECK(ft_size_batch(f, Q));
        auto place = [&](const int *reps, const int *boff_nf, const int *boff_fl, const int *total_nf) {
            hipLaunchKernelGGL(ft_place_kernel, dim3(nb), dim3(256), 0, stream, Q, (const uint8_t *)f.fflag, reps,
                               boff_nf, boff_fl, total_nf, f.fperm, f.dpos);
        };
        const int *cnt = f.fcnt;  // device count of the searched batch's non-flat tiles
        bool engaged = false;     // the searched batch is the representatives
        if (dedup) {
            size_t slots = 1;
            while (slots < 2 * (size_t)Q) slots <<= 1;
            if (slots > f.cap_tab) TILER_HIP_CHECK(ft_size_table(f, slots));
            if (!f.h_cnt && !(f.h_cnt = pinned_slot())) {
                set_error("frame tiling: pinned host allocation failed");
                return -1;
            }
            {
                KTimer tm("ft_dedup", stream);
                TILER_HIP_CHECK(hipMemsetAsync(f.dkey, 0xff, slots * sizeof(unsigned long long), stream));
                TILER_HIP_CHECK(hipMemsetAsync(f.dmin, 0xff, slots * sizeof(unsigned int), stream));
                hipLaunchKernelGGL(ft_dedup_hash_kernel, dim3(nb), dim3(256), 0, stream, d_rgb, Q,
                                   dd_mode == 2 ? 15ull : ~0ull, f.dkey, f.dmin, (unsigned int)(slots - 1), f.fflag,
                                   f.dslot);
                hipLaunchKernelGGL(ft_dedup_rep_kernel, dim3(nb), dim3(256), 0, stream, d_rgb, Q,
                                   (const unsigned int *)f.dmin, (const int *)f.dslot, (const uint8_t *)f.fflag, f.drep,
                                   f.fbcnt, nb);
                hipLaunchKernelGGL(ft_flat_scan_kernel, dim3(3), dim3(1024), 0, stream, f.fbcnt, nb, f.fcnt);
                TILER_HIP_CHECK(hipGetLastError());
                TILER_HIP_CHECK(hipMemcpyAsync(f.h_cnt, f.fcnt, 3 * sizeof(int), hipMemcpyDeviceToHost, stream));
                // the representatives placed while the counts travel (wasted only on a batch without repeats)
                place(f.drep, f.fbcnt, f.fbcnt + nb, f.fcnt);
                TILER_HIP_CHECK(hipGetLastError());
            }
            TILER_HIP_CHECK(hipStreamSynchronize(stream));  // this stream only: the launches below are sized by U
            const int U = f.h_cnt[0] + f.h_cnt[1];
            if (U < 1 || U > Q) {
                set_error("frame tiling: inconsistent representative count");
                return -1;
            }
            engaged = U <= Q - Q / 8;
            if (engaged) {
                nq = U;
                rep_of = f.drep;
            } else if (group) {  // few repeats: all Q tiles grouped, from the flags and the third row of counts
                cnt = f.fcnt + 2;
                place(nullptr, f.fbcnt + (size_t)2 * nb, nullptr, cnt);
            }
        } else {  // the switch off: no hash pass, no table fill, no host wait
            hipLaunchKernelGGL(ft_flat_flag_kernel, dim3(nb), dim3(256), 0, stream, d_rgb, Q, f.fflag, f.fbcnt);
            hipLaunchKernelGGL(ft_flat_scan_kernel, dim3(1), dim3(1024), 0, stream, f.fbcnt, nb, f.fcnt);
            place(nullptr, f.fbcnt, nullptr, cnt);
        }
        TILER_HIP_CHECK(hipGetLastError());
        if (engaged || group) {
            perm = f.fperm;
            if (group) flat_cnt = cnt;  // the shortlist reads the non-flat count on the device (no host sync)
        }
    }

    // descriptors + search, once: into the caller's outputs, or in searched order for ft_output_kernel
    FtMaps fm;
    if (maps) fm = perm ? FtMaps{f.ftile, f.fpal, f.fhm, f.fvm} : *maps;
    SearchOpts so;
    so.rootbox_ready = fuse_rb;
    so.orbit_prepared = orbit;
    so.flat_cnt = flat_cnt;
    const float *box = fuse_rb ? ix->kd->d_box : nullptr;
    float *rootbox = fuse_rb ? ix->scratch.kd_rootbox : nullptr;
    if (orbit) {
        // one kernel: descriptors + the orbit search's q' fragments and statistics (+ the kd root box)
        if (orbit_ft_queries(ix, d_rgb, nq, gamma, f.qrows, box, rootbox, stream, perm)) return -1;
    } else {
        PsyvArgs pa;
        pa.n = nq;
        pa.rgb = d_rgb;
        pa.perm = perm;
        pa.flags = use_wavelets ? PSYV_WAVELETS : 0;
        pa.gamma = gamma;
        pa.out32 = f.qrows;
        pa.box = box;  // annBoxDistance of each query descriptor, in the descriptor kernel (kd pruning check)
        pa.rootbox = rootbox;
        if (launch_psyv(pa, stream)) return -1;
    }
    if (nn_search_dev(ix, f.qrows, nq, 1, perm ? f.fidx : d_idx, perm ? f.ferr : d_err, maps ? &fm : nullptr, stream, so))
        return -1;
    if (!perm) return 0;
    if (rep_of) {
        ix->last.queries = Q;
        ix->last.dup = Q - nq;
        ix->last.ft_nonflat = f.h_cnt[2];
    }
    KTimer tm(rep_of ? "ft_dedup" : nullptr, stream);
    hipLaunchKernelGGL(ft_output_kernel, dim3(nb), dim3(256), 0, stream, Q, rep_of, (const int *)f.dpos,
                       (const int *)f.fidx, (const float *)f.ferr, (const int32_t *)f.ftile, (const int32_t *)f.fpal,
                       (const uint8_t *)f.fhm, (const uint8_t *)f.fvm, d_idx, d_err, maps ? *maps : FtMaps{});
    TILER_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tiler
