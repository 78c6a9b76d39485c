// search_plan.hpp -- the launch plans of the searches as pure functions: how many workgroups, how many candidate
// splits, how many blocks per split and which kernel instance, from sizes alone.  Plain C++17 for a host compiler:
// no HIP header, no globals, no state; every input (device CU count, scan limits, recent tier-2 counts) is a
// parameter.  orbit.hip, nn_search.hip and ann_api.hip launch what these return; tools/search_plan_check.cpp pins
// them on the CPU (tests/test_search_plan_host.py).
#pragma once
#include <algorithm>
#include <cmath>

#ifdef __HIPCC__
#define SEARCH_PLAN_HD __host__ __device__
#else
#define SEARCH_PLAN_HD
#endif

namespace tiler {

// ------------------------------------------------------------------------------------------
// All-flat workgroups.  A batch whose flat query tiles come last (FrameTiling's grouping) keeps the count of the
// others on the device; the shortlist workgroups from first_flat_wg on hold flat tiles only.
// ------------------------------------------------------------------------------------------
struct FlatLayout {
    long nq = 0, queries_per_wg = 0, wgs = 0;  // the launch: queries, queries per workgroup, workgroups
};

// the first workgroup made of flat queries alone, nonflat >= 0 others placed before them (the kernels' boundary)
template <class T>
SEARCH_PLAN_HD constexpr T first_flat_wg(T nonflat, T queries_per_wg) {
    return (nonflat + queries_per_wg - 1) / queries_per_wg;
}

inline FlatLayout flat_layout(long nq, long queries_per_wg) {
    return FlatLayout{nq, queries_per_wg, (nq + queries_per_wg - 1) / queries_per_wg};
}

// queries in all-flat workgroups (the stats' flat_queries): over the searched tiles with the device count, or over
// a FrameTiling call's own tiles (flat_layout of its Q) with its non-flat count; a layout a launcher filled in
// (queries_per_wg > 0: LastSearch::flat_dev says whether one did)
inline long flat_queries(const FlatLayout &f, long nonflat) {
    const long w0 = std::min(f.wgs, first_flat_wg(nonflat, f.queries_per_wg));
    return w0 < f.wgs ? f.nq - w0 * f.queries_per_wg : 0;
}

// ------------------------------------------------------------------------------------------
// Mirror-orbit shortlist (nn_orbit_shortlist_pipe_kernel<ORB_L, ORB_CB, ORB_NW, ORB_QB>)
// ------------------------------------------------------------------------------------------
constexpr int ORB_L = 4, ORB_CB = 4, ORB_NW = 8, ORB_QB = 2;
// A workgroup pays a fixed cost of about ORB_WG_FIXED tile blocks (prologue, list start-up, epilogue: C2 with 3
// splits ran 1.72 us per block-round against 1.26 at C3), so a round is priced as its blocks + that.
constexpr double ORB_WG_FIXED = 64.0;

struct OrbitPlan {
    int wgs;             // workgroups over the queries (ORB_NW * ORB_QB query blocks of 32 each)
    int nsplit, bps;     // candidate splits (the lists' stride for every query) of bps 32-group blocks each
    int mix_full;        // 0: one launch of wgs x nsplit; else the first mix_full workgroups scan every block
                         // unsplit and the other wgs - mix_full split theirs nsplit ways
    int queries_per_wg;
};

// nq queries against gblk candidate blocks on n_cu compute units; has_flat: the batch's flat tiles come last and
// the kernel derives its all-flat workgroups from a device count.
inline OrbitPlan orbit_plan(int nq, int gblk, int n_cu, bool has_flat) {
    const int nqblk = (nq + 31) / 32;
    const int qpw = ORB_NW * ORB_QB;  // query blocks per workgroup (ORB_QB per wave)
    const int wgs = (nqblk + qpw - 1) / qpw;
    const int max_split = 32 / (2 * ORB_L);  // rescore: one list entry per lane of a half-wave
    // One 8-wave workgroup fills a CU (2 waves per SIMD), so a launch runs in rounds of n_cu workgroups of
    // ceil(gblk / ns) tile blocks each for ns candidate splits: pick the cheapest, preferring fewer splits (each adds
    // list entries to rescore) unless more are >= 2 % faster.  C3: 1,519 workgroups, 1 split (5.93 -> 6 rounds);
    // C2: 675 workgroups, 1 split (3 rounds of 512 blocks: 2.22 ms; 3 splits, 8 rounds of 171: 2.36 ms).
    int nsplit = 1;
    double best_t = 1e30;
    for (int ns = 1; ns <= max_split && ns <= gblk; ns++) {
        const double t = std::ceil((double)wgs * ns / n_cu) * (std::ceil((double)gblk / ns) + ORB_WG_FIXED);
        if (t < best_t * 0.98) {
            best_t = t;
            nsplit = ns;
        }
    }
    // Mixed: when the last round of whole-candidate workgroups is ragged (C2: 675 workgroups = 2.64 rounds), the
    // first R * n_cu workgroups scan every block and only the remaining ones split their blocks mix_ns ways
    // (C2: 3 rounds of 576 -> 2 x 576 + 2 x 235 block-times).  Lists keep the mix_ns stride for every query;
    // the whole-candidate part's other splits are empty entries.
    int mix_full = 0;
    {
        const int R = wgs / n_cu, rem = wgs - R * n_cu;
        for (int ns = 2; R >= 1 && rem > 0 && ns <= max_split && ns <= gblk; ns++) {
            const double t = R * (gblk + ORB_WG_FIXED) +
                             std::ceil((double)rem * ns / n_cu) * (std::ceil((double)gblk / ns) + ORB_WG_FIXED);
            if (t < best_t * 0.98) {
                best_t = t;
                nsplit = ns;
                mix_full = R * n_cu;
            }
        }
    }
    // Flat query tiles: the kernel derives its first all-flat workgroup from the device count, with any candidate
    // split, in ONE launch; the mixed launch is not used then.
    // KNOWN QUIRK, kept on purpose and pinned by tools/search_plan_check.cpp: mix_full is cleared AFTER the mixed
    // pricing chose nsplit, so a has_flat batch whose plain plan is mixed runs that many WHOLE-BATCH splits.  At
    // gblk = 512, 675 workgroups, 256 CUs that is 3 splits, 8 rounds of 171 + 64 = 1880, where 1 split costs
    // 3 x 576 = 1728 and measured faster (above).  Changing it is a plan change: measure it first.
    if (has_flat) mix_full = 0;
    const int bps = (gblk + nsplit - 1) / nsplit;
    nsplit = (gblk + bps - 1) / bps;
    return OrbitPlan{wgs, nsplit, bps, mix_full, qpw * 32};
}

// ------------------------------------------------------------------------------------------
// Generic MFMA shortlist (nn_shortlist_kernel, nn_shortlist16_kernel)
// ------------------------------------------------------------------------------------------
// waves per workgroup of the 32x32x16 shortlist on 64-d rows (UseOne's k = 8 preselection, main.pas:3830): two query
// blocks of 32 per wave, so 64 * NW queries per workgroup
constexpr int GEN_NW_S4 = 4;
constexpr int GEN_QB_S4 = 1;  // query blocks per wave there: 16,384 items x 4 splits fill 2 waves per SIMD
#ifndef GEN_QB_S4_BIG
#define GEN_QB_S4_BIG 2  // ... and from 32,768 items (whole-tileset keyframes: ~64k) two, each A fragment feeding 2 MFMAs
                         // (r06qb, profiles/r06/qb_preselect_qb2_encoder_ab.txt: whole-tileset loop 9.51 -> 9.59 Mtiles/s)
#endif
inline int gen_qb_s4(int nq) { return nq >= 32768 ? GEN_QB_S4_BIG : GEN_QB_S4; }

// 16x16x32 shortlist (nn_shortlist16_kernel) for D = 161..192 float datasets without mirror orbits: SL16_L list
// entries per lane; QB = 4 query blocks per wave; 5 (252 VGPRs) measured the same at 388k candidates (r03h: 80.6-81.2
// vs 80.9-81.1 ms)
constexpr int SL16_NW = 8, SL16_QB = 4, SL16_CB = 8, SL16_L = 4;

struct GenericPlan {
    int L, lpq;       // list entries per lane, lanes per query
    int qpwg, wgs;    // queries per workgroup, workgroups over the queries
    int nsplit, bps;  // candidate splits of bps blocks each
    int nblk_used;    // the candidate blocks split: nblk16 on the 16-row path, else nblk
};

// S, S16: the index's fragment depths (S16 > 0: the 16-row path); nblk, nblk16: its candidate blocks in each layout
inline GenericPlan generic_plan(int S, int S16, int nblk, int nblk16, int nq) {
    // 32x32x16 shortlist: 2 lanes x L = 8 per query (>= 2x the 4-way mirror near-ties of one tile per
    // lane, row_perm spreads them 2+2); 16x16x32: 4 lanes x L16 (perm16 spreads them 1 per lane)
    const int v16 = S16 > 0 ? SL16_L : 0;
    const int L = v16 ? v16 : 8;
    const int lpq = v16 ? 4 : 2;
    const int nb = v16 ? nblk16 : nblk;
    const int max_split = 64 / (lpq * L);  // the rescore reads a query's lists with one wave
    const int qpwg = v16 ? SL16_NW * SL16_QB * 16 : (S == 12 ? 512 : S == 4 ? 32 * gen_qb_s4(nq) * GEN_NW_S4 : 256);
    const int wgs = (nq + qpwg - 1) / qpwg;
    int nsplit = std::max(1, std::min(max_split, (1024 + wgs - 1) / wgs));
    nsplit = std::min(nsplit, nb);
    const int bps = (nb + nsplit - 1) / nsplit;
    nsplit = (nb + bps - 1) / bps;
    return GenericPlan{L, lpq, qpwg, wgs, nsplit, bps, nb};
}

// generic tier-2 slots of a search: whole chunks covering 1.5x the largest tier-2 count of the recent searches (own:
// this index's last count; recent: the last one seen on any index, an encoder builds a new index per keyframe), >= 1
// chunk.  A fresh index (own >= 1 << 30, the sentinel: no search of its own yet) takes 3x the recent count of the
// other indexes, a margin for an unrelated one.  Queries past the slots go to the exhaustive tier 3: exact either
// way, slower.
constexpr int TIER2_MAX = 65536;  // generic tier 2: queries per collect chunk (every tier-2 query has a slot)
inline int tier2_slots(int own, int recent, int nq) {
    const bool fresh = own >= (1 << 30);
    const int prev = fresh ? 2 * recent : std::max(own, recent);
    const long want = (long)prev + prev / 2 + 1;
    const long chunks = std::max(1L, (want + TIER2_MAX - 1) / TIER2_MAX);
    return (int)std::min<long>(nq, chunks * TIER2_MAX);
}

// ------------------------------------------------------------------------------------------
// Small-batch exhaustive scan (nn_scan_small_kernel, nn_scan_rows_kernel, nn_scan_orbit_kernel)
// ------------------------------------------------------------------------------------------
// groups of up to 16 queries (k = 1) or 4 (k <= 8) per workgroup row, batches of up to max1 / max8 queries
constexpr int SCAN_D_MAX = 256;
constexpr int SCAN_QN1 = 16, SCAN_QN8 = 4;
constexpr long SCAN_ROWS_MAXN = 65536;   // nn_scan_rows_kernel up to this many candidates
constexpr long SCAN_ORB_MAXBLK = 1024;  // the orbit scan's splits (64-group blocks) at most: the wide merge's
constexpr int SCAN_MAX_SPLIT = 1024;    // the merge holds one split per thread of one workgroup

// whether a batch of nq queries of k on d-dimensional rows takes the scan (max1, max8: tiler_set_scan_limits)
inline bool scan_takes(int d, int nq, int k, int max1, int max8) {
    return d <= SCAN_D_MAX && d % 4 == 0 && ((k == 1 && nq <= max1) || (k <= 8 && nq <= max8));
}

enum class ScanKind {
    orbit,    // mirror orbits: base rows only (nn_scan_orbit_kernel), one wave per (64-group block, query)
    rows,     // k = 1 on a plain index: the row-interleaved scan (nn_scan_rows_kernel)
    plain,    // nn_scan_small_kernel<qn, K>
    refused,  // nsplit > SCAN_MAX_SPLIT (the caps above keep this from happening)
};
struct ScanPlan {
    ScanKind kind;
    int nsplit;  // candidate splits, merged one per thread
    int qn;      // queries per workgroup row: the smallest kernel instance that holds a group
    int K;       // the kernels' list length: 1 or 8
};

// n rows of d dimensions; orbit_groups: the groups of the index's mirror-orbit base rows, 0 when it has none
// (at larger n the split-per-thread scan reads each row once for the batch's queries at near HBM peak: r05w2, the
// shuffled 262,144-row handle, 1 query 73 vs 77 us, batches slower)
inline ScanPlan scan_plan(long n, int d, long orbit_groups, int nq, int k) {
    const long nblk = (orbit_groups + 63) / 64;
    const bool orb = orbit_groups > 0 && d == 192 && nblk <= SCAN_ORB_MAXBLK;
    const int K = k == 1 ? 1 : 8;
    const bool rows_scan = !orb && K == 1 && d % 64 == 0 && n <= SCAN_ROWS_MAXN;
    const int nsplit = orb ? (int)nblk
                           : rows_scan ? (int)std::max<long>(1, (n + 63) / 64)
                                       : (int)std::max<long>(1, std::min<long>(1024, (n + 255) / 256));
    const int qn = K == 1 ? (nq == 1 ? 1 : nq <= 4 ? 4 : SCAN_QN1) : (nq == 1 ? 1 : SCAN_QN8);
    const ScanKind kind = nsplit > SCAN_MAX_SPLIT ? ScanKind::refused
                          : orb                   ? ScanKind::orbit
                          : rows_scan             ? ScanKind::rows
                                                  : ScanKind::plain;
    return ScanPlan{kind, nsplit, qn, K};
}

}  // namespace tiler
