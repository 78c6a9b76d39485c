// search_plan_check.cpp -- the searches' launch plans (tiler_amd/csrc/search_plan.hpp) pinned on the CPU: a program
// of its own that includes the header alone.  The expected orbit plans are derived by hand from the pricing rule
// (rounds of n_cu workgroups, a round priced at its blocks + ORB_WG_FIXED = 64, a plan taken only when >= 2 % cheaper)
// with n_cu = 256; the rest are the invariants the launchers and kernels rely on.  tests/test_search_plan_host.py
// builds it with a host compiler (and the host sanitizers where they link) and runs it.
#include <cstdio>

#include "../tiler_amd/csrc/search_plan.hpp"

using namespace tiler;

static int g_fail = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            if (g_fail++ < 20) printf("%s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                          \
    } while (0)

static bool same(const OrbitPlan &a, const OrbitPlan &b) {
    return a.wgs == b.wgs && a.nsplit == b.nsplit && a.bps == b.bps && a.mix_full == b.mix_full &&
           a.queries_per_wg == b.queries_per_wg;
}

static void orbit_cases() {
    const int n_cu = 256;
    {  // C3: 1080p x 24 frames = 777,600 tiles -> 1,519 workgroups; 65,536 groups -> 2,048 blocks.  1 split: 6 rounds
        // x 2112 = 12672; 2, 3, 4 splits: 13056, 13446, 13824; mixed (5 full rounds + 239): 12736, 12801, 12864
        const OrbitPlan p = orbit_plan(777600, 2048, n_cu, false);
        CHECK(p.wgs == 1519 && p.nsplit == 1 && p.bps == 2048 && p.mix_full == 0 && p.queries_per_wg == 512);
        CHECK(same(p, orbit_plan(777600, 2048, n_cu, true)));
    }
    {  // C2: 720p x 96 frames = 345,600 tiles -> 675 workgroups, 512 blocks.  1 split: 3 x 576 = 1728; 2, 3, 4
        // splits: 1920, 1880, 2112; mixed (2 full rounds = 1152, + 163 workgroups): 1792, 1152 + 2 x 235 = 1622
        // (< 0.98 x 1728), 1728 -> 3 splits of 171, the first 512 workgroups unsplit
        const OrbitPlan p = orbit_plan(345600, 512, n_cu, false);
        CHECK(p.wgs == 675 && p.nsplit == 3 && p.bps == 171 && p.mix_full == 512);
        // THE QUIRK (kept on purpose, see orbit_plan): with flat tiles grouped last the mixed launch is dropped but
        // its split count stays: 3 whole-batch splits (8 rounds x 235 = 1880), not the 1-split plan (1728)
        const OrbitPlan f = orbit_plan(345600, 512, n_cu, true);
        CHECK(f.wgs == 675 && f.nsplit == 3 && f.bps == 171 && f.mix_full == 0);
    }
    {  // test_orbit_mixed_launch: 64 blocks, n_cu + 44 workgroups.  1 split: 2 x 128 = 256 (2, 3, 4: 288, 344, 400);
        // mixed: 128 + (ceil(64 / ns) + 64) = 224, 214, 208, each >= 2 % under the one before -> 4 splits of 16
        const int nq = (n_cu + 44) * 512;
        const OrbitPlan p = orbit_plan(nq, 64, n_cu, false);
        CHECK(p.wgs == n_cu + 44 && p.nsplit == 4 && p.bps == 16 && p.mix_full == n_cu);
        CHECK(same(p, orbit_plan(nq - 173, 64, n_cu, false)));  // last workgroup and last query block partial
    }
}

static void orbit_sweep() {
    const int gblks[] = {1, 2, 3, 63, 64, 171, 512, 2048}, cus[] = {1, 64, 256, 304};
    long n = 0;
    auto one = [&](int nq) {
        for (int gblk : gblks)
            for (int n_cu : cus)
                for (int flat = 0; flat < 2; flat++) {
                    const OrbitPlan p = orbit_plan(nq, gblk, n_cu, flat != 0);
                    n++;
                    CHECK(p.wgs == (nq + 511) / 512 && p.queries_per_wg == ORB_NW * ORB_QB * 32);
                    CHECK(p.nsplit >= 1 && p.nsplit <= std::min(4, gblk));
                    CHECK((long)(p.nsplit - 1) * p.bps < gblk && gblk <= (long)p.nsplit * p.bps);
                    CHECK(p.mix_full >= 0 && p.mix_full % n_cu == 0 && p.mix_full < p.wgs);
                    CHECK(!flat || p.mix_full == 0);
                    CHECK(p.nsplit * 2 * ORB_L <= 32);  // the rescore's half-wave holds a query's lists
                }
    };
    for (int nq = 1; nq <= 200000; nq += 97) one(nq);
    one(200000);
    printf("orbit sweep: %ld plans\n", n);
}

static void generic_cases() {
    CHECK(generic_plan(4, 0, 100, 0, 32767).qpwg == 128);
    CHECK(generic_plan(4, 0, 100, 0, 32768).qpwg == 256);
    CHECK(generic_plan(8, 0, 100, 0, 5000).qpwg == 256);
    CHECK(generic_plan(12, 0, 100, 0, 5000).qpwg == 512);
    CHECK(generic_plan(16, 0, 100, 0, 5000).qpwg == 256);
    {  // the 16-row path: its own blocks, 4 lanes x SL16_L entries, 8 waves x 4 blocks of 16 queries
        const GenericPlan p = generic_plan(12, 6, 100, 777, 5000);
        CHECK(p.qpwg == 512 && p.L == SL16_L && p.lpq == 4 && p.nblk_used == 777 && p.wgs == 10 && p.nsplit == 4 &&
              p.bps == 195);
    }
    {  // 1,024 workgroup-splits wanted: 400 workgroups -> ceil(1024 / 400) = 3 splits; 2,000 -> 1
        const GenericPlan p = generic_plan(8, 0, 1000, 0, 400 * 256);
        CHECK(p.L == 8 && p.lpq == 2 && p.wgs == 400 && p.nsplit == 3 && p.bps == 334 && p.nblk_used == 1000);
        CHECK(generic_plan(8, 0, 1000, 0, 2000 * 256).nsplit == 1);
    }
    const int Ss[] = {4, 8, 12, 16}, nblks[] = {1, 2, 3, 5, 64, 1000, 8192};
    long n = 0;
    auto one = [&](int nq) {
        for (int S : Ss)
            for (int S16 = 0; S16 <= 6; S16 += 6)
                for (int nblk : nblks) {
                    const int nblk16 = 2 * nblk - 1;
                    const GenericPlan p = generic_plan(S, S16, nblk, nblk16, nq);
                    n++;
                    CHECK(p.nblk_used == (S16 ? nblk16 : nblk));
                    CHECK(p.wgs == (nq + p.qpwg - 1) / p.qpwg);
                    CHECK(p.nsplit >= 1 && p.nsplit * p.lpq * p.L <= 64);  // one wave reads a query's lists
                    CHECK((long)(p.nsplit - 1) * p.bps < p.nblk_used && p.nblk_used <= (long)p.nsplit * p.bps);
                }
    };
    for (int nq = 1; nq <= 200000; nq += 97) one(nq);
    one(200000);
    printf("generic sweep: %ld plans\n", n);
}

static void scan_cases() {
    const int one_qn[][2] = {{1, 1}, {2, 4}, {4, 4}, {5, 16}, {16, 16}, {17, 16}, {64, 16}};
    for (auto &c : one_qn) {
        const ScanPlan p = scan_plan(100000, 48, 0, c[0], 1);
        CHECK(p.qn == c[1] && p.K == 1 && p.kind == ScanKind::plain);
    }
    const int eight_qn[][2] = {{1, 1}, {2, 4}, {16, 4}};
    for (auto &c : eight_qn)
        for (int k : {2, 8}) {
            const ScanPlan p = scan_plan(100000, 192, 0, c[0], k);
            CHECK(p.qn == c[1] && p.K == 8 && p.kind == ScanKind::plain);
        }
    // the three kinds.  Orbit: 192-d rows with base rows, one split per 64 groups, any k <= 8
    CHECK(scan_plan(262144, 192, 65536, 3, 1).kind == ScanKind::orbit && scan_plan(262144, 192, 65536, 3, 1).nsplit == 1024);
    CHECK(scan_plan(262144, 192, 65536, 3, 8).kind == ScanKind::orbit);
    CHECK(scan_plan(8192, 192, 2049, 1, 1).nsplit == 33);
    // rows: k = 1, d a multiple of 64, up to 65,536 rows, one split per 64 rows
    CHECK(scan_plan(65536, 192, 0, 3, 1).kind == ScanKind::rows && scan_plan(65536, 192, 0, 3, 1).nsplit == 1024);
    CHECK(scan_plan(65, 64, 0, 3, 1).kind == ScanKind::rows && scan_plan(65, 64, 0, 3, 1).nsplit == 2);
    CHECK(scan_plan(65536, 192, 0, 3, 8).kind == ScanKind::plain);  // k > 1
    CHECK(scan_plan(65536, 48, 0, 3, 1).kind == ScanKind::plain);   // d % 64
    // the 1,024-split cap: past either limit the plain scan, one split per 256 rows and 1,024 at most
    CHECK(scan_plan(262148, 192, 65537, 3, 1).kind == ScanKind::plain && scan_plan(262148, 192, 65537, 3, 1).nsplit == 1024);
    CHECK(scan_plan(65537, 192, 0, 3, 1).kind == ScanKind::plain && scan_plan(65537, 192, 0, 3, 1).nsplit == 257);
    CHECK(scan_plan(1, 48, 0, 1, 1).nsplit == 1 && scan_plan(257, 48, 0, 1, 1).nsplit == 2);
    CHECK(scan_plan(1 << 30, 48, 0, 1, 1).nsplit == 1024);
    long n = 0;  // no reachable plan is refused: the caps keep every kind within the merge's one split per thread
    for (long rows = 1; rows <= (1L << 31); rows = rows * 3 + 1)
        for (long G : {0L, 1L, 64L, 65L, 65536L, 65537L, 1L << 30})
            for (int d : {4, 48, 64, 192, 256})
                for (int k : {1, 8}) {
                    const ScanPlan p = scan_plan(rows, d, G, 3, k);
                    n++;
                    CHECK(p.kind != ScanKind::refused && p.nsplit >= 1 && p.nsplit <= SCAN_MAX_SPLIT);
                }
    printf("scan sweep: %ld plans\n", n);
    // who takes the scan: d <= 256 and a multiple of 4; k = 1 up to max1 queries, k <= 8 up to max8
    CHECK(scan_takes(192, 64, 1, 64, 16) && !scan_takes(192, 65, 1, 64, 16));
    CHECK(scan_takes(192, 16, 8, 64, 16) && !scan_takes(192, 17, 8, 64, 16) && !scan_takes(192, 1, 9, 64, 16));
    CHECK(scan_takes(256, 1, 1, 64, 16) && !scan_takes(260, 1, 1, 64, 16) && !scan_takes(190, 1, 1, 64, 16));
    CHECK(scan_takes(192, 10, 1, 0, 16));  // k = 1 is also k <= 8
    CHECK(!scan_takes(192, 1, 1, 0, 0));   // 0 disables it
}

static void tier2_cases() {
    const int fresh = 1 << 30;
    CHECK(tier2_slots(fresh, 0, 1000000) == 65536);        // nothing seen yet: one chunk
    CHECK(tier2_slots(fresh, 50000, 1000000) == 196608);   // 3 x 50,000 + 1 -> 3 chunks
    CHECK(tier2_slots(100, 70000, 1000000) == 131072);     // own below recent: 1.5 x 70,000 + 1 -> 2 chunks
    CHECK(tier2_slots(70000, 100, 1000000) == 131072);     // own above recent
    CHECK(tier2_slots(10, 20, 1000000) == 65536);
    CHECK(tier2_slots(43690, 0, 1000000) == 65536 && tier2_slots(43691, 0, 1000000) == 131072);  // 1.5 x + 1 at the seam
    CHECK(tier2_slots(fresh, 50000, 1000) == 1000 && tier2_slots(10, 20, 65537) == 65536);  // clamped to nq
}

static void flat_cases() {
    const long qpw_orbit = orbit_plan(10000, 64, 256, true).queries_per_wg;
    const long qpw_16 = generic_plan(12, 6, 100, 200, 10000).qpwg;
    CHECK(qpw_orbit == 512 && qpw_16 == SL16_NW * SL16_QB * 16);
    CHECK(first_flat_wg(0, 512) == 0 && first_flat_wg(1, 512) == 1 && first_flat_wg(512, 512) == 1 &&
          first_flat_wg(513, 512) == 2);
    for (long qpw : {qpw_orbit, qpw_16}) {
        const FlatLayout f = flat_layout(10000, qpw);  // 20 workgroups, the last one of 272 queries
        CHECK(f.nq == 10000 && f.queries_per_wg == qpw && f.wgs == 20);
        CHECK(f.wgs == orbit_plan(10000, 64, 256, true).wgs && f.wgs == generic_plan(12, 6, 100, 200, 10000).wgs);
        CHECK(flat_queries(f, 0) == 10000);            // every workgroup all-flat
        CHECK(flat_queries(f, 1024) == 10000 - 1024);  // on a workgroup boundary
        CHECK(flat_queries(f, 1025) == 10000 - 1536);  // one past it: the mixed workgroup is not counted
        CHECK(flat_queries(f, 9728) == 272 && flat_queries(f, 9729) == 0);
        CHECK(flat_queries(f, 10000) == 0);            // all non-flat
        // a FrameTiling call that searched its distinct tiles: the same layout over its own Q = 25,000 tiles
        CHECK(flat_queries(flat_layout(25000, f.queries_per_wg), 20000) == 25000 - 40 * 512);
        CHECK(flat_queries(flat_layout(25000, f.queries_per_wg), 25000) == 0);
    }
}

int main() {
    orbit_cases();
    orbit_sweep();
    generic_cases();
    scan_cases();
    tier2_cases();
    flat_cases();
    if (g_fail) {
        printf("search_plan_check: %d checks failed\n", g_fail);
        return 1;
    }
    printf("search_plan_check ok\n");
    return 0;
}
