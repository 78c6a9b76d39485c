// gtm_write_check.cpp -- stand-alone check of the plain-C++ half of the .gtm writer (gtm_write.cpp: the compressor pool
// and the container) under the host sanitizers, read back with the host reader.  No HIP, no GPU, nothing loaded into
// another process:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/gtm_write_check.cpp tiler_amd/csrc/lzma_alone.cpp tiler_amd/csrc/lzma_dec.cpp tiler_amd/csrc/gtm_read.cpp \
//       tiler_amd/csrc/gtm_write.cpp -lpthread -o gtm_write_check && ./gtm_write_check
// (tests/test_gtm_write_host.py does this, source by source).  It writes the command streams of a small clip by
// hand, hands them to GtmPacker out of order on 1, 2, 3 and the default number of threads, assembles the file,
// parses it with gtm_parse and compares every item; then the packer's and the container's error paths and FPC
// Round's ties.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../include/tiler_ann.h"
#include "../tiler_amd/csrc/gtm_read.hpp"
#include "../tiler_amd/csrc/gtm_write.hpp"
#include "../tiler_amd/csrc/host_error.hpp"

namespace tiler {
static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
const char *last_error() { return g_err.c_str(); }
}  // namespace tiler

namespace {

using Bytes = std::vector<uint8_t>;

void w16(Bytes &b, uint32_t v) {
    b.push_back((uint8_t)v);
    b.push_back((uint8_t)(v >> 8));
}
void w32(Bytes &b, uint32_t v) {
    w16(b, v & 0xFFFF);
    w16(b, v >> 16);
}
void cmd(Bytes &b, int c, uint32_t arg) { w16(b, (arg << 6) | (uint32_t)c); }

struct Clip {
    int W = 6, H = 5, T = 70000, P = 3;
    std::vector<int32_t> kf_start{0, 2, 3, 7};
    std::vector<int32_t> tile;  // [F][Q], -1 = skipped
    std::vector<uint16_t> attrs;
    std::vector<Bytes> raws;
};

Clip make_clip(std::mt19937 &rng) {
    Clip c;
    const int Q = c.W * c.H, KF = (int)c.kf_start.size() - 1;
    for (int k = 0; k < KF; k++) {
        Bytes z;
        if (k == 0) {
            cmd(z, TILER_GTM_SET_DIMENSIONS, 0);
            w16(z, c.W);
            w16(z, c.H);
            w32(z, 41666667);
            w32(z, c.T);
            cmd(z, TILER_GTM_TILE_SET, 16);
            w32(z, 0);
            w32(z, c.T - 1);
            // mostly zeros: quick to compress
            for (int i = 0; i < c.T * 64; i++) z.push_back((uint8_t)(i % 64 ? 0 : rng() % 16));
        }
        for (int j = 0; j < c.P; j++) {
            cmd(z, TILER_GTM_LOAD_PALETTE, 0);
            z.push_back((uint8_t)j);
            z.push_back(0);
            for (int i = 0; i < 16; i++) w32(z, (uint32_t)rng() | 0xFF000000u);
        }
        for (int f = c.kf_start[k]; f < c.kf_start[k + 1]; f++) {
            for (int q = 0; q < Q;) {
                if (f > 0 && rng() % 3 == 0) {
                    const int n = std::min(1 + (int)(rng() % 7), Q - q);
                    cmd(z, TILER_GTM_SKIP_BLOCK, n - 1);
                    c.tile.insert(c.tile.end(), n, -1);
                    c.attrs.insert(c.attrs.end(), n, 0);
                    q += n;
                    continue;
                }
                const uint32_t t = rng() % c.T, a = ((rng() % c.P) << 2) | (rng() & 3);
                if (t >= 65536) {
                    cmd(z, TILER_GTM_LONG_TILE_IDX, a);
                    w32(z, t);
                } else {
                    cmd(z, TILER_GTM_SHORT_TILE_IDX, a);
                    w16(z, t);
                }
                c.tile.push_back((int32_t)t);
                c.attrs.push_back((uint16_t)a);
                q++;
            }
            cmd(z, TILER_GTM_FRAME_END, f == c.kf_start[k + 1] - 1);
        }
        c.raws.push_back(z);
    }
    return c;
}

int failures = 0;
void expect(bool ok, const std::string &what) {
    if (ok) return;
    failures++;
    std::fprintf(stderr, "FAIL: %s\n", what.c_str());
}

uint32_t rd32(const Bytes &b, size_t at) {
    return (uint32_t)b[at] | (uint32_t)b[at + 1] << 8 | (uint32_t)b[at + 2] << 16 | (uint32_t)b[at + 3] << 24;
}

// the clip through the pool on `threads` threads, streams made ready in the given order -> the file
bool pack(const Clip &c, int threads, const std::vector<int> &order, Bytes &file) {
    const int KF = (int)c.raws.size();
    tiler::GtmPacker pk(KF, threads);
    for (int k : order) {
        pk.raw(k) = c.raws[(size_t)k];
        pk.ready(k);
    }
    if (!pk.finish()) return false;
    Bytes all;
    std::vector<size_t> len;
    for (int k = 0; k < KF; k++) {
        len.push_back(pk.comp(k).size());
        all.insert(all.end(), pk.comp(k).begin(), pk.comp(k).end());
    }
    return tiler::gtm_assemble(all.data(), len.data(), c.kf_start.data(), KF, c.W * 8, c.H * 8, 29.97, file);
}

}  // namespace

int main() {
    std::mt19937 rng(20241020);
    const Clip c = make_clip(rng);
    Bytes first, file;
    const std::vector<std::pair<int, std::vector<int>>> runs = {
        {1, {0, 1, 2}}, {2, {2, 0, 1}}, {3, {1, 2, 0}}, {0, {2, 1, 0}}, {64, {0, 2, 1}}};
    for (const auto &r : runs) {
        expect(pack(c, r.first, r.second, file), std::string("pack: ") + tiler::last_error());
        if (first.empty()) first = file;
        expect(file == first, "the file does not depend on the thread count or the order the streams arrive in");
    }
    // the container: sizes, the records, and the reader's view of it
    expect(first.size() > 40 + 28 * 3 && std::memcmp(first.data(), "GTMv", 4) == 0, "GTMv header");
    expect(rd32(first, 8) == 40 + 28 * 3 && rd32(first, 24) == 3 && rd32(first, 28) == 7, "header counts");
    size_t body = 0;
    for (int k = 0; k < 3; k++) {
        const size_t at = 40 + 28 * (size_t)k;
        expect(std::memcmp(first.data() + at, "GTMk", 4) == 0 && rd32(first, at + 8) == (uint32_t)k &&
                   rd32(first, at + 12) == (uint32_t)c.kf_start[(size_t)k] && rd32(first, at + 16) == 0,
               "keyframe record");
        body += rd32(first, at + 20);
    }
    expect(first.size() == 40 + 28 * 3 + body, "the CompressedSize fields add up to the file");
    tiler::GtmData g;
    expect(tiler::gtm_parse(first.data(), first.size(), 2, 0, g), std::string("parse: ") + tiler::last_error());
    expect(g.frames() == 7 && g.keyframes() == 3 && g.n_tiles == c.T && g.width == c.W && g.height == c.H &&
               g.pal_rows() == 9,
           "parsed counts");
    expect(g.kf_start == c.kf_start && g.tile == c.tile, "parsed tiles and keyframes");
    bool attrs_ok = g.attrs.size() == c.attrs.size();
    for (size_t i = 0; attrs_ok && i < c.attrs.size(); i++) attrs_ok = c.tile[i] < 0 || g.attrs[i] == c.attrs[i];
    expect(attrs_ok, "parsed attributes");
    for (size_t k = 0; k < 3; k++) expect(g.stream_raw[k] == c.raws[k].size(), "a stream decodes to its raw size");

    // an empty stream compresses and decodes; a stream never made ready is an error, not a wait
    {
        tiler::GtmPacker pk(2, 2);
        pk.raw(0).clear();
        pk.ready(0);
        expect(!pk.finish() && std::strstr(tiler::last_error(), "never written"), "finish with a stream missing");
    }
    {
        tiler::GtmPacker pk(1, 0);
        pk.ready(0);
        expect(pk.finish() && pk.comp(0).size() >= 13, "an empty stream is a valid LZMA stream");
        Bytes out(16);
        size_t n = 99, used = 0;
        expect(tiler_lzma_decode(pk.comp(0).data(), pk.comp(0).size(), out.data(), out.size(), &n, &used) == 0 &&
                   n == 0 && used == pk.comp(0).size(),
               "the empty stream decodes to nothing");
    }
    { tiler::GtmPacker idle(3, 3); }  // destroyed with nothing handed over: the workers stop

    // the container's argument checks
    const size_t len3[3] = {5, 6, 7};
    const uint8_t blob[18] = {};
    const int32_t bad0[4] = {1, 2, 3, 4}, flat[4] = {0, 2, 2, 4}, good[4] = {0, 1, 2, 4};
    Bytes out;
    expect(!tiler::gtm_assemble(blob, len3, bad0, 3, 8, 8, 24.0, out), "kf_start[0] != 0");
    expect(!tiler::gtm_assemble(blob, len3, flat, 3, 8, 8, 24.0, out), "an empty keyframe");
    expect(!tiler::gtm_assemble(blob, len3, good, 0, 8, 8, 24.0, out), "no keyframes");
    expect(!tiler::gtm_assemble(blob, len3, good, 3, 8, 8, 0.0, out), "fps 0");
    expect(!tiler::gtm_assemble(nullptr, len3, good, 3, 8, 8, 24.0, out), "null streams");
    expect(tiler::gtm_assemble(blob, len3, good, 3, 8, 8, 24.0, out) && out.size() == 40 + 28 * 3 + 18, "a good call");
    // KFMaxBytesPerSec: keyframes 1 and 2 only -> max(6 * 24 / 1, 7 * 24 / 2) = 144; average 18 * 24 / 4 = 108
    expect(rd32(out, 32) == 108 && rd32(out, 36) == 144, "byte rates");
    // FPC Round: ties to even
    expect(tiler::fpc_round(0.5) == 0 && tiler::fpc_round(1.5) == 2 && tiler::fpc_round(2.5) == 2 &&
               tiler::fpc_round(3.5) == 4 && tiler::fpc_round(2.4999) == 2 && tiler::fpc_round(2.5001) == 3 &&
               tiler::fpc_round(-0.5) == 0 && tiler::fpc_round(-1.5) == -2,
           "fpc_round");
    const size_t one[1] = {5};
    const int32_t kf1[2] = {0, 2};
    expect(tiler::gtm_assemble(blob, one, kf1, 1, 8, 8, 1.0, out) && rd32(out, 32) == 2 && rd32(out, 36) == 2,
           "5 / 2 = 2.5 rounds to 2 in both rate fields");
    if (failures) return 1;
    std::printf("gtm_write_check ok: %zu-byte file\n", first.size());
    return 0;
}
