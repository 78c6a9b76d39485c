// gtm_read_check.cpp -- stand-alone check of the plain-C++ playback host code (lzma_dec.cpp, gtm_read.cpp, with
// lzma_alone.cpp to write its input) under the host sanitizers.  No HIP, no GPU, nothing loaded into another process:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/gtm_read_check.cpp tiler_amd/csrc/lzma_alone.cpp tiler_amd/csrc/lzma_dec.cpp tiler_amd/csrc/gtm_read.cpp \
//       -lpthread -o gtm_read_check && ./gtm_read_check
// (tests/test_gtm_decode.py does this, source by source).  It builds a small .gtm file, checks that it parses, then sweeps
// truncations (every offset of the LZMA stream's first 64 bytes and 20 seeded later ones; every offset of the file)
// and 200 seeded single-byte corruptions of both (the LZMA header's dictionary size aside): each must end in an error
// or -- corruption only -- in a result that differs from the original, never in a bad access (the sanitizers abort)
// or a short "success".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../include/tiler_ann.h"
#include "../tiler_amd/csrc/gtm_read.hpp"
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

Bytes compress(const Bytes &raw, int eos) {
    size_t need = 0;
    tiler_lzma_encode(raw.data(), raw.size(), 8, 0, 2, 1u << 21, eos, nullptr, 0, &need);
    Bytes out(need);
    if (tiler_lzma_encode(raw.data(), raw.size(), 8, 0, 2, 1u << 21, eos, out.data(), out.size(), &need) != 0) out.clear();
    return out;
}

// W x H tilemap, T tiles, palsize 16, two keyframes of `frames` frames each, random skips and mirrors
Bytes make_file(std::mt19937 &rng, int W, int H, int T, int frames, Bytes *first_stream) {
    const int Q = W * H, P = 3;
    std::vector<Bytes> comps;
    for (int k = 0; k < 2; k++) {
        Bytes z;
        if (k == 0) {
            cmd(z, TILER_GTM_SET_DIMENSIONS, 0);
            w16(z, W);
            w16(z, H);
            w32(z, 41666667);
            w32(z, T);
            cmd(z, TILER_GTM_TILE_SET, 16);
            w32(z, 0);
            w32(z, T - 1);
            for (int i = 0; i < T * 64; i++) z.push_back((uint8_t)(rng() % 16));
        }
        for (int j = 0; j < P; j++) {
            cmd(z, TILER_GTM_LOAD_PALETTE, 0);
            z.push_back((uint8_t)j);
            z.push_back(0);
            for (int i = 0; i < 16; i++) w32(z, (uint32_t)rng() | 0xFF000000u);
        }
        for (int f = 0; f < frames; f++) {
            for (int q = 0; q < Q;) {
                const int run = (f > 0 || k > 0) && rng() % 3 == 0 ? 1 + (int)(rng() % 5) : 0;
                if (run) {
                    const int n = std::min(run, Q - q);
                    cmd(z, TILER_GTM_SKIP_BLOCK, n - 1);
                    q += n;
                    continue;
                }
                const uint32_t t = rng() % T, attrs = ((rng() % P) << 2) | (rng() & 3);
                if (rng() % 4 == 0) {
                    cmd(z, TILER_GTM_LONG_TILE_IDX, attrs);
                    w32(z, t);
                } else {
                    cmd(z, TILER_GTM_SHORT_TILE_IDX, attrs);
                    w16(z, t);
                }
                q++;
            }
            cmd(z, TILER_GTM_FRAME_END, f == frames - 1);
        }
        comps.push_back(compress(z, 1));
        if (k == 0 && first_stream) *first_stream = comps.back();
    }
    Bytes file;
    const uint32_t hdr[10] = {0, 32, 40 + 28 * 2, 1, (uint32_t)W * 8, (uint32_t)H * 8, 2, (uint32_t)frames * 2, 0, 0};
    file.insert(file.end(), {'G', 'T', 'M', 'v'});
    for (int i = 1; i < 10; i++) w32(file, hdr[i]);
    for (int k = 0; k < 2; k++) {
        file.insert(file.end(), {'G', 'T', 'M', 'k'});
        const uint32_t rec[6] = {20, (uint32_t)k, (uint32_t)(k * frames), 0, (uint32_t)comps[k].size(), 0};
        for (uint32_t v : rec) w32(file, v);
    }
    for (auto &c : comps) file.insert(file.end(), c.begin(), c.end());
    return file;
}

int failures = 0;
void expect(bool ok, const char *what, size_t at) {
    if (ok) return;
    failures++;
    std::fprintf(stderr, "FAIL: %s (offset %zu)\n", what, at);
}

// 0 and the output, or the decoder's code; the output buffer is exactly `cap` bytes so an overrun is caught
int decode(const Bytes &comp, size_t n, size_t cap, Bytes &out) {
    Bytes src(comp.begin(), comp.begin() + n);  // exactly n bytes: an over-read is caught
    out.assign(cap, 0);
    size_t len = 0, used = 0;
    const int rc = tiler_lzma_decode(src.data(), n, out.data(), cap, &len, &used);
    if (rc == 0) out.resize(len);
    return rc;
}

// Any byte but the dictionary size (offsets 1..4): that field only bounds the distances a stream may use, so a
// corrupted value that is still large enough describes the same, valid stream.
size_t corrupt_at(std::mt19937 &rng, size_t n) {
    const size_t at = rng() % (n - 4);
    return at >= 1 ? at + 4 : at;
}

void sweep_lzma(std::mt19937 &rng, const Bytes &raw, int eos) {
    const Bytes comp = compress(raw, eos);
    Bytes out;
    expect(decode(comp, comp.size(), raw.size(), out) == 0 && out == raw, "LZMA round trip", 0);
    expect(decode(comp, comp.size(), raw.size() / 2, out) == TILER_LZMA_GROW, "a small cap asks to grow", 0);
    std::vector<size_t> cuts;
    for (size_t i = 0; i < 64 && i < comp.size(); i++) cuts.push_back(i);
    for (int i = 0; i < 20; i++) cuts.push_back(64 + rng() % (comp.size() - 64));
    for (size_t c : cuts) expect(decode(comp, c, raw.size(), out) == -1, "a truncated LZMA stream is an error", c);
    for (int i = 0; i < 200; i++) {
        Bytes bad = comp;
        const size_t at = corrupt_at(rng, bad.size());
        bad[at] ^= (uint8_t)(1 + rng() % 255);
        const int rc = decode(bad, bad.size(), raw.size() + 4096, out);
        expect(rc != 0 || out != raw, "a corrupted LZMA stream errs or decodes differently", at);
    }
}

bool same(const tiler::GtmData &a, const tiler::GtmData &b) {
    return a.tiles == b.tiles && a.palettes == b.palettes && a.tile == b.tile && a.attrs == b.attrs &&
           a.palrow == b.palrow && a.kf_end == b.kf_end && a.width == b.width && a.height == b.height &&
           a.frame_ns == b.frame_ns && a.n_tiles == b.n_tiles;
}

}  // namespace

int main() {
    std::mt19937 rng(20240611);
    Bytes raw(60000);
    for (size_t i = 0; i < raw.size(); i++) raw[i] = (uint8_t)(i % 7 == 0 ? rng() : rng() % 4);
    sweep_lzma(rng, raw, 1);
    sweep_lzma(rng, raw, 0);

    Bytes first;
    const Bytes file = make_file(rng, 5, 4, 20, 4, &first);
    tiler::GtmData good, g;
    expect(tiler::gtm_parse(file.data(), file.size(), 2, 0, good), tiler::last_error(), 0);
    expect(good.frames() == 8 && good.keyframes() == 2 && good.pal_rows() == 6 && good.Q() == 20, "parsed counts", 0);
    expect(!tiler::gtm_parse(file.data(), file.size(), 2, 1024, g), "max_raw_bytes is honoured", 0);
    // headerless: the streams alone hold the same frames
    expect(tiler::gtm_parse(file.data() + 96, file.size() - 96, 0, 0, g) && !g.has_header && same(g, good),
           "headerless parse", 0);
    for (size_t cut = 0; cut < file.size(); cut++) {
        Bytes part(file.begin(), file.begin() + cut);
        expect(!tiler::gtm_parse(part.data(), part.size(), 1, 0, g), "a truncated file is an error", cut);
    }
    // corruptions inside the streams; a stream's dictionary-size field is left alone (see corrupt_at)
    for (int i = 0; i < 200; i++) {
        Bytes bad = file;
        size_t at = 96 + rng() % (bad.size() - 96);
        const size_t in_stream = at < 96 + first.size() ? at - 96 : at - 96 - first.size();
        if (in_stream >= 1 && in_stream <= 4) at += 4;
        bad[at] ^= (uint8_t)(1 + rng() % 255);
        const bool ok = tiler::gtm_parse(bad.data(), bad.size(), 1, 1 << 22, g);
        expect(!ok || !same(g, good), "a corrupted file errs or parses differently", at);
    }
    if (failures) return 1;
    std::printf("gtm_read_check ok: %zu-byte file, %zu-byte LZMA stream\n", file.size(), first.size());
    return 0;
}
