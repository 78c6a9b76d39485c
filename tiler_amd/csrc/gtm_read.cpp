// gtm_read.cpp -- the .gtm reader (host code in libANN.so, no HIP headers: it also builds into the stand-alone
// sanitizer check, tools/gtm_read_check.cpp).
//
// Container (SaveStream main.pas:4529-4763, the player's parseHeader gtm.player.js:103-139): an optional GTMv header
// of 10 dwords (WholeHeaderSize = offset of the first stream) and KFCount GTMk records of 7 dwords (CompressedSize is
// valid, RawSize is 0 in the files this writer and the reference produce), then the LZMA-alone streams back to back.
// Without the header the file is just the streams.  The decoded streams, joined, are one sequence of commands
// (decodeFrame gtm.player.js:274-353): a 16-bit word, cmd = w & 63, arg = w >> 6:
//   SetDimensions 30   width, height (words, in tiles), frame length in ns (dword), tile count (dword)
//   TileSet       29   arg = palette size; first, last tile (dwords), 64 bytes per tile
//   LoadPalette    3   palette index, format (bytes), palsize RGBA dwords
//   SkipBlock      0   the position advances by arg + 1
//   Short/LongTileIdx 1 / 2   a word / dword tile index; arg = pal << 2 | V << 1 | H; draws at the position
//   FrameEnd      28   arg bit 0 = last frame of a keyframe
// The walk turns them into dense per-frame items; every LoadPalette appends a row to the palette table and an item
// records the row its palette index had when it was drawn, so pixels carried over skipped positions keep their
// colours when that index is reloaded later.
//
// Stricter than the JS player, which logs these and carries on -- here each is an error naming the frame and the
// position: a FrameEnd with the position != width * height, a skip or an item past the end of the tilemap, a tile
// index >= the tile count, a palette index that was never loaded, an unknown command, a truncated token (or a stream
// that ends inside a frame), a tile byte >= the palette size.  Two things the format allows are NOT supported and are
// errors too: a second SetDimensions that changes the size or the tile count, and a TileSet after the first frame.
#include "gtm_read.hpp"

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <thread>

#include "../../include/tiler_ann.h"
#include "host_error.hpp"

namespace tiler {
namespace {

uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

bool fail(const std::string &what) {
    set_error("gtm: " + what);
    return false;
}

// One LZMA-alone stream at src into out, growing the buffer up to max_raw; msg receives the failure.
bool decode_stream(const uint8_t *src, size_t n, size_t max_raw, std::vector<uint8_t> &out, size_t &consumed,
                   std::string &msg) {
    size_t cap = std::min(max_raw, std::max<size_t>((size_t)1 << 20, 4 * n));
    for (;;) {
        out.resize(cap);
        size_t len = 0;
        const int rc = tiler_lzma_decode(src, n, out.data(), cap, &len, &consumed);
        if (rc == 0) {
            out.resize(len);
            return true;
        }
        if (rc != TILER_LZMA_GROW) {
            msg = last_error();
            return false;
        }
        if (cap >= max_raw || len > max_raw) {
            msg = "stream expands past max_raw_bytes (" + std::to_string(max_raw) + ")";
            return false;
        }
        cap = std::min(max_raw, std::max(len, cap * 4));  // len: the header's size for a known-size stream
    }
}

int usable_cpus() {
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) return std::max(1, CPU_COUNT(&set));
    return std::max(1u, std::thread::hardware_concurrency());
}

// the decoded streams read as one byte sequence
struct Cursor {
    const std::vector<std::vector<uint8_t>> &s;
    size_t k = 0, pos = 0;
    explicit Cursor(const std::vector<std::vector<uint8_t>> &streams) : s(streams) { settle(); }
    void settle() {
        while (k < s.size() && pos >= s[k].size()) {
            k++;
            pos = 0;
        }
    }
    bool at_end() const { return k >= s.size(); }
    bool get(uint8_t *out, size_t n) {
        while (n) {
            if (at_end()) return false;
            const size_t m = std::min(n, s[k].size() - pos);
            std::memcpy(out, s[k].data() + pos, m);
            out += m;
            n -= m;
            pos += m;
            settle();
        }
        return true;
    }
    bool u8(uint32_t &v) {
        uint8_t b;
        if (!get(&b, 1)) return false;
        v = b;
        return true;
    }
    bool u16(uint32_t &v) {
        uint8_t b[2];
        if (!get(b, 2)) return false;
        v = (uint32_t)b[0] | (uint32_t)b[1] << 8;
        return true;
    }
    bool u32(uint32_t &v) {
        uint8_t b[4];
        if (!get(b, 4)) return false;
        v = rd32(b);
        return true;
    }
};

bool walk(const std::vector<std::vector<uint8_t>> &streams, size_t max_raw, GtmData &g) {
    Cursor c(streams);
    bool have_dims = false, frame_open = false;
    int64_t Q = 0, tm = 0, undrawn_now = 0;
    int32_t skipped_now = 0;
    int32_t palcur[256];
    for (auto &p : palcur) p = -1;
    std::vector<uint8_t> drawn;
    const uint64_t item_budget = (uint64_t)max_raw * 16;  // bytes of dense items a file may expand to
    auto where = [&]() { return " (frame " + std::to_string(g.frames()) + ", position " + std::to_string(tm) + ")"; };
    auto open_frame = [&]() -> bool {
        if (frame_open) return true;
        const uint64_t need = ((uint64_t)g.frames() + 1) * (uint64_t)Q * 10;
        if (need > item_budget) return fail("the frames' items exceed 16 x max_raw_bytes" + where());
        const size_t sz = (size_t)(g.frames() + 1) * (size_t)Q;
        g.tile.resize(sz, -1);
        g.palrow.resize(sz, -1);
        g.attrs.resize(sz, 0);
        frame_open = true;
        return true;
    };
    while (!c.at_end()) {
        uint32_t w;
        if (!c.u16(w)) return fail("truncated token" + where());
        const uint32_t cmd = w & 63, arg = w >> 6;
        if (cmd != TILER_GTM_SET_DIMENSIONS && !have_dims)
            return fail("command " + std::to_string(cmd) + " before SetDimensions" + where());
        switch (cmd) {
        case TILER_GTM_SET_DIMENSIONS: {
            uint32_t tw, th, ns, cnt;
            if (!c.u16(tw) || !c.u16(th) || !c.u32(ns) || !c.u32(cnt)) return fail("truncated token" + where());
            if (have_dims) {
                if ((int)tw != g.width || (int)th != g.height || (int64_t)cnt != g.n_tiles)
                    return fail("a second SetDimensions changes the size or the tile count (unsupported)" + where());
                break;
            }
            if (tw == 0 || th == 0 || (uint64_t)tw * th > ((uint64_t)1 << 24))
                return fail("SetDimensions: the tilemap is empty or larger than 2^24 positions" + where());
            if ((uint64_t)cnt * 64 > max_raw) return fail("SetDimensions: the tileset exceeds max_raw_bytes" + where());
            g.width = (int)tw;
            g.height = (int)th;
            g.frame_ns = ns;
            g.n_tiles = cnt;
            g.tiles.assign((size_t)cnt * 64, 0);
            Q = g.Q();
            drawn.assign((size_t)Q, 0);
            undrawn_now = Q;
            have_dims = true;
            break;
        }
        case TILER_GTM_TILE_SET: {
            uint32_t t0, t1;
            if (!c.u32(t0) || !c.u32(t1)) return fail("truncated token" + where());
            if (g.frames() > 0 || frame_open) return fail("a TileSet after the first frame (unsupported)" + where());
            if (arg == 0 || (g.palsize && (int)arg != g.palsize))
                return fail("TileSet: palette size 0, or different from an earlier TileSet's" + where());
            if (t0 > t1 || (int64_t)t1 >= g.n_tiles)
                return fail("TileSet: tiles " + std::to_string(t0) + ".." + std::to_string(t1) +
                            " outside the tile count " + std::to_string(g.n_tiles) + where());
            g.palsize = (int)arg;
            uint8_t *dst = g.tiles.data() + (size_t)t0 * 64;
            const size_t nb = ((size_t)t1 - t0 + 1) * 64;
            if (!c.get(dst, nb)) return fail("truncated token (TileSet data)" + where());
            if (g.palsize < 256)
                for (size_t i = 0; i < nb; i++)
                    if (dst[i] >= g.palsize)
                        return fail("TileSet: tile " + std::to_string(t0 + i / 64) + " has a byte >= the palette size" +
                                    where());
            break;
        }
        case TILER_GTM_LOAD_PALETTE: {
            uint32_t idx, fmt;
            if (!c.u8(idx) || !c.u8(fmt)) return fail("truncated token" + where());
            if (!g.palsize) return fail("LoadPalette before any TileSet gave the palette size" + where());
            if (g.pal_rows() >= GTM_MAX_PALROWS) return fail("more than 2^29 LoadPalette commands" + where());
            const size_t at = g.palettes.size();
            g.palettes.resize(at + (size_t)g.palsize);
            std::vector<uint8_t> raw((size_t)g.palsize * 4);
            if (!c.get(raw.data(), raw.size())) return fail("truncated token (LoadPalette data)" + where());
            for (int i = 0; i < g.palsize; i++) g.palettes[at + i] = rd32(raw.data() + 4 * i);
            palcur[idx] = (int32_t)(at / (size_t)g.palsize);
            break;
        }
        case TILER_GTM_SKIP_BLOCK:
            if (!open_frame()) return false;
            if (tm + (int64_t)arg + 1 > Q) return fail("a skip past the end of the tilemap" + where());
            tm += arg + 1;
            skipped_now += (int32_t)arg + 1;
            break;
        case TILER_GTM_SHORT_TILE_IDX:
        case TILER_GTM_LONG_TILE_IDX: {
            uint32_t idx;
            if (!(cmd == TILER_GTM_SHORT_TILE_IDX ? c.u16(idx) : c.u32(idx))) return fail("truncated token" + where());
            if (!open_frame()) return false;
            if (tm >= Q) return fail("an item past the end of the tilemap" + where());
            if ((int64_t)idx >= g.n_tiles)
                return fail("tile index " + std::to_string(idx) + " >= the tile count " + std::to_string(g.n_tiles) +
                            where());
            const int32_t row = palcur[arg >> 2];
            if (row < 0) return fail("palette index " + std::to_string(arg >> 2) + " was never loaded" + where());
            const size_t at = (size_t)g.frames() * (size_t)Q + (size_t)tm;
            g.tile[at] = (int32_t)idx;
            g.attrs[at] = (uint16_t)arg;
            g.palrow[at] = row;
            if (!drawn[(size_t)tm]) {
                drawn[(size_t)tm] = 1;
                undrawn_now--;
            }
            tm++;
            break;
        }
        case TILER_GTM_FRAME_END:
            if (tm != Q)
                return fail("FrameEnd with an incomplete tilemap: position " + std::to_string(tm) + " != " +
                            std::to_string(Q) + where());
            if (!open_frame()) return false;  // (a tilemap can only be complete after a token opened the frame)
            if (g.kf_start.empty() || g.kf_end.back()) g.kf_start.push_back((int32_t)g.frames());
            g.kf_end.push_back((uint8_t)(arg & 1));
            g.skipped.push_back(skipped_now);
            g.undrawn.push_back((int32_t)undrawn_now);
            frame_open = false;
            tm = 0;
            skipped_now = 0;
            break;
        default:
            return fail("unknown command " + std::to_string(cmd) + where());
        }
        if (g.frames() >= INT32_MAX) return fail("more than 2^31 - 1 frames");
    }
    if (frame_open) return fail("truncated token: the stream ends inside a frame" + where());
    if (!have_dims) return fail("no SetDimensions command: not a GTM stream");
    g.kf_start.push_back((int32_t)g.frames());
    return true;
}

}  // namespace

bool gtm_parse(const uint8_t *data, size_t n, int threads, size_t max_raw, GtmData &g) {
    g = GtmData();
    if (!data || n == 0) return fail("empty input");
    if (threads < 0) return fail("threads < 0");
    if (max_raw == 0) max_raw = GTM_DEFAULT_MAX_RAW;
    std::vector<std::vector<uint8_t>> streams;
    uint32_t hdr_w = 0, hdr_h = 0, hdr_kf = 0, hdr_frames = 0;
    if (n >= 4 && std::memcmp(data, "GTMv", 4) == 0) {
        if (n < 40) return fail("truncated GTMv header");
        const uint32_t whole = rd32(data + 8);
        hdr_w = rd32(data + 16);
        hdr_h = rd32(data + 20);
        hdr_kf = rd32(data + 24);
        hdr_frames = rd32(data + 28);
        g.has_header = true;
        g.avg_bytes_per_sec = rd32(data + 32);
        g.kf_max_bytes_per_sec = rd32(data + 36);
        if (whole > n || (uint64_t)40 + (uint64_t)28 * hdr_kf > whole)
            return fail("header: WholeHeaderSize does not hold KFCount keyframe records, or exceeds the file");
        std::vector<size_t> off(hdr_kf), len(hdr_kf);
        size_t at = whole;
        for (uint32_t k = 0; k < hdr_kf; k++) {
            const uint8_t *r = data + 40 + (size_t)28 * k;
            if (std::memcmp(r, "GTMk", 4) != 0) return fail("keyframe record " + std::to_string(k) + ": no GTMk tag");
            const uint32_t comp = rd32(r + 20);
            if (comp > n - at)
                return fail("keyframe record " + std::to_string(k) + ": CompressedSize runs past the end of the file");
            off[k] = at;
            len[k] = comp;
            at += comp;
        }
        if (at != n) return fail(std::to_string(n - at) + " bytes after the last stream");
        streams.resize(hdr_kf);
        std::vector<std::string> msgs(hdr_kf);
        std::vector<size_t> used(hdr_kf, 0);
        std::atomic<uint32_t> next{0};
        auto work = [&]() {
            for (uint32_t k; (k = next.fetch_add(1)) < hdr_kf;)
                if (!decode_stream(data + off[k], len[k], max_raw, streams[k], used[k], msgs[k]) && msgs[k].empty())
                    msgs[k] = "decode failed";
        };
        const int want = threads ? threads : std::min(16, usable_cpus());
        const int nthreads = (int)std::min<uint32_t>((uint32_t)std::max(1, want), std::max<uint32_t>(hdr_kf, 1));
        std::vector<std::thread> pool;
        for (int t = 1; t < nthreads; t++) pool.emplace_back(work);
        work();
        for (auto &t : pool) t.join();
        for (uint32_t k = 0; k < hdr_kf; k++) {
            if (!msgs[k].empty()) return fail("stream " + std::to_string(k) + ": " + msgs[k]);
            if (used[k] != len[k])
                return fail("stream " + std::to_string(k) + " consumed " + std::to_string(used[k]) +
                            " bytes, its CompressedSize is " + std::to_string(len[k]));
            g.stream_comp.push_back(len[k]);
        }
    } else {
        for (size_t at = 0; at < n;) {
            streams.emplace_back();
            std::string msg;
            size_t used = 0;
            if (!decode_stream(data + at, n - at, max_raw, streams.back(), used, msg))
                return fail("stream " + std::to_string(streams.size() - 1) + " at offset " + std::to_string(at) + ": " +
                            msg);
            if (used == 0) return fail("stream at offset " + std::to_string(at) + " consumed nothing");
            g.stream_comp.push_back(used);
            at += used;
        }
    }
    for (auto &s : streams) g.stream_raw.push_back(s.size());
    if (!walk(streams, max_raw, g)) return false;
    if (g.has_header) {
        if ((int64_t)hdr_kf != g.keyframes() || (int64_t)hdr_frames != g.frames())
            return fail("header: KFCount " + std::to_string(hdr_kf) + " / FrameCount " + std::to_string(hdr_frames) +
                        " but the streams hold " + std::to_string(g.keyframes()) + " keyframes / " +
                        std::to_string(g.frames()) + " frames");
        if ((int64_t)(hdr_w / 8) != g.width || (int64_t)(hdr_h / 8) != g.height)
            return fail("header: " + std::to_string(hdr_w) + " x " + std::to_string(hdr_h) +
                        " pixels but SetDimensions gives " + std::to_string(g.width) + " x " +
                        std::to_string(g.height) + " tiles");
    }
    return true;
}

}  // namespace tiler
