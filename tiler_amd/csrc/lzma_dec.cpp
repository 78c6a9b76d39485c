// lzma_dec.cpp -- LZMA-alone (.lzma) decoder for the GTM keyframe streams (host code in libANN.so, no HIP headers:
// it also builds into the stand-alone sanitizer check, tools/gtm_read_check.cpp).
//
// The inverse of lzma_alone.cpp over the published LZMA bitstream: 13-byte header (properties (pb * 5 + lp) * 9 + lc,
// dictionary size u32, uncompressed size u64, all ones = an end marker is required), then the range-coded body.  Any
// valid lc / lp / pb is accepted.  The output buffer is the window (a GTM keyframe stream is decoded whole); a
// distance past the bytes written so far, or not below the dictionary size, is corrupt, and so is a range coder that
// does not end at 0 (what an encoder's flush leaves), which catches damage in a stream's last bytes.
// The range decoder normalises after each bit, so `consumed` is exact: the bytes an encoder wrote for this stream,
// which lets concatenated streams be walked.  Every input byte is fetched through a bounds check (a read past `n`
// marks the stream truncated) and every output byte is stored below `cap`.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tiler_ann.h"
#include "host_error.hpp"

namespace {

constexpr uint16_t kInit = 1024;  // probability 0.5 in 11 bits

struct RangeDec {
    const uint8_t *in;
    size_t n, pos = 0;
    uint32_t range = 0xFFFFFFFFu, code = 0;
    bool eof = false;  // a byte past the end was asked for

    uint8_t byte() {
        if (pos >= n) {
            eof = true;
            return 0;
        }
        return in[pos++];
    }
    void norm() {
        if (range < (1u << 24)) {
            range <<= 8;
            code = (code << 8) | byte();
        }
    }
    int bit(uint16_t &p) {
        const uint32_t bound = (range >> 11) * p;
        int b;
        if (code < bound) {
            range = bound;
            p += (uint16_t)((2048 - p) >> 5);
            b = 0;
        } else {
            range -= bound;
            code -= bound;
            p -= (uint16_t)(p >> 5);
            b = 1;
        }
        norm();
        return b;
    }
    uint32_t direct(int nbits) {
        uint32_t v = 0;
        for (int i = 0; i < nbits; i++) {
            range >>= 1;
            const uint32_t t = code >= range;
            if (t) code -= range;
            v = (v << 1) | t;
            norm();
        }
        return v;
    }
    uint32_t tree(uint16_t *p, int nbits) {  // MSB first
        uint32_t m = 1;
        for (int i = 0; i < nbits; i++) m = (m << 1) | (uint32_t)bit(p[m]);
        return m - (1u << nbits);
    }
    uint32_t tree_rev(uint16_t *p, int nbits) {  // LSB first
        uint32_t m = 1, v = 0;
        for (int i = 0; i < nbits; i++) {
            const uint32_t b = (uint32_t)bit(p[m]);
            m = (m << 1) | b;
            v |= b << i;
        }
        return v;
    }
};

struct LenDec {
    uint16_t choice = kInit, choice2 = kInit, low[16][8], mid[16][8], high[256];
    LenDec() {
        for (auto &a : low) for (auto &p : a) p = kInit;
        for (auto &a : mid) for (auto &p : a) p = kInit;
        for (auto &p : high) p = kInit;
    }
    uint32_t decode(RangeDec &rc, int ps) {  // length - 2
        if (!rc.bit(choice)) return rc.tree(low[ps], 3);
        if (!rc.bit(choice2)) return 8 + rc.tree(mid[ps], 3);
        return 16 + rc.tree(high, 8);
    }
};

int fail(const char *what) {
    tiler::set_error(std::string("tiler_lzma_decode: ") + what);
    return -1;
}

}  // namespace

extern "C" int tiler_lzma_decode(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *out_len,
                                 size_t *consumed) {
    if (out_len) *out_len = 0;
    if (consumed) *consumed = 0;
    if ((!src && n) || (!dst && cap) || !out_len) return fail("bad arguments");
    if (n < 13) return fail("truncated stream (the header is 13 bytes)");
    const int props = src[0];
    if (props >= 9 * 5 * 5) return fail("corrupt stream (properties byte out of range)");
    const int lc = props % 9, lp = (props / 9) % 5, pb = props / 45;
    uint64_t usize = 0;
    for (int i = 0; i < 8; i++) usize |= (uint64_t)src[5 + i] << (8 * i);
    const bool known = usize != UINT64_MAX;
    uint32_t dict = (uint32_t)src[1] | (uint32_t)src[2] << 8 | (uint32_t)src[3] << 16 | (uint32_t)src[4] << 24;
    if (dict < 4096) dict = 4096;  // the format's minimum
    if (known && usize > cap) {  // nothing is decoded: the header says how much room the caller needs
        *out_len = usize > (uint64_t)SIZE_MAX ? SIZE_MAX : (size_t)usize;
        return TILER_LZMA_GROW;
    }

    std::vector<uint16_t> lit((size_t)0x300 << (lc + lp), kInit);
    uint16_t is_match[12][16], is_rep[12], is_rep_g0[12], is_rep_g1[12], is_rep_g2[12], is_rep0_long[12][16];
    uint16_t pos_slot[4][64], pos_special[128], align[16];
    for (int s = 0; s < 12; s++) {
        is_rep[s] = is_rep_g0[s] = is_rep_g1[s] = is_rep_g2[s] = kInit;
        for (int j = 0; j < 16; j++) is_match[s][j] = is_rep0_long[s][j] = kInit;
    }
    for (auto &a : pos_slot) for (auto &p : a) p = kInit;
    for (auto &p : pos_special) p = kInit;
    for (auto &p : align) p = kInit;
    LenDec len_dec, rep_len_dec;

    RangeDec rc{src, n, 13};
    if (rc.byte() != 0) return fail("corrupt stream (the first range-coder byte is not 0)");
    for (int i = 0; i < 4; i++) rc.code = (rc.code << 8) | rc.byte();

    const uint32_t pb_mask = (1u << pb) - 1, lp_mask = (1u << lp) - 1;
    uint32_t rep0 = 0, rep1 = 0, rep2 = 0, rep3 = 0;
    int state = 0;
    size_t op = 0;
    const char *bad = nullptr;
    bool grow = false, done = false;
    while (!rc.eof) {
        if (known && op == usize) {
            done = true;
            break;
        }
        const int ps = (int)(op & pb_mask);
        if (!rc.bit(is_match[state][ps])) {  // literal
            const uint32_t prev = op ? dst[op - 1] : 0;
            uint16_t *p = &lit[(size_t)0x300 * ((((uint32_t)op & lp_mask) << lc) + (prev >> (8 - lc)))];
            uint32_t sym = 1;
            if (state >= 7) {  // after a match: the byte at rep0 steers the tree until the first differing bit
                if (op <= rep0 || rep0 >= dict) {
                    bad = "corrupt stream (distance past the start of the output)";
                    break;
                }
                uint32_t mb = dst[op - rep0 - 1], offs = 0x100;
                while (sym < 0x100) {
                    mb <<= 1;
                    const uint32_t mbit = mb & offs;
                    const int b = rc.bit(p[offs + mbit + sym]);
                    sym = (sym << 1) | (uint32_t)b;
                    offs &= b ? mbit : ~mbit;
                }
            } else {
                while (sym < 0x100) sym = (sym << 1) | (uint32_t)rc.bit(p[sym]);
            }
            if (op >= cap) {
                grow = true;
                break;
            }
            dst[op++] = (uint8_t)sym;
            state = state < 4 ? 0 : state < 10 ? state - 3 : state - 6;
            continue;
        }
        uint32_t len;
        if (rc.bit(is_rep[state])) {
            if (op == 0) {
                bad = "corrupt stream (repeated match before any output)";
                break;
            }
            if (!rc.bit(is_rep_g0[state])) {
                if (!rc.bit(is_rep0_long[state][ps])) {  // short rep: one byte at rep0
                    state = state < 7 ? 9 : 11;
                    if (op <= rep0 || rep0 >= dict) {
                        bad = "corrupt stream (distance past the start of the output)";
                        break;
                    }
                    if (op >= cap) {
                        grow = true;
                        break;
                    }
                    dst[op] = dst[op - rep0 - 1];
                    op++;
                    continue;
                }
            } else {
                uint32_t d;
                if (!rc.bit(is_rep_g1[state])) {
                    d = rep1;
                } else if (!rc.bit(is_rep_g2[state])) {
                    d = rep2;
                    rep2 = rep1;
                } else {
                    d = rep3;
                    rep3 = rep2;
                    rep2 = rep1;
                }
                rep1 = rep0;
                rep0 = d;
            }
            len = rep_len_dec.decode(rc, ps);
            state = state < 7 ? 8 : 11;
        } else {
            rep3 = rep2;
            rep2 = rep1;
            rep1 = rep0;
            len = len_dec.decode(rc, ps);
            state = state < 7 ? 7 : 10;
            const uint32_t slot = rc.tree(pos_slot[len < 3 ? len : 3], 6);
            uint32_t dist = slot;
            if (slot >= 4) {
                const int footer = (int)(slot >> 1) - 1;
                dist = (2 | (slot & 1)) << footer;
                if (slot < 14) {
                    dist += rc.tree_rev(pos_special + dist - slot - 1, footer);
                } else {
                    dist += rc.direct(footer - 4) << 4;
                    dist += rc.tree_rev(align, 4);
                }
            }
            if (dist == 0xFFFFFFFFu) {  // end marker
                if (known && op != usize)
                    bad = "corrupt stream (end marker before the size in the header)";
                else
                    done = true;
                break;
            }
            rep0 = dist;
        }
        len += 2;
        if (op <= rep0 || rep0 >= dict) {
            bad = "corrupt stream (distance past the start of the output)";
            break;
        }
        if (known && len > usize - op) {
            bad = "corrupt stream (match runs past the size in the header)";
            break;
        }
        if (len > cap - op) {
            grow = true;
            break;
        }
        const uint8_t *from = dst + op - rep0 - 1;  // may overlap the bytes being written: byte by byte
        for (uint32_t i = 0; i < len; i++) dst[op + i] = from[i];
        op += len;
    }
    if (rc.eof) return fail("truncated stream");
    if (bad) return fail(bad);
    *out_len = op;
    if (grow) return TILER_LZMA_GROW;
    if (!done) return fail("truncated stream");
    if (rc.code != 0) return fail("corrupt stream (the range coder does not end at 0)");
    if (consumed) *consumed = rc.pos;
    return 0;
}
