// lzma_table_check.cpp -- stand-alone check of the LZMA match-table host code (lzma_alone.cpp: tiler_lzma_match_table,
// tiler_lzma_encode_table) under the host sanitizers.  No HIP, no GPU, nothing loaded into another process:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/lzma_table_check.cpp tiler_amd/csrc/lzma_alone.cpp tiler_amd/csrc/lzma_dec.cpp -o lzma_table_check \
//       && ./lzma_table_check
// (tests/test_lzma_match_host.py does this).  Over the kinds of input of that test -- lengths 0 to 5, equal bytes,
// random bytes, words of a small alphabet, text, a near copy in front of an exact one, a period -- it builds the host
// table, runs both encoders for three lc / lp / pb settings, compares the bytes and decodes them; then it feeds
// tables with one wrong entry of every kind (and tables of random words) and expects -1, or a stream that decodes to
// the input, never anything else.  Every buffer is a heap block of the exact size, so a read past it is reported.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../include/tiler_ann.h"
#include "../tiler_amd/csrc/host_error.hpp"

namespace tiler {
static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
const char *last_error() { return g_err.c_str(); }
}  // namespace tiler

namespace {

using Bytes = std::vector<uint8_t>;
using Table = std::vector<uint32_t>;
constexpr uint32_t kDict = 1u << 21;

int failures = 0;
void expect(bool ok, const std::string &what) {
    if (ok) return;
    failures++;
    std::fprintf(stderr, "FAIL: %s\n", what.c_str());
}

// 0 and the stream, or -1; src and table are handed over as exact-size heap blocks
int encode(const Bytes &src, int lc, int lp, int pb, uint32_t dict, int eos, const Table *table, Bytes &out) {
    const uint8_t none = 0;
    const uint8_t *s = src.empty() ? &none : src.data();
    size_t n = 0;
    const uint32_t *t = table && !table->empty() ? table->data() : nullptr;
    if (tiler_lzma_encode_table(s, src.size(), lc, lp, pb, dict, eos, t, nullptr, 0, &n) != 0) return -1;
    out.assign(n, 0);
    return tiler_lzma_encode_table(s, src.size(), lc, lp, pb, dict, eos, t, out.data(), out.size(), &n);
}

bool decodes_to(const Bytes &comp, const Bytes &want) {
    Bytes out(want.size() + 1);
    size_t n = 0, used = 0;
    return tiler_lzma_decode(comp.data(), comp.size(), out.data(), out.size(), &n, &used) == 0 && n == want.size() &&
           used == comp.size() && (n == 0 || std::memcmp(out.data(), want.data(), n) == 0);
}

Table table_of(const Bytes &src, uint32_t dict) {
    Table t(src.size());
    uint32_t none = 0;
    expect(tiler_lzma_match_table(src.data(), src.size(), dict, t.empty() ? &none : t.data()) == 0,
           std::string("match_table: ") + tiler::last_error());
    return t;
}

Bytes random_bytes(std::mt19937 &rng, size_t n, int alphabet = 256) {
    Bytes b(n);
    for (auto &x : b) x = (uint8_t)(rng() % (uint32_t)alphabet);
    return b;
}

std::vector<std::pair<std::string, Bytes>> inputs() {
    std::mt19937 rng(20241021);
    std::vector<std::pair<std::string, Bytes>> in;
    const char *small[] = {"", "a", "ab", "aaa", "abca", "abcab"};
    for (const char *s : small) in.push_back({std::string("len ") + std::to_string(std::strlen(s)), Bytes(s, s + std::strlen(s))});
    in.push_back({"equal", Bytes(1000, 0)});
    in.push_back({"random", random_bytes(rng, 4096)});
    Bytes words;
    for (int i = 0; i < 1500; i++) {
        words.push_back((uint8_t)(rng() % 8));
        words.push_back(0);
    }
    in.push_back({"words8", words});
    Bytes text;
    const std::string line = "the quick brown fox jumps over the lazy dog. ";
    while (text.size() < 2500) text.insert(text.end(), line.begin(), line.end());
    text.resize(2500);
    in.push_back({"text", text});
    Bytes block = random_bytes(rng, 300), near = block, nice = block;
    near[200] ^= 0x55;
    nice.insert(nice.end(), 10, 0);
    nice.insert(nice.end(), near.begin(), near.end());
    nice.insert(nice.end(), 10, 0);
    nice.insert(nice.end(), block.begin(), block.end());
    in.push_back({"nice", nice});
    Bytes unit = random_bytes(rng, 700), period;
    while (period.size() < 4000) period.insert(period.end(), unit.begin(), unit.end());
    period.resize(4000);
    in.push_back({"period", period});
    return in;
}

}  // namespace

int main() {
    const int props[3][3] = {{8, 0, 2}, {3, 0, 2}, {0, 2, 0}};
    size_t streams = 0;
    for (const auto &in : inputs()) {
        const Bytes &src = in.second;
        const Table t = table_of(src, kDict);
        for (const auto &pr : props)
            for (int eos = 0; eos < 2; eos++) {
                Bytes a, b;
                expect(encode(src, pr[0], pr[1], pr[2], kDict, eos, nullptr, a) == 0, in.first + ": encode");
                expect(encode(src, pr[0], pr[1], pr[2], kDict, eos, &t, b) == 0,
                       in.first + ": encode_table: " + tiler::last_error());
                expect(a == b, in.first + ": the table encoder writes the encoder's bytes");
                expect(decodes_to(b, src), in.first + ": the stream decodes to the input");
                streams++;
            }
    }

    // one wrong entry of every kind, at the first entry the parse reads
    const auto in = inputs();
    const Bytes &text = in[9].second;
    const Table good = table_of(text, kDict);
    size_t p = 0;
    while (p < good.size() && good[p] == 0) p++;
    expect(p > 0 && p < good.size(), "the text has a match");
    auto refused = [&](const Bytes &src, const Table &t, uint32_t dict, size_t at, const std::string &what) {
        Bytes out;
        const int rc = encode(src, 8, 0, 2, dict, 1, &t, out);
        expect(rc == -1 && std::strstr(tiler::last_error(), ("position " + std::to_string(at) + " ").c_str()),
               what + ": refused, naming the position (" + tiler::last_error() + ")");
    };
    {
        Bytes cut(text.begin(), text.begin() + 200);
        Table t = table_of(cut, kDict);
        size_t q = 0;
        while (t[q] == 0) q++;
        t[q] = (uint32_t)(cut.size() - q + 1) | (t[q] >> 9) << 9;
        refused(cut, t, kDict, q, "a length past the end of the buffer");
    }
    {
        Table t = good;
        t[p] = (t[p] & 511) | (uint32_t)p << 9;
        refused(text, t, kDict, p, "a distance past the start of the buffer");
        t[p] = 1 | (good[p] >> 9) << 9;
        refused(text, t, kDict, p, "length 1");
        t[p] = 274;
        refused(text, t, kDict, p, "length 274");
        uint32_t d = 0;
        while (text[p - d - 1] == text[p]) d++;
        t[p] = 2 | d << 9;
        refused(text, t, kDict, p, "bytes that differ");
    }
    {
        std::mt19937 rng(5);
        const Bytes unit = random_bytes(rng, 4300);
        Bytes far = unit;
        far.insert(far.end(), unit.begin(), unit.begin() + 300);
        const Table full = table_of(far, kDict);
        Table t(far.size(), 0);
        t[4300] = full[4300];
        expect((full[4300] >> 9) == 4299, "a match 4,300 bytes back");
        refused(far, t, 4096, 4300, "a distance past the dictionary");
    }
    {
        Bytes out;
        const Table t(text.size(), 0);
        expect(encode(text, 8, 0, 2, kDict + 1, 1, &t, out) == -1 && std::strstr(tiler::last_error(), "2^21"),
               "a dictionary above 2^21 with a table");
        Table u(text.size());
        expect(tiler_lzma_match_table(text.data(), text.size(), kDict + 1, u.data()) == -1, "match_table, dict > 2^21");
        expect(encode(text, 8, 0, 2, 1u << 24, 1, nullptr, out) == 0 && decodes_to(out, text), "no table: any dictionary");
    }
    // tables of arbitrary words: -1, or a stream that decodes to the input
    {
        std::mt19937 rng(99);
        int refusals = 0, accepted = 0;
        for (int round = 0; round < 200; round++) {
            Table t = good;
            for (int k = 0; k < 4; k++) {
                const size_t at = rng() % t.size();
                t[at] = round % 2 ? (uint32_t)rng() : (2 + rng() % 272) | (rng() % 3000) << 9;
            }
            Bytes out;
            if (encode(text, 8, 0, 2, kDict, 1, &t, out) == 0) {
                accepted++;
                expect(decodes_to(out, text), "an accepted table decodes to the input");
            } else {
                refusals++;
            }
        }
        expect(refusals > 0 && accepted > 0, "random tables are both refused and accepted");
    }
    if (failures) return 1;
    std::printf("lzma_table_check ok: %zu streams compared\n", streams);
    return 0;
}
