// gtm_write.cpp -- the host half of the .gtm writer (plain C++, no HIP headers: it also builds into the stand-alone
// sanitizer check, tools/gtm_write_check.cpp).
//
// GtmPacker: LZCompress (extern.pas:202-240: `lzma.exe e -lc8 -eos`) of a call's keyframe streams with
// tiler_lzma_encode(lc 8, lp 0, pb 2, dictionary 2^21, end marker), one stream per task on a pool of worker threads.
// A stream is handed over as soon as its bytes are on the host, so it is compressed while the next one is copied.
// gtm_assemble: the container as SaveStream leaves it (main.pas:4735-4757) -- the restatement of
// tiler_amd.gtm.assemble_stream, byte for byte.
#include "gtm_write.hpp"

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>

#include "host_error.hpp"

namespace tiler {
namespace {

int usable_cpus() {
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) return std::max(1, CPU_COUNT(&set));
    return (int)std::max(1u, std::thread::hardware_concurrency());
}

std::atomic<int> g_gpu_matches{0};

// with a table of raw's size the finder's answers are read from it (the same bytes); else the host finder
bool compress(const std::vector<uint8_t> &raw, const std::vector<uint32_t> &table, std::vector<uint8_t> &out,
              std::string &msg) {
    const uint8_t none = 0;
    const uint8_t *src = raw.empty() ? &none : raw.data();
    const uint32_t *tab = !raw.empty() && table.size() == raw.size() ? table.data() : nullptr;
    out.resize(raw.size() + raw.size() / 32 + 4096);  // LZMA expands incompressible data by less than 2 %
    size_t n = 0;
    int rc = tiler_lzma_encode_table(src, raw.size(), 8, 0, 2, 1u << 21, 1, tab, out.data(), out.size(), &n);
    if (rc != 0 && n > out.size()) {
        out.resize(n);
        rc = tiler_lzma_encode_table(src, raw.size(), 8, 0, 2, 1u << 21, 1, tab, out.data(), out.size(), &n);
    }
    if (rc != 0) {
        msg = last_error();
        if (msg.empty()) msg = "tiler_lzma_encode failed";
        return false;
    }
    out.resize(n);
    return true;
}

void w32(std::vector<uint8_t> &b, uint32_t v) {
    for (int i = 0; i < 4; i++) b.push_back((uint8_t)(v >> (8 * i)));
}

// an already rounded value as the dword SaveStream stores (Python: fpc_round(x) & 0xFFFFFFFF)
bool as_u32(double r, uint32_t &out) {
    if (!(r > -9.0e18 && r < 9.0e18)) return false;
    out = (uint32_t)(uint64_t)(int64_t)r;
    return true;
}

}  // namespace

int gtm_set_gpu_matches(int on) { return g_gpu_matches.exchange(on ? 1 : 0); }
bool gtm_gpu_matches() { return g_gpu_matches.load() != 0; }

double fpc_round(double x) {
    const double lo = std::floor(x), d = x - lo;  // exact
    if (d > 0.5) return lo + 1.0;
    if (d < 0.5) return lo;
    return std::fmod(lo, 2.0) == 0.0 ? lo : lo + 1.0;
}

GtmPacker::GtmPacker(int keyframes, int threads)
    : raw_((size_t)std::max(0, keyframes)), comp_(raw_.size()), table_(raw_.size()), msg_(raw_.size()) {
    const int want = threads > 0 ? threads : std::min(16, usable_cpus());
    const int n = std::min(want, (int)raw_.size());
    for (int t = 0; t < n; t++) pool_.emplace_back([this] { work(); });
}

GtmPacker::~GtmPacker() {
    {
        std::lock_guard<std::mutex> lk(mu_);
        stop_ = true;
    }
    cv_.notify_all();
    for (auto &t : pool_) t.join();
}

void GtmPacker::ready(int k) {
    {
        std::lock_guard<std::mutex> lk(mu_);
        queue_.push_back(k);
        made_ready_++;
    }
    cv_.notify_one();
}

void GtmPacker::work() {
    for (;;) {
        int k;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [this] { return stop_ || !queue_.empty(); });
            if (stop_) return;
            k = queue_.front();
            queue_.pop_front();
        }
        compress(raw_[(size_t)k], table_[(size_t)k], comp_[(size_t)k], msg_[(size_t)k]);
        {
            std::lock_guard<std::mutex> lk(mu_);
            done_++;
        }
        done_cv_.notify_all();
    }
}

bool GtmPacker::finish() {
    {
        std::unique_lock<std::mutex> lk(mu_);
        if (made_ready_ != keyframes()) {
            set_error("gtm_write: " + std::to_string(keyframes() - made_ready_) + " keyframe streams were never written");
            return false;
        }
        done_cv_.wait(lk, [this] { return done_ == made_ready_; });
    }
    for (int k = 0; k < keyframes(); k++)
        if (!msg_[(size_t)k].empty()) {
            set_error("gtm_write: keyframe stream " + std::to_string(k) + ": " + msg_[(size_t)k]);
            return false;
        }
    return true;
}

bool gtm_assemble(const uint8_t *comps, const size_t *comp_len, const int32_t *kf_start, int keyframes, int width,
                  int height, double fps, std::vector<uint8_t> &out) {
    auto fail = [](const std::string &what) {
        set_error("gtm_assemble: " + what);
        return false;
    };
    if (keyframes <= 0 || !comp_len || !kf_start) return fail("no keyframes, or a null array");
    if (!(fps > 0.0) || !std::isfinite(fps) || width < 0 || height < 0) return fail("fps must be positive and finite");
    if ((uint64_t)keyframes > (UINT32_MAX - 40) / 28) return fail("too many keyframes for WholeHeaderSize");
    if (kf_start[0] != 0) return fail("kf_start[0] must be 0");
    size_t total = 0;
    for (int k = 0; k < keyframes; k++) {
        if (kf_start[k + 1] <= kf_start[k]) return fail("kf_start must increase (keyframe " + std::to_string(k) + ")");
        if (comp_len[k] > UINT32_MAX) return fail("keyframe " + std::to_string(k) + ": CompressedSize exceeds 32 bits");
        total += comp_len[k];
    }
    if (total && !comps) return fail("null streams");
    const int64_t F = kf_start[keyframes];
    uint32_t avg = 0, kfmax = 0;
    double mx = 0.0;
    for (int k = 0; k < keyframes; k++) {
        const int64_t kf_count = (int64_t)kf_start[k + 1] - kf_start[k];
        if (k > 0 || keyframes == 1) mx = std::max(mx, fpc_round((double)comp_len[k] * fps / (double)kf_count));
    }
    if (!as_u32(mx, kfmax) || !as_u32(fpc_round((double)total * fps / (double)F), avg))
        return fail("a byte rate does not fit 64 bits");
    const uint32_t whole = 40 + 28 * (uint32_t)keyframes;
    out.clear();
    out.reserve((size_t)whole + total);
    out.insert(out.end(), {'G', 'T', 'M', 'v'});
    for (uint32_t d : {40u - 8u, whole, 1u, (uint32_t)width, (uint32_t)height, (uint32_t)keyframes, (uint32_t)F, avg,
                       kfmax})
        w32(out, d);
    for (int k = 0; k < keyframes; k++) {
        uint32_t ms = 0;
        if (!as_u32(fpc_round(1000.0 * (double)kf_start[k] / fps), ms)) return fail("a time code does not fit 64 bits");
        out.insert(out.end(), {'G', 'T', 'M', 'k'});
        // RawSize 0: the reference reads ZStream.Size after ZStream.Clear (main.pas:4735-4739)
        for (uint32_t d : {28u - 8u, (uint32_t)k, (uint32_t)kf_start[k], 0u, (uint32_t)comp_len[k], ms}) w32(out, d);
    }
    if (total) out.insert(out.end(), comps, comps + total);
    return true;
}

}  // namespace tiler
