// gtm_write.hpp -- the .gtm writer (SaveStream main.pas:4529-4763): the command words built on gfx950 (gtm_write.hip)
// and the host half, LZMA per keyframe on a thread pool and the container (gtm_write.cpp).  Plain C++, no HIP headers:
// the host half also builds into the stand-alone sanitizer check (tools/gtm_write_check.cpp).
#pragma once

#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/tiler_ann.h"

namespace tiler {

// ---- host half (gtm_write.cpp) --------------------------------------------------------------------------------------
// LZCompress (extern.pas:202-240) of a call's keyframe streams: at most `threads` workers (0: min(16, usable CPUs)),
// never more than keyframes.  The producer fills raw(k) and calls ready(k); a worker compresses k from then on, so
// keyframe k is compressed while k + 1 is still being copied from the device.
class GtmPacker {
  public:
    GtmPacker(int keyframes, int threads);
    ~GtmPacker();  // stops and joins the workers (streams never made ready are dropped)
    GtmPacker(const GtmPacker &) = delete;
    GtmPacker &operator=(const GtmPacker &) = delete;
    std::vector<uint8_t> &raw(int k) { return raw_[(size_t)k]; }
    // stream k's match table (tiler_lzma_encode_table), one entry per byte of raw(k); left empty: the host finder
    std::vector<uint32_t> &table(int k) { return table_[(size_t)k]; }
    void ready(int k);
    // waits until every keyframe is compressed; false with set_error() when one failed (or was never made ready)
    bool finish();
    const std::vector<uint8_t> &comp(int k) const { return comp_[(size_t)k]; }
    int keyframes() const { return (int)raw_.size(); }

  private:
    void work();
    std::vector<std::vector<uint8_t>> raw_, comp_;
    std::vector<std::vector<uint32_t>> table_;
    std::vector<std::string> msg_;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    std::deque<int> queue_;
    int made_ready_ = 0, done_ = 0;
    bool stop_ = false;
    std::vector<std::thread> pool_;
};

// tiler_gtm_set_gpu_matches: the process-wide switch (atomic), read by gtm_pack_dev
int gtm_set_gpu_matches(int on);
bool gtm_gpu_matches();

// FPC Round: to nearest, ties to even, whatever the floating-point rounding mode is
double fpc_round(double x);

// TGTMHeader (main.pas:103-114), one TGTMKeyFrameInfo per keyframe (116-124) and the streams, as SaveStream leaves
// them (4735-4757): RawSize 0, KFMaxBytesPerSec over keyframes k > 0 (or the only one), FPC Round.  comps = the
// keyframes' compressed streams back to back, comp_len[KF]; kf_start[KF + 1] = 0 < ... < F.  false with set_error().
bool gtm_assemble(const uint8_t *comps, const size_t *comp_len, const int32_t *kf_start, int keyframes, int width,
                  int height, double fps, std::vector<uint8_t> &out);

// ---- device half (gtm_write.hip); `stream` is a hipStream_t ------------------------------------------------------------
// See include/tiler_ann.h: tiler_gtm_commands_dev / tiler_gtm_commands / tiler_gtm_streams(_dev) / tiler_gtm_write(_dev).
int gtm_commands_dev(const tiler_gtm_source_t *src, uint8_t *d_raw, size_t cap, int64_t *raw_off, void *stream);
int gtm_commands_host(const tiler_gtm_source_t *src, uint8_t *raw, size_t cap, int64_t *raw_off);
// whole_file: assemble the streams (src->first_keyframe must be set); else the streams back to back + comp_len[KF]
int gtm_pack_dev(const tiler_gtm_source_t *src, int threads, bool whole_file, uint8_t *dst, size_t cap,
                 size_t *comp_len, size_t *out_len, void *stream);
int gtm_pack_host(const tiler_gtm_source_t *src, int threads, bool whole_file, uint8_t *dst, size_t cap,
                  size_t *comp_len, size_t *out_len);

}  // namespace tiler
