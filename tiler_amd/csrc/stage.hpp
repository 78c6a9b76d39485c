// stage.hpp -- per-call device blocks, pool streams and the staging of every host-buffer entry point.
#pragma once

#include <algorithm>
#include <string>
#include <vector>

#include "tiler_common.hpp"

namespace tiler {

// device blocks of one call: the stream is drained before they go back to the cache (dfree's rule)
struct Blocks {
    hipStream_t st;
    std::vector<void *> p;
    explicit Blocks(hipStream_t s) : st(s) {}
    ~Blocks() {
        if (p.empty()) return;
        (void)hipStreamSynchronize(st);
        for (void *b : p) dfree(b);
    }
    template <class T>
    bool get(T *&out, size_t bytes) {
        void *b = nullptr;
        if (dmalloc(&b, std::max<size_t>(bytes, 256)) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        p.push_back(b);
        out = (T *)b;
        return true;
    }
};

struct PoolStream {
    hipStream_t st = nullptr;
    bool ok;
    PoolStream() : ok(stream_get(&st) == hipSuccess) {}
    ~PoolStream() {
        if (ok) stream_put(st);
    }
};

// The host-buffer form of an operation: every array is a block of its own (256-byte aligned), copied in on a pool
// stream as it is requested; the _dev form then runs on stream(), and finish() copies the results back and waits for
// that stream alone.  A null host array is a null device array (an optional argument); an empty one still has a block.
// A failure is sticky and sets "<who>: ..." once; the message of a failed _dev callee is the callee's own.
class HostStage {
  public:
    explicit HostStage(const char *who) : who_(who), blocks_(ps_.st) {
        if (!ps_.ok) fail("no stream");
    }
    template <class T>
    T *in(const T *h, size_t count) {
        return (T *)add(const_cast<T *>(h), count * sizeof(T), true, false);
    }
    template <class T>
    T *out(T *h, size_t count) {
        return (T *)add(h, count * sizeof(T), false, true);
    }
    template <class T>
    T *inout(T *h, size_t count) {
        return (T *)add(h, count * sizeof(T), true, true);
    }
    bool ok() const { return ok_; }
    hipStream_t stream() const { return ps_.st; }
    // the results to the host arrays; 0, or -1 with the error set
    int finish() {
        for (const Out &o : outs_)
            if (ok_ && o.bytes) check(hipMemcpyAsync(o.h, o.d, o.bytes, hipMemcpyDeviceToHost, ps_.st));
        if (ok_) check(hipStreamSynchronize(ps_.st));
        return ok_ ? 0 : -1;
    }

  private:
    struct Out {
        void *h, *d;
        size_t bytes;
    };
    void *add(void *h, size_t bytes, bool copy_in, bool copy_out) {
        void *d = nullptr;
        if (!h || !ok_) return nullptr;
        if (!blocks_.get(d, bytes)) {
            fail("out of device memory");
            return nullptr;
        }
        if (copy_in && bytes) check(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ps_.st));
        if (copy_out) outs_.push_back({h, d, bytes});
        return d;
    }
    void check(hipError_t e) {
        if (e == hipSuccess) return;
        (void)hipGetLastError();
        fail(std::string("copy failed: ") + hipGetErrorString(e));
    }
    void fail(const std::string &what) {
        if (ok_) set_error(std::string(who_) + ": " + what);
        ok_ = false;
    }
    const char *who_;
    bool ok_ = true;
    PoolStream ps_;   // destroyed last: the blocks drain the stream and go back first
    Blocks blocks_;
    std::vector<Out> outs_;
};

}  // namespace tiler
