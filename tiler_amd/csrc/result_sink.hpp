// result_sink.hpp -- where a search publishes a query's answer.  Every tier of nn_search.hip, orbit.hip and the kd
// replay of kdtree.hip ends here: the functions below are the only code that writes through these pointers.
// (Its own header: KdFixArgs of kdtree.hpp embeds the struct, and nn_dev.hpp's MFMA / LDS-DMA helpers have no place
// in the host-side translation units that include kdtree.hpp.)
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tiler {

struct ResultSink {
    int *idx = nullptr;      // [nq][k] results in HBM
    float *err = nullptr;
    int *h_idx = nullptr;    // host-visible pinned copies of the same (SearchOpts::h_idx), null: none
    float *h_err = nullptr;
    // FrameTiling (k == 1): candidate -> tilemap item lookup and the tilemap outputs [nq]; m_tile null: no maps
    const int32_t *tr_tile = nullptr, *tr_pal = nullptr;
    const uint8_t *tr_attr = nullptr;
    int32_t *m_tile = nullptr, *m_pal = nullptr;
    uint8_t *m_hm = nullptr, *m_vm = nullptr;

    // "no candidate": a negative id or the lists' 0x7fffffff sentinel
    static __device__ __forceinline__ bool none(int c) { return (unsigned)c >= 0x7fffffffu; }

    // result slot r of query q in a search of k: candidate c at distance d, or -1 / FLT_MAX
    __device__ __forceinline__ void put(long q, int r, int k, int c, float d) const {
        const bool ok = !none(c);
        const int oi = ok ? c : -1;
        const float oe = ok ? d : FLT_MAX;
        idx[q * k + r] = oi;
        err[q * k + r] = oe;
        if (h_idx) {
            h_idx[q * k + r] = oi;
            h_err[q * k + r] = oe;
        }
    }
    // the tilemap item of query q from its best candidate, or -1, -1, 0, 0
    __device__ __forceinline__ void put_map(long q, int best) const {
        if (!m_tile) return;
        const bool ok = !none(best);
        m_tile[q] = ok ? tr_tile[best] : -1;
        m_pal[q] = ok ? tr_pal[best] : -1;
        const int at = ok ? tr_attr[best] : 0;
        m_hm[q] = (at & 1) != 0;
        m_vm[q] = (at & 2) != 0;
    }
    // both, for a k == 1 search
    __device__ __forceinline__ void put1(long q, int c, float d) const {
        put(q, 0, 1, c, d);
        put_map(q, c);
    }
};

}  // namespace tiler
