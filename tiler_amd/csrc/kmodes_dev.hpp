// kmodes_dev.hpp -- device helpers of the K-Modes dissimilarity (kmodes.pas:316-453), shared by kmodes.hip and
// reload.hip:  dis = 2048 * #mismatch(80 B) + W0 + W4,  W0 = (|i8(r0-x0)| + 256|i8(r1-x1)| + S_lo) mod 2^16, ...
#pragma once

#include "tiler_common.hpp"

namespace tiler {

static constexpr int KM_A = 80;     // cKModesFeatureCount (kmodes.pas:15)

__device__ __forceinline__ unsigned abs_i8(unsigned r, unsigned x) {
    const int d = (int)(int8_t)(uint8_t)(r - x);  // psubb + pabsb
    return (unsigned)(d < 0 ? -d : d);
}

__device__ __forceinline__ unsigned nz_bytes(unsigned t) {  // number of non-zero bytes of t
    const unsigned m = (((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) & 0x80808080u;
    return __popc(m);
}

// row = list entry (centroid / member), x = item (kmodes.pas:341-412)
__device__ __forceinline__ unsigned long long km_dissim(const uint32_t *__restrict__ r, const uint32_t *__restrict__ x) {
    unsigned mism = 0, slo = 0, shi = 0;
#pragma unroll
    for (int w = 0; w < 20; w++) mism += nz_bytes(r[w] ^ x[w]);
#pragma unroll
    for (int w = 4; w < 20; w += 4) {
        slo = __builtin_amdgcn_sad_u8(r[w], x[w], slo);
        slo = __builtin_amdgcn_sad_u8(r[w + 1], x[w + 1], slo);
        shi = __builtin_amdgcn_sad_u8(r[w + 2], x[w + 2], shi);
        shi = __builtin_amdgcn_sad_u8(r[w + 3], x[w + 3], shi);
    }
    const unsigned r0 = r[0], x0 = x[0], r2 = r[2], x2 = x[2];
    const unsigned w0 = (abs_i8(r0 & 255, x0 & 255) + 256u * abs_i8((r0 >> 8) & 255, (x0 >> 8) & 255) + slo) & 0xffffu;
    const unsigned w4 = (abs_i8(r2 & 255, x2 & 255) + 256u * abs_i8((r2 >> 8) & 255, (x2 >> 8) & 255) + shi) & 0xffffu;
    return ((unsigned long long)mism << 11) + w0 + w4;
}

__device__ __forceinline__ void load_row(const uint8_t *__restrict__ p, uint32_t (&w)[20]) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const uint4 v = q[i];
        w[4 * i] = v.x;
        w[4 * i + 1] = v.y;
        w[4 * i + 2] = v.z;
        w[4 * i + 3] = v.w;
    }
}

// ---- rows with at most 16 modalities (round 3) ----
// With every byte of both rows < 16 the asm's int8 |r - x| is the plain |r - x| <= 15 and W0 / W4 never wrap (a0 +
// 256 a1 + S_lo <= 15 + 3,840 + 480 < 2^16):
//   dis = 2048 #mismatch + (a0 + a8) + 256 (a1 + a9) + sum_{k=16..79} |r_k - x_k|   (= km_dissim).
// A byte differs iff one of its 4 bit planes differs, so #mismatch is, per 32 bytes, the popcount of the OR of the
// 4 planes' XORs (3 words) instead of a nonzero-byte count per dword, and the L1 is one v_sad_u8 chain over bytes
// 16..79 plus two over the packed words (byte 0 | byte 8 << 8) and (byte 1 | byte 9 << 8): ~40 VALU per pair
// instead of ~155.  Prepared row, KM_PW words: [0, 16) bytes 16..79, [16, 28) planes (word 16 + 3p + k = bit p of
// bytes 32k .. 32k + 31), 28 the low word, 29 the high word, 30-31 zero.
static constexpr int KM_PW = 32;

__device__ __forceinline__ uint32_t km_prep_word(const uint32_t *row, int w) {
    if (w < 16) return row[4 + w];
    if (w < 28) {
        const int p = (w - 16) / 3, k = (w - 16) % 3;
        uint32_t r = 0;
        for (int j = 0; j < 8 && 8 * k + j < 20; j++) {
            // bits p of the 4 bytes of dword 8k + j -> 4 consecutive bits: (b0 | b1 << 8 | b2 << 16 | b3 << 24) *
            // 0x01020408 puts b_i at bit 24 + i and nothing else in bits 24..31
            const uint32_t v = (row[8 * k + j] >> p) & 0x01010101u;
            r |= ((v * 0x01020408u) >> 24) << (4 * j);
        }
        return r;
    }
    if (w == 28) return (row[0] & 0xFFu) | ((row[2] & 0xFFu) << 8);
    if (w == 29) return ((row[0] >> 8) & 0xFFu) | (((row[2] >> 8) & 0xFFu) << 8);
    return 0;
}

__device__ __forceinline__ unsigned km_dissim16(const uint32_t *__restrict__ r, const uint32_t *__restrict__ x) {
    unsigned l1 = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) l1 = __builtin_amdgcn_sad_u8(r[w], x[w], l1);
    l1 = __builtin_amdgcn_sad_u8(r[28], x[28], l1);
    const unsigned hi = __builtin_amdgcn_sad_u8(r[29], x[29], 0u);
    unsigned mism = 0;
#pragma unroll
    for (int k = 0; k < 3; k++)
        mism += __popc((r[16 + k] ^ x[16 + k]) | (r[19 + k] ^ x[19 + k]) | (r[22 + k] ^ x[22 + k]) | (r[25 + k] ^ x[25 + k]));
    return (mism << 11) + l1 + (hi << 8);
}

}  // namespace tiler
