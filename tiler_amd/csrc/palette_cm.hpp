// palette_cm.hpp -- the colour-map items of QuantizePalette (TCountIndexArray, main.pas:193-196) and the integer
// colour helpers around them, one definition for host and device so both give the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tiler {

struct CmItem {  // TCountIndexArray without Count
    int index, luma;
    uint8_t hue, sat, val;
};

__host__ __device__ inline int muldiv_win(int a, int b, int c) {  // Windows MulDiv: rounded half away from 0
    if (c == 0) return -1;
    if (c < 0) {
        a = -a;
        c = -c;
    }
    const long long prod = (long long)a * b;
    const bool add = (a < 0 && b < 0) || (a >= 0 && b >= 0);  // the operands' signs pick the rounding direction
    const long long r = add ? (prod + c / 2) / c : (prod - c / 2) / c;
    if (r > 2147483647LL || r < -2147483647LL) return -1;
    return (int)r;
}

// FColorMap / FColorMapLuma (main.pas:4835-4847) + RGBToHSV (main.pas:3496-3543)
__host__ __device__ inline CmItem cm_item(int32_t col) {
    const int rr = col & 255, gg = (col >> 8) & 255, bb = (col >> 16) & 255;
    const int mgb = gg > bb ? gg : bb, ngb = gg < bb ? gg : bb;
    const int mx = rr > mgb ? rr : mgb, mn = rr < ngb ? rr : ngb;
    int hh = 0, ss = 0;
    if (mx != mn) {
        const int delta = mx - mn;
        ss = muldiv_win(delta, 255, mx);
        if (rr == mx)
            hh = muldiv_win(42, gg - bb, delta);
        else if (gg == mx)
            hh = muldiv_win(42, bb - rr, delta) + 84;
        else
            hh = muldiv_win(42, rr - gg, delta) + 168;
        hh %= 252;
    }
    CmItem it;
    it.index = col;
    it.luma = (rr * 2126 + gg * 7152 + bb * 722) / 10000;
    it.hue = (uint8_t)(hh & 255);
    it.sat = (uint8_t)(ss & 255);
    it.val = (uint8_t)(mx & 255);
    return it;
}

__host__ __device__ inline int32_t cm_to_rgb(int r, int g, int b) { return (b << 16) | (g << 8) | r; }  // main.pas:566

__host__ __device__ inline int32_t cm_hsv_to_rgb(int h, int s, int v) {  // HSVToRGB (main.pas:3545-3579), bytes in
    if (s == 0) return cm_to_rgb(v, v, v);
    h %= 252;
    const int f = h % 42;
    h /= 42;
    const int ls = v * s;
    const int p = v - ls / 255, q = v - (ls * f) / (255 * 42), r = v - (ls * (42 - f)) / (255 * 42);
    switch (h) {
        case 0: return cm_to_rgb(v, r, p);
        case 1: return cm_to_rgb(q, v, p);
        case 2: return cm_to_rgb(p, v, r);
        case 3: return cm_to_rgb(p, q, v);
        case 4: return cm_to_rgb(r, p, v);
        default: return cm_to_rgb(v, p, q);  // 5: h < 252
    }
}

// ColorCompare (main.pas:1557-1571) of two 0x00BBGGRR colours; at most 13 * 3 * 255^2 + 255^2 * 32 < 2^23
__host__ __device__ inline uint32_t cm_color_compare(int32_t c1, int32_t c2) {
    const int r1 = c1 & 255, g1 = (c1 >> 8) & 255, b1 = (c1 >> 16) & 255;
    const int r2 = c2 & 255, g2 = (c2 >> 8) & 255, b2 = (c2 >> 16) & 255;
    const int luma1 = r1 * 2126 + g1 * 7152 + b1 * 722, luma2 = r2 * 2126 + g2 * 7152 + b2 * 722;
    const int ld = (luma1 - luma2) / 10000;  // div: truncating
    const int dr = r1 - r2, dg = g1 - g2, db = b1 - b2;
    return (uint32_t)(13 * (dr * dr + dg * dg + db * db) + ((ld * ld) << 5));
}

}  // namespace tiler
