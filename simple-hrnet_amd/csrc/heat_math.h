// The arithmetic of the heat-map overlay (include/hrnet_mi355.h: hrn_draw_heatmaps_dev, hrn_draw_heatmaps_host,
// hrn_heatmap_quantise), written ONCE for the host and the device: the maximum that no NaN wins, the quantiser, the sample
// coordinate, the bilinear sample, the alpha rule and the blend are compiled into the kernels of heat.hip, into the two host
// entries, and into the stand-alone program of tests/test_heatmaps_host.py (a plain C++ compiler: nothing of HIP is needed).
// Integer arithmetic throughout; the one floating-point step, the quantiser, is a subtraction, a product and a sum in float32
// with fp contraction off -- the same bits on both sides.  No library call.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define HRN_HEAT_FN __host__ __device__ inline
#else
#define HRN_HEAT_FN inline
#endif

namespace hrn {

constexpr int kHeatLo = -8192, kHeatHi = 16383;   // a drawn box has all four coordinates in [kHeatLo, kHeatHi] (the labels' rule)
constexpr int kHeatMaxSide = 1024;                // hq, wq in [1, kHeatMaxSide]
enum { HEAT_ALPHA_CONST = 0, HEAT_ALPHA_VALUE = 1 };   // = HRN_HEAT_ALPHA_*

// the running maximum over the masked joints, started from NaN: a NaN never wins a comparison, all-NaN stays NaN
HRN_HEAT_FN float heat_max(float v, float x) { return (x > v || v != v) ? x : v; }

// Q of a cell from its maximum: t = (v - lo) * k, each operation rounded once; 0 unless t > 0 (NaN, -inf), 255 from t >= 255 (+inf)
HRN_HEAT_FN int heat_quantise(float v, float lo, float k) {
#pragma clang fp contract(off)
    const float d = v - lo;
    const float t = d * k;
    if (!(t > 0.0f)) return 0;
    if (t >= 255.0f) return 255;
    const float lifted = t + 0.5f;
    return (int)lifted;
}

// is a person with this box drawn at all?
HRN_HEAT_FN bool heat_box_drawn(int x1, int y1, int x2, int y2) {
    return x1 >= kHeatLo && x1 <= kHeatHi && y1 >= kHeatLo && y1 <= kHeatHi && x2 >= kHeatLo && x2 <= kHeatHi && y2 >= kHeatLo &&
           y2 <= kHeatHi && x2 > x1 && y2 > y1;
}

// The sample coordinate in 1/256 cells of frame pixel p = first + d of a box `side` pixels long over m cells:
// min(floor(d m 256 / side), (m - 1) 256).  d is in [0, 16383] (a canvas pixel is in [0, 8191], a drawn box starts at -8192 or
// later) and m <= 1024, so d m 256 <= 16383 * 2^18 < 2^32: the header's 64-bit product, held in 32 unsigned bits.
HRN_HEAT_FN int heat_coord(int d, int m, int side) {
    const uint32_t u = ((uint32_t)d * (uint32_t)(m * 256)) / (uint32_t)side;
    const uint32_t top = (uint32_t)(m - 1) * 256u;
    return (int)(u < top ? u : top);
}

// S of one pixel from a person's quantised map q (hq rows of wq bytes) at the sample coordinates (ux, uy)
HRN_HEAT_FN int heat_sample(const uint8_t *q, int hq, int wq, int ux, int uy) {
    const int c0 = ux >> 8, fx = ux & 255, c1 = c0 + 1 < wq ? c0 + 1 : wq - 1;
    const int r0 = uy >> 8, fy = uy & 255, r1 = r0 + 1 < hq ? r0 + 1 : hq - 1;
    const uint8_t *row0 = q + (long long)r0 * wq, *row1 = q + (long long)r1 * wq;
    const int top = row0[c0] * (256 - fx) + row0[c1] * fx;
    const int bot = row1[c0] * (256 - fx) + row1[c1] * fx;
    return (top * (256 - fy) + bot * fy + 32768) >> 16;
}

// a of a value V (a pixel's, or a 2 x 2 block's Vc)
HRN_HEAT_FN int heat_alpha(int V, int alpha, int mode) { return mode == HEAT_ALPHA_CONST ? alpha : (alpha * V + 127) / 255; }

// is a pixel of value V written, and with which a
HRN_HEAT_FN bool heat_written(int V, int alpha, int mode, int cutoff, int *a) {
    *a = heat_alpha(V, alpha, mode);
    return V >= cutoff && *a > 0;
}

HRN_HEAT_FN int heat_blend(int src, int colour, int a) { return (src * (255 - a) + colour * a + 127) / 255; }

// Vc of a 2 x 2 block from the V of its four pixels, written or not
HRN_HEAT_FN int heat_block_value(int v0, int v1, int v2, int v3) { return (v0 + v1 + v2 + v3 + 2) >> 2; }

}  // namespace hrn
