// The arithmetic of the face mosaic (include/hrnet_mi355.h: hrn_mosaic_dev, hrn_mosaic_host, hrn_mosaic_regions), written ONCE
// for the host and the device: the live test of a joint, the extent of a set of joints, the square around it, the clip to the
// canvas, the region of a box, the cell size rule, a cell's pixel count and its mean are compiled into the kernels of mosaic.hip,
// into the host entries, and into the stand-alone program of tests/test_mosaic_host.py (a plain C++ compiler: nothing of HIP is
// needed).  Integer arithmetic throughout; the one floating-point step is the live test (a float32 compare, two range tests and
// two conversions that truncate).  No library call.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define HRN_MOSAIC_FN __host__ __device__ inline
#else
#define HRN_MOSAIC_FN inline
#endif

namespace hrn {

constexpr int kMosaicMaxList = 256;     // K, the joints of the list, in [1, kMosaicMaxList]
constexpr int kMosaicMaxScale = 64;     // scale_num, scale_den in [1, kMosaicMaxScale]
constexpr int kMosaicMaxHalf = 4096;    // min_half in [0, kMosaicMaxHalf] (0: the rule)
enum { MOSAIC_OK = 0, MOSAIC_NO_REGION = 1, MOSAIC_OUTSIDE = 2 };   // a person's status

HRN_MOSAIC_FN int mosaic_min(int a, int b) { return a < b ? a : b; }
HRN_MOSAIC_FN int mosaic_max(int a, int b) { return a > b ? a : b; }

// trunc(v) when it is finite and lies in [-8192, 16383] (hrn_draw_poses' rule: -0.7 -> 0); false otherwise.  trunc(v) is in that
// range iff -8193 < v < 16384, and NaN fails both tests; the conversion then truncates towards zero and cannot overflow.
HRN_MOSAIC_FN bool mosaic_coordinate(float v, int *out) {
    if (!(v > -8193.0f && v < 16384.0f)) return false;
    *out = (int)v;
    return true;
}

// hrn_draw_poses' predicate, literally: confidence > threshold in float32 (equality and NaN: not live), y and x finite and
// X = trunc(x), Y = trunc(y) in [-8192, 16383]
HRN_MOSAIC_FN bool mosaic_joint_live(const float *p /* (y, x, confidence) */, float threshold, int *X, int *Y) {
    bool live = p[2] > threshold;
    live = mosaic_coordinate(p[1], X) && live;
    live = mosaic_coordinate(p[0], Y) && live;
    return live;
}

// the extent of a set of live joints: empty (x1 < x0) until the first one is added
struct MosaicExtent {
    int x0, y0, x1, y1;
};
HRN_MOSAIC_FN MosaicExtent mosaic_extent_empty() { return MosaicExtent{0x7fffffff, 0x7fffffff, -0x7fffffff, -0x7fffffff}; }
HRN_MOSAIC_FN void mosaic_extent_add(MosaicExtent &e, int X, int Y) {
    e.x0 = mosaic_min(e.x0, X), e.y0 = mosaic_min(e.y0, Y), e.x1 = mosaic_max(e.x1, X), e.y1 = mosaic_max(e.y1, Y);
}
// max(X1 - X0, Y1 - Y0) of an extent that is not empty: at most 16383 + 8192 = 24575
HRN_MOSAIC_FN int mosaic_extent_size(const MosaicExtent &e) { return mosaic_max(e.x1 - e.x0, e.y1 - e.y0); }

// the clip of the half-open rectangle (x_lo, y_lo, x_hi, y_hi) to a canvas of H rows and W columns into out (x1, y1, x2, y2);
// nothing left: out = (0, 0, 0, 0) and MOSAIC_OUTSIDE
HRN_MOSAIC_FN int mosaic_clip(int x_lo, int y_lo, int x_hi, int y_hi, int H, int W, int *out) {
    const int x1 = mosaic_max(x_lo, 0), y1 = mosaic_max(y_lo, 0), x2 = mosaic_min(x_hi, W), y2 = mosaic_min(y_hi, H);
    if (x2 <= x1 || y2 <= y1) {
        out[0] = out[1] = out[2] = out[3] = 0;
        return MOSAIC_OUTSIDE;
    }
    out[0] = x1, out[1] = y1, out[2] = x2, out[3] = y2;
    return MOSAIC_OK;
}

// The region of a person from the extent `listed` of the live joints of the list and the extent `person` of all its live joints.
// E <= 24575 and scale_num <= 64, so E * scale_num + scale_den - 1 < 2^21; the centre sums lie in [-16384, 32766]: int32 holds
// everything.  >> on a negative sum is an arithmetic shift (floor), as the header says.
HRN_MOSAIC_FN int mosaic_region(const MosaicExtent &listed, const MosaicExtent &person, int scale_num, int scale_den, int min_half,
                                int H, int W, int *out) {
    if (listed.x1 < listed.x0) {
        out[0] = out[1] = out[2] = out[3] = 0;
        return MOSAIC_NO_REGION;
    }
    const int E = mosaic_extent_size(listed), P = mosaic_extent_size(person);   // (a listed live joint is a live joint: P >= E)
    const int rmin = min_half > 0 ? min_half : (P + 15) / 16;
    const int R = mosaic_max(rmin, (E * scale_num + scale_den - 1) / scale_den);
    const int cx2 = listed.x0 + listed.x1, cy2 = listed.y0 + listed.y1;
    return mosaic_clip((cx2 >> 1) - R, (cy2 >> 1) - R, ((cx2 + 1) >> 1) + R + 1, ((cy2 + 1) >> 1) + R + 1, H, W, out);
}

// one person from host or device memory, joint by joint: what the build kernel does with a wave
HRN_MOSAIC_FN int mosaic_region_of_person(const float *pts /* (J, 3) */, int J, const uint32_t *listed_bits /* bit j: joint j is listed */,
                                          float threshold, int scale_num, int scale_den, int min_half, int H, int W, int *out) {
    MosaicExtent listed = mosaic_extent_empty(), person = mosaic_extent_empty();
    for (int j = 0; j < J; ++j) {
        int X = 0, Y = 0;
        if (!mosaic_joint_live(pts + 3 * (long long)j, threshold, &X, &Y)) continue;
        mosaic_extent_add(person, X, Y);
        if ((listed_bits[j >> 5] >> (j & 31)) & 1u) mosaic_extent_add(listed, X, Y);
    }
    return mosaic_region(listed, person, scale_num, scale_den, min_half, H, W, out);
}

// the region of a box (x1, y1, x2, y2), half-open: the box itself, clipped; all-zero or degenerate: no region.  Any int32 does:
// the clip compares, it never adds.
HRN_MOSAIC_FN int mosaic_region_of_box(const int32_t *b, int H, int W, int *out) {
    if (b[2] <= b[0] || b[3] <= b[1]) {   // (an all-zero box is degenerate)
        out[0] = out[1] = out[2] = out[3] = 0;
        return MOSAIC_NO_REGION;
    }
    return mosaic_clip(b[0], b[1], b[2], b[3], H, W, out);
}

HRN_MOSAIC_FN bool mosaic_cell_valid(int cell) { return cell == 0 || cell == 2 || cell == 4 || cell == 8 || cell == 16 || cell == 32; }

// the cell size of a canvas: `cell`, or for 0 the largest power of two not above clamp(min(H, W) / 64, 8, 32)
HRN_MOSAIC_FN int mosaic_cell_size(int cell, int H, int W) {
    if (cell > 0) return cell;
    const int m = mosaic_min(H, W) / 64;
    return m >= 32 ? 32 : m >= 16 ? 16 : 8;
}

// pixels of the cell that starts at (x0, y0) inside the canvas: a product of two minima
HRN_MOSAIC_FN int mosaic_cell_count(int x0, int y0, int s, int H, int W) { return mosaic_min(s, W - x0) * mosaic_min(s, H - y0); }

// the byte every pixel of a cell takes from the sum over its c pixels (sum <= 32 * 32 * 255)
HRN_MOSAIC_FN int mosaic_mean(int sum, int c) { return (sum + (c >> 1)) / c; }

// does the clipped region r = (x1, y1, x2, y2) meet the cell that starts at (x0, y0)?  (an empty region meets nothing)
HRN_MOSAIC_FN bool mosaic_meets(int rx1, int ry1, int rx2, int ry2, int x0, int y0, int s) {
    return rx2 > rx1 && ry2 > ry1 && rx1 < x0 + s && rx2 > x0 && ry1 < y0 + s && ry2 > y0;
}

}  // namespace hrn
