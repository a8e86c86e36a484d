// One pixel of a 4:2:0 YCbCr frame (NV12 / I420) through the conversion of cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420), for the
// kernels that read their taps from YUV frames (prepath.hip, letterbox.hip): the chroma sample of a 2x2 block is shared
// (nearest), 20-bit fixed point in int32 (coef = y0, CY, CUB, CUG, CVG, CVR of hrn_yuv_coefficients):
//   yy = max(0, Y - y0) * CY;  u = U - 128;  v = V - 128;  h = 1 << 19
//   B = clip8((yy + h + CUB*u) >> 20);  G = clip8((yy + h + CVG*v + CUG*u) >> 20);  R = clip8((yy + h + CVR*v) >> 20)
#pragma once

#include "kernels.h"

namespace hrn {

constexpr int kPixNV12 = 1;   // HRN_PIX_NV12, HRN_PIX_I420 of include/hrnet_mi355.h
constexpr int kPixI420 = 2;

struct Rgb {
    int r, g, b;
};

__device__ __forceinline__ int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ Rgb yuv_rgb(const int *coef, int Y, int U, int V) {
    int yy = Y - coef[0];
    yy = (yy < 0 ? 0 : yy) * coef[1] + (1 << 19);
    const int u = U - 128, v = V - 128;
    Rgb o;
    o.b = sat8((yy + coef[2] * u) >> 20);
    o.g = sat8((yy + coef[4] * v + coef[3] * u) >> 20);
    o.r = sat8((yy + coef[5] * v) >> 20);
    return o;
}

// pixel (fy, fx) of the frame: one Y byte, one chroma pair, one conversion
template <int FMT>
__device__ __forceinline__ Rgb yuv_frame_px(const YuvSource &ys, int fy, int fx) {
    const int Y = ys.y[(size_t)fy * ys.pitch_y + fx];
    int U, V;
    if (FMT == kPixNV12) {
        const unsigned char *c = ys.u + (size_t)(fy >> 1) * ys.pitch_c + (fx & ~1);
        U = c[0], V = c[1];
    } else {
        const size_t off = (size_t)(fy >> 1) * ys.pitch_c + (fx >> 1);
        U = ys.u[off], V = ys.v[off];
    }
    return yuv_rgb(ys.coef, Y, U, V);
}

}  // namespace hrn
