// One pixel of a 4:2:0 YCbCr frame through the conversion of cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420), for the kernels that read
// their taps from YUV frames (prepath.hip, letterbox.hip): the chroma sample of a 2x2 block is shared (nearest).
// 8-bit layouts (NV12, NV21, I420): 20-bit fixed point in int32 (coef = y0, CY, CUB, CUG, CVG, CVR of hrn_yuv_coefficients):
//   yy = max(0, Y - y0) * CY;  u = U - 128;  v = V - 128;  h = 1 << 19
//   B = clip8((yy + h + CUB*u) >> 20);  G = clip8((yy + h + CVG*v + CUG*u) >> 20);  R = clip8((yy + h + CVR*v) >> 20)
// 10-bit layouts (P010: the sample is word >> 6; I010: word & 1023), the same table, ONE rounding from the 10-bit samples:
//   yy = max(0, Y - 4*y0) * CY;  u = U - 512;  v = V - 512;  h = 1 << 21
//   B = clip8((yy + h + CUB*u) >> 22);  G = clip8((yy + h + CVG*v + CUG*u) >> 22);  R = clip8((yy + h + CVR*v) >> 22)
// Every product fits int32; the SUMS do not (BT.709 limited: yy + h + CUB*u reaches 2 304 855 561), so they are 64-bit.
// For samples that are multiples of 4 every term is 4 x the 8-bit one: the 10-bit form contains the 8-bit form bit for bit.
// A 10-bit plane is read in aligned 16-bit words: the host refuses an odd plane address or pitch.
#pragma once

#include "kernels.h"

namespace hrn {

constexpr int kPixNV12 = 1;   // HRN_PIX_* of include/hrnet_mi355.h (3 is unassigned)
constexpr int kPixI420 = 2;
constexpr int kPixNV21 = 4;
constexpr int kPixP010 = 5;
constexpr int kPixI010 = 6;

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

// the 10-bit conversion: Y, U, V in [0, 1023]
__device__ __forceinline__ Rgb yuv_rgb10(const int *coef, int Y, int U, int V) {
    int y = Y - 4 * coef[0];
    y = y < 0 ? 0 : y;
    const long long yy = (long long)(y * coef[1] + (1 << 21));   // at most 1023 * CY + 2^21 < 2^31
    const int u = U - 512, v = V - 512;
    Rgb o;
    o.b = sat8((int)((yy + (long long)(coef[2] * u)) >> 22));
    o.g = sat8((int)((yy + (long long)(coef[4] * v + coef[3] * u)) >> 22));
    o.r = sat8((int)((yy + (long long)(coef[5] * v)) >> 22));
    return o;
}

template <int FMT>
constexpr bool yuv_is10() { return FMT == kPixP010 || FMT == kPixI010; }

// the sample of one 16-bit word of a 10-bit plane: the top 10 bits (P010) or the low 10 (I010); the other six are ignored
template <int FMT>
__device__ __forceinline__ int yuv_sample10(unsigned w) { return FMT == kPixP010 ? (int)((w & 0xffffu) >> 6) : (int)(w & 1023u); }

// the conversion of layout FMT's samples
template <int FMT>
__device__ __forceinline__ Rgb yuv_rgb_of(const int *coef, int Y, int U, int V) {
    if (yuv_is10<FMT>()) return yuv_rgb10(coef, Y, U, V);
    return yuv_rgb(coef, Y, U, V);
}

// pixel (fy, fx) of the frame: one Y sample, one chroma pair, one conversion
template <int FMT>
__device__ __forceinline__ Rgb yuv_frame_px(const YuvSource &ys, int fy, int fx) {
    static_assert(FMT == kPixNV12 || FMT == kPixI420 || FMT == kPixNV21 || FMT == kPixP010 || FMT == kPixI010, "a layout is named");
    if (yuv_is10<FMT>()) {
        const int Y = yuv_sample10<FMT>(((const unsigned short *)(ys.y + (size_t)fy * ys.pitch_y))[fx]);
        int U, V;
        if (FMT == kPixP010) {
            const unsigned short *c = (const unsigned short *)(ys.u + (size_t)(fy >> 1) * ys.pitch_c) + (fx & ~1);
            U = yuv_sample10<FMT>(c[0]), V = yuv_sample10<FMT>(c[1]);
        } else {
            const size_t row = (size_t)(fy >> 1) * ys.pitch_c;
            U = yuv_sample10<FMT>(((const unsigned short *)(ys.u + row))[fx >> 1]);
            V = yuv_sample10<FMT>(((const unsigned short *)(ys.v + row))[fx >> 1]);
        }
        return yuv_rgb10(ys.coef, Y, U, V);
    }
    const int Y = ys.y[(size_t)fy * ys.pitch_y + fx];
    int U, V;
    if (FMT == kPixNV12) {
        const unsigned char *c = ys.u + (size_t)(fy >> 1) * ys.pitch_c + (fx & ~1);
        U = c[0], V = c[1];
    } else if (FMT == kPixNV21) {
        const unsigned char *c = ys.u + (size_t)(fy >> 1) * ys.pitch_c + (fx & ~1);
        V = c[0], U = c[1];
    } else {
        const size_t off = (size_t)(fy >> 1) * ys.pitch_c + (fx >> 1);
        U = ys.u[off], V = ys.v[off];
    }
    return yuv_rgb(ys.coef, Y, U, V);
}

}  // namespace hrn
