// BGR -> 4:2:0 YCbCr, the arithmetic of include/hrnet_mi355.h: hrn_bgr_to_yuv_frames, hrn_bgr_to_yuv_blocks and
// hrn_yuv_forward_coefficients, written ONCE for the host and the device: bgr_to_yuv_kernel (yuv_out.hip), the two host entries
// (hrnet_mi355.cpp) and the stand-alone program of tests/test_bgr2yuv_host.py (a plain C++ compiler: nothing of HIP is needed)
// compile these functions.
//
// THE TABLE.  Ten int32: y0, then the rows (R, G, B) of Y, U and V at scale 2^20, q(x) = floor(x * 2^20 + 0.5) of the EXACT forward
// coefficients of the matrix (Kr / Kb = 0.299 / 0.114 or 0.2126 / 0.0722, Kg = 1 - Kr - Kb) and the range (limited: sy = 219/255,
// sc = 224/255, y0 = 16; full: sy = sc = 1, y0 = 0):
//   CYR = q(sy Kr)                    CYG = q(sy Kg)                    CYB = q(sy Kb)
//   CUR = q(-sc Kr / (2 (1 - Kb)))    CUG = q(-sc Kg / (2 (1 - Kb)))    CUB = -(CUR + CUG)
//   CVG = q(-sc Kg / (2 (1 - Kr)))    CVB = q(-sc Kb / (2 (1 - Kr)))    CVR = -(CVG + CVB)
// A chroma row sums to zero, so a grey pixel gives exactly 128 / 512.  BT.601 limited follows the SAME rule: it is NOT OpenCV's
// forward table (cv2.cvtColor(COLOR_BGR2YUV_I420)'s 14-bit one, which is coarser); parity with cv2 is not pinned.
//
// THE PIXEL RULE.  Integers, arithmetic shift, one rounding each; R, G, B are the 8-bit values of a pixel, Rs, Gs, Bs the SUMS over
// the four pixels of a 2x2 block (0 .. 1020) -- one chroma sample per block is the conversion of the block's mean (a definition of
// this library: MPEG-1 centre siting):
//   8 bit:   Y = clip8 ((CYR R  + CYG G  + CYB B  + (y0  << 20) + (1 << 19)) >> 20)
//            U = clip8 ((CUR Rs + CUG Gs + CUB Bs + (128 << 22) + (1 << 21)) >> 22)     V likewise
//   10 bit:  Y = clip10((CYR R  + CYG G  + CYB B  + (y0  << 20) + (1 << 17)) >> 18)
//            U = clip10((CUR Rs + CUG Gs + CUB Bs + (128 << 22) + (1 << 19)) >> 20)     V likewise
// Every sum fits int32: the largest is exactly 2^30 (a full-range chroma sum).  For 8-bit input no clip engages in limited range;
// in full range exactly two values meet one: pure blue's U and pure red's V are 256 before the 8-bit clip (128 + 127.5, as in
// the float64 formula).
// P010 stores s << 6, I010 stores s.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HRN_YUVFWD_FN __host__ __device__ inline
#else
#define HRN_YUVFWD_FN inline
#endif

namespace hrn {

constexpr int kYuvFwdCoefs = 10;   // y0, CYR CYG CYB, CUR CUG CUB, CVR CVG CVB

// the table of (matrix, range) = (HRN_YUV_BT601 0 | HRN_YUV_BT709 1, HRN_YUV_LIMITED 0 | HRN_YUV_FULL 1); false: unknown (host)
inline bool yuv_forward_table(int matrix, int range, int32_t out[kYuvFwdCoefs]) {
    if ((matrix != 0 && matrix != 1) || (range != 0 && range != 1)) return false;
    const double kr = matrix == 0 ? 0.299 : 0.2126, kb = matrix == 0 ? 0.114 : 0.0722, kg = 1.0 - kr - kb;
    const double sy = range == 0 ? 219.0 / 255.0 : 1.0, sc = range == 0 ? 224.0 / 255.0 : 1.0;
    const auto q = [](double x) { return (int32_t)floor(x * 1048576.0 + 0.5); };
    out[0] = range == 0 ? 16 : 0;
    out[1] = q(sy * kr), out[2] = q(sy * kg), out[3] = q(sy * kb);
    out[4] = q(-sc * kr / (2.0 * (1.0 - kb))), out[5] = q(-sc * kg / (2.0 * (1.0 - kb))), out[6] = -(out[4] + out[5]);
    out[8] = q(-sc * kg / (2.0 * (1.0 - kr))), out[9] = q(-sc * kb / (2.0 * (1.0 - kr))), out[7] = -(out[8] + out[9]);
    return true;
}

HRN_YUVFWD_FN int yuv_fwd_clip(int v, int top) { return v < 0 ? 0 : (v > top ? top : v); }

// the luma sample of one pixel: 8 bits, or 10 (ten)
HRN_YUVFWD_FN int yuv_fwd_luma(const int32_t *c, bool ten, int r, int g, int b) {
    const int sum = c[1] * r + c[2] * g + c[3] * b + (c[0] << 20);
    return ten ? yuv_fwd_clip((sum + (1 << 17)) >> 18, 1023) : yuv_fwd_clip((sum + (1 << 19)) >> 20, 255);
}

// a chroma sample of one 2x2 block from the sums of its four pixels; row: c + 4 (U) or c + 7 (V)
HRN_YUVFWD_FN int yuv_fwd_chroma(const int32_t *row, bool ten, int rs, int gs, int bs) {
    const int sum = row[0] * rs + row[1] * gs + row[2] * bs + (128 << 22);
    return ten ? yuv_fwd_clip((sum + (1 << 19)) >> 20, 1023) : yuv_fwd_clip((sum + (1 << 21)) >> 22, 255);
}

// one 2x2 block, (B, G, R) of its pixels row-major -> Y00 Y01 Y10 Y11 U V, sample values
HRN_YUVFWD_FN void yuv_fwd_block(const int32_t *c, bool ten, const uint8_t *bgr, uint16_t *out) {
    int rs = 0, gs = 0, bs = 0;
    for (int k = 0; k < 4; ++k) {
        const int b = bgr[3 * k], g = bgr[3 * k + 1], r = bgr[3 * k + 2];
        out[k] = (uint16_t)yuv_fwd_luma(c, ten, r, g, b);
        rs += r, gs += g, bs += b;
    }
    out[4] = (uint16_t)yuv_fwd_chroma(c + 4, ten, rs, gs, bs);
    out[5] = (uint16_t)yuv_fwd_chroma(c + 7, ten, rs, gs, bs);
}

}  // namespace hrn
