// The tap arithmetic of cv2.resize's generic 8-bit path (modules/imgproc/src/resize.cpp; oracle/cv2_resize_oracle.py restates it),
// written ONCE for the kernels that resize whole frames: resize_taps_kernel (prepath.hip, the single-person pre-path) and
// letterbox_kernel (letterbox.hip, the detector tensor).  Both compile this text, so the two cannot drift apart.
//   position      f = (float)((d + 0.5) * scale - 0.5), scale = 1 / ((double)dst / src); s = floor(f); f -= s
//   INTER_LINEAR  x side: s < 0 -> (0, f = 0), s >= src - 1 -> (src - 1, f = 0); coefficients (1 - f, f) * 2048, nearest even
//   INTER_CUBIC   interpolateCubic (A = -0.75, float32), saturate_cast<short>(c * 2048)
//   INTER_NEAREST s = min(floor(d * scale), src - 1)
// No contraction into fused multiply-adds anywhere: the reference rounds after every operation.
#pragma once

#include "kernels.h"

namespace hrn {

// the window of output sample d of an axis of `src` samples; interp = HRN_INTER_* (0 nearest, 1 linear, 2 cubic)
__device__ __forceinline__ ResizeTaps resize_tap_of(int d, int src, double scale, int interp, bool is_x) {
#pragma clang fp contract(off)
    ResizeTaps o;
    o.ofs = 0, o.c[0] = o.c[1] = o.c[2] = o.c[3] = 0;
    if (interp == 0) {   // resizeNN
        int s = (int)floor(__dmul_rn((double)d, scale));
        o.ofs = s < src - 1 ? s : src - 1, o.c[0] = 2048;
    } else {
        float f = (float)__dsub_rn(__dmul_rn(__dadd_rn((double)d, 0.5), scale), 0.5);
        int s = (int)floorf(f);
        f = __fsub_rn(f, (float)s);
        if (interp == 2) {   // interpolateCubic, A = -0.75
            const float A = -0.75f;
            const float x1 = __fadd_rn(f, 1.f), xm = __fsub_rn(1.f, f);
            const float c0 = __fsub_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(A, x1), __fmul_rn(5.f, A)), x1), __fmul_rn(8.f, A)), x1),
                                       __fmul_rn(4.f, A));
            const float c1 = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(A, 2.f), f), __fadd_rn(A, 3.f)), f), f), 1.f);
            const float c2 = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(A, 2.f), xm), __fadd_rn(A, 3.f)), xm), xm), 1.f);
            const float c3 = __fsub_rn(__fsub_rn(__fsub_rn(1.f, c0), c1), c2);
            const float c[4] = {c0, c1, c2, c3};
            o.ofs = s - 1;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int v = __float2int_rn(__fmul_rn(c[k], 2048.f));   // saturate_cast<short>: nearest, ties to even
                o.c[k] = (short)(v < -32768 ? -32768 : v > 32767 ? 32767 : v);
            }
        } else {             // INTER_LINEAR
            if (is_x && s < 0) s = 0, f = 0.f;
            if (is_x && s >= src - 1) s = src - 1, f = 0.f;
            o.ofs = s;
            o.c[0] = (short)__float2int_rn(__fmul_rn(__fsub_rn(1.f, f), 2048.f));
            o.c[1] = (short)__float2int_rn(__fmul_rn(f, 2048.f));
        }
    }
    return o;
}

// VResizeLinear<uchar, int, short>: two horizontally filtered rows S0, S1 (int32, 11 fractional bits) and the row coefficients
__device__ __forceinline__ int vresize_linear(int b0, int S0, int b1, int S1) {
    return (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
}

}  // namespace hrn
