// People between a frame and its rotation (include/hrnet_mi355.h: hrn_rotate_people, hrn_rotate_people_dev), written ONCE for the
// host and the device: the host entry (postproc.cpp) and rotate_people_kernel (rotate.hip) compile these functions, so the two sides
// cannot drift apart.  (Hs, Ws) is the SOURCE frame; the codes are cv2.ROTATE_*'s.  A joint costs one float32 subtraction per
// coordinate at most (nothing to contract, nothing to reorder); a box is int32 arithmetic.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace hrn {

constexpr int kRotateMaxJoints = 256;   // = HRN_MAX_JOINTS

// last - v in float32; a NaN is COPIED, bits and all: what a subtraction does to a NaN's sign differs between an x86 host (the
// operand comes back as it is) and the GPU (whose negated-operand form flips it), and the two sides give the same bits
__host__ __device__ inline float rotate_mirror(int last, float v) {
#pragma clang fp contract(off)
    return v != v ? v : (float)last - v;
}

// (y, x, c) -> (y', x', c); out may be in
__host__ __device__ inline void rotate_joint(int code, int hs, int ws, const float *in, float *out) {
    const float y = in[0], x = in[1], c = in[2];
    if (code == 0) out[0] = x, out[1] = rotate_mirror(hs - 1, y);
    else if (code == 1) out[0] = rotate_mirror(hs - 1, y), out[1] = rotate_mirror(ws - 1, x);
    else out[0] = rotate_mirror(ws - 1, x), out[1] = y;
    out[2] = c;
}

// the half-open pixel range (x1, y1, x2, y2) -> the range the rotated slice occupies; the all-zero box stays all-zero; out may be in
__host__ __device__ inline void rotate_box(int code, int hs, int ws, const int32_t *in, int32_t *out) {
    const int32_t x1 = in[0], y1 = in[1], x2 = in[2], y2 = in[3];
    if ((x1 | y1 | x2 | y2) == 0) out[0] = out[1] = out[2] = out[3] = 0;
    else if (code == 0) out[0] = hs - y2, out[1] = x1, out[2] = hs - y1, out[3] = x2;
    else if (code == 1) out[0] = ws - x2, out[1] = hs - y2, out[2] = ws - x1, out[3] = hs - y1;
    else out[0] = y1, out[1] = ws - x2, out[2] = y2, out[3] = ws - x1;
}

// what is wrong with the arguments of hrn_rotate_people / hrn_rotate_people_dev, or nullptr; needs no device
inline const char *rotate_people_fault(int n, int J, const int32_t *frame_hw, int per_person_hw, const int32_t *codes, int per_person_code,
                                       const void *pts, const void *boxes, const void *pts_out, const void *boxes_out) {
    if (n < 0) return "n is negative";
    if (J < 1 || J > kRotateMaxJoints) return "J must be in [1, HRN_MAX_JOINTS]";
    if (!pts && !boxes) return "pts and boxes are both null";
    if ((pts && !pts_out) || (boxes && !boxes_out)) return "an input without its output";
    if (n > 0 && (!frame_hw || !codes)) return "null frame sizes / codes";
    for (int i = 0; i < (per_person_code ? n : (n < 1 ? n : 1)); ++i)
        if (codes[i] < 0 || codes[i] > 2) return "a rotation code is outside {0, 1, 2}";
    for (int i = 0; i < (per_person_hw ? n : (n < 1 ? n : 1)); ++i)
        if (frame_hw[2 * (size_t)i] <= 0 || frame_hw[2 * (size_t)i + 1] <= 0) return "a frame has a non-positive side";
    return nullptr;
}

}  // namespace hrn
