// The arithmetic of the tracking link (include/hrnet_mi355.h: hrn_pose_boxes, hrn_boxes_from_poses, hrn_preprocess_frames_dev),
// written ONCE for the host and the device: every function here is compiled into the host entries (hrn_crop_geometry,
// hrn_pose_boxes, the host-detection pre-path) and into the kernels of track.hip, so the two sides cannot drift apart.
// Everything is double arithmetic in a fixed operation order, fp contraction off, no fast-math: the same bits on both sides.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "kernels.h"

namespace hrn {

// ---- the crop box of one detection ------------------------------------------------------------------------------------
// SimpleHRNet.py:236-278 (PAD) / :383-412 (CLAMP) for ONE detection in a frame of frame_h x frame_w, network input H x W.
// The box arithmetic is Python's, restated in double: round() is round-half-even on a float, `//` on non-negative ints is
// C's `/`, int(round(x)) = rint under the default rounding mode.  Fills the slice / pad numbers of `cp` (tmp_off and the
// frame are the caller's) and the reported box, and returns CROP_OK; or one of the three refusals -- where the reference would
// wrap around or divide by zero -- with `cp` and `box` untouched.  pad_hw = (h_pad, w_pad) before they are narrowed to int.
// The four coordinates must be finite and at most 2^30 in magnitude (the host entries take a detector's rows, the record kernel
// tests it: CROP_NOT_FINITE).
enum { CROP_OK = 0, CROP_DEGENERATE = 1, CROP_OUTSIDE = 2, CROP_DEGENERATE_CLAMPED = 3, CROP_TOO_TALL = 4, CROP_NOT_FINITE = 5 };

__host__ __device__ inline long crop_min(long a, long b) { return a < b ? a : b; }
__host__ __device__ inline long crop_max(long a, long b) { return a > b ? a : b; }
__host__ __device__ inline long crop_abs(long a) { return a < 0 ? -a : a; }

__host__ __device__ inline int crop_geometry_one(const float *d, int frame_h, int frame_w, int H, int W, int variant, CropParams &cp,
                                                 int32_t *box, long pad_hw[2]) {
#pragma clang fp contract(off)
    const long x1 = (long)rint((double)d[0]), y1 = (long)rint((double)d[1]);
    const long x2 = (long)rint((double)d[2]), y2 = (long)rint((double)d[3]);
    if (x2 <= x1 || y2 <= y1) return CROP_DEGENERATE;
    const double cf = (double)H / (double)W * (double)(x2 - x1) / (double)(y2 - y1);
    // The reference slices numpy arrays with these numbers: a negative start would wrap around.  The PAD variant
    // slices with the rounded box itself; the CLAMP variant re-derives (and clamps to the frame) the side it
    // enlarges, so only the OTHER side has to be inside the frame as given (SimpleHRNet.py:396-407).
    const bool clamp = variant != 0;   // HRN_CROP_CLAMP
    const bool x_as_given = !clamp || !(cf < 1), y_as_given = !clamp || !(cf > 1);
    if ((x_as_given && (x1 < 0 || x1 >= frame_w)) || (y_as_given && (y1 < 0 || y1 >= frame_h))) return CROP_OUTSIDE;
    long x1n = x1, x2n = x2, y1n = y1, y2n = y2, pt = 0, pb = 0, pl = 0, pr = 0;
    long sx1 = x1, sy1 = y1, sx2 = x2, sy2 = y2;  // what is sliced out of the frame
    if (clamp) {  // SimpleHRNet.py:396-407: enlarge, clamp to the frame, slice the enlarged box
        if (cf > 1) {
            const long center = y1 + (y2 - y1) / 2;
            const long length = (long)rint((double)(y2 - y1) * cf);
            y1n = crop_max(0, center - length / 2), y2n = crop_min(frame_h, center + length / 2);
        } else if (cf < 1) {
            const long center = x1 + (x2 - x1) / 2;
            const long length = (long)rint((double)(x2 - x1) * 1 / cf);
            x1n = crop_max(0, center - length / 2), x2n = crop_min(frame_w, center + length / 2);
        }
        sx1 = x1n, sy1 = y1n, sx2 = x2n, sy2 = y2n;
        if (sx2 <= sx1 || sy2 <= sy1 || sx1 >= frame_w || sy1 >= frame_h) return CROP_DEGENERATE_CLAMPED;
    } else if (cf > 1) {  // increase y side
        const long center = y1 + (y2 - y1) / 2;
        const long length = (long)rint((double)(y2 - y1) * cf);
        y1n = center - length / 2, y2n = center + length / 2;
        pt = crop_abs(y1n - y1), pb = crop_abs(y2n - y2);
    } else if (cf < 1) {
        const long center = x1 + (x2 - x1) / 2;
        const long length = (long)rint((double)(x2 - x1) * 1 / cf);
        x1n = center - length / 2, x2n = center + length / 2;
        pl = crop_abs(x1n - x1), pr = crop_abs(x2n - x2);
    }
    const long w_crop = crop_min(sx2, frame_w) - sx1, h_crop = crop_min(sy2, frame_h) - sy1;  // numpy slicing
    pad_hw[0] = h_crop + pt + pb, pad_hw[1] = w_crop + pl + pr;
    cp.x1 = (int)sx1, cp.y1 = (int)sy1;
    cp.w_crop = (int)w_crop, cp.h_crop = (int)h_crop;
    cp.pad_top = (int)pt, cp.pad_left = (int)pl;
    cp.h_pad = (int)pad_hw[0], cp.w_pad = (int)pad_hw[1];
    box[0] = (int32_t)x1n, box[1] = (int32_t)y1n, box[2] = (int32_t)x2n, box[3] = (int32_t)y2n;
    return CROP_OK;
}

// rows of the intermediate a person of a frame_h x frame_w frame can need when its box lies inside the frame: the frame's
// height (nothing padded), or the height that brings a frame-wide box to the aspect H : W, plus two for the roundings
__host__ __device__ inline long crop_hcap(int frame_h, int frame_w, int H, int W) {
    const long grown = ((long)H * frame_w + W - 1) / W;
    return (frame_h > grown ? (long)frame_h : grown) + 2;
}

// ---- a detection-shaped box from one person's joints ----------------------------------------------------------------------
// include/hrnet_mi355.h: hrn_pose_boxes.  A joint (y, x, confidence) is live iff confidence > threshold in float32 (equality and
// NaN: not live) and y and x are finite; a live coordinate enters as (double)v + 0.0, so that a negative zero cannot make the
// minimum and maximum depend on the order they are taken in.
__host__ __device__ inline bool pose_joint_live(float y, float x, float confidence, float threshold) {
    return confidence > threshold && __builtin_isfinite(y) && __builtin_isfinite(x);
}
__host__ __device__ inline double pose_coordinate(float v) {
#pragma clang fp contract(off)
    return (double)v + 0.0;
}

// one axis: the extent [lo, hi] of the live joints grown by `scale` about its centre, at least min_side long, cut to [0, limit]
__host__ __device__ inline void pose_box_side(double lo, double hi, int limit, double scale, double min_side, float *first, float *last) {
#pragma clang fp contract(off)
    const double centre = (lo + hi) * 0.5;
    const double grown = (hi - lo) * scale;
    const double side = grown > min_side ? grown : min_side;
    const double half = side * 0.5;
    const double a = centre - half, b = centre + half;
    *first = (float)(a > 0.0 ? a : 0.0);
    *last = (float)(b < (double)limit ? b : (double)limit);
}

// the row (x1, y1, x2, y2, score) from the extent of the live joints, the sum of their confidences IN JOINT ORDER and their number
__host__ __device__ inline void pose_box_finish(double xmin, double xmax, double ymin, double ymax, double sum, int nlive, int min_joints,
                                                int frame_h, int frame_w, double scale, double min_side, float out[5]) {
#pragma clang fp contract(off)
    if (nlive < min_joints) {
        out[0] = out[1] = out[2] = out[3] = out[4] = 0.0f;
        return;
    }
    pose_box_side(xmin, xmax, frame_w, scale, min_side, &out[0], &out[2]);
    pose_box_side(ymin, ymax, frame_h, scale, min_side, &out[1], &out[3]);
    out[4] = (float)(sum / (double)nlive);
}

// the whole definition for one person, joint after joint: the host form (the kernel takes extent and count over a wave -- exact
// in any order -- and the sum in this order)
inline void pose_box_one(const float *pts, int J, int frame_h, int frame_w, float threshold, int min_joints, double scale,
                         double min_side, float out[5]) {
#pragma clang fp contract(off)
    double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY, sum = 0.0;
    int nlive = 0;
    for (int j = 0; j < J; ++j) {
        const float *p = pts + (size_t)j * 3;
        if (!pose_joint_live(p[0], p[1], p[2], threshold)) continue;
        const double y = pose_coordinate(p[0]), x = pose_coordinate(p[1]);
        xmin = x < xmin ? x : xmin, xmax = x > xmax ? x : xmax;
        ymin = y < ymin ? y : ymin, ymax = y > ymax ? y : ymax;
        sum = sum + (double)p[2];
        ++nlive;
    }
    pose_box_finish(xmin, xmax, ymin, ymax, sum, nlive, min_joints, frame_h, frame_w, scale, min_side, out);
}

}  // namespace hrn
