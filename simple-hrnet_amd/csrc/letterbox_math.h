// The arithmetic of the detector link (include/hrnet_mi355.h: hrn_letterbox_geometry, hrn_letterbox_frames,
// hrn_detections_to_frame, hrn_detections_to_frame_dev), written ONCE for the host and the device, in the role track_geometry.h
// has for the tracking link: the host entries (postproc.cpp, hrnet_mi355.cpp) and the kernels of letterbox.hip compile this text,
// so the two sides cannot drift apart.  Fixed operation order, fp contraction off, no fast-math.
//
// FORWARD, the geometry of one frame of h x w (both wrappers restated; round = rint on a double under the default rounding
// mode = Python's round, nearest with ties to even):
//   HRN_LETTERBOX_MAX_SIDE (YOLOv3, mode 'square', out_h == out_w == S)   ratio = (double)S / max(h, w)
//   HRN_LETTERBOX_MIN_RATIO (YOLOv5, auto / scaleFill off, scaleup on)    ratio = min((double)out_h / h, (double)out_w / w)
//   new_w = round(w * ratio), new_h = round(h * ratio); dw = (out_w - new_w) / 2, dh = (out_h - new_h) / 2 in double;
//   top = round(dh - 0.1), bottom = round(dh + 0.1), left = round(dw - 0.1), right = round(dw + 0.1)
//
// INVERSE, one detection row (x1, y1, x2, y2, ...) from letterbox to frame coordinates, float32 throughout:
//   MAX_SIDE (scale_coords)  gain = (double)max(out_h, out_w) / max(h, w); pad_x = (out_w - w * gain) / 2, pad_y likewise;
//                            v' = max((v - (float)pad) / (float)gain, 0) for all four coordinates
//   MIN_RATIO                v' = (v - (float)dw) / (float)ratio, no clamp
//   The division is a true float32 division: torch's CPU kernel.  Torch's GPU kernel multiplies by the reciprocal, so the
//   reference differs from itself by an ulp between devices; the CPU result is the definition.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/hrnet_mi355.h"

namespace hrn {

enum { LB_OK = 0, LB_BAD_RULE = 1, LB_BAD_SIZE = 2, LB_NOT_SQUARE = 3, LB_EMPTY = 4, LB_SUM = 5 };

// the geometry of one frame; `bottom_right` (may be null) receives the two paddings hrn_letterbox does not carry
inline int letterbox_geometry_one(int rule, int h, int w, int out_h, int out_w, hrn_letterbox *g, int32_t bottom_right[2]) {
#pragma clang fp contract(off)
    if (rule != HRN_LETTERBOX_MAX_SIDE && rule != HRN_LETTERBOX_MIN_RATIO) return LB_BAD_RULE;
    if (h <= 0 || w <= 0 || out_h <= 0 || out_w <= 0) return LB_BAD_SIZE;
    if (rule == HRN_LETTERBOX_MAX_SIDE && out_h != out_w) return LB_NOT_SQUARE;
    double ratio;
    if (rule == HRN_LETTERBOX_MAX_SIDE) {
        ratio = (double)out_h / (double)(h > w ? h : w);
    } else {
        const double rh = (double)out_h / (double)h, rw = (double)out_w / (double)w;
        ratio = rh < rw ? rh : rw;
    }
    const long new_w = (long)rint((double)w * ratio), new_h = (long)rint((double)h * ratio);
    if (new_w < 1 || new_h < 1) return LB_EMPTY;
    const double dw = (double)(out_w - new_w) / 2.0, dh = (double)(out_h - new_h) / 2.0;
    const long top = (long)rint(dh - 0.1), bottom = (long)rint(dh + 0.1), left = (long)rint(dw - 0.1), right = (long)rint(dw + 0.1);
    if (top < 0 || left < 0 || top + new_h + bottom != out_h || left + new_w + right != out_w) return LB_SUM;
    g->new_w = (int32_t)new_w, g->new_h = (int32_t)new_h, g->left = (int32_t)left, g->top = (int32_t)top;
    g->ratio_w = ratio, g->ratio_h = ratio, g->dw = dw, g->dh = dh;
    if (bottom_right) bottom_right[0] = (int32_t)bottom, bottom_right[1] = (int32_t)right;
    return LB_OK;
}

inline const char *letterbox_fault_text(int code) {
    switch (code) {
        case LB_BAD_RULE: return "rule must be HRN_LETTERBOX_MAX_SIDE or HRN_LETTERBOX_MIN_RATIO";
        case LB_BAD_SIZE: return "has a non-positive side, or the output has";
        case LB_NOT_SQUARE: return "HRN_LETTERBOX_MAX_SIDE needs out_h == out_w";
        case LB_EMPTY: return "is resized to nothing (new_w or new_h is 0): cv2.resize would raise";
        case LB_SUM: return "has paddings that do not add up to the output size";
    }
    return "";
}

// ---- the inverse ----------------------------------------------------------------------------------------------------------
constexpr int kDetMaxClasses = 16;   // = HRN_DET_MAX_CLASSES
constexpr int kDetCompact = 1;       // = HRN_DET_COMPACT
enum { DET_KEPT = 0, DET_BELOW = 1, DET_CLASS = 2, DET_NOT_FINITE = 5 };

struct DetFrame {          // one frame of a call: its rows and the float32 constants of its inverse
    int first, n;
    float sub_x, sub_y, div_x, div_y;
    int clamp0, pad_;
};

// what every row of a call shares
struct DetFilter {
    int det_stride, conf_col, class_col;   // class_col resolved: in [0, det_stride), or det_stride = no class filter
    float conf_thres;
    int nclasses;
    float classes[kDetMaxClasses];
};

inline DetFrame det_frame(int rule, const hrn_letterbox &g, int h, int w, int out_h, int out_w, int first, int n) {
#pragma clang fp contract(off)
    DetFrame f{};
    f.first = first, f.n = n;
    if (rule == HRN_LETTERBOX_MAX_SIDE) {
        const double gain = (double)(out_h > out_w ? out_h : out_w) / (double)(h > w ? h : w);
        const double pad_x = ((double)out_w - (double)w * gain) / 2.0, pad_y = ((double)out_h - (double)h * gain) / 2.0;
        f.sub_x = (float)pad_x, f.sub_y = (float)pad_y, f.div_x = f.div_y = (float)gain, f.clamp0 = 1;
    } else {
        f.sub_x = (float)g.dw, f.sub_y = (float)g.dh, f.div_x = (float)g.ratio_w, f.div_y = (float)g.ratio_h, f.clamp0 = 0;
    }
    return f;
}

__host__ __device__ inline float det_divide(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);   // correctly rounded, whatever the compiler's division mode
#else
    return a / b;
#endif
}

__host__ __device__ inline float det_coordinate(float v, float sub, float div, int clamp0) {
#pragma clang fp contract(off)
    const float r = det_divide(v - sub, div);
    return clamp0 ? (r > 0.0f ? r : 0.0f) : r;
}

// the status of one input row
__host__ __device__ inline int det_status(const float *row, const DetFilter &q) {
    const float conf = row[q.conf_col];
    if (!(__builtin_isfinite(row[0]) && __builtin_isfinite(row[1]) && __builtin_isfinite(row[2]) && __builtin_isfinite(row[3]) &&
          __builtin_isfinite(conf)))
        return DET_NOT_FINITE;
    if (!(conf >= q.conf_thres)) return DET_BELOW;
    if (q.class_col < q.det_stride) {
        const float cls = row[q.class_col];
        bool hit = false;
        for (int k = 0; k < q.nclasses; ++k) hit = hit || cls == q.classes[k];
        if (!hit) return DET_CLASS;
    }
    return DET_KEPT;
}

// a kept row into `out`: the four mapped coordinates, the other columns as they are
__host__ __device__ inline void det_map_row(const float *row, const DetFrame &f, int det_stride, float *out) {
    out[0] = det_coordinate(row[0], f.sub_x, f.div_x, f.clamp0);
    out[1] = det_coordinate(row[1], f.sub_y, f.div_y, f.clamp0);
    out[2] = det_coordinate(row[2], f.sub_x, f.div_x, f.clamp0);
    out[3] = det_coordinate(row[3], f.sub_y, f.div_y, f.clamp0);
    for (int k = 4; k < det_stride; ++k) out[k] = row[k];
}

// The refusals both entries share (they need no device); nullptr when the arguments pass.  On success `q` is filled.
inline const char *det_fault(int rule, const void *dets, int det_stride, const int32_t *start, int P, const hrn_letterbox *geometry,
                             const int32_t *frame_hw, int out_h, int out_w, int conf_col, float conf_thres, int class_col,
                             const int32_t *classes, int nclasses, int flags, const void *dets_out, const void *counts,
                             const void *status, DetFilter &q) {
    if (rule != HRN_LETTERBOX_MAX_SIDE && rule != HRN_LETTERBOX_MIN_RATIO) return letterbox_fault_text(LB_BAD_RULE);
    if (P < 0) return "P is negative";
    if (det_stride < 5) return "det_stride must be at least 5";
    if (flags & ~kDetCompact) return "unknown flags (HRN_DET_COMPACT)";
    if (out_h <= 0 || out_w <= 0) return "the letterbox size is not positive";
    if (rule == HRN_LETTERBOX_MAX_SIDE && out_h != out_w) return letterbox_fault_text(LB_NOT_SQUARE);
    if (conf_col < 4 || conf_col >= det_stride) return "conf_col must be in [4, det_stride)";
    if (conf_thres != conf_thres) return "conf_thres is NaN";
    const int cc = class_col < 0 ? class_col + det_stride : class_col;
    if (cc < 0 || cc > det_stride) return "class_col must be in [-det_stride, det_stride]";
    if (nclasses < 0 || nclasses > kDetMaxClasses) return "at most HRN_DET_MAX_CLASSES classes";
    if (cc < det_stride && nclasses > 0 && !classes) return "null classes";
    if (P > 0 && (!start || !geometry || !frame_hw || !counts)) return "null start / geometry / frame sizes / counts";
    if (P > 0 && start[0] != 0) return "start[0] must be 0";
    for (int p = 0; p < P; ++p) {
        if (start[p + 1] < start[p]) return "start must ascend";
        if (frame_hw[2 * p] <= 0 || frame_hw[2 * p + 1] <= 0) return "a frame has a non-positive side";
        const hrn_letterbox &g = geometry[p];
        if (rule == HRN_LETTERBOX_MIN_RATIO && !(__builtin_isfinite(g.dw) && __builtin_isfinite(g.dh) && g.ratio_w > 0 && g.ratio_h > 0 &&
                                                 __builtin_isfinite(g.ratio_w) && __builtin_isfinite(g.ratio_h)))
            return "a geometry has a ratio that is not positive and finite, or a padding that is not finite";
    }
    const long n = P > 0 ? start[P] : 0;
    if (n > 0 && (!dets || !dets_out || !status)) return "null detections / output / status";
    if (n > 0) {
        const char *a = (const char *)dets, *b = (const char *)dets_out;
        const size_t bytes = (size_t)n * det_stride * sizeof(float);
        if (a < b + bytes && b < a + bytes) return "the output overlaps the input";
    }
    q.det_stride = det_stride, q.conf_col = conf_col, q.class_col = cc, q.conf_thres = conf_thres;
    q.nclasses = cc < det_stride ? nclasses : 0;
    for (int k = 0; k < kDetMaxClasses; ++k) q.classes[k] = k < q.nclasses ? (float)classes[k] : 0.0f;
    return nullptr;
}

// one frame on the host, row after row: the definition the kernel follows chunk by chunk
inline int det_frame_host(const float *dets, const DetFrame &f, const DetFilter &q, bool compact, float *out, int32_t *status) {
    int kept = 0;
    const int ds = q.det_stride;
    for (int i = 0; i < f.n; ++i) {
        const float *row = dets + (size_t)(f.first + i) * ds;
        const int st = det_status(row, q);
        status[f.first + i] = st;
        if (st == DET_KEPT) {
            det_map_row(row, f, ds, out + (size_t)(f.first + (compact ? kept : i)) * ds);
            ++kept;
        } else if (!compact) {
            for (int k = 0; k < ds; ++k) out[(size_t)(f.first + i) * ds + k] = 0.0f;
        }
    }
    if (compact)
        for (size_t k = (size_t)(f.first + kept) * ds; k < (size_t)(f.first + f.n) * ds; ++k) out[k] = 0.0f;
    return kept;
}

}  // namespace hrn
