// The arithmetic of detector NMS -- the raw (B, N, 5 + C) output of a YOLO head to kept rows (include/hrnet_mi355.h:
// hrn_detector_nms, hrn_detector_nms_dev) -- written ONCE for the host and the device: every function here is compiled into the host
// entry (postproc.cpp) and into the kernels of detector_nms.hip, so the two sides cannot drift apart.  Plain C++, float32
// throughout, fp contraction off, no FMA, no fast-math, no library call.  The rule in full is in the header; in short:
//
//   row        cx, cy, w, h, obj, cls_0 .. cls_{C-1}; float16 is widened exactly (dnms_half)
//   box        x1 = cx - w / 2, y1 = cy - h / 2, x2 = cx + w / 2, y2 = cy + h / 2
//   best       first maximum of the classes: best = 0, v = cls_0; for c = 1 ..: if cls_c > v: best = c, v = cls_c (dnms_best_step;
//              the kernel reduces (value, index) pairs with dnms_best_join, which gives the same pair)
//   YOLOV5     candidate iff obj > t and obj * v > t; key = obj * v; row = box, key, best
//   YOLOV3     candidate iff obj >= t; key = obj * v; row = merged box, obj, v, best
//   NaN key    the candidate is dropped, status bit 2
//   order      descending key (-0 == +0), equal keys by ascending row: ONE strict total order, the 64-bit dnms_order_key ascending
//   min / max  max(a, b) = a > b ? a : b, min(a, b) = a < b ? a : b (a NaN gives b)
//   IoU        dnms_iou, per rule; a NaN never suppresses
//   merge      YOLOV3: acc = w_p * box_p, W = w_p, then acc = acc + w_q * box_q, W = W + w_q over the suppressed q in ascending
//              position, box = acc / W
//   a NaN in an output row is written as the canonical quiet NaN 0x7FC00000 (the payload a NaN operation leaves differs between
//   processors)
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace hrn {

constexpr int kDnmsYoloV3 = 0, kDnmsYoloV5 = 1;      // = HRN_DNMS_YOLOV3 / _YOLOV5
constexpr int kDnmsAgnostic = 1;                      // = HRN_DNMS_AGNOSTIC
constexpr int kDnmsMaxCandidates = 4096, kDnmsMaxClasses = 4096, kDnmsMaxRows = 1 << 24;
constexpr int kDnmsTruncated = 1, kDnmsMaxDetHit = 2, kDnmsNanKey = 4;   // status bits
constexpr int kDnmsF32 = 0, kDnmsF16 = 2;             // = HRN_F32 / HRN_F16

// one candidate as the scoring pass leaves it: 32 bytes
struct __attribute__((aligned(16))) DnmsCand {
    float x1, y1, x2, y2, obj, cls_conf;
    int32_t best, row;
};

__host__ __device__ inline float dnms_bits_float(uint32_t u) {
    union {
        uint32_t u;
        float f;
    } c;
    c.u = u;
    return c.f;
}
__host__ __device__ inline uint32_t dnms_float_bits(float f) {
    union {
        uint32_t u;
        float f;
    } c;
    c.f = f;
    return c.u;
}

// IEEE binary16 to binary32, exactly (subnormals, infinities; a NaN keeps its sign and its payload's top bits, quieted)
__host__ __device__ inline float dnms_half(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1Fu, man = h & 0x3FFu;
    if (exp == 0x1Fu) return dnms_bits_float(sign | 0x7F800000u | (man ? 0x00400000u | (man << 13) : 0u));
    if (exp != 0) return dnms_bits_float(sign | ((exp + 112u) << 23) | (man << 13));
    if (man == 0) return dnms_bits_float(sign);
    int e = 113;   // a subnormal: man * 2^-24; shift the leading one up to bit 10
    uint32_t m = man;
    while (!(m & 0x400u)) m <<= 1, --e;
    return dnms_bits_float(sign | ((uint32_t)e << 23) | ((m & 0x3FFu) << 13));
}

// element `at` of pred
__host__ __device__ inline float dnms_load(const void *pred, int dtype, size_t at) {
    return dtype == kDnmsF16 ? dnms_half(((const uint16_t *)pred)[at]) : ((const float *)pred)[at];
}

__host__ __device__ inline float dnms_max(float a, float b) { return a > b ? a : b; }
__host__ __device__ inline float dnms_min(float a, float b) { return a < b ? a : b; }
__host__ __device__ inline float dnms_canon(float v) { return v != v ? dnms_bits_float(0x7FC00000u) : v; }

// does obj let the row through?  (Both rules admit a row only if it does: the classes are read for these rows alone.)
__host__ __device__ inline bool dnms_obj_passes(int rule, float obj, float conf_thres) {
    return rule == kDnmsYoloV3 ? obj >= conf_thres : obj > conf_thres;
}

// the best class: the sequential rule, and the join of two partial results over DISJOINT class ranges (present = the range held
// a class that is not NaN).  Joining the ranges in any order gives the sequential result, except when cls_0 is NaN: the caller
// then takes (0, cls_0), as the sequential rule does.
struct DnmsBest {
    float v;
    int idx;
    bool present;
};
__host__ __device__ inline void dnms_best_step(float &v, int &best, float cls, int c) {
    if (cls > v) v = cls, best = c;
}
__host__ __device__ inline DnmsBest dnms_best_join(DnmsBest a, DnmsBest b) {
    if (!b.present) return a;
    if (!a.present) return b;
    return (b.v > a.v || (b.v == a.v && b.idx < a.idx)) ? b : a;
}

__host__ __device__ inline float dnms_key(const DnmsCand &c) {
#pragma clang fp contract(off)
    return c.obj * c.cls_conf;
}

// a row whose obj passed, with its best class: 1 a candidate (*out filled), 2 dropped for a NaN key, 0 neither
__host__ __device__ inline int dnms_candidate(int rule, float conf_thres, float cx, float cy, float w, float h, float obj, float cls_conf,
                                              int best, int row, DnmsCand *out) {
#pragma clang fp contract(off)
    DnmsCand c;
    c.obj = obj, c.cls_conf = cls_conf, c.best = best, c.row = row;
    const float key = dnms_key(c);
    if (rule == kDnmsYoloV5 && !(key > conf_thres)) return 0;
    if (key != key) return 2;
    const float hw = w / 2, hh = h / 2;
    c.x1 = cx - hw, c.y1 = cy - hh, c.x2 = cx + hw, c.y2 = cy + hh;
    *out = c;
    return 1;
}

// a key that is not NaN as an unsigned integer that ascends with it; -0 and +0 give the same integer
__host__ __device__ inline uint32_t dnms_key_bits(float key) {
    if (key == 0.0f) return 0x80000000u;
    const uint32_t u = dnms_float_bits(key);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the order: ascending in this integer = descending key, equal keys by ascending row.  No two candidates of an image share one.
__host__ __device__ inline uint64_t dnms_order_key(uint32_t key_bits, int32_t row) {
    return ((uint64_t)(~key_bits) << 32) | (uint32_t)row;
}

__host__ __device__ inline float dnms_area(int rule, const DnmsCand &c) {
#pragma clang fp contract(off)
    if (rule == kDnmsYoloV3) return (c.x2 - c.x1 + 1) * (c.y2 - c.y1 + 1);
    return (c.x2 - c.x1) * (c.y2 - c.y1);
}

// IoU of two boxes (x1, y1, x2, y2) with their areas
__host__ __device__ inline float dnms_iou(int rule, float ax1, float ay1, float ax2, float ay2, float area_a, float bx1, float by1,
                                          float bx2, float by2, float area_b) {
#pragma clang fp contract(off)
    const float dw = dnms_min(ax2, bx2) - dnms_max(ax1, bx1), dh = dnms_min(ay2, by2) - dnms_max(ay1, by1);
    if (rule == kDnmsYoloV3) {
        const float inter = dnms_max(dw + 1, 0.0f) * dnms_max(dh + 1, 0.0f);
        return inter / (area_a + area_b - inter + 1e-16f);
    }
    const float inter = dnms_max(dw, 0.0f) * dnms_max(dh, 0.0f);
    return inter / (area_a + area_b - inter);
}

// the YOLOV3 merge: one more member of a keeper's merge set
__host__ __device__ inline void dnms_merge_first(float w, float x1, float y1, float x2, float y2, float acc[4], float &sum) {
#pragma clang fp contract(off)
    acc[0] = w * x1, acc[1] = w * y1, acc[2] = w * x2, acc[3] = w * y2, sum = w;
}
__host__ __device__ inline void dnms_merge_add(float w, float x1, float y1, float x2, float y2, float acc[4], float &sum) {
#pragma clang fp contract(off)
    acc[0] = acc[0] + w * x1, acc[1] = acc[1] + w * y1, acc[2] = acc[2] + w * x2, acc[3] = acc[3] + w * y2, sum = sum + w;
}

__host__ __device__ inline int dnms_row_floats(int rule) { return rule == kDnmsYoloV3 ? 7 : 6; }

// one kept row: the box (YOLOV3: acc / sum of its merge set), then the rule's columns
__host__ __device__ inline void dnms_write_row(int rule, const DnmsCand &c, const float acc[4], float sum, float *out) {
#pragma clang fp contract(off)
    if (rule == kDnmsYoloV3) {
        out[0] = dnms_canon(acc[0] / sum), out[1] = dnms_canon(acc[1] / sum), out[2] = dnms_canon(acc[2] / sum);
        out[3] = dnms_canon(acc[3] / sum), out[4] = dnms_canon(c.obj), out[5] = dnms_canon(c.cls_conf), out[6] = (float)c.best;
    } else {
        out[0] = dnms_canon(c.x1), out[1] = dnms_canon(c.y1), out[2] = dnms_canon(c.x2), out[3] = dnms_canon(c.y2);
        out[4] = dnms_canon(dnms_key(c)), out[5] = (float)c.best;
    }
}

// ---- what is wrong with the arguments of the two entries, or nullptr; needs no device -------------------------------------------
inline const char *dnms_fault(const void *pred, int dtype, int B, int N, int C, int rule, int flags, float conf_thres, float iou_thres,
                              int max_candidates, int max_det, const void *rows, const void *index, const void *counts,
                              const void *status) {
    if (dtype != kDnmsF32 && dtype != kDnmsF16) return "dtype must be HRN_F32 or HRN_F16";
    if (B < 0) return "B is negative";
    if (N < 0 || N > kDnmsMaxRows) return "N must be in [0, 2^24]";
    if (C < 1 || C > kDnmsMaxClasses) return "C must be in [1, 4096]";
    if (rule != kDnmsYoloV3 && rule != kDnmsYoloV5) return "rule must be HRN_DNMS_YOLOV3 or HRN_DNMS_YOLOV5";
    if (flags & ~kDnmsAgnostic) return "unknown flag bits";
    if (!(conf_thres - conf_thres == 0.0f) || !(iou_thres - iou_thres == 0.0f)) return "conf_thres and iou_thres must be finite";
    if (max_candidates < 1 || max_candidates > kDnmsMaxCandidates) return "max_candidates must be in [1, 4096]";
    if (max_det < 1 || max_det > max_candidates) return "max_det must be in [1, max_candidates]";
    if (B == 0) return nullptr;
    if (!rows || !index || !counts || !status) return "null rows / index / counts / status";
    if (N > 0 && !pred) return "null pred";
    return nullptr;
}

}  // namespace hrn
