// The arithmetic of the COCO keypoint evaluation -- OKS matching of detections to ground truth per image, precision / recall
// accumulation over the set, the ten AP / AR statistics (include/hrnet_mi355.h: hrn_keypoint_eval, hrn_keypoint_eval_dev) -- written
// ONCE for the host and the device: every function here is compiled into the host entry (postproc.cpp) and into the kernels of
// keypoint_eval.hip, so the two sides cannot drift apart.  Plain C++ and fp64, fp contraction off, no FMA, no fast-math, no library
// call; exp is assoc_math.h's assoc_exp: the same bits on both sides.  It restates what pycocotools' COCOeval does for
// iouType = 'keypoints' with one category and maxDets = [20] (the reference's datasets/COCO.py:574-588 calls it); pycocotools is
// not available where this library is built, so THIS TEXT IS THE CONTRACT and parity with pycocotools is not pinned.
//
// INPUTS.  P images in ascending image-id order; dt_start / gt_start: P + 1 non-decreasing int32 each, image p has the detections
//   [dt_start[p], dt_start[p + 1]) and the ground-truth people [gt_start[p], gt_start[p + 1]).  dt_kpts (N, J, 3) fp64 (x, y,
//   score), dt_scores (N) fp64; gt_kpts (M, J, 3) fp64 (x, y, v), gt_area (M) fp64, gt_bbox (M, 4) fp64 (x, y, w, h), gt_iscrowd (M)
//   int32; sigmas: J fp64, or null for COCO's 17 (assoc_coco_var; then J must be 17).
// CONSTANTS.  iouThrs = np.linspace(0.5, 0.95, 10) (kEvalIouThrs), recThrs = np.linspace(0, 1, 101) (kEvalRecThrs), maxDet = 20,
//   area ranges all [0, 1e10], medium [32^2, 96^2], large [96^2, 1e10] (kEvalAreaLo / kEvalAreaHi).
//
// PER IMAGE
//   1. DETECTION ORDER: descending score and STABLE (equal scores keep index order); a NaN score goes last and sets status bit 0
//      (pose_nms_math.h's rule and routine: a detection's position is the number of detections before it).  The first 20 are the
//      image's SLOTS; the rest take no part.  A detection's area is (max_j x - min_j x) * (max_j y - min_j y) over all J joints
//      (max / min by `v > m ? v : m` from the first joint on).
//   2. OKS(d, g), k1 = the number of joints of g with v > 0.
//        k1 > 0: dx = x_d - x_g, dy = y_d - y_g; the joints that count are g's with v > 0.
//        k1 = 0: x0 = bx - bw, x1 = bx + 2 * bw, y0 = by - bh, y1 = by + 2 * bh;
//                dx = max(0, x0 - x_d) + max(0, x_d - x1), dy likewise (max(0, v) = v > 0 ? v : 0); all J joints count.
//        e_j = (dx * dx + dy * dy) / vars_j / (area_g + spacing(1)) / 2, every operation rounded on its own, left to right;
//        vars_j = (2 sigma_j)^2.  OKS = the sum of assoc_exp(-e_j) over the counting joints in joint order and numpy's pairwise
//        summation order, divided by their count.  A NON-FINITE OKS counts as 0.0 and sets status bit 1.
//   3. GROUND-TRUTH FLAGS: ignore_g = iscrowd_g or k1 == 0; for area range a: ig_g = ignore_g or area_g < lo_a or area_g > hi_a.
//      The people are visited "ig = 0 first, then ig = 1", each part in index order.
//   4. MATCHING, for each of the 3 ranges x 10 thresholds t, over the slots in order: best = min(t, 1 - 1e-10), m = none; walk
//      the people in the order of step 3: skip g if it is taken at this (a, t) and not a crowd; STOP if m is set, ig_m = 0 and
//      ig_g = 1; skip if OKS(d, g) < best; else best = OKS(d, g), m = g (an equal value replaces).  A match marks g taken; the slot
//      is MATCHED, and IGNORED if ig_m.  An unmatched slot whose own area a_d has a_d < lo_a or a_d > hi_a is IGNORED.
//   5. npig(image, a) = the number of people with ig = 0.
// OVER THE SET, per (a, t): all slots of all images in descending score, stably (ties: image order, then slot order; NaN last).
//   tp_i / fp_i: the running counts of slots that are matched / not matched, and not ignored (ignored slots stay in the sequence
//   and add to neither).  npig_a = the sum of npig(image, a).  npig_a == 0: precision and recall are -1 for that range.  Otherwise
//   rc_i = tp_i / npig_a, pr_i = tp_i / (fp_i + tp_i + spacing(1)); recall(a, t) = rc_last, or 0 without slots; pr is made
//   non-increasing from the end (pr_{i-1} = max(pr_{i-1}, pr_i)); for each recThr, i = the first index with rc_i >= recThr:
//   precision(a, t, r) = pr_i, or 0 if there is none.
//   (Both sides find that index without keeping the sequences: slot i owns threshold r when rc_i >= recThr_r and i = 0 or
//   rc_{i-1} < recThr_r -- eval_owns -- and its enveloped precision is the maximum of pr over i and everything after it.)
// STATISTICS: AP over `all`, AP at t index 0, AP at t index 5, AP over `medium`, AP over `large`, then the five ARs likewise from
//   recall: each the mean over the entries > -1 of its slice, -1 if there is none; the sum is SEQUENTIAL fp64 in (t, r) order,
//   then one division (a definition of this library: numpy's mean adds pairwise).
//
// SIZES: J in [1, HRN_MAX_JOINTS = 256]; at most HRN_MAX_TRACKED = 256 detections and 256 ground-truth people per image.
#pragma once

#include "pose_nms_math.h"

namespace hrn {

constexpr int kEvalMaxDet = 20, kEvalAreas = 3, kEvalThrs = 10, kEvalRecs = 101;
constexpr double kEvalSpacing1 = 2.220446049250313e-16;   // np.spacing(1)
constexpr double kEvalIouThrs[kEvalThrs] = {0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.8999999999999999, 0.95};
constexpr double kEvalRecThrs[kEvalRecs] = {
    0.0,  0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09, 0.1,  0.11, 0.12, 0.13, 0.14, 0.15, 0.16,
    0.17, 0.18, 0.19, 0.2,  0.21, 0.22, 0.23, 0.24, 0.25, 0.26, 0.27, 0.28, 0.29, 0.3,  0.31, 0.32, 0.33,
    0.34, 0.35000000000000003, 0.36, 0.37, 0.38, 0.39, 0.4, 0.41000000000000003, 0.42, 0.43, 0.44, 0.45, 0.46,
    0.47000000000000003, 0.48, 0.49, 0.5, 0.51, 0.52, 0.53, 0.54, 0.55, 0.56, 0.5700000000000001, 0.58, 0.59, 0.6,
    0.61, 0.62, 0.63, 0.64, 0.65, 0.66, 0.67, 0.68, 0.6900000000000001, 0.7000000000000001, 0.71, 0.72, 0.73,
    0.74, 0.75, 0.76, 0.77, 0.78, 0.79, 0.8,  0.81, 0.8200000000000001, 0.8300000000000001, 0.84, 0.85, 0.86,
    0.87, 0.88, 0.89, 0.9,  0.91, 0.92, 0.93, 0.9400000000000001, 0.9500000000000001, 0.96, 0.97, 0.98, 0.99, 1.0};
constexpr double kEvalAreaLo[kEvalAreas] = {0.0, 32.0 * 32.0, 96.0 * 96.0};
constexpr double kEvalAreaHi[kEvalAreas] = {1e10, 96.0 * 96.0, 1e10};

// one image of a call: its detections, its people, and where its slots start among the S slots of the set
struct EvalImage {
    int dt_first, dt_n, gt_first, gt_n, slot_first, slots;
};

// ---- step 1: a detection's area -------------------------------------------------------------------------------------------------
__host__ __device__ inline double eval_dt_area(const double *k, int J) {   // k: the detection's (J, 3)
#pragma clang fp contract(off)
    double x0 = k[0], x1 = k[0], y0 = k[1], y1 = k[1];
    for (int j = 1; j < J; ++j) {
        const double x = k[j * 3], y = k[j * 3 + 1];
        x0 = x < x0 ? x : x0, x1 = x > x1 ? x : x1, y0 = y < y0 ? y : y0, y1 = y > y1 ? y : y1;
    }
    return (x1 - x0) * (y1 - y0);
}

// ---- step 2: OKS of one (detection, person) pair --------------------------------------------------------------------------------
__host__ __device__ inline int eval_k1(const double *g, int J) {   // g: the person's (J, 3)
    int k1 = 0;
    for (int j = 0; j < J; ++j) k1 += g[j * 3 + 2] > 0 ? 1 : 0;
    return k1;
}

// walks the joints of one pair in order and yields exp(-e) of those that count
struct EvalCursor {
    const double *d, *g, *vars;   // (J, 3), (J, 3), J
    bool vis;                     // k1 > 0
    double x0, x1, y0, y1, denom;
    int j;

    // the next term; called at most (k1 > 0 ? k1 : J) times after j = 0
    __host__ __device__ double next() {
#pragma clang fp contract(off)
        for (;;) {
            const int jj = j++;
            double dx, dy;
            if (vis) {
                if (!(g[jj * 3 + 2] > 0)) continue;
                dx = d[jj * 3] - g[jj * 3], dy = d[jj * 3 + 1] - g[jj * 3 + 1];
            } else {
                const double x = d[jj * 3], y = d[jj * 3 + 1];
                const double ax = x0 - x, bx = x - x1, ay = y0 - y, by = y - y1;
                dx = (ax > 0 ? ax : 0.0) + (bx > 0 ? bx : 0.0), dy = (ay > 0 ? ay : 0.0) + (by > 0 ? by : 0.0);
            }
            const double e = (dx * dx + dy * dy) / vars[jj] / denom / 2;
            return assoc_exp(-e);
        }
    }
};

// numpy's pairwise summation over a cursor (assoc_math.h's assoc_sum_leaf / assoc_np_sum, statement for statement)
template <class Cursor>
__host__ __device__ inline double eval_sum_leaf(Cursor &c, int len) {
#pragma clang fp contract(off)
    if (len < 8) {
        double res = 0.;
        for (int i = 0; i < len; ++i) res += c.next();
        return res;
    }
    double r0 = c.next(), r1 = c.next(), r2 = c.next(), r3 = c.next(), r4 = c.next(), r5 = c.next(), r6 = c.next(), r7 = c.next();
    int i;
    for (i = 8; i < len - (len % 8); i += 8) {
        r0 += c.next(), r1 += c.next(), r2 += c.next(), r3 += c.next();
        r4 += c.next(), r5 += c.next(), r6 += c.next(), r7 += c.next();
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < len; ++i) res += c.next();
    return res;
}
template <class Cursor>
__host__ __device__ inline double eval_np_sum(Cursor &c, int n) {
#pragma clang fp contract(off)
    if (n <= 128) return eval_sum_leaf(c, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    const double left = eval_sum_leaf(c, n2);
    const int rest = n - n2;
    if (rest <= 128) return left + eval_sum_leaf(c, rest);
    int n3 = rest / 2;
    n3 -= n3 % 8;
    const double mid = eval_sum_leaf(c, n3);
    return left + (mid + eval_sum_leaf(c, rest - n3));
}

// OKS of detection d (J, 3) against person g (J, 3) with k1 visible joints, bbox (x, y, w, h) and area; a non-finite value comes
// back as 0.0 with *bad set
__host__ __device__ inline double eval_oks(const double *d, const double *g, int J, int k1, const double *bbox, double area,
                                           const double *vars, int *bad) {
#pragma clang fp contract(off)
    EvalCursor c;
    c.d = d, c.g = g, c.vars = vars, c.vis = k1 > 0, c.j = 0;
    c.x0 = bbox[0] - bbox[2], c.x1 = bbox[0] + 2 * bbox[2], c.y0 = bbox[1] - bbox[3], c.y1 = bbox[1] + 2 * bbox[3];
    c.denom = area + kEvalSpacing1;
    const int n = k1 > 0 ? k1 : J;
    const double o = eval_np_sum(c, n) / (double)n;
    if (o - o == 0.0) return o;
    *bad = 1;
    return 0.0;
}

// ---- step 3: a person's flag in range a, and the order the people are visited in -----------------------------------------------------
__host__ __device__ inline bool eval_gt_ig(bool ignore, double area, int a) {
    return ignore || area < kEvalAreaLo[a] || area > kEvalAreaHi[a];
}
// order[0 .. n): the people with ig = 0 in index order, then those with ig = 1; returns how many have ig = 0 (npig).  n <= 256.
__host__ __device__ inline int eval_gt_order(const unsigned char *ig, int n, unsigned char *order) {
    int at = 0;
    for (int g = 0; g < n; ++g)
        if (!ig[g]) order[at++] = (unsigned char)g;
    const int npig = at;
    for (int g = 0; g < n; ++g)
        if (ig[g]) order[at++] = (unsigned char)g;
    return npig;
}

// ---- step 4: the greedy matching of one image at one (a, t) ---------------------------------------------------------------------------
// oks: (slots, gt_n) row-major; order / ig: range a's; crowd: iscrowd != 0; dt_area: per slot; taken: gt_n bytes of scratch.
// match_out[s] = gt_first + the person, or -1; ignore_out[s] = 0 / 1.
__host__ __device__ inline void eval_match(const double *oks, int slots, int gt_n, const unsigned char *order, const unsigned char *ig,
                                           const unsigned char *crowd, const double *dt_area, int a, double t, int gt_first,
                                           unsigned char *taken, int32_t *match_out, uint8_t *ignore_out) {
    for (int g = 0; g < gt_n; ++g) taken[g] = 0;
    for (int s = 0; s < slots; ++s) {
        double best = t < 1 - 1e-10 ? t : 1 - 1e-10;
        int m = -1;
        for (int q = 0; q < gt_n; ++q) {
            const int g = order[q];
            if (taken[g] && !crowd[g]) continue;
            if (m >= 0 && !ig[m] && ig[g]) break;
            const double o = oks[s * gt_n + g];
            if (o < best) continue;
            best = o, m = g;
        }
        if (m >= 0) {
            taken[m] = 1;
            match_out[s] = gt_first + m, ignore_out[s] = ig[m] ? 1 : 0;
        } else {
            const double ad = dt_area[s];
            match_out[s] = -1, ignore_out[s] = (ad < kEvalAreaLo[a] || ad > kEvalAreaHi[a]) ? 1 : 0;
        }
    }
}

// ---- over the set -----------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline double eval_precision(int tp, int fp) {
#pragma clang fp contract(off)
    return (double)tp / ((double)fp + (double)tp + kEvalSpacing1);
}
__host__ __device__ inline double eval_recall(int tp, int npig) { return (double)tp / (double)npig; }
// does the slot with running count tp (tp_before: the count of the slot before it, ignored when first) own recThr r?
__host__ __device__ inline bool eval_owns(int tp, int tp_before, bool first, int npig, int r) {
    const double thr = kEvalRecThrs[r];
    return eval_recall(tp, npig) >= thr && (first || !(eval_recall(tp_before, npig) >= thr));
}

// statistic `which` (0 .. 9) from precision (3, 10, 101) and recall (3, 10)
__host__ __device__ inline double eval_stat(const double *precision, const double *recall, int which) {
#pragma clang fp contract(off)
    const bool ap = which < 5;
    const int w = which % 5;
    const int a = w == 3 ? 1 : w == 4 ? 2 : 0;
    const int t0 = w == 1 ? 0 : w == 2 ? 5 : 0, t1 = w == 1 ? 1 : w == 2 ? 6 : kEvalThrs;
    double sum = 0.0;
    int count = 0;
    for (int t = t0; t < t1; ++t) {
        if (ap) {
            for (int r = 0; r < kEvalRecs; ++r) {
                const double v = precision[(a * kEvalThrs + t) * kEvalRecs + r];
                if (v > -1) sum = sum + v, ++count;
            }
        } else {
            const double v = recall[a * kEvalThrs + t];
            if (v > -1) sum = sum + v, ++count;
        }
    }
    return count ? sum / (double)count : -1.0;
}

// ---- what is wrong with the arguments of the two entries, or nullptr; needs no device -------------------------------------------
inline const char *keypoint_eval_fault(int P, const int32_t *dt_start, const int32_t *gt_start, int J, const void *dt_kpts,
                                       const void *dt_scores, const void *gt_kpts, const void *gt_area, const void *gt_bbox,
                                       const void *gt_iscrowd, const double *sigmas, const void *stats, const void *precision,
                                       const void *recall, const void *slot_person, const void *slot_score, const void *dt_match,
                                       const void *dt_ignore, const void *npig, const void *status) {
    if (P < 0) return "P is negative";
    if (J < 1 || J > kAssocMaxJoints) return "J must be in [1, HRN_MAX_JOINTS]";
    if (!sigmas && J != 17) return "the default sigmas are COCO's 17: pass sigmas for another J";
    if (!stats || !precision || !recall) return "null stats / precision / recall";
    if (P == 0) return nullptr;
    if (!dt_start || !gt_start || !npig || !status) return "null segment tables / npig / status";
    if (dt_start[0] < 0 || gt_start[0] < 0) return "a segment table starts below zero";
    long long slots = 0;
    for (int p = 0; p < P; ++p) {
        if (dt_start[p + 1] < dt_start[p] || gt_start[p + 1] < gt_start[p]) return "a segment table decreases";
        if (dt_start[p + 1] - dt_start[p] > kMaxTracked) return "more than HRN_MAX_TRACKED detections in one image";
        if (gt_start[p + 1] - gt_start[p] > kMaxTracked) return "more than HRN_MAX_TRACKED ground-truth people in one image";
        const int n = dt_start[p + 1] - dt_start[p];
        slots += n < kEvalMaxDet ? n : kEvalMaxDet;
    }
    if (slots > 0x7fffffffLL / (kEvalAreas * kEvalThrs)) return "too many slots for 32-bit indices";
    if (dt_start[P] > dt_start[0] && (!dt_kpts || !dt_scores || !slot_person || !slot_score || !dt_match || !dt_ignore))
        return "null detections / slot outputs";
    if (gt_start[P] > gt_start[0] && (!gt_kpts || !gt_area || !gt_bbox || !gt_iscrowd)) return "null ground truth";
    return nullptr;
}

// the images of a call (P entries) and the number of slots S
inline int keypoint_eval_images(int P, const int32_t *dt_start, const int32_t *gt_start, EvalImage *out) {
    int S = 0;
    for (int p = 0; p < P; ++p) {
        EvalImage &im = out[p];
        im.dt_first = dt_start[p], im.dt_n = dt_start[p + 1] - dt_start[p];
        im.gt_first = gt_start[p], im.gt_n = gt_start[p + 1] - gt_start[p];
        im.slot_first = S, im.slots = im.dt_n < kEvalMaxDet ? im.dt_n : kEvalMaxDet;
        S += im.slots;
    }
    return S;
}

}  // namespace hrn
