// The arithmetic of person re-identification between two frames (include/hrnet_mi355.h: hrn_associate_people,
// hrn_associate_people_dev), written ONCE for the host and the device: every function here is compiled into the host entry
// (postproc.cpp) and into the kernel of assoc.hip, so the two sides cannot drift apart.  Plain C++, fp contraction off, no
// fast-math, no library call: the same bits on both sides.
//
// It restates what postproc.find_person_id_associations computes (postproc.py over hrn_pose_similarity / hrn_assignment, which
// restate misc/utils.py:251-429 of the reference), quirks included:
//   box IoU     fp64 from int32 boxes; zero intersection when disjoint; union = a + b - i; rounded once to float32
//   OKS         float32 (y, x, v) differences; COCO's sigmas as fp64 for J == 17, float32 1/10 otherwise (the dtype decides where the
//               first division is rounded); / denom / 2; only e <= 29 enters (`2 ^ 32 - 1` is XOR in Python); numpy's pairwise
//               summation order; / count; rounded once to float32
//   blend       sim_pose * f32(pose_alpha) + sim_box * f32(1 - pose_alpha) in float32, pose term first
//   cost        (double)(1.0f - sim)
//   acceptance  sim > f32(threshold): a float32 compare, what numpy >= 2 makes of `float32 scalar > python float`
//   smoothing   joints f32(1 - a) * now + f32(a) * before in float32; boxes (1 - a) * now + a * before in fp64, truncated towards
//               zero to int32 (numpy's cast into the caller's int32 array)
//   new people  everybody whose id is -1 after the carry-over (an accepted match with a previous id of -1 included, as in the
//               reference) is numbered in index order from next_id; then next_id = max(next_id, max(ids) + 1)
//
// Three points are this header's own:
//   EXP.  Host std::exp and the device library's exp are different functions, so assoc_exp below is used on both sides: k =
//   round(x / ln 2), r = (x - k * ln2_hi) - k * ln2_lo with k * ln2_hi exact, a degree-13 Taylor polynomial by Horner's rule,
//   and a multiplication by 2^k built from exponent bits.  No FMA, no library call: the device result equals the host result bit
//   for bit.  MEASURED against math.exp (glibc) over 2,900,001 evenly spaced arguments of [-29, 0]: at most 1 ulp apart
//   (tests/test_assoc_host.py repeats the measurement and bounds it by 2), so an OKS differs from the numpy one by a few fp64 ulp
//   before it is rounded to float32 and a blended similarity by at most 1 float32 ulp.
//   NON-FINITE SIMILARITY.  Two zero boxes give IoU 0 / 0, and people lost by the tracking link have zero boxes.  A stream-ordered
//   call cannot raise, so a non-finite blended similarity counts as 0 in the cost and is never accepted; the problem's status says
//   so (0 clean, 1 some entry replaced).  Every cost is then finite and the assignment always completes.
//   SIZES.  At most HRN_MAX_TRACKED = 256 people on either side of one problem, J <= HRN_MAX_JOINTS = 256 (the pairwise summation
//   below is written out for at most 256 terms).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace hrn {

constexpr int kMaxTracked = 256;      // = HRN_MAX_TRACKED (include/hrnet_mi355.h)
constexpr int kAssocMaxJoints = 256;  // = HRN_MAX_JOINTS

// ---- exp ----------------------------------------------------------------------------------------------------------------------
// exp(x) for x in [-29, 0] (what the OKS needs), defined for every x so that odd boxes cannot leave the function undefined: NaN
// stays NaN, x > 709 is +inf, x < -700 is 0.
__host__ __device__ inline double assoc_exp(double x) {
#pragma clang fp contract(off)
    if (x != x) return x;
    if (x > 709.0) return __builtin_huge_val();
    if (x < -700.0) return 0.0;
    const double t = x * 1.44269504088896338700e+00;   // 1 / ln 2
    const int k = (int)(t < 0.0 ? t - 0.5 : t + 0.5);  // to nearest (the cast truncates)
    const double kd = (double)k;
    // ln 2 = hi + lo, hi with 32 trailing zero bits: k * hi is exact for |k| < 2^11
    const double r = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10;   // |r| <= 0.3466
    double p = 1.0 / 6227020800.0;   // 1 / 13!: the first term left out, r^14 / 14!, is below 2^-57
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    const double scale = __builtin_bit_cast(double, (uint64_t)(1023 + k) << 52);   // 2^k, k in [-1010, 1023]: a normal number
    return p * scale;
}

// ---- OKS of one pair ----------------------------------------------------------------------------------------------------------
// (sigma_j * 2)^2 of COCO's 17 joints in fp64 (misc/utils.py:343-345)
__host__ __device__ inline double assoc_coco_var(int j) {
#pragma clang fp contract(off)
    double s = .89;
    switch (j) {
        case 0: s = .26; break;
        case 1: case 2: s = .25; break;
        case 3: case 4: s = .35; break;
        case 5: case 6: s = .79; break;
        case 7: case 8: s = .72; break;
        case 9: case 10: s = .62; break;
        case 11: case 12: s = 1.07; break;
        case 13: case 14: s = .87; break;
        default: break;
    }
    s = s / 10.0;
    return (s * 2) * (s * 2);
}

__host__ __device__ inline double assoc_area(const int32_t *b) {
#pragma clang fp contract(off)
    return ((double)b[2] - (double)b[0]) * ((double)b[3] - (double)b[1]);
}

// walks the joints of one (current g, previous d) pair in order and yields exp(-e) of those with e <= 29
struct OksCursor {
    const float *g, *d;    // (J, 3) float32 (y, x, v)
    const double *vars64;  // J == 17: the 17 values of assoc_coco_var; otherwise unused
    double denom;
    int J, j;
    bool coco;

    __host__ __device__ double e_of(int jj) const {
#pragma clang fp contract(off)
        const float dy = d[3 * jj] - g[3 * jj], dx = d[3 * jj + 1] - g[3 * jj + 1];
        const float sq = dx * dx + dy * dy;
        const float s32 = 1.0f / 10.0f;
        const float var32 = (s32 * 2) * (s32 * 2);
        return (coco ? (double)sq / vars64[jj] : (double)(sq / var32)) / denom / 2;
    }
    __host__ __device__ int count() const {
        int c = 0;
        for (int jj = 0; jj < J; ++jj) c += e_of(jj) <= 29 ? 1 : 0;
        return c;
    }
    // the next kept term; called at most count() times after j = 0
    __host__ __device__ double next() {
        for (;;) {
            const double e = e_of(j++);
            if (e <= 29) return assoc_exp(-e);
        }
    }
};

// numpy's pairwise summation of `len` <= 128 consecutive terms of the cursor (pairwise_sum's unrolled leaf)
__host__ __device__ inline double assoc_sum_leaf(OksCursor &c, int len) {
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

// np.sum of the cursor's `n` <= 256 terms: pairwise_sum's recursion (n2 = n / 2 rounded down to a multiple of 8; left half, then
// right half) written out -- a left half never exceeds 128 terms, a right half splits at most once more
__host__ __device__ inline double assoc_np_sum(OksCursor &c, int n) {
#pragma clang fp contract(off)
    if (n <= 128) return assoc_sum_leaf(c, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    const double left = assoc_sum_leaf(c, n2);
    const int rest = n - n2;
    if (rest <= 128) return left + assoc_sum_leaf(c, rest);
    int n3 = rest / 2;
    n3 -= n3 % 8;
    const double mid = assoc_sum_leaf(c, n3);
    return left + (mid + assoc_sum_leaf(c, rest - n3));
}

__host__ __device__ inline float assoc_oks(const float *g, const float *d, int J, const int32_t *box_g, const int32_t *box_d,
                                           const double *vars64) {
#pragma clang fp contract(off)
    OksCursor c;
    c.g = g, c.d = d, c.vars64 = vars64, c.J = J, c.j = 0, c.coco = J == 17;
    c.denom = (assoc_area(box_g) + assoc_area(box_d)) / 2 + 2.220446049250313e-16;   // np.spacing(1)
    const int n = c.count();
    return (float)(n == 0 ? 0.0 : assoc_np_sum(c, n) / (double)n);
}

__host__ __device__ inline float assoc_iou(const int32_t *p, const int32_t *q) {
#pragma clang fp contract(off)
    const double px1 = p[0], py1 = p[1], px2 = p[2], py2 = p[3], qx1 = q[0], qy1 = q[1], qx2 = q[2], qy2 = q[3];
    const double x1 = px1 > qx1 ? px1 : qx1, x2 = px2 < qx2 ? px2 : qx2, y1 = py1 > qy1 ? py1 : qy1, y2 = py2 < qy2 ? py2 : qy2;
    const double area_i = (x2 < x1 || y2 < y1) ? 0.0 : (x2 - x1) * (y2 - y1);
    const double area_u = assoc_area(p) + assoc_area(q) - area_i;
    return (float)(area_i / area_u);
}

// the parameters as the float32 / fp64 values the expressions above use
struct AssocParams {
    float alpha, beta;    // f32(pose_alpha), f32(1 - pose_alpha)
    float threshold;      // f32(similarity_threshold)
    float now, before;    // f32(1 - smoothing_alpha), f32(smoothing_alpha)
    double smoothing;     // smoothing_alpha; 0: no smoothing
};
__host__ __device__ inline AssocParams assoc_params(double pose_alpha, double similarity_threshold, double smoothing_alpha) {
#pragma clang fp contract(off)
    AssocParams p;
    p.alpha = (float)pose_alpha, p.beta = (float)(1.0 - pose_alpha);
    p.threshold = (float)similarity_threshold;
    p.now = (float)(1.0 - smoothing_alpha), p.before = (float)smoothing_alpha;
    p.smoothing = smoothing_alpha;
    return p;
}

// one (current, previous) pair: its cost for the assignment and the similarity the threshold is applied to -- NaN, which no
// threshold accepts, where the blend was not finite; returns 1 then
__host__ __device__ inline int assoc_pair(const float *g, const float *d, int J, const int32_t *box_g, const int32_t *box_d,
                                          const double *vars64, const AssocParams &prm, double *cost, float *sim) {
#pragma clang fp contract(off)
    const float sp = assoc_oks(g, d, J, box_g, box_d, vars64), sb = assoc_iou(box_g, box_d);
    const float a = sp * prm.alpha, b = sb * prm.beta;
    const float s = a + b;
    const bool finite = s - s == 0.0f;   // (inf - inf and NaN - NaN are NaN)
    *cost = (double)(1.0f - (finite ? s : 0.0f));
    *sim = finite ? s : __builtin_nanf("");
    return finite ? 0 : 1;
}

__host__ __device__ inline bool assoc_accepted(float sim, const AssocParams &prm) { return sim > prm.threshold; }

__host__ __device__ inline float assoc_smooth_joint(float now, float before, const AssocParams &prm) {
#pragma clang fp contract(off)
    const float a = prm.now * now, b = prm.before * before;
    return a + b;
}
__host__ __device__ inline int32_t assoc_smooth_box(int32_t now, int32_t before, const AssocParams &prm) {
#pragma clang fp contract(off)
    const double a = (1.0 - prm.smoothing) * (double)now, b = prm.smoothing * (double)before;
    return (int32_t)(a + b);   // between the two int32 operands for smoothing in [0, 1]; checked by the entries
}
// the id of the rank-th new person of a problem, in index order
__host__ __device__ inline int32_t assoc_fresh_id(int32_t next_id, int rank) { return (int32_t)((uint32_t)next_id + (uint32_t)rank); }
// next_id after everybody is numbered (scripts/live-demo.py:124)
__host__ __device__ inline int32_t assoc_next_id(int32_t next_id, int32_t max_id) {
    const long long after = (long long)max_id + 1;
    return after > next_id ? (int32_t)(after > 2147483647LL ? 2147483647LL : after) : next_id;
}

// ---- what is wrong with the arguments of the two entries, or nullptr; needs no device -------------------------------------------
inline const char *assoc_fault(int P, const int32_t *cur_start, const int32_t *prev_start, int J, const void *boxes, const void *pts,
                               const void *prev_boxes, const void *prev_pts, const void *prev_ids, const void *next_id,
                               double pose_alpha, double similarity_threshold, double smoothing_alpha, const void *ids,
                               const void *match, const void *status) {
    if (P < 0) return "P is negative";
    if (J < 1 || J > kAssocMaxJoints) return "J must be in [1, HRN_MAX_JOINTS]";
    if (!(pose_alpha - pose_alpha == 0.0) || !(similarity_threshold - similarity_threshold == 0.0))
        return "pose_alpha and similarity_threshold must be finite";
    if (!(smoothing_alpha >= 0.0 && smoothing_alpha <= 1.0)) return "smoothing_alpha must be in [0, 1]";
    if (P == 0) return nullptr;
    if (!cur_start || !prev_start || !next_id || !status) return "null segment tables / next_id / status";
    if (cur_start[0] < 0 || prev_start[0] < 0) return "a segment table starts below zero";
    for (int p = 0; p < P; ++p) {
        if (cur_start[p + 1] < cur_start[p] || prev_start[p + 1] < prev_start[p]) return "a segment table decreases";
        if (cur_start[p + 1] - cur_start[p] > kMaxTracked || prev_start[p + 1] - prev_start[p] > kMaxTracked)
            return "more than HRN_MAX_TRACKED people on one side of a problem";
    }
    if (cur_start[P] > cur_start[0] && (!boxes || !pts || !ids || !match)) return "null boxes / pts / ids / match";
    if (prev_start[P] > prev_start[0] && (!prev_boxes || !prev_pts || !prev_ids)) return "null previous boxes / pts / ids";
    return nullptr;
}

}  // namespace hrn
