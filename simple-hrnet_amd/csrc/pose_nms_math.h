// The arithmetic of pose NMS -- rescoring and OKS non-maximum suppression, hard and soft (include/hrnet_mi355.h: hrn_pose_nms,
// hrn_pose_nms_dev) -- written ONCE for the host and the device: every function here is compiled into the host entry
// (postproc.cpp) and into the kernel of pose_nms.hip, so the two sides cannot drift apart.  Plain C++, fp contraction off, no FMA,
// no fast-math, no library call; exp is assoc_math.h's assoc_exp: the same bits on both sides.
//
// INPUTS, in one of two layouts; every value is widened exactly to fp64 before any arithmetic:
//   COCO layout    kpts (n, J, 3) float64 (x, y, score), areas float64, scores float64 -- hrn_oks_nms's
//   engine layout  pts (n, J, 3) float32 (y, x, confidence), boxes (n, 4) int32 with area (x2 - x1) * (y2 - y1) in fp64
//                  (assoc_area), det_scores float32 or NULL = 1.0 -- what predict_frame / track_frame return
//
// RESCORING (datasets/COCO.py:360-372; rescore_thre NaN: off, the score stays): sum = 0; for j in joint order: if c_j >
//   rescore_thre: sum = sum + c_j, count += 1; if count != 0: sum = sum / count; score = sum * score.  Sequential fp64 on the
//   widened values.  (The reference's own arrays are float32 there, so numpy would add in float32; this definition is fp64.)
//
// ORDER: descending score and STABLE -- equal scores keep index order (soft NMS's re-ordering: their previous positions).  A NaN
//   score comes after everybody, NaNs among themselves in index order, and sets status bit 0.  This is a definition of ours:
//   numpy's argsort()[::-1] is not stable, and a stream-ordered call cannot raise.  A person's position is the number of people
//   that come before it (pose_nms_rank: n comparisons), on both sides.
//
// OKS(g kept, d candidate) (misc/nms/nms.py:75-94): dx = x_d - x_g, dy = y_d - y_g;
//   e_j = (dx * dx + dy * dy) / vars_j / ((a_g + a_d) / 2 + spacing(1)) / 2, every operation rounded on its own, left to right;
//   vars_j = (sigma_j * 2) * (sigma_j * 2) from J given fp64 sigmas, or COCO's 17 (assoc_coco_var) without;
//   the joints that count are those with c_d > in_vis_thre -- the CANDIDATE's only: the reference's `list(vg > t) and list(vd > t)`
//   is the second list (postproc.cpp keeps the same quirk); in_vis_thre NaN: all joints;
//   terms assoc_exp(-e_j) in joint order, summed in numpy's pairwise order (8-way unrolled leaf, splits above 128 terms, written
//   out for at most 256 terms as in assoc_np_sum), divided by the term count; no term: 0.0.
//   A NON-FINITE OKS (negative areas, NaN or overflowing coordinates, zero sigmas) counts as 0.0 and sets status bit 1.
//
// HARD NMS (nms.py:97-124): walk the order; a person still alive is kept and removes every later alive person whose OKS against
//   it is > thresh; suppressor = the kept person that removed it.
// SOFT NMS (nms.py:138-177): at most 20 people are kept.  After each pick every remaining score becomes
//   s * assoc_exp(-(o * o) / thresh) (o * o, negated, divided, exp, multiplied: each rounded once), and the rest is re-ordered:
//   descending, equal scores keeping their previous positions -- what postproc.cpp's stable_sort does.  People left over at the
//   cap have suppressor -2.
//
// SIZES: at most HRN_MAX_TRACKED = 256 people per problem, J in [1, HRN_MAX_JOINTS = 256].
#pragma once

#include "assoc_math.h"

namespace hrn {

constexpr int kPoseNmsMaxKeep = 20;                                            // misc/nms/nms.py:157
constexpr int kPoseNmsSoft = 1, kPoseNmsSuppress = 2, kPoseNmsEngine = 4;      // = HRN_POSE_NMS_SOFT / _SUPPRESS / _ENGINE

// the people of one call, in either layout (the pointers of the other layout are unused)
struct PoseNmsPeople {
    bool engine;
    int J;
    const double *kpts, *areas, *scores;   // COCO layout
    const float *pts, *det_scores;         // engine layout
    const int32_t *boxes;
    double vis, rescore;                   // in_vis_thre, rescore_thre; NaN: off
};

__host__ __device__ inline double pose_nms_x(const PoseNmsPeople &p, size_t i, int j) {
    return p.engine ? (double)p.pts[(i * p.J + j) * 3 + 1] : p.kpts[(i * p.J + j) * 3];
}
__host__ __device__ inline double pose_nms_y(const PoseNmsPeople &p, size_t i, int j) {
    return p.engine ? (double)p.pts[(i * p.J + j) * 3] : p.kpts[(i * p.J + j) * 3 + 1];
}
__host__ __device__ inline double pose_nms_c(const PoseNmsPeople &p, size_t i, int j) {
    return p.engine ? (double)p.pts[(i * p.J + j) * 3 + 2] : p.kpts[(i * p.J + j) * 3 + 2];
}
__host__ __device__ inline double pose_nms_area(const PoseNmsPeople &p, size_t i) {
    return p.engine ? assoc_area(p.boxes + i * 4) : p.areas[i];
}

// the score a person is ordered by (and scores_out): the given one, rescored when rescore_thre is not NaN
__host__ __device__ inline double pose_nms_score(const PoseNmsPeople &p, size_t i) {
#pragma clang fp contract(off)
    const double s = p.engine ? (p.det_scores ? (double)p.det_scores[i] : 1.0) : p.scores[i];
    if (p.rescore != p.rescore) return s;
    double sum = 0.0;
    int count = 0;
    for (int j = 0; j < p.J; ++j) {
        const double c = pose_nms_c(p, i, j);
        if (c > p.rescore) sum = sum + c, ++count;
    }
    if (count != 0) sum = sum / (double)count;
    return sum * s;
}

__host__ __device__ inline double pose_nms_var(const double *sigmas, int j) {
#pragma clang fp contract(off)
    if (!sigmas) return assoc_coco_var(j);
    const double s = sigmas[j];
    return (s * 2) * (s * 2);
}

// does (score sa at position pa) come before (sb at pb)?  A strict total order for pa != pb.
__host__ __device__ inline bool pose_nms_before(double sa, int pa, double sb, int pb) {
    const bool na = sa != sa, nb = sb != sb;
    if (na || nb) return na == nb ? pa < pb : nb;
    return sa > sb || (sa == sb && pa < pb);
}
// the position of entry `me` of sc[0 .. n) in that order
__host__ __device__ inline int pose_nms_rank(const double *sc, int n, int me) {
    const double s = sc[me];
    int r = 0;
    for (int k = 0; k < n; ++k) r += (k != me && pose_nms_before(sc[k], k, s, me)) ? 1 : 0;
    return r;
}

// walks the joints of one (kept g, candidate d) pair in order and yields exp(-e) of those the candidate's mask lets through;
// g's coordinates are given widened (the kernel stages them once per row)
struct PoseNmsCursor {
    const PoseNmsPeople *p;
    const double *gx, *gy, *vars;
    size_t d;
    double denom;
    int j;

    __host__ __device__ bool counts(int jj) const { return p->vis != p->vis || pose_nms_c(*p, d, jj) > p->vis; }
    __host__ __device__ int count() const {
        int c = 0;
        for (int jj = 0; jj < p->J; ++jj) c += counts(jj) ? 1 : 0;
        return c;
    }
    // the next term; called at most count() times after j = 0
    __host__ __device__ double next() {
#pragma clang fp contract(off)
        for (;;) {
            const int jj = j++;
            if (!counts(jj)) continue;
            const double dx = pose_nms_x(*p, d, jj) - gx[jj], dy = pose_nms_y(*p, d, jj) - gy[jj];
            const double e = (dx * dx + dy * dy) / vars[jj] / denom / 2;
            return assoc_exp(-e);
        }
    }
};

// numpy's pairwise summation over the cursor: assoc_sum_leaf / assoc_np_sum of assoc_math.h, statement for statement (they are
// written for that header's cursor type)
__host__ __device__ inline double pose_nms_sum_leaf(PoseNmsCursor &c, int len) {
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
__host__ __device__ inline double pose_nms_np_sum(PoseNmsCursor &c, int n) {
#pragma clang fp contract(off)
    if (n <= 128) return pose_nms_sum_leaf(c, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    const double left = pose_nms_sum_leaf(c, n2);
    const int rest = n - n2;
    if (rest <= 128) return left + pose_nms_sum_leaf(c, rest);
    int n3 = rest / 2;
    n3 -= n3 % 8;
    const double mid = pose_nms_sum_leaf(c, n3);
    return left + (mid + pose_nms_sum_leaf(c, rest - n3));
}

// OKS of candidate d against the kept person whose widened coordinates are gx / gy and whose area is a_g; a non-finite value
// comes back as 0.0 with *bad set
__host__ __device__ inline double pose_nms_oks(const PoseNmsPeople &p, const double *gx, const double *gy, double a_g, size_t d,
                                               double a_d, const double *vars, int *bad) {
#pragma clang fp contract(off)
    PoseNmsCursor c;
    c.p = &p, c.gx = gx, c.gy = gy, c.vars = vars, c.d = d, c.j = 0;
    c.denom = (a_g + a_d) / 2 + 2.220446049250313e-16;   // np.spacing(1)
    const int n = c.count();
    const double o = n == 0 ? 0.0 : pose_nms_np_sum(c, n) / (double)n;
    if (o - o == 0.0) return o;
    *bad = 1;
    return 0.0;
}

// soft NMS: a remaining person's score after a pick whose OKS against it is o (rescore(..., type='gaussian'), nms.py:133)
__host__ __device__ inline double pose_nms_soften(double s, double o, double thresh) {
#pragma clang fp contract(off)
    const double q = -(o * o) / thresh;
    return s * assoc_exp(q);
}

// ---- what is wrong with the arguments of the two entries, or nullptr; needs no device -------------------------------------------
inline const char *pose_nms_fault(int P, const int32_t *start, int J, int flags, const void *kpts, const void *areas, const void *scores,
                                  double thresh, const double *sigmas, const void *keep, const void *num, const void *scores_out,
                                  const void *suppressor, const void *status) {
    if (P < 0) return "P is negative";
    if (J < 1 || J > kAssocMaxJoints) return "J must be in [1, HRN_MAX_JOINTS]";
    if (flags & ~(kPoseNmsSoft | kPoseNmsSuppress | kPoseNmsEngine)) return "unknown flag bits";
    if ((flags & kPoseNmsSuppress) && !(flags & kPoseNmsEngine)) return "suppress needs the engine layout";
    if (!(thresh - thresh == 0.0)) return "thresh must be finite";
    if ((flags & kPoseNmsSoft) && !(thresh > 0.0)) return "soft NMS needs thresh > 0";
    if (!sigmas && J != 17) return "the default sigmas are COCO's 17: pass sigmas for another J";
    if (P == 0) return nullptr;
    if (!start || !num || !status) return "null segment table / num / status";
    if (start[0] < 0) return "the segment table starts below zero";
    for (int p = 0; p < P; ++p) {
        if (start[p + 1] < start[p]) return "the segment table decreases";
        if (start[p + 1] - start[p] > kMaxTracked) return "more than HRN_MAX_TRACKED people in one problem";
    }
    if (start[P] > start[0]) {
        if (!kpts || !areas || !keep || !scores_out || !suppressor) return "null keypoints / areas or boxes / keep / scores_out / suppressor";
        if (!(flags & kPoseNmsEngine) && !scores) return "null scores";
    }
    return nullptr;
}

}  // namespace hrn
