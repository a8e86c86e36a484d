// Pose NMS on the GPU (include/hrnet_mi355.h: hrn_pose_nms_dev): rescoring and hard or soft OKS non-maximum suppression per image
// or stream -- the one step of the video loop and of the evaluation chain that still forced the joints through the host.  One
// launch per call, one 256-thread block per problem (one video: one problem; a camera wall: one per stream; an evaluation set: one
// per image):
//
//   phase 1   one thread per person: its score (rescored on request) and its area, into LDS; scores_out
//   phase 2   one thread per person: its position in the order by counting who comes before it (n comparisons)
//   phase 3   a block-uniform loop over the order.  Each kept person's coordinates are staged in LDS, then ONE row of OKS is
//             computed against the people still alive (hard) or still in the list (soft): one thread per candidate, serial over
//             the joints -- numpy's pairwise summation order forbids splitting a pair across lanes.  Hard NMS clears the alive flag
//             of whoever exceeds the threshold; soft NMS rescales the remaining scores and re-orders them with phase 2's routine.
//             Rows of suppressed people are never computed and no n x n matrix exists.
//   phase 4   keep's padding, suppressor, num, status; with `suppress`, zero confidences and boxes for everybody not kept
//
// Order, alive flags, scores, areas and the current row live in LDS (about 17 KiB); nothing is kept on the handle beyond the
// problem table of a call with several problems.  No atomics; every byte has one writer.  This is a latency link, not a throughput
// kernel: a 256-person, 133-joint problem costs up to 256 serial rows of 133 exps per thread, on one CU.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "pose_nms_math.h"

namespace hrn {

__global__ __launch_bounds__(256) void pose_nms_kernel(PoseNmsArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_vars[kAssocMaxJoints], s_gx[kAssocMaxJoints], s_gy[kAssocMaxJoints];
    __shared__ double s_area[kMaxTracked], s_row[kMaxTracked], s_sc[2][kMaxTracked];   // s_sc: the scores by position (soft)
    __shared__ int s_ord[2][kMaxTracked], s_sup[kMaxTracked];
    __shared__ unsigned char s_alive[kMaxTracked];
    const int tid = threadIdx.x;
    const PoseNmsProblem pr = a.P == 1 ? a.one : a.table[blockIdx.x];
    const int n = pr.n, J = a.J;   // n <= kMaxTracked, J <= kAssocMaxJoints: the entry refuses more
    const size_t first = (size_t)pr.first;
    if (n == 0) {
        if (tid == 0) a.num[blockIdx.x] = 0, a.status[blockIdx.x] = 0;
        return;
    }
    PoseNmsPeople ppl{};
    ppl.engine = (a.flags & kPoseNmsEngine) != 0, ppl.J = J, ppl.vis = a.in_vis_thre, ppl.rescore = a.rescore_thre;
    if (ppl.engine)
        ppl.pts = (const float *)a.kpts, ppl.boxes = (const int32_t *)a.areas, ppl.det_scores = (const float *)a.scores;
    else
        ppl.kpts = (const double *)a.kpts, ppl.areas = (const double *)a.areas, ppl.scores = (const double *)a.scores;
    const bool soft = (a.flags & kPoseNmsSoft) != 0;
    const double thresh = a.thresh;

    // ---- phase 1: scores and areas ----
    if (tid < J) s_vars[tid] = pose_nms_var(a.sigmas, tid);
    double sc = 0.0;
    if (tid < n) {
        sc = pose_nms_score(ppl, first + tid);
        a.scores_out[first + tid] = sc;
        s_row[tid] = sc;
        s_area[tid] = pose_nms_area(ppl, first + tid);
        s_sup[tid] = -1;
        s_alive[tid] = 1;
    }
    int status = __syncthreads_or(tid < n && sc != sc) ? 1 : 0;

    // ---- phase 2: the order ----
    if (tid < n) {
        const int r = pose_nms_rank(s_row, n, tid);
        s_ord[0][r] = tid, s_sc[0][r] = sc;
    }
    __syncthreads();

    // ---- phase 3: the sweep (every branch that holds a barrier is block-uniform: it depends on LDS values read after a barrier) ----
    int kept = 0, bad = 0, cur = 0, left = 0;
    if (!soft) {
        for (int pos = 0; pos < n; ++pos) {
            const int i = s_ord[0][pos];
            if (!s_alive[i]) continue;
            if (tid < J) s_gx[tid] = pose_nms_x(ppl, first + i, tid), s_gy[tid] = pose_nms_y(ppl, first + i, tid);
            if (tid == 0) a.keep[first + kept] = i;
            ++kept;
            __syncthreads();
            if (tid > pos && tid < n) {
                const int c = s_ord[0][tid];
                if (s_alive[c]) {
                    const double o = pose_nms_oks(ppl, s_gx, s_gy, s_area[i], first + c, s_area[c], s_vars, &bad);
                    if (o > thresh) s_alive[c] = 0, s_sup[c] = i;
                }
            }
            __syncthreads();
        }
    } else {
        int m = n;
        while (m > 0 && kept < kPoseNmsMaxKeep) {
            const int i = s_ord[cur][0];
            if (tid < J) s_gx[tid] = pose_nms_x(ppl, first + i, tid), s_gy[tid] = pose_nms_y(ppl, first + i, tid);
            if (tid == 0) a.keep[first + kept] = i;
            ++kept;
            __syncthreads();
            const bool mine = tid >= 1 && tid < m;
            int c = -1;
            double rs = 0.0;
            if (mine) {
                c = s_ord[cur][tid];
                const double o = pose_nms_oks(ppl, s_gx, s_gy, s_area[i], first + c, s_area[c], s_vars, &bad);
                rs = pose_nms_soften(s_sc[cur][tid], o, thresh);
                s_row[tid - 1] = rs;
            }
            __syncthreads();
            if (mine) {
                const int r = pose_nms_rank(s_row, m - 1, tid - 1);
                s_ord[cur ^ 1][r] = c, s_sc[cur ^ 1][r] = rs;
            }
            __syncthreads();
            cur ^= 1, --m;
        }
        left = m;
        if (tid < left) s_sup[s_ord[cur][tid]] = -2;   // left over at the cap
    }
    if (__syncthreads_or(bad)) status |= 2;

    // ---- phase 4: the outputs ----
    if (tid < n) {
        a.suppressor[first + tid] = s_sup[tid];
        if (tid >= kept) a.keep[first + tid] = -1;
    }
    if (tid == 0) a.num[blockIdx.x] = kept, a.status[blockIdx.x] = status;
    if (a.flags & kPoseNmsSuppress) {   // (engine layout: the entry refuses the other)
        float *pts = (float *)a.kpts;
        int *boxes = (int *)a.areas;
        for (int idx = tid; idx < n * J; idx += 256) {
            const int i = idx / J;
            if (s_sup[i] != -1) pts[(first * J + idx) * 3 + 2] = 0.0f;
        }
        for (int idx = tid; idx < n * 4; idx += 256)
            if (s_sup[idx >> 2] != -1) boxes[first * 4 + idx] = 0;
    }
}

hipError_t launch_pose_nms(const PoseNmsArgs &a, hipStream_t s) {
    if (a.P <= 0) return hipSuccess;
    hipLaunchKernelGGL(pose_nms_kernel, dim3((unsigned)a.P), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace hrn
